"""Operator-level tests of the decode GEMV family (csrc/decode_gemv.hip, csrc/decode.hip) through the C ABI.

itts_gemv_bf16 is the 1-4 row bf16 GEMV of the launch path's decode step (gemv_bf16: four prologues, fp32 / bf16 input and
output, bf16 / fp8 weights, 4- and 5-wave workgroups, a block-cooperative and a wave-autonomous form); itts_gemv the fp32
kernels gemv2 (version 2) and gemv (version 1) that take the calls the bf16 GEMV refuses.  Every reference is fp64 torch on the
CPU from the SAME rounded inputs, computed once per (variant, K, N) for the four pool rows and shared by every call of that test:

  prologue 0  x (bf16) . W + bias
  prologue 1  LayerNorm(x, eps 1e-5, no affine) in fp64, rounded to bf16, . W + bias
  prologue 2  LayerNorm(gamma, beta), then LayerNorm without affine, rounded to bf16
  prologue 3  the unsplit softmax attention output in fp64, rounded to bf16 - the kernel is handed the same problem as
              ATTN_NSPLIT = 4 per-range partials (max, sum, un-normalised weighted V), some ranges empty
  fp8         the decoded e4m3 values times the power-of-two row scale (pack.quantize_gpt_fp8's construction)

Bounds (relerr of test_gpu_ops.py, the project's own classes for the same constructions): 2e-5 for fp32 output from bf16 x
(test_skinny_gemm); 2e-3 for fp32 output behind a LayerNorm (or a merge) that is rounded to bf16 and 1e-2 for bf16 output
(test_skinny_gemm_layernorm_prologue: a bf16 rounding may land on the neighbouring value where the moments differ in the last ulp).
itts_gemv: 2e-5 (fp32 accumulation; bf16 weights against the same bf16 values in fp64).

relerr is the largest error over the largest reference of what it is given, and a single output has no such scale: the GELU
of a negative pre-activation, or a dot product that happens to cancel, is small for good reason and carries the absolute error
of its terms (measured: 1.1e-2 "relative" on the one output gelu(..) = -2.1e-6 at N = 1, B = 1, every neighbour at 1e-7).  So the
three widths of one (variant, K, B) are judged together, as one 108-wide output against the largest reference among them; the
bit-exact properties, the NaN and the sentinel checks stay per call.

Every call: the selector is asked first (itts_gemv_which >= 0), the X / partial rows past B and one weight row past N hold NaN (a
stray read shows in the result instead of leaving the allocation), Y has 4 rows - NaN where the call stores, a sentinel in the
rows past B that has to survive.  Bit-exact properties of gemv_bf16_kernel: a row alone (B = 1) = that row inside a 2-, 3-, 4-row
call; identical rows give identical outputs; two runs agree.

The K ranges the block-cooperative kernel cannot run (fp32 x at 512 < K < 1024, bf16 x at 2048 < K < 4608: it masks only its
last chunk) are refused by the selector and never launched here - test_rejected_ranges checks that on the host.

ITTS_GEMV_MODE / ITTS_GEMV_W5 are read once per process: their cases run in a fresh child Python (this file, `child` argument)
that reports its errors as JSON, held to the same bounds.  The measured maxima are printed and, where
ITTS_TEST_OUT names a directory, written to decode_gemv_ops.txt there (committed as profiles/decode_gemv_ops.txt)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

if __name__ == "__main__":  # the child process: same import roots as tests/conftest.py
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "index-tts-ipex_amd")]

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from itts_hip import prng

DEV = "cuda:0"
NSPLIT = 4  # csrc/itts_decode.h ATTN_NSPLIT
SENT = 777.0
NS = (1, 37, 70)  # small and ragged: K, B and the variant exercise the kernel, not the width
KS_ALL = (64, 72, 504, 512, 1024, 1032, 1280, 1528, 1536, 1544, 2040, 2048, 4608, 4616, 5112, 5120)  # NCH 1 | 3 | 4 | 10
# what the selector takes of them (test_case_lists_match_the_selector holds these lists against itts_gemv_which)
KS_F32X = (64, 72, 504, 512, 1024, 1032, 1280, 1528, 1536)  # fp32 x (prologue 1, 2): 1 or 3 chunks
KS_BF16X = tuple(K for K in KS_ALL if K != 1024)             # bf16 x, prologue 0: two chunks have no kernel
KS_SPLIT = (64, 512, 1280, 1536)                             # prologue 3: whole heads, 1 or 3 chunks


def rnd(name, shape, std=1.0):
    return torch.from_numpy(prng.tensor(name, 5, shape, std=std))


def relerr(a, b):  # tests/test_gpu_ops.py
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    """Wait for the launch; a device fault ends the session there (nothing more is started on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


def gelu_new(v):
    return 0.5 * v * (1 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v ** 3)))


# name -> prologue, x bf16, y bf16, GELU_NEW, accumulate, bias, fp8 weights, bound
VARIANTS = {
    "ln_f32": (1, 0, 0, 0, 0, 1, 0, 2e-3),
    "ln_f32_gelu_nobias": (1, 0, 0, 1, 0, 0, 0, 2e-3),
    "ln_bf16_gelu": (1, 0, 1, 1, 0, 1, 0, 1e-2),
    "ln_bf16_nobias": (1, 0, 1, 0, 0, 0, 0, 1e-2),
    "ln2_affine": (2, 0, 0, 0, 0, 1, 0, 2e-3),
    "bf16x": (0, 1, 0, 0, 0, 1, 0, 2e-5),
    "bf16x_acc": (0, 1, 0, 0, 1, 1, 0, 2e-5),
    "bf16x_acc_nobias": (0, 1, 0, 0, 1, 0, 0, 2e-5),
    "bf16x_gelu": (0, 1, 0, 1, 0, 1, 0, 2e-5),
    "split": (3, 1, 0, 0, 0, 0, 0, 2e-3),
    "split_acc": (3, 1, 0, 0, 1, 1, 0, 2e-3),
    "fp8_ln_f32": (1, 0, 0, 0, 0, 1, 1, 2e-3),
    "fp8_bf16x_acc": (0, 1, 0, 0, 1, 1, 1, 2e-5),
}


def ks_of(variant):
    pro, xbf, fp8 = VARIANTS[variant][0], VARIANTS[variant][1], VARIANTS[variant][6]
    ks = KS_SPLIT if pro == 3 else KS_BF16X if xbf else KS_F32X
    return tuple(K for K in ks if K in (512, 1280, 5120)) if fp8 else ks


# ---- inputs and fp64 references (CPU), one pool of 4 rows per K -------------------------------------------------------------
# split-attention fixture: key counts of the 4 ranges of one (row, head); zero = an empty range, as short or left-padded
# sequences produce (max = -inf, sum 0, o 0)
RANGES = [(5, 4, 6, 3), (7, 0, 3, 2), (0, 0, 9, 4), (1, 1, 1, 1), (3, 2, 0, 0), (16, 16, 16, 5), (0, 5, 0, 2), (2, 3, 4, 0)]


@functools.lru_cache(maxsize=None)
def split_fixture(K):
    """A random softmax-attention problem per (row, head) of the 4 pool rows: the unsplit fp64 output [4, K] and the partials
    as decode_attn2 leaves them, attn_o [4][K/64][4][64] and attn_ml [4][K/64][2][4] (fp32)."""
    H = K // 64
    full = torch.zeros(4, K, dtype=torch.float64)
    o = torch.zeros(4, H, NSPLIT, 64, dtype=torch.float64)
    ml = torch.zeros(4, H, 2, NSPLIT, dtype=torch.float64)
    for r in range(4):
        for h in range(H):
            cnt = RANGES[(r * H + h + r) % len(RANGES)]
            T = sum(cnt)
            s = (rnd(f"dg.s{K}.{r}.{h}", (T,)) * 2.0).double()
            v = rnd(f"dg.v{K}.{r}.{h}", (T, 64)).double()
            full[r, h * 64:(h + 1) * 64] = torch.softmax(s, 0) @ v
            t0 = 0
            for p, n in enumerate(cnt):
                if n == 0:
                    ml[r, h, 0, p] = float("-inf")
                    continue
                sp, vp_ = s[t0:t0 + n], v[t0:t0 + n]
                e = torch.exp(sp - sp.max())
                ml[r, h, 0, p], ml[r, h, 1, p] = sp.max(), e.sum()
                o[r, h, p] = e @ vp_
                t0 += n
    return full, o.float(), ml.float()


def merge_partials(o, ml):
    """fp64 merge of the partials: weights exp(max_p - max), one division per head -> [rows, K]."""
    o, ml = o.double(), ml.double()
    m, l = ml[:, :, 0], ml[:, :, 1]
    wgt = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - m.max(-1, keepdim=True).values))
    x = (wgt[..., None] * o).sum(2) / (wgt * l).sum(-1)[..., None]
    return x.reshape(o.shape[0], -1)


def quantize_rows_e4m3(w):
    """pack.quantize_gpt_fp8's construction for one matrix: e4m3 bytes and one power-of-two scale per output row."""
    w = w.float()
    amax = w.abs().amax(dim=1).clamp_min(1e-30)
    scale = torch.pow(2.0, torch.ceil(torch.log2(amax / 448.0)))
    q = (w / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.float(), q.float() * scale[:, None]


@functools.lru_cache(maxsize=8)
def pool(variant, K, N):
    """Inputs of the 4 pool rows and the fp64 reference [4, N] for them (every row is independent of the others)."""
    pro, xbf, ybf, gelu, acc, has_bias, fp8, _ = VARIANTS[variant]
    p = {}
    p["w"] = (rnd(f"dg.w{N}x{K}", (N, K)) * 0.05).to(torch.bfloat16)
    wref = p["w"].double()
    if fp8:
        p["w8"], p["wscale"], deq = quantize_rows_e4m3(rnd(f"dg.w{N}x{K}", (N, K)) * 0.05)
        wref = deq.double()
    p["bias"] = rnd(f"dg.b{N}", (N,)) if has_bias else None
    p["y0"] = rnd(f"dg.y{N}", (4, N))
    if pro == 3:
        full, p["attn_o"], p["attn_ml"] = split_fixture(K)
        xn = full.to(torch.bfloat16)
    elif xbf:
        p["x"] = (rnd(f"dg.xb{K}", (4, K)) * 1.5).to(torch.bfloat16)
        xn = p["x"]
    else:
        p["x"] = rnd(f"dg.x{K}", (4, K)) * 2.5 + 0.3
        xn = p["x"].double()
        if pro == 2:
            p["gamma"], p["beta"] = rnd(f"dg.g{K}", (K,)) * 0.2 + 1, rnd(f"dg.be{K}", (K,)) * 0.1
            xn = torch.nn.functional.layer_norm(xn, (K,), p["gamma"].double(), p["beta"].double(), 1e-5)
        xn = torch.nn.functional.layer_norm(xn, (K,), None, None, 1e-5).to(torch.bfloat16)
    ref = xn.double() @ wref.T
    if has_bias:
        ref = ref + p["bias"].double()
    if gelu:
        ref = gelu_new(ref)
    if acc:
        ref = ref + p["y0"].double()
    p["ref"] = ref
    return p


# ---- one call ----------------------------------------------------------------------------------------------------------------
def pad_rows(t, rows, fill=float("nan")):
    """rows of the pool as the call's first len(rows) rows; the rows up to 4 hold `fill`"""
    out = torch.full((4,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:len(rows)] = t[list(rows)]
    return out.to(DEV)


def nan_row(t, fill=float("nan")):
    """[N, ...] -> [N + 1, ...] on the device with `fill` behind the last row"""
    pad = torch.full((1,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    return torch.cat([t, pad]).contiguous().to(DEV)


def call_bf16(lib, variant, K, N, rows, w5=0):
    """itts_gemv_bf16 on the pool rows `rows` (B = len(rows)) -> the B output rows on the CPU.  Asks the selector first and checks
    the sentinel rows."""
    pro, xbf, ybf, gelu, acc, has_bias, fp8, _ = VARIANTS[variant]
    p, B = pool(variant, K, N), len(rows)
    assert int(lib.itts_gemv_which(B, N, K, pro, xbf, ybf, w5)) >= 0, (variant, B, N, K)
    keep = {"w": nan_row(p["w"])}
    ptr = {k: None for k in ("x", "bias", "gamma", "beta", "attn_o", "attn_ml", "w8", "wscale")}
    if fp8:
        keep["w"] = torch.full_like(keep["w"], float("nan"))  # the fp8 instantiation must not read the bf16 weights
        keep["w8"], keep["wscale"] = nan_row(p["w8"], 0x7F), nan_row(p["wscale"])
    if has_bias:
        keep["bias"] = nan_row(p["bias"])
    for k in ("x", "attn_o", "attn_ml"):
        if k in p:
            keep[k] = pad_rows(p[k], rows)
    for k in ("gamma", "beta"):
        if k in p:
            keep[k] = p[k].to(DEV)
    for k, t in keep.items():
        ptr[k] = t.data_ptr()
    y = torch.full((4, N), float("nan"), dtype=torch.bfloat16 if ybf else torch.float32)
    if acc:
        y[:B] = p["y0"][list(rows)]
    y[B:] = SENT
    y = y.to(DEV)
    L.check(lib.itts_gemv_bf16(y.data_ptr(), ybf, ptr["x"], xbf, ptr["w"], ptr["bias"], B, N, K,
                               L.ACT_GELU_NEW if gelu else L.ACT_NONE, acc, pro, ptr["gamma"], ptr["beta"], ptr["attn_o"],
                               ptr["attn_ml"], ptr["w8"], ptr["wscale"], stream()), "gemv_bf16")
    sync()
    out = y.cpu()
    assert bool((out[B:] == SENT).all()), (variant, K, N, B, "rows past B were written")
    return out[:B]


MEASURED = {}  # table line -> (max relerr, bound)


def record(line, err, bound):
    MEASURED[line] = (max(err, MEASURED.get(line, (0.0, bound))[0]), bound)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [f"{k:<44s} max relerr {e:9.3e}   bound {b:.0e}" for k, (e, b) in sorted(MEASURED.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_gemv_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def nch_of(K):
    n = (K + 511) // 512
    return 1 if n <= 1 else 3 if n <= 3 else 4 if n <= 4 else 10


# ---- CPU: the fixtures and the selector -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS_SPLIT)
def test_split_fixture_merges_to_the_unsplit_attention(K):
    """The fixture itself: the fp64 merge of the synthetic partials is the unsplit attention.  The maxima are fp32 scores (exact);
    sums and weighted V are rounded to fp32, 2^-24 relative each and a handful of them per output, hence 1e-6 of the largest
    output.  Heads with no, one and two empty ranges occur."""
    full, o, ml = split_fixture(K)
    assert relerr(merge_partials(o, ml), full) < 1e-6
    empty = torch.isinf(ml[:, :, 0]).sum(-1).flatten().tolist()
    if K >= 512:
        assert {0, 1, 2} <= set(empty)
    assert bool((ml[:, :, 1][torch.isinf(ml[:, :, 0])] == 0).all()) and bool((o[torch.isinf(ml[:, :, 0])] == 0).all())
    assert not bool(torch.isinf(ml[:, :, 0]).all(-1).any())  # every head has keys


def test_case_lists_match_the_selector(lib):
    """The K lists above are what itts_gemv_which takes of the issue's shapes - nothing is dropped quietly: the only refusals
    are two chunks of bf16 x (K = 1024: the ladder never had that kernel), fp32 x past 3 chunks, and part heads."""
    for B in (1, 2, 3, 4):
        for N in NS:
            for K in KS_ALL:
                for pro, ybf in ((1, 0), (1, 1), (2, 0)):
                    assert (lib.itts_gemv_which(B, N, K, pro, 0, ybf, 0) >= 0) == (K in KS_F32X), (B, N, K, pro)
                assert (lib.itts_gemv_which(B, N, K, 0, 1, 0, 0) >= 0) == (K in KS_BF16X), (B, N, K)
                assert (lib.itts_gemv_which(B, N, K, 3, 1, 0, 0) >= 0) == (K in KS_SPLIT), (B, N, K)
                got = int(lib.itts_gemv_which(B, N, K, 0, 1, 0, 0))
                if got >= 0:
                    assert (got >> 8) & 255 == nch_of(K) and K >= (nch_of(K) - 1) * 512
    assert {nch_of(K) for K in KS_F32X} == {1, 3} and {nch_of(K) for K in KS_BF16X} == {1, 3, 4, 10}


def test_rejected_ranges(lib):
    """Host only: the K ranges gemv_bf16_kernel cannot run (it masks only its last chunk) are refused by the selector and by the
    entry point, which returns the error before any launch; their neighbours K = 1024 (fp32 x) and K = 4608 (bf16 x) are taken."""
    host = np.zeros(16, dtype=np.float32)  # never read: the call is refused on the host
    hp = host.ctypes.data
    for B, N, K, pro, xbf in ((2, 37, 768, 1, 0), (2, 37, 4096, 0, 1), (2, 37, 2056, 0, 1)):
        assert lib.itts_gemv_which(B, N, K, pro, xbf, 0, 0) == -1 and lib.itts_gemv_which(B, N, K, pro, xbf, 0, 1) == -1
        st = lib.itts_gemv_bf16(hp, 0, hp, xbf, hp, None, B, N, K, L.ACT_NONE, 0, pro, None, None, None, None, None, None, None)
        assert st != 0 and b"unsupported shape" in lib.itts_last_error(), (B, N, K, st, lib.itts_last_error())
    assert lib.itts_gemv_which(2, 37, 1024, 1, 0, 0, 0) >= 0
    assert lib.itts_gemv_which(2, 37, 4608, 0, 1, 0, 0) >= 0
    # gemv2 / gemv take what was refused: the engine's fallback
    assert lib.itts_gemv_which(2, 37, 1016, 2, 0, 0, 0) == -1 and lib.itts_gemv_which(2, 37, 520, 1, 0, 1, 0) == -1


# ---- GPU: gemv_bf16, default form ---------------------------------------------------------------------------------------------
BF16_CASES = [(v, K) for v in VARIANTS for K in ks_of(v)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,K", BF16_CASES)
def test_gemv_bf16(lib, variant, K):
    bound = VARIANTS[variant][7]
    outs, refs = {}, {}
    for N in NS:
        refs[N] = pool(variant, K, N)["ref"]
        for B in (1, 2, 3, 4):
            outs[N, B] = call_bf16(lib, variant, K, N, range(B))
            assert not bool(torch.isnan(outs[N, B].float()).any()), (variant, K, N, B)
        # a row computed alone has the bits of that row inside a 2-, 3- and 4-row call
        alone = {0: outs[N, 1]}
        alone.update({r: call_bf16(lib, variant, K, N, [r]) for r in (1, 2, 3)})
        for B in (2, 3, 4):
            for r in range(B):
                assert torch.equal(outs[N, B][r], alone[r][0]), (variant, K, N, f"row {r} alone differs from row {r} of {B}")
        # identical input rows give identical output rows
        same = call_bf16(lib, variant, K, N, [1, 1, 1, 1])
        for r in range(1, 4):
            assert torch.equal(same[r], same[0]), (variant, K, N, r)
        # two runs of the same call agree
        assert torch.equal(call_bf16(lib, variant, K, N, range(4)), outs[N, 4]), (variant, K, N)
    # relerr per row count over the three widths together (see the file's docstring: one output has no scale of its own)
    worst = 0.0
    for B in (1, 2, 3, 4):
        e = relerr(torch.cat([outs[N, B].float() for N in NS], 1), torch.cat([refs[N][:B] for N in NS], 1))
        print(f"gemv_bf16 {variant} K={K} N={NS} B={B}: relerr {e:.3e} (bound {bound:.0e})")
        worst = max(worst, e)
    record(f"gemv_bf16 {variant} NCH={nch_of(K)}", worst, bound)
    assert worst < bound, (variant, K, worst)


# ---- GPU: itts_gemv (gemv2 = version 2, gemv = version 1) -----------------------------------------------------------------
KS_GEMV = (8, 72, 512, 520, 768, 1280, 1544, 5120)  # gemv2 masks every chunk: two chunks are in range for it
# name -> prologue, first LayerNorm has gamma / beta, second LayerNorm has gamma / beta
GEMV_PRO = {"plain": (0, 0, 0), "ln_affine": (1, 1, 0), "ln_null_gamma": (1, 0, 0), "ln_ln": (2, 1, 1), "ln_ln_null_gamma2": (2, 1, 0)}
GEMV_CASES = [(ver, wdt, pn, K) for ver in (2, 1) for wdt in ("f32", "bf16") for pn in GEMV_PRO for K in KS_GEMV
              if ver == 2 or GEMV_PRO[pn][0] < 2]


@functools.lru_cache(maxsize=8)
def gemv_pool(wdt, pn, K, N):
    pro, aff1, aff2 = GEMV_PRO[pn]
    p = {"x": rnd(f"gv.x{K}", (4, K)) * 2.5 + 0.3, "bias": rnd(f"gv.b{N}", (N,)), "y0": rnd(f"gv.y{N}", (4, N))}
    w = rnd(f"gv.w{N}x{K}", (N, K)) * 0.05
    p["w"] = w.to(torch.bfloat16) if wdt == "bf16" else w
    xn = p["x"].double()
    for i, aff in ((1, aff1), (2, aff2)):
        if pro >= i:
            if aff:
                p[f"g{i}"], p[f"b{i}"] = rnd(f"gv.g{i}.{K}", (K,)) * 0.2 + 1, rnd(f"gv.be{i}.{K}", (K,)) * 0.1
            xn = torch.nn.functional.layer_norm(xn, (K,), p[f"g{i}"].double() if aff else None, p[f"b{i}"].double() if aff else None, 1e-5)
    p["lin"] = xn @ p["w"].double().T + p["bias"].double()
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("ver,wdt,pn,K", GEMV_CASES)
def test_itts_gemv(lib, ver, wdt, pn, K):
    pro = GEMV_PRO[pn][0]
    groups = {}  # (gelu, accumulate, B) -> [(got, ref)] over the widths that run this pair
    for N in NS:
        p = gemv_pool(wdt, pn, K, N)
        dev = {k: (nan_row(p[k]) if k in ("w", "bias") else p[k].to(DEV)) for k in p if k in ("w", "bias", "g1", "b1", "g2", "b2")}
        ptr = {k: dev[k].data_ptr() if k in dev else None for k in ("g1", "b1", "g2", "b2")}
        # every (activation, accumulate) pair: two per width
        for gelu, acc in ((0, 0), (1, 1)) if N != 37 else ((1, 0), (0, 1)):
            for B in (1, 2, 3, 4):
                x = pad_rows(p["x"], range(B))
                y = torch.full((4, N), float("nan"))
                if acc:
                    y[:B] = p["y0"][:B]
                y[B:] = SENT
                yd = [y.to(DEV), y.to(DEV)]
                sts = [lib.itts_gemv(t.data_ptr(), x.data_ptr(), dev["w"].data_ptr(), dev["bias"].data_ptr(), B, N, K,
                                     L.ACT_GELU_NEW if gelu else L.ACT_NONE, acc, pro, ptr["g1"], ptr["b1"], ptr["g2"], ptr["b2"],
                                     L.BF16 if wdt == "bf16" else L.F32, ver, stream()) for t in yd]
                if ver == 2 and B > 2 and K == 5120:
                    # gemv2 keeps 4 rows x K floats in 64 KiB of LDS: 3 and 4 rows of K = 5120 are the generic kernel's
                    assert sts[0] != 0 and b"unsupported shape" in lib.itts_last_error()
                    continue
                L.check(sts[0], "gemv"), L.check(sts[1], "gemv")
                sync()
                got = yd[0].cpu()
                assert bool((got[B:] == SENT).all()) and torch.equal(got, yd[1].cpu()), (ver, wdt, pn, K, N, B)
                assert not bool(torch.isnan(got[:B]).any()), (ver, wdt, pn, K, N, B)
                ref = gelu_new(p["lin"][:B]) if gelu else p["lin"][:B]
                ref = ref + p["y0"][:B].double() if acc else ref
                groups.setdefault((gelu, acc, B), []).append((got[:B], ref))
    worst = 0.0
    for (gelu, acc, B), parts in sorted(groups.items()):  # the widths of one pair together: one output has no scale of its own
        e = relerr(torch.cat([g for g, _ in parts], 1), torch.cat([r for _, r in parts], 1))
        print(f"itts_gemv v{ver} W {wdt} {pn} K={K} B={B} gelu={gelu} acc={acc} ({sum(g.shape[1] for g, _ in parts)} outputs): "
              f"relerr {e:.3e} (bound 2e-05)")
        worst = max(worst, e)
    record(f"itts_gemv v{ver} W {wdt} {pn}", worst, 2e-5)
    assert worst < 2e-5, (ver, wdt, pn, K, worst)


# ---- GPU: the non-default forms, each in a fresh process --------------------------------------------------------------------
D = 1280
# (variant, K, N): the 5-wave rows name their N
W5_CASES = [("ln_f32", D, 3 * D), ("ln_bf16_gelu", D, 4 * D), ("bf16x_acc", D, D), ("bf16x_acc", 4 * D, D), ("split_acc", D, D),
            ("fp8_bf16x_acc", 4 * D, D)]
MODE1_CASES = [(v, K, 37) for v, ks in (("ln_f32", (72, 512, 1032, 1536)), ("ln_bf16_gelu", (504, 1280)), ("ln2_affine", (512, 1280)),
                                        ("bf16x_acc", (64, 1528, 2040, 4616, 5120)), ("fp8_ln_f32", (1280,)),
                                        ("fp8_bf16x_acc", (512, 5120))) for K in ks]


def child_main(cases, rows_max, w5):
    """The child's side: every case at B = 1 .. rows_max against its reference -> {"variant K N": max relerr} as one JSON line."""
    lib = L.load()
    out = {}
    for variant, K, N in cases:
        ref = pool(variant, K, N)["ref"]
        ys = [call_bf16(lib, variant, K, N, range(B), w5) for B in range(1, rows_max + 1)]
        assert all(not bool(torch.isnan(y.float()).any()) for y in ys), (variant, K, N)
        out[f"{variant} {K} {N}"] = max(relerr(y.float(), ref[:len(y)]) for y in ys)
    print("RESULT " + json.dumps(out))


def run_child(env_name, cases, rows_max, w5):
    env = dict(os.environ, **{env_name: "1"})
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "child", json.dumps(cases), str(rows_max), str(w5)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode not in (0, 1):  # not a failed comparison: a fault or an abort in the child
        pytest.exit(f"child process ended with {r.returncode}, nothing more is launched: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][7:])


def check_child(tag, res, cases):
    assert set(res) == {f"{v} {K} {N}" for v, K, N in cases}
    for v, K, N in cases:
        e, bound = res[f"{v} {K} {N}"], VARIANTS[v][7]
        print(f"gemv_bf16 [{tag}] {v} K={K} N={N}: relerr {e:.3e} (bound {bound:.0e})")
        record(f"gemv_bf16 [{tag}] {v} NCH={nch_of(K)}", e, bound)
    bad = [(c, res[f"{c[0]} {c[1]} {c[2]}"]) for c in cases if not res[f"{c[0]} {c[1]} {c[2]}"] < VARIANTS[c[0]][7]]
    assert not bad, bad


@pytest.mark.gpu
def test_wave_autonomous_form_in_a_child_process(lib):
    """ITTS_GEMV_MODE=1: gemv_wave_kernel for every call with 4 waves.  Same bounds; to tolerance, not to bits (the wave kernel does
    not pin its LayerNorm arithmetic)."""
    check_child("ITTS_GEMV_MODE=1", run_child("ITTS_GEMV_MODE", MODE1_CASES, 4, 0), MODE1_CASES)


@pytest.mark.gpu
def test_five_wave_rows_in_a_child_process(lib):
    """ITTS_GEMV_W5=1: the 5-wave workgroups of the full-size projections at 1 and 2 rows (256 workgroups of 5 waves)."""
    for v, K, N in W5_CASES:
        pro, xbf, ybf = VARIANTS[v][:3]
        for B in (1, 2):
            assert lib.itts_gemv_which(B, N, K, pro, xbf, ybf, 1) >> 16 == 5, (v, K, N, B)
            assert lib.itts_gemv_which(B, N, K, pro, xbf, ybf, 0) >> 16 == 4
    assert len(W5_CASES) == 6
    check_child("ITTS_GEMV_W5=1", run_child("ITTS_GEMV_W5", W5_CASES, 2, 1), W5_CASES)


# ---- GPU: the engine's fallback at a width whose projections the bf16 GEMV refuses --------------------------------------------
@pytest.mark.gpu
def test_engine_width_576_decodes_through_the_fallback():
    """Model width 576 (9 heads, 2 layers, the micro topology otherwise): K = 576 and K = 4 x 576 = 2304 lie in the two refused
    ranges, so the bf16 engine's decode step has to run its projections on gemv2 / gemv with fp32 activations (the bf_act / bf_ctx
    probes and run() of csrc/model_gpt.hip agree, no requirement trips).  Teacher-forced, 2 identical rows, 8 decode steps: the
    logits against the fp32 engine on the bf16-rounded weights - the control of tests/test_gpu_bf16_accuracy.py, its rms_rel and
    its BOUND; the fp32 engine runs other kernels on other activations, so a wrong bf16 projection shows."""
    from itts_hip import config as icfg
    from itts_hip import engine as ieng
    from itts_hip import synth
    from test_gpu_bf16_accuracy import BOUND, rms_rel

    cfg = icfg.micro()
    cfg.gpt.model_dim, cfg.gpt.heads = 576, 9
    lib = L.load()
    for B in (1, 2, 3, 4):  # what the decode step will ask the selector
        assert lib.itts_gemv_which(B, 3 * 576, 576, 1, 0, 0, 0) == -1 and lib.itts_gemv_which(B, 576, 4 * 576, 0, 1, 0, 0) == -1
    sd = synth.gpt_state_dict(cfg, 1234, profile="smooth")
    rounded = {k: (torch.from_numpy(np.asarray(v)).to(torch.bfloat16).float().numpy() if np.asarray(v).ndim >= 2 else v)
               for k, v in sd.items()}
    steps = 8
    cond = rnd("dg.cond", (32, 576))
    text = np.repeat(synth.text_ids(11, 11, cfg.gpt.number_text_tokens).reshape(1, -1).astype(np.int32), 2, 0)
    forced = prng.randint("dg.forced", 5, steps, 0, cfg.gpt.start_mel_token).astype(np.int32).reshape(1, -1)
    trace = {}
    for dt, weights in (("bf16", sd), ("fp32", rounded)):
        eng = ieng.build_engine(cfg, dt, parts=("gpt",), state_dicts={"gpt": weights})
        eng.set_forced(forced)
        try:
            eng.prefill(cond, text, steps + 1, 10.0, True)
            lgs = []
            for k in range(steps + 1):
                if k:
                    eng.decode(1)
                codes, lg = eng.fetch(logits=True)
                n = min(k + 1, steps)  # the sampler has already chosen token k from these logits
                assert np.array_equal(codes[:, :n], np.repeat(forced[:, :n], 2, 0)), k  # forcing took effect
                lgs.append(lg.copy())
            eng._exit()
            assert eng.decode_mode() == 0  # the launch path: the persistent engine is the full-size width's
        finally:
            eng.set_forced(None)
        trace[dt] = lgs
    worst = 0.0
    for k in range(steps + 1):
        assert np.isfinite(trace["bf16"][k]).all(), k
        assert np.array_equal(trace["bf16"][k][1], trace["bf16"][k][0]), k  # identical rows: identical logits
        e = rms_rel(trace["bf16"][k][0], trace["fp32"][k][0])
        print(f"width 576, step {k}: bf16 logits vs the fp32 control, rel RMS {e:.3e} (bound {BOUND:.0e})")
        worst = max(worst, e)
    record("engine width 576 bf16 vs fp32 control", worst, BOUND)
    assert worst < BOUND, worst


if __name__ == "__main__" and len(sys.argv) == 5 and sys.argv[1] == "child":
    child_main([tuple(c) for c in json.loads(sys.argv[2])], int(sys.argv[3]), int(sys.argv[4]))
