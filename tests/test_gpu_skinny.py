"""Operator-level tests of the batched decode projections (csrc/decode_mfma.hip) through the C ABI: skinny_mfma_kernel in every
instantiation the launcher can pick (itts_skinny_gemm for bf16 weights, itts_skinny_gemm_fp8 for e4m3 weights with a row scale),
ln_rows_bf16_kernel<5> and <8> (itts_ln_rows_bf16) and the two weight retilers.  Conventions of tests/test_gpu_decode_gemv.py.

Every reference is fp64 torch on the CPU from the SAME rounded inputs, computed once per case and cached:

  bf16 X       x.double() @ w.double().T (+ bias), then gelu_new, then + y0
  prologue     LayerNorm(x, eps 1e-5, no affine) in fp64, rounded to bf16, then as above
  fp8          w = the decoded e4m3 values times the power-of-two row scale (quantize_rows_e4m3: pack.quantize_gpt_fp8's construction)
  split K      h0 + x . W^T + bias for the residual stream, its fp64 LayerNorm for the bf16 output of itts_ln_rows_bf16

Bounds (relerr of tests/test_gpu_ops.py, the project's own for the same constructions): 2e-5 fp32 output from bf16 X; 2e-3 fp32 output
behind a bf16-rounded LayerNorm; 1e-2 bf16 output; 6e-3 the output of ln_rows_bf16; 2e-5 the residual stream after absorbing partials.
A GELU case is judged over its three widths together (one output of gelu(..) has no scale of its own: test_gpu_decode_gemv.py).

Every call: itts_skinny_gemm_supported is asked first; row-major X has a NaN row past B, tiled X NaN in the padded rows of the last
tile; row-major W / W8 one poisoned row past N (NaN, byte 0x7F); bias and wscale a NaN past N; partial is NaN everywhere; Y holds NaN
where the call stores (y0 when accumulating) and a sentinel in the row past B (tiled Y: in the padded rows and past the last tile)
that has to survive; no NaN may come out.  The weights' rows carry gains 1/2, 1, 2 in turn, so that neighbouring rows have
different fp8 scales.

Bit-exact properties: a row alone (B = 1, row-major) = that row inside the batch (non-accumulating forms); row-major W = tiled W;
two runs agree; half tiles = whole tiles; tiled = row-major output of ln_rows_bf16; and the fp8 kernel on (W8, wscale) = the bf16
kernel on W = the dequantised weights (exactly representable in bf16, scale a power of two) - the largest ulp distance seen is
recorded.  The measured maxima are printed and, where ITTS_TEST_OUT names a directory, written to skinny_ops.txt there (committed
as profiles/skinny_ops.txt).  tests/test_skinny_api.py holds the case tables below against the launcher's rule on the host."""
import ctypes as C
import functools
import os

import pytest
import torch

from itts_hip import lib as L
from itts_hip import prng

DEV = "cuda:0"
SENT = 768.0  # exact in bf16
NAN = float("nan")
FORMS = ("bf16", "bf16t", "fp8", "fp8t")  # weights: bf16 row-major / fragment-tiled, e4m3 row-major / with the tiled copy
NS_FREE = (8, 40, 66)    # less than a tile (one half-tile workgroup of the pair is empty) | N % 16 = 8 | ragged last tile
NS_TILED = (32, 64, 96)  # bf16 Y in fragment tiles: N % 32 == 0
BOUND_F32, BOUND_LN_F32, BOUND_BF16, BOUND_LNROWS, BOUND_RESID = 2e-5, 2e-3, 1e-2, 6e-3, 2e-5


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


def quantize_rows_e4m3(w):
    """pack.quantize_gpt_fp8's construction for one matrix: e4m3 bytes and one power-of-two scale per output row."""
    w = w.float()
    amax = w.abs().amax(dim=1).clamp_min(1e-30)
    scale = torch.pow(2.0, torch.ceil(torch.log2(amax / 448.0)))
    q = (w / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.float(), q.float() * scale[:, None]


def ulps(a, b):
    """largest distance of two fp32 / bf16 tensors in units of the last place (0 = the same bits, +0 = -0 aside)"""
    if a.dtype == torch.bfloat16:
        ia, ib = a.view(torch.int16).int(), b.view(torch.int16).int()
        ia, ib = torch.where(ia < 0, -(ia & 0x7FFF), ia), torch.where(ib < 0, -(ib & 0x7FFF), ib)
    else:
        ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
        ia, ib = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia), torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max())


# ---- the fragment-tile layouts (csrc/itts_decode.h tile_off, wtile_off) ---------------------------------------------------------
def to_tiles(x, BT, fill=NAN):
    """row-major [B, K] -> tile_off order, BT tiles of 16 rows; the padded rows hold `fill`"""
    B, K = x.shape
    xp = torch.full((BT * 16, K), fill, dtype=x.dtype)
    xp[:B] = x
    return xp.view(BT, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)


def from_tiles(t, rows, K):
    """tile_off order -> row-major [rows, K] (rows = 16 BT gives the padded rows too)"""
    BT = (rows + 15) // 16
    return t.view(K // 32, BT, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(BT * 16, K)[:rows]


def w_tiles(w):
    """W [N, K] -> wtile_off order, rows past N zero"""
    N, K = w.shape
    wp = torch.zeros((N + 15) // 16 * 16, K, dtype=w.dtype)
    wp[:N] = w
    return wp.view(-1, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def nan_row(t, fill=NAN):
    """[N, ...] -> [N + 1, ...] on the device with `fill` behind the last row"""
    pad = torch.full((1,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    return torch.cat([t, pad]).contiguous().to(DEV)


# ---- inputs (CPU, cached) ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(N, K):
    """One matrix in both number formats: w bf16 [N, K]; w8 / wscale / deq its e4m3 quantisation (deq as bf16: exact); bias."""
    base = rnd(f"sk.w{N}x{K}", (N, K)) * 0.05 * torch.pow(2.0, (torch.arange(N) % 3 - 1).float())[:, None]
    w8, wscale, deq = quantize_rows_e4m3(base)
    return {"w": base.to(torch.bfloat16), "w8": w8, "wscale": wscale, "deq": deq.to(torch.bfloat16), "bias": rnd(f"sk.b{N}", (N,))}


@functools.lru_cache(maxsize=None)
def x_bf16(K):
    return (rnd(f"sk.x{K}", (128, K)) * 1.5).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def x_f32(K, offset=0.3):
    return rnd(f"sk.h{K}", (16, K)) * 2.5 + offset


@functools.lru_cache(maxsize=None)
def y0_of(N):
    return rnd(f"sk.y{N}", (128, N))


def w_ref(N, K, fam):
    return (weights(N, K)["deq"] if fam == "fp8" else weights(N, K)["w"]).double()


@functools.lru_cache(maxsize=None)
def ref_plain(K, N, fam, bias, gelu, acc):
    """fp64 reference for the 128 pool rows (every row is independent of the others)"""
    ref = x_bf16(K).double() @ w_ref(N, K, fam).T
    if bias:
        ref = ref + weights(N, K)["bias"].double()
    if gelu:
        ref = gelu_new(ref)
    return ref + y0_of(N).double() if acc else ref


@functools.lru_cache(maxsize=None)
def ref_prologue(K, N, fam, bias, gelu, offset):
    xn = torch.nn.functional.layer_norm(x_f32(K, offset).double(), (K,), None, None, 1e-5).to(torch.bfloat16)
    ref = xn.double() @ w_ref(N, K, fam).T
    if bias:
        ref = ref + weights(N, K)["bias"].double()
    return gelu_new(ref) if gelu else ref


# ---- device copies of the weights, made once; the tiled ones by the library's retilers ------------------------------------------
_DEVW = {}


def dev_weights(lib, N, K):
    if (N, K) not in _DEVW:
        w = weights(N, K)
        d = {"w": nan_row(w["w"]), "deq": nan_row(w["deq"]), "w8": nan_row(w["w8"], 0x7F), "wscale": nan_row(w["wscale"]),
             "bias": nan_row(w["bias"])}
        npad = (N + 15) // 16 * 16
        for k in ("w", "deq"):
            d[k + "t"] = torch.full((npad * K,), NAN, dtype=torch.bfloat16, device=DEV)
            L.check(lib.itts_retile_weights(d[k + "t"].data_ptr(), d[k].data_ptr(), N, K, stream()), "retile_weights")
        d["w8t"] = torch.full((npad * K,), 0x7F, dtype=torch.uint8, device=DEV)
        L.check(lib.itts_retile_weights_fp8(d["w8t"].data_ptr(), d["w8"].data_ptr(), N, K, stream()), "retile_weights_fp8")
        sync()
        _DEVW[N, K] = d
    return _DEVW[N, K]


def layout_of(form, xt=0, yt=0, lnp=0, half=0):
    return xt | (yt << 1) | (4 if form == "bf16t" else 0) | (8 if lnp else 0) | (16 if half else 0)


# ---- one call -------------------------------------------------------------------------------------------------------------------
def skinny(lib, form, x, N, K, *, ybf=0, yt=0, xt=0, gelu=0, acc=0, bias=1, S=1, lnp=0, half=0, y0=None, wkind="w"):
    """One launch of form `form` on the rows x ([B, K] bf16, or fp32 with lnp) -> the B output rows on the CPU (S > 1: the partial
    sums [S, B, N]).  wkind "deq": the bf16 forms run on the dequantised fp8 weights.  Checks the selector, the sentinels, NaN."""
    B, fp8, BT = x.shape[0], form.startswith("fp8"), (x.shape[0] + 15) // 16
    layout, act = layout_of(form, xt, yt, lnp, half), (L.ACT_GELU_NEW if gelu else L.ACT_NONE)
    what = (form, B, N, K, layout, S)
    assert lib.itts_skinny_gemm_supported(ybf, B, N, K, act, acc, S, layout, int(fp8)) == 1, what
    d = dev_weights(lib, N, K)
    xd = to_tiles(x, BT).to(DEV) if xt else nan_row(x)
    ydt = torch.bfloat16 if ybf else torch.float32
    part = torch.full((S, B, N), NAN, device=DEV) if S > 1 else None
    y = None
    if S == 1:
        body = y0[:B].clone() if acc else torch.full((B, N), NAN, dtype=ydt)
        if ybf and yt:
            y = torch.cat([to_tiles(body, BT, SENT), torch.full((N,), SENT, dtype=ydt)]).to(DEV)
        else:
            y = nan_row(body, SENT)
    yp, pp, bp = (y.data_ptr() if y is not None else None), (part.data_ptr() if S > 1 else None), (d["bias"].data_ptr() if bias else None)
    if fp8:
        st = lib.itts_skinny_gemm_fp8(yp, ybf, xd.data_ptr(), d["w8"].data_ptr(), d["w8t"].data_ptr() if form == "fp8t" else None,
                                      d["wscale"].data_ptr(), bp, B, N, K, act, acc, S, pp, layout, stream())
    else:
        st = lib.itts_skinny_gemm(yp, ybf, xd.data_ptr(), d[wkind + ("t" if form == "bf16t" else "")].data_ptr(), bp, B, N, K, act, acc, S,
                                  pp, layout, stream())
    L.check(st, "skinny_gemm")
    sync()
    if S > 1:
        got = part.cpu()
    elif ybf and yt:
        out = y.cpu()
        full = from_tiles(out[:BT * 16 * N], BT * 16, N)
        assert bool((out[BT * 16 * N:] == SENT).all()) and bool((full[B:] == SENT).all()), (what, "padded rows / past the last tile written")
        got = full[:B].contiguous()
    else:
        out = y.cpu()
        assert bool((out[B] == SENT).all()), (what, "the row past B was written")
        got = out[:B]
    assert not bool(torch.isnan(got.float()).any()), (what, "NaN in the result")
    return got


MEASURED = {}  # table line -> (max, bound, unit)


def record(line, val, bound, unit="relerr"):
    MEASURED[line] = (max(val, MEASURED.get(line, (0, bound, unit))[0]), bound, unit)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [(f"{k:<58s} max {u} {v:9.3e}   bound {b:.0e}" if u == "relerr" else f"{k:<58s} max {u} {v:d}   expected {b:d}")
             for k, (v, b, u) in sorted(MEASURED.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "skinny_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def bt_of(B):
    t = (B + 15) // 16
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 8


def same_as_bf16_on_deq(tag, got8, got16):
    """the fp8 kernel's bits against the bf16 kernel's on the dequantised weights: the distance is recorded, then held to zero"""
    u = ulps(got8, got16)
    record(f"fp8 vs bf16 on deq, ulp distance: {tag}", u, 0, "ulp")
    assert u == 0 and torch.equal(got8, got16), (tag, u)


# ---- case tables (tests/test_skinny_api.py holds them against the launcher's rule) ----------------------------------------------
MODES = {"f32": (0, 0, 0), "acc": (0, 0, 1), "bf16": (1, 0, 0), "f32_gelu": (0, 1, 0), "bf16_gelu": (1, 1, 0)}  # y_bf16, GELU, accumulate
BS = (1, 5, 16, 17, 32, 33, 64, 65, 128)  # every row-tile template (BT = 1, 2, 4, 8) at both edges
KS = (32, 224, 288, 1312)  # k-steps: 1 (seven idle waves) | 7 (one idle wave) | 9 (wave 0 leaves its unrolled requests early) | 41 (second round)
# (B, K, weight family, X tiled, mode, bias): both weight layouts of the family run inside the case
PLAIN_CASES = [(B, KS[(b + 2 * f + xt) % 4], fam, xt, list(MODES)[(2 * b + f + 3 * xt) % 5], (b + f + xt) % 3 != 0)
               for b, B in enumerate(BS) for f, fam in enumerate(("bf16", "fp8")) for xt in (0, 1)]
# two tiles per workgroup: 301 tiles (odd: a surplus tile; N % 16 = 8); B = 128 must take one tile per workgroup (BT = 8)
NT2_CASES = [(16, 4808, 64, "bf16", 0), (16, 4808, 64, "fp8", 1), (32, 4808, 64, "bf16", 1), (32, 4808, 64, "fp8", 0), (64, 4808, 64, "bf16", 1),
             (64, 4808, 64, "fp8", 0), (128, 4808, 64, "bf16", 1), (128, 4808, 64, "fp8", 1)]
# LayerNorm prologue: (B, K, family, mode, bf16 Y tiled, bias, offset of the inputs); B = 9 is one live row in wave 4's pair, B = 5 one in
# wave 2's with waves 3 .. 7 rowless; K < 256 leaves lanes without elements (the K - 4 clamp)
LNP_KS = (32, 96, 288, 1056, 1280)
LNP_MODES = ("f32", "bf16", "f32_gelu", "bf16_gelu")
LNP_CASES = [(B, K, ("bf16", "fp8")[(b + k) % 2], LNP_MODES[(b + 2 * k) % 4], (b + k) % 3 == 0, (b + k) % 4 != 1, 0.3)
             for b, B in enumerate((1, 5, 9, 16)) for k, K in enumerate(LNP_KS)]
LNP_CASES += [(9, 1280, "bf16", "f32", 0, 1, 300.3), (5, 288, "fp8", "f32", 0, 1, 300.3)]  # a large common offset: the pivoted moments
LNP_NT2 = (9, 4808, 64)
# half tiles (tiled X): (B, K, family, mode, bias); K = 1312 enters the deep form (SU = 20) with an uneven wave load, 5152 = 161 k-steps
# runs its second round
HALF_NS = (8, 40, 72)
HALF_KS = (96, 1280, 1312, 5152)
HALF_CASES = [(B, K, ("bf16", "fp8")[(b + k) % 2], ("acc", "f32", "bf16")[(b + k // 2) % 3], (b + k) % 4 != 3)
              for b, B in enumerate((1, 11, 16)) for k, K in enumerate(HALF_KS)]
# split K absorbed by itts_ln_rows_bf16: (B, N, K, S); (160, 4) has an empty last split, (1280, 3) and (5120, 5) are the engine's
# divisions, (256, 8) the most splits ln_rows_bf16 absorbs; N = 616 at S = 8 is 39 x 8 >= 300 workgroups: two tiles each, odd count
SPLIT_CASES = [(B, (96 if K == 5120 or (b + k) % 2 else 128), K, S)
               for b, B in enumerate((9, 20, 64)) for k, (K, S) in enumerate(((160, 4), (1280, 3), (5120, 5), (256, 8)))]
SPLIT_CASES += [(20, 616, 256, 8)]
LN_DS = (32, 96, 1056, 1280, 1312, 2048)  # <5> up to 1280, <8> above; D % 256 != 0 among them
LN_ROWS = (1, 17, 37)
# (passes, affine, nsplit, partial_bias)
LN_CONFIGS = ((1, 0, 0, 0), (1, 1, 0, 0), (2, 0, 0, 0), (2, 1, 0, 0), (1, 0, 1, 1), (1, 1, 1, 0), (1, 0, 3, 0), (1, 1, 3, 1), (2, 1, 3, 1),
              (1, 0, 8, 1), (2, 0, 8, 0))
RETILE_CASES = ((8, 32), (66, 96), (4808, 64))


def planned_calls():
    """(form, y_bf16, B, N, K, GELU, accumulate, ksplit, layout) of every whole-batch launch the tables below lead to"""
    out = []
    for B, K, fam, xt, mode, _ in PLAIN_CASES:
        ybf, gelu, acc = MODES[mode]
        yt = int(bool(ybf and xt))
        out += [(form, ybf, B, N, K, gelu, acc, 1, layout_of(form, xt, yt)) for N in (NS_TILED if yt else NS_FREE) for form in (fam, fam + "t")]
    for B, N, K, fam, xt in NT2_CASES:
        out += [(form, 0, B, N, K, 0, acc, 1, layout_of(form, xt)) for form in (fam, fam + "t") for acc in (0, 1)]
    for B, K, fam, mode, yt, _, _ in LNP_CASES:
        ybf, gelu, _ = MODES[mode]
        yt = int(bool(yt and ybf))
        out += [(form, ybf, B, N, K, gelu, 0, 1, layout_of(form, 0, yt, lnp=1)) for N in (NS_TILED if yt else NS_FREE) for form in (fam, fam + "t")]
    out += [(form, 0) + LNP_NT2 + (0, 0, 1, layout_of(form, lnp=1)) for form in FORMS]
    for B, K, fam, mode, _ in HALF_CASES:
        ybf, gelu, acc = MODES[mode]
        out += [(form, ybf, B, N, K, gelu, acc, 1, layout_of(form, 1, half=h)) for N in HALF_NS for form in (fam, fam + "t") for h in (1, 0)]
    for B, N, K, S in SPLIT_CASES:
        out += [(form, 0, B, N, K, 0, 0, S, layout_of(form, int(form.endswith("t")))) for form in FORMS]
    return out


# ---- skinny_mfma_kernel<BT, NT, 5, W8, WT> --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,K,fam,xt,mode,bias", PLAIN_CASES)
def test_skinny_gemm(lib, B, K, fam, xt, mode, bias):
    ybf, gelu, acc = MODES[mode]
    yt = int(bool(ybf and xt))
    bound = BOUND_BF16 if ybf else BOUND_F32
    kw = dict(ybf=ybf, gelu=gelu, acc=acc, bias=bias)
    x, gots, refs = x_bf16(K)[:B], [], []
    for N in (NS_TILED if yt else NS_FREE):
        y0 = y0_of(N)
        got = skinny(lib, fam, x, N, K, xt=xt, yt=yt, y0=y0, **kw)
        tiled = skinny(lib, fam + "t", x, N, K, xt=xt, yt=yt, y0=y0, **kw)
        assert torch.equal(tiled, got), (N, "tiled W differs from row-major W")
        assert torch.equal(skinny(lib, fam + "t", x, N, K, xt=xt, yt=yt, y0=y0, **kw), tiled), (N, "two runs differ")
        if fam == "fp8":
            same_as_bf16_on_deq(f"BT={bt_of(B)} {mode}", got, skinny(lib, "bf16", x, N, K, xt=xt, yt=yt, y0=y0, wkind="deq", **kw))
        if not acc:  # a row alone, row-major, has the bits of that row inside the batch
            for r in sorted({B // 2, B - 1}):
                alone = skinny(lib, fam, x[r:r + 1], N, K, **kw)
                assert torch.equal(alone[0], got[r]), (N, f"row {r} alone differs from row {r} of {B}")
        gots.append(got.float())
        refs.append(ref_plain(K, N, fam, bias, gelu, acc)[:B])
    errs = [relerr(torch.cat(gots, 1), torch.cat(refs, 1))] if gelu else [relerr(g, r) for g, r in zip(gots, refs)]
    print(f"skinny {fam} B={B} K={K} xt={xt} {mode} bias={int(bias)}: relerr {max(errs):.3e} (bound {bound:.0e})")
    record(f"skinny {fam} BT={bt_of(B)} {mode}", max(errs), bound)
    assert max(errs) < bound, errs


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,K,fam,xt", NT2_CASES)
def test_skinny_gemm_two_tiles_per_workgroup(lib, B, N, K, fam, xt):
    x, y0 = x_bf16(K)[:B], y0_of(N)
    got = skinny(lib, fam, x, N, K, xt=xt)
    tiled = skinny(lib, fam + "t", x, N, K, xt=xt)
    assert torch.equal(tiled, got) and torch.equal(skinny(lib, fam, x, N, K, xt=xt), got)
    if fam == "fp8":
        same_as_bf16_on_deq(f"BT={bt_of(B)} N=4808", got, skinny(lib, "bf16t", x, N, K, xt=xt, wkind="deq"))
    assert torch.equal(skinny(lib, fam + "t", x[B - 1:B], N, K)[0], got[B - 1])
    e = relerr(got, ref_plain(K, N, fam, 1, 0, 0)[:B])
    accd = skinny(lib, fam + "t", x, N, K, xt=xt, acc=1, y0=y0)
    ea = relerr(accd, ref_plain(K, N, fam, 1, 0, 1)[:B])
    print(f"skinny {fam} B={B} N={N} K={K}: relerr {e:.3e}, accumulating {ea:.3e} (bound {BOUND_F32:.0e})")
    record(f"skinny {fam} BT={bt_of(B)} N=4808 ({'one tile' if bt_of(B) == 8 else 'two tiles'} per workgroup)", max(e, ea), BOUND_F32)
    assert max(e, ea) < BOUND_F32


# ---- skinny_mfma_kernel<1, NT, 5, W8, WT, LNP> ----------------------------------------------------------------------------------
def run_prologue(lib, B, N, K, fam, mode, yt, bias, offset):
    ybf, gelu, _ = MODES[mode]
    kw = dict(ybf=ybf, gelu=gelu, bias=bias, lnp=1)
    x = x_f32(K, offset)[:B]
    got = skinny(lib, fam, x, N, K, yt=yt, **kw)
    tiled = skinny(lib, fam + "t", x, N, K, yt=yt, **kw)
    assert torch.equal(tiled, got), (N, "tiled W differs from row-major W")
    assert torch.equal(skinny(lib, fam, x, N, K, yt=yt, **kw), got), (N, "two runs differ")
    if fam == "fp8":
        same_as_bf16_on_deq(f"prologue {mode}", got, skinny(lib, "bf16", x, N, K, yt=yt, wkind="deq", **kw))
    for r in sorted({B // 2, B - 1}):
        assert torch.equal(skinny(lib, fam + "t", x[r:r + 1], N, K, **kw)[0], got[r]), (N, f"row {r} alone differs from row {r} of {B}")
    return got.float(), ref_prologue(K, N, fam, bias, gelu, offset)[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,fam,mode,yt,bias,offset", LNP_CASES)
def test_skinny_gemm_layernorm_prologue(lib, B, K, fam, mode, yt, bias, offset):
    ybf, gelu, _ = MODES[mode]
    yt = int(bool(yt and ybf))
    bound = BOUND_BF16 if ybf else BOUND_LN_F32
    pairs = [run_prologue(lib, B, N, K, fam, mode, yt, bias, offset) for N in (NS_TILED if yt else NS_FREE)]
    errs = [relerr(torch.cat([g for g, _ in pairs], 1), torch.cat([r for _, r in pairs], 1))] if gelu else [relerr(g, r) for g, r in pairs]
    print(f"skinny prologue {fam} B={B} K={K} {mode} yt={yt} offset={offset}: relerr {max(errs):.3e} (bound {bound:.0e})")
    record(f"skinny prologue {fam} {mode}" + (" offset 300" if offset > 1 else ""), max(errs), bound)
    assert max(errs) < bound, errs


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ("bf16", "fp8"))
def test_skinny_gemm_layernorm_prologue_two_tiles(lib, fam):
    B, N, K = LNP_NT2
    got, ref = run_prologue(lib, B, N, K, fam, "f32", 0, 1, 0.3)
    e = relerr(got, ref)
    print(f"skinny prologue {fam} B={B} N={N} K={K}: relerr {e:.3e} (bound {BOUND_LN_F32:.0e})")
    record(f"skinny prologue {fam} N=4808 (two tiles per workgroup)", e, BOUND_LN_F32)
    assert e < BOUND_LN_F32


# ---- skinny_mfma_kernel<1, 1, 5 | 20, W8, WT, false, HALF> ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,K,fam,mode,bias", HALF_CASES)
def test_skinny_gemm_half_tiles(lib, B, K, fam, mode, bias):
    """8-feature workgroups on tiled X: the bits of the whole-tile form.  K = 1312 and 5152 are the deep form (SU = 20) with waves
    that hold fewer than 20 k-steps: before its k-step guard became a scalar branch that form multiplied registers it had never
    loaded (v_mfma runs under an empty EXEC mask): NaN at K = 1312, a wrong sum at K = 5152; only K / 32 a multiple of 160 was right."""
    ybf, gelu, acc = MODES[mode]
    bound = BOUND_BF16 if ybf else BOUND_F32
    kw = dict(ybf=ybf, acc=acc, bias=bias, xt=1)
    x, errs = x_bf16(K)[:B], []
    for N in HALF_NS:
        y0 = y0_of(N)
        got = skinny(lib, fam, x, N, K, half=1, y0=y0, **kw)
        assert torch.equal(skinny(lib, fam + "t", x, N, K, half=1, y0=y0, **kw), got), (N, "tiled W differs from row-major W")
        assert torch.equal(skinny(lib, fam + "t", x, N, K, half=1, y0=y0, **kw), got), (N, "two runs differ")
        assert torch.equal(skinny(lib, fam + "t", x, N, K, half=0, y0=y0, **kw), got), (N, "half tiles differ from whole tiles")
        if fam == "fp8":
            same_as_bf16_on_deq(f"half tiles {'deep ' if K // 32 > 40 else ''}{mode}", got,
                                skinny(lib, "bf16t", x, N, K, half=1, y0=y0, wkind="deq", **kw))
        if not acc:
            r = B - 1
            assert torch.equal(skinny(lib, fam, x[r:r + 1], N, K, ybf=ybf, bias=bias, half=1)[0], got[r]), (N, f"row {r} alone differs")
        errs.append(relerr(got.float(), ref_plain(K, N, fam, bias, 0, acc)[:B]))
    print(f"skinny half tiles {fam} B={B} K={K} {mode} bias={int(bias)}: relerr {max(errs):.3e} (bound {bound:.0e})")
    record(f"skinny half tiles {fam} {'SU=20' if K // 32 > 40 else 'SU=5'} {mode}", max(errs), bound)
    assert max(errs) < bound, errs


# ---- itts_ln_rows_bf16 ----------------------------------------------------------------------------------------------------------
def ln_rows(lib, x, rows, D, *, gamma=None, beta=None, passes=1, partial=None, pbias=None, tiled=0):
    """One launch on x [rows, D] fp32 (+ partial [S, rows, D]) -> (y bf16 [rows, D], x after the call), both on the CPU.  x has a
    NaN row behind it, partial NaN behind its last element, gamma / beta / partial_bias one NaN past D; y a sentinel past its rows."""
    BT, S = (rows + 15) // 16, (0 if partial is None else partial.shape[0])
    xd = nan_row(x)
    opt = {k: (None if t is None else nan_row(t)) for k, t in (("g", gamma), ("b", beta), ("pb", pbias))}
    pd = None if partial is None else torch.cat([partial.reshape(-1), torch.full((D,), NAN)]).to(DEV)
    body = torch.full((rows, D), NAN, dtype=torch.bfloat16)
    y = (torch.cat([to_tiles(body, BT, SENT), torch.full((D,), SENT, dtype=torch.bfloat16)]) if tiled else torch.cat([body, torch.full((1, D), SENT, dtype=torch.bfloat16)])).to(DEV)
    ptr = {k: (None if t is None else t.data_ptr()) for k, t in opt.items()}
    L.check(lib.itts_ln_rows_bf16(y.data_ptr(), xd.data_ptr(), ptr["g"], ptr["b"], rows, D, 1e-5, passes, None if pd is None else pd.data_ptr(), S,
                                  ptr["pb"], tiled, stream()), "ln_rows_bf16")
    sync()
    out, xo = y.cpu(), xd.cpu()
    if tiled:
        full = from_tiles(out[:BT * 16 * D], BT * 16, D)
        assert bool((out[BT * 16 * D:] == SENT).all()) and bool((full[rows:] == SENT).all()), (rows, D, "padded rows / past the last tile written")
        got = full[:rows].contiguous()
    else:
        assert bool((out[rows] == SENT).all()), (rows, D, "the row past the last was written")
        got = out[:rows]
    assert bool(torch.isnan(xo[rows]).all()) and not bool(torch.isnan(xo[:rows]).any()) and not bool(torch.isnan(got.float()).any()), (rows, D)
    return got, xo[:rows]


@functools.lru_cache(maxsize=None)
def ln_inputs(D):
    return {"x": rnd(f"lnr.x{D}", (37, D)) * 3 + 0.7, "g": rnd(f"lnr.g{D}", (D,)) * 0.2 + 1, "b": rnd(f"lnr.b{D}", (D,)) * 0.1,
            "part": rnd(f"lnr.p{D}", (8, 37, D)) * 0.5, "pb": rnd(f"lnr.pb{D}", (D,))}


def ln_ref(h, g, b, passes):
    D = h.shape[-1]
    ref = torch.nn.functional.layer_norm(h, (D,), None if g is None else g.double(), None if b is None else b.double(), 1e-5)
    return torch.nn.functional.layer_norm(ref, (D,), None, None, 1e-5) if passes == 2 else ref


@pytest.mark.gpu
@pytest.mark.parametrize("D", LN_DS)
def test_ln_rows_bf16(lib, D):
    p = ln_inputs(D)
    for rows in LN_ROWS:
        for passes, affine, nsplit, pbias in LN_CONFIGS:
            x = p["x"][:rows]
            part = p["part"][:nsplit, :rows].contiguous() if nsplit else None
            kw = dict(gamma=p["g"] if affine else None, beta=p["b"] if affine else None, passes=passes, partial=part, pbias=p["pb"] if pbias else None)
            y, xo = ln_rows(lib, x, rows, D, **kw)
            h = x.double()
            if nsplit:
                h = h + part.double().sum(0) + (p["pb"].double() if pbias else 0.0)
                ex = relerr(xo, h)
                record(f"ln_rows_bf16<{5 if D <= 1280 else 8}> residual stream", ex, BOUND_RESID)
                assert ex < BOUND_RESID, (D, rows, passes, affine, nsplit, pbias, ex)
            else:
                assert torch.equal(xo, x), (D, rows, "x was written without partial sums to absorb")
            e = relerr(y.float(), ln_ref(h, kw["gamma"], kw["beta"], passes))
            record(f"ln_rows_bf16<{5 if D <= 1280 else 8}> passes={passes} affine={affine} {'absorbing' if nsplit else 'plain'}", e, BOUND_LNROWS)
            assert e < BOUND_LNROWS, (D, rows, passes, affine, nsplit, pbias, e)
            if D % 32 == 0:
                yt, xt = ln_rows(lib, x, rows, D, tiled=1, **kw)
                assert torch.equal(yt, y) and torch.equal(xt, xo), (D, rows, passes, affine, nsplit, "tiled output differs from row-major")
    print(f"ln_rows_bf16 D={D}: " + ", ".join(f"{k.split('> ')[1]} {v:.2e}" for k, (v, _, _) in sorted(MEASURED.items())
                                              if k.startswith(f"ln_rows_bf16<{5 if D <= 1280 else 8}>")))


# ---- split K: skinny_mfma_kernel with gridDim.y > 1, absorbed by ln_rows_bf16 ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,N,K,S", SPLIT_CASES)
def test_skinny_splitk_absorbed_by_layernorm(lib, B, N, K, S):
    x = x_bf16(K)[:B]
    h0 = y0_of(N)[:B] * 2
    parts = {}
    for fam in ("bf16", "fp8"):
        bias = weights(N, K)["bias"]
        h_ref = h0.double() + x.double() @ w_ref(N, K, fam).T + bias.double()
        y_ref = ln_ref(h_ref, None, None, 1)
        for form, xt in ((fam, 0), (fam + "t", 1)):  # layout 0, and tiled X with tiled W as the engine runs it
            part = skinny(lib, form, x, N, K, xt=xt, S=S, bias=1)
            assert torch.equal(skinny(lib, form, x, N, K, xt=xt, S=S, bias=1), part), (form, "two runs differ")
            if (K // 32 + S - 1) // S * (S - 1) >= K // 32:  # the last split has no k-step: exact zeros, not the buffer's NaN
                assert bool((part[S - 1] == 0).all()), (form, "an empty split has to write zeros")
            parts[form] = part
            y, h = ln_rows(lib, h0, B, N, partial=part, pbias=bias, tiled=int(N % 32 == 0 and xt))
            y2, h2 = ln_rows(lib, h0, B, N, partial=part, pbias=bias, tiled=int(N % 32 == 0 and xt))
            assert torch.equal(y2, y) and torch.equal(h2, h)
            eh, ey = relerr(h, h_ref), relerr(y.float(), y_ref)
            print(f"split K {form} B={B} N={N} K={K} S={S}: residual stream {eh:.3e} (bound {BOUND_RESID:.0e}), LayerNorm {ey:.3e} (bound {BOUND_LNROWS:.0e})")
            record(f"split K {fam} S={S} residual stream", eh, BOUND_RESID)
            record(f"split K {fam} S={S} LayerNorm output", ey, BOUND_LNROWS)
            assert eh < BOUND_RESID and ey < BOUND_LNROWS, (form, eh, ey)
        assert torch.equal(parts[fam], parts[fam + "t"]), (fam, "tiled X / W differ from row-major")
    same_as_bf16_on_deq(f"split K S={S}", parts["fp8t"], skinny(lib, "bf16t", x, N, K, xt=1, S=S, bias=1, wkind="deq"))
    if S == 4:
        assert K == 160  # the case with the empty split ran the zero check above
    # the residual rows do not depend on the batch either: one row alone gives the same partial sums
    assert torch.equal(skinny(lib, "bf16", x[B - 1:B], N, K, S=S)[:, 0], parts["bf16"][:, B - 1])


# ---- the retilers ---------------------------------------------------------------------------------------------------------------
def wtile_off(n, k, K):  # csrc/itts_decode.h
    return ((n >> 4) * (K >> 5) + (k >> 5)) * 512 + ((((k & 31) >> 3) << 4) + (n & 15)) * 8 + (k & 7)


def tile_off(b, k, BT):  # csrc/itts_decode.h
    return ((k >> 5) * BT + (b >> 4)) * 512 + ((((k & 31) >> 3) << 4) + (b & 15)) * 8 + (k & 7)


def retiled_by_formula(w):
    """wtile_off element by element (as index arithmetic on whole arrays); rows past N zero"""
    N, K = w.shape
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    out = torch.zeros((N + 15) // 16 * 16 * K, dtype=w.dtype)
    out[wtile_off(n, k, K).reshape(-1)] = w.reshape(-1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", RETILE_CASES)
def test_retilers_follow_wtile_off(lib, N, K):
    d, w = dev_weights(lib, N, K), weights(N, K)  # made from sources with a poisoned row past N, into poisoned destinations
    assert torch.equal(d["wt"].cpu().view(torch.int16), retiled_by_formula(w["w"].view(torch.int16)))
    assert torch.equal(d["deqt"].cpu().view(torch.int16), retiled_by_formula(w["deq"].view(torch.int16)))
    assert torch.equal(d["w8t"].cpu(), retiled_by_formula(w["w8"]))
    npad = (N + 15) // 16 * 16
    if npad > N:  # rows past N: zero bytes
        rows = from_w_tiles(d["w8t"].cpu(), npad, K)[N:]
        assert bool((rows == 0).all()) and bool((from_w_tiles(d["wt"].cpu().view(torch.int16), npad, K)[N:] == 0).all())


def from_w_tiles(t, npad, K):
    return t.view(npad // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(npad, K)
