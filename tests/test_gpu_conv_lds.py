"""Operator-level tests of the LDS-tiled narrow convolution (csrc/conv_lds.hip) in both forms, through the C ABI: the plain form
(itts_gemm, family 4) and the form with Activation1d applied while the input tile is staged (itts_act_conv, ACT = true), in both
builds of the library (16-bit type bf16 / IEEE half).  Operands are rounded to the build's 16-bit torch dtype; inputs come from
itts_hip.prng.

Reference: fp64 torch on the CPU from the same rounded inputs - oracle.vocoder.activation1d on doubles (replicate pad 5/5, 2 x
transposed conv, crop, SnakeBeta, replicate pad 5/6, stride-2 conv), the zero-padded dilated conv1d, the GemmArgs epilogue in its
documented order (bias, act, scale / shift, act2, + R, * alpha, + beta * ADD): `exact`.  `floor` is the same with the activation
rounded to the 16-bit type before the convolution and the result rounded to it - what a perfect kernel of this design produces.
The plain form has the same two without the activation.

Bounds, all computed here from the references:
  per element  |got - exact| <= ulp * |alpha| * S + (ulp / 2) * |exact| + 1e-6, S the fp64 convolution of |activation| with |w|,
               ulp = 2^-7 (bf16) / 2^-10 (f16), the largest relative spacing: an activated value landing on the neighbouring 16-bit
               value, and the output rounding; fp32 accumulation is three orders below both.  The general epilogue (relu, scale /
               shift, tanh) keeps the bound: relu and tanh are 1-Lipschitz and the scales here lie in (0.5, 1).
  RMS ratio    rms(got - exact) <= 1.25 * rms(floor - exact) over the whole output, per batch item, and over the edge band of each
               item (the first and last 16 + pad_left time steps).  An fp32 model of the kernel gives 1.000; the mildest wrong
               kernels (one channel with its neighbour's alpha, zero instead of replicate padding) give 1.55 over the whole output
               and 3.2 in the band (tests/test_act_conv_api.py runs that model, right and wrong, on the CPU).
The measured maxima are printed and, where ITTS_TEST_OUT names a directory, written to conv_lds_ops.txt there (committed as
profiles/conv_lds_ops.txt).

Bit-exact properties of the ACT form: itts_act_conv = itts_snake_aa_fwd (layout 1) into a scratch tensor, then itts_gemm on it; two
runs agree; the in-place accumulate ADD == C (as model_vocoder.hip issues it) = a separate ADD buffer; item b of a B-item call =
that item alone.

Every call: the selector is asked first; the output lives inside a NaN-filled buffer (T guard rows before and after, pad columns
where ldc > N) whose guard bits have to survive, everything stored has to be finite; A has NaN rows before its first and after its
last item (a read that escapes the clamp shows), R / ADD have NaN pad columns, W a NaN row behind its last; after the launch the
stream is synchronised and a device error ends the session.

log_alpha, log_beta ~ uniform with std 0.4 as in test_snake_vs_oracle, one extra run of the C = 96 case draws both from
[-1.5, 1.5].  Nobody has taken the range from a real checkpoint."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from itts_hip import lib as L
from itts_hip import pack, prng
from oracle import vocoder as ovoc

DEV = "cuda:0"
HALF = {"bf16": (torch.bfloat16, 2.0 ** -7), "f16": (torch.float16, 2.0 ** -10)}
RMS_LIMIT = 1.25
AGUARD = 72  # NaN rows around A: more than the 64-row halo plus the 6 rows of the FIR windows

# (B, T, Cin, N, k, dil[, where the halo goes]) - the smallest shapes that reach each path (T >= 256 is the gate)
CASES = (
    (2, 256, 24, 24, 3, 1),      # BM = 256: one tile per item, both sequence ends in one tile
    (1, 257, 24, 24, 11, 5),     # one live row in the last tile, its 50-row halo almost all zero padding
    (2, 383, 48, 48, 7, 3),      # ACT BM = 128 (plain 256): last tile 127 rows, item boundary
    (1, 320, 96, 96, 11, 5),     # BM = 128, half-filled last tile (an odd frame count), two runs per channel, 64 idle threads
    (3, 300, 96, 96, 3, 1),      # three items
    (1, 256, 16, 40, 3, 5),      # Cin under one plane (two slots cleared), N != Cin, NP = 48 with 8 dead columns
    (1, 513, 88, 96, 11, 1),     # three planes, the last with 24 of 32 channels
    (2, 320, 40, 24, 7, 5),      # two planes, the last with 8 of 32; N = 24
    (1, 260, 96, 8, 3, 1),       # N = 8, the narrowest output
    (1, 300, 32, 32, 5, 16),     # halo exactly 64 (dilation 17 is refused: tests/test_act_conv_api.py)
    (1, 300, 48, 48, 7, 3, "right"),  # pad_left = 0: the whole halo to the right
    (1, 300, 48, 48, 7, 3, "left"),   # pad_left = (k - 1) * dil: the whole halo to the left
)
EXTRA = (0, 3, 5)   # the cases that also run the other epilogue variants
LDA = (0, 5)        # ... and, plain form only, lda = Cin + 8
WIDE = 3            # ... and the wide alpha / beta run


def case_id(case):
    return "x".join(str(v) for v in case)


def pad_left_of(case):
    k, dil = case[4], case[5]
    side = case[6] if len(case) > 6 else None
    return 0 if side == "right" else (k - 1) * dil if side == "left" else (k - 1) * dil // 2


def variants_of(case, fused=True):
    i = CASES.index(case)
    v = ["amp"] + (["none", "general", "bias4", "ld"] if i in EXTRA else [])
    return v + (["lda"] if not fused and i in LDA else [])


def leading_dims(case, variant):
    Cin, N = case[2], case[3]
    if variant == "ld":
        return dict(lda=Cin, ldc=N + 8, ldr=N + 8, ldadd=N + 16)
    return dict(lda=Cin + 8 if variant == "lda" else Cin, ldc=N, ldr=N, ldadd=N)


def rnd(name, shape, std=1.0):
    return torch.from_numpy(prng.tensor(name, 5, shape, std=std))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    """Wait for the launch; a device fault ends the session there (nothing more is started on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


def ok(lib, status, what):
    """A refused call fails the test; a HIP error ends the session like a fault seen at the synchronisation."""
    if status == -2:  # ITTS_E_HIP
        pytest.exit(f"HIP error in {what}, nothing more is launched: {lib.itts_last_error()}", returncode=3)
    L.check(status, what, lib)


# ---- inputs and references (CPU) -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case, half, wide=False):
    """Everything a call of this case may read, channels-first ([B, C, T]) as torch's conv1d wants it, rounded to the 16-bit type."""
    B, T, Cin, N, k, _ = case[:6]
    tdt, tag = HALF[half][0], case_id(case)
    spread = 1.5 / np.sqrt(3.0) if wide else 0.4  # prng draws uniformly: std s = [-s sqrt(3), s sqrt(3)]
    p = dict(x=rnd(f"cl.x{tag}", (B, Cin, T), 1.5).to(tdt), w=rnd(f"cl.w{tag}", (N, Cin, k), 1.0 / np.sqrt(Cin * k)).to(tdt),
             la=rnd(f"cl.a{tag}", (Cin,), spread), lb=rnd(f"cl.be{tag}", (Cin,), spread), bias=rnd(f"cl.b{tag}", (B, N), 0.1),
             res=rnd(f"cl.r{tag}", (B, N, T)).to(tdt), run=rnd(f"cl.s{tag}", (B, N, T)).to(tdt),
             scale=0.75 + rnd(f"cl.sc{tag}", (N,), 0.1), shift=rnd(f"cl.sh{tag}", (N,), 0.1), filt=ovoc.kaiser_sinc_filter12())
    p["act64"] = ovoc.activation1d(p["x"].double(), p["la"].double(), p["lb"].double(), p["filt"].double())
    return p


def conv(a, w, case):
    k, dil = case[4], case[5]
    pl = pad_left_of(case)
    return F.conv1d(F.pad(a, (pl, (k - 1) * dil - pl)), w, None, dilation=dil)


def epilogue_terms(variant):
    """bias, general branch, R, alpha, beta (0 = no ADD) of a variant"""
    if variant == "none":
        return False, False, False, 1.0, 0.0
    return True, variant == "general", True, 1.0 / 3.0, 1.0


def epilogue(v, p, variant):
    """GemmArgs' epilogue on v [B, N, T] in v's own precision"""
    has_bias, general, has_r, alpha, beta = epilogue_terms(variant)
    cast = lambda t: t.to(v.dtype)  # noqa: E731
    if has_bias:
        v = v + cast(p["bias"])[:, :, None]
    if general:
        v = torch.tanh(torch.relu(v) * cast(p["scale"])[None, :, None] + cast(p["shift"])[None, :, None])
    if has_r:
        v = v + cast(p["res"])
    v = v * torch.tensor(alpha, dtype=torch.float32).to(v.dtype)  # (the kernel's alpha is an fp32 number)
    if beta:
        v = v + beta * cast(p["run"])
    return v


@functools.lru_cache(maxsize=None)
def fixture(case, variant, half, fused, wide=False):
    """inputs, `exact`, `floor` and the per-element bound of one (case, variant, build, form); never modified"""
    tdt, ulp = HALF[half]
    p = inputs(case, half, wide)
    a64 = p["act64"] if fused else p["x"].double()
    w64 = p["w"].double()
    alpha = float(torch.tensor(epilogue_terms(variant)[3], dtype=torch.float32))
    exact = epilogue(conv(a64, w64, case), p, variant)
    floor = epilogue(conv(a64.to(tdt).double(), w64, case), p, variant).to(tdt).double()
    S = conv(a64.abs(), w64.abs(), case)
    return dict(case=case, variant=variant, half=half, fused=fused, p=p, exact=exact, floor=floor,
                bound=ulp * abs(alpha) * S + 0.5 * ulp * exact.abs() + 1e-6)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def judge(fx, got):
    """got [B, N, T] against the two bounds -> the largest per-element error over its bound, the largest RMS ratio of each kind"""
    exact, floor = fx["exact"], fx["floor"]
    got = got.double()
    err = (got - exact).abs() / fx["bound"]
    elem = float("inf") if not bool(torch.isfinite(got).all()) else float(err.max())
    band = 16 + pad_left_of(fx["case"])
    e, f = got - exact, floor - exact
    ratio = lambda a, b: float("inf") if not np.isfinite(rms(a)) else rms(a) / rms(b)  # noqa: E731
    items = [ratio(e[b], f[b]) for b in range(e.shape[0])]
    bands = [ratio(torch.cat([e[b, :, :band], e[b, :, -band:]], 1), torch.cat([f[b, :, :band], f[b, :, -band:]], 1))
             for b in range(e.shape[0])]
    out = dict(elem=elem, whole=ratio(e, f), item=max(items), band=max(bands))
    out["rms"] = max(out["whole"], out["item"], out["band"])
    return out


def model_fp32(fx, plant=None):
    """The fused kernel's arithmetic on the CPU: Activation1d in fp32, rounded to the 16-bit type, fp32 products and sums, the epilogue
    in fp32, one rounding of the output.  plant: an error of the kind a wrong kernel would make."""
    case, p, tdt = fx["case"], fx["p"], HALF[fx["half"]][0]
    x, la, lb, filt = p["x"].float(), p["la"].clone(), p["lb"], p["filt"]
    Cin = x.shape[1]
    if plant == "neighbour_alpha":
        la[Cin // 2] = la[Cin // 2 + 1]
    fw = filt.view(1, 1, 12).expand(Cin, -1, -1)
    pad = dict(mode="constant") if plant == "zero_pad" else dict(mode="replicate")
    u = 2 * F.conv_transpose1d(F.pad(x, (5, 5), **pad), fw, stride=2, groups=Cin)[..., 15:-15]
    u = F.pad(ovoc.snakebeta(u, la, lb), (5, 6), **pad)
    a = F.conv1d(u, fw, stride=2, groups=Cin).to(tdt).float()
    w = p["w"].float()
    if plant == "halo_shift":
        a = torch.roll(a, 1, dims=2)
    if plant == "pad_channel":  # the channels behind Cin of the last 32-channel plane left as they were: weights of zero times a NaN
        fill = -Cin % 32 or 32
        a = torch.cat([a, torch.full((a.shape[0], fill, a.shape[2]), float("nan"))], 1)
        w = torch.cat([w, torch.zeros(w.shape[0], fill, w.shape[2])], 1)
    return epilogue(conv(a, w, case), p, fx["variant"]).to(tdt)


# ---- one call -----------------------------------------------------------------------------------------------------------------
def channels_last(t, ld, dtype, before=0, after=0):
    """[B, C, T] -> the [before + B * T + after, ld] device buffer: NaN guard rows, NaN pad columns"""
    B, Cc, T = t.shape
    buf = torch.full((before + B * T + after, ld), float("nan"), dtype=dtype)
    buf[before:before + B * T, :Cc] = t.transpose(1, 2).reshape(B * T, Cc).to(dtype)
    return buf.to(DEV)


def call(lib, fx, how="entry", item=None, inplace=False):
    """One launch of the case -> the stored output [B, N, T] on the CPU (16-bit).  how: "entry" = itts_act_conv for the fused form and
    itts_gemm for the plain one; "two" = itts_snake_aa_fwd into a scratch tensor, then itts_gemm.  item: that batch item alone."""
    case, variant, p = fx["case"], fx["variant"], fx["p"]
    T, Cin, N, k, dil = case[1:6]
    tdt = HALF[fx["half"]][0]
    sel = slice(None) if item is None else slice(item, item + 1)
    x, bias, res, run = p["x"][sel], p["bias"][sel], p["res"][sel], p["run"][sel]
    B = x.shape[0]
    has_bias, general, has_r, alpha, beta = epilogue_terms(variant)
    ld = leading_dims(case, variant)
    if inplace:
        ld["ldadd"] = ld["ldc"]
    es = 2
    keep = dict(A=channels_last(x, ld["lda"], tdt, AGUARD, AGUARD),
                W=torch.cat([torch.from_numpy(pack.conv_w(p["w"].float().numpy())).to(tdt),
                             torch.full((1, k * Cin), float("nan"), dtype=tdt)]).to(DEV),
                C=torch.full((T + B * T + T, ld["ldc"]), float("nan"), dtype=tdt))
    if inplace:  # the running sum is in the output buffer already
        keep["C"][T:T + B * T, :N] = run.transpose(1, 2).reshape(B * T, N)
    keep["C"] = keep["C"].to(DEV)
    before = keep["C"].cpu().view(torch.int16).clone()
    g = L.GemmArgs()
    g.A, g.W, g.C = keep["A"].data_ptr() + AGUARD * ld["lda"] * es, keep["W"].data_ptr(), keep["C"].data_ptr() + T * ld["ldc"] * es
    g.M, g.N, g.Cin, g.taps, g.T, g.dil, g.pad_left, g.pad_mode, g.in_up, g.nphase = B * T, N, Cin, k, T, dil, pad_left_of(case), 0, 1, 1
    g.lda, g.ldc, g.alpha, g.beta = ld["lda"], ld["ldc"], alpha, beta
    g.dtype_a = g.dtype_w = g.dtype_c = L.BF16
    if has_bias:
        off = 1 if variant == "bias4" else 0  # 4 bytes past a 16-byte boundary: the general branch with the plain arithmetic
        keep["bias"] = torch.cat([torch.full((off,), float("nan")), bias.reshape(-1), torch.full((1,), float("nan"))]).to(DEV)
        g.bias, g.bias_bstride = keep["bias"].data_ptr() + 4 * off, N
    if general:
        keep["scale"], keep["shift"] = p["scale"].to(DEV), p["shift"].to(DEV)
        g.act, g.scale, g.shift, g.act2 = L.ACT_RELU, keep["scale"].data_ptr(), keep["shift"].data_ptr(), L.ACT_TANH
    if has_r:
        keep["R"] = channels_last(res, ld["ldr"], tdt)
        g.R, g.ldr = keep["R"].data_ptr(), ld["ldr"]
    if beta:
        if not inplace:
            keep["ADD"] = channels_last(run, ld["ldadd"], tdt)
        g.ADD, g.ldadd = (g.C if inplace else keep["ADD"].data_ptr()), ld["ldadd"]
    assert lib.itts_gemm_which(C.byref(g)) == 4, (case, variant)
    if fx["fused"]:
        assert lib.itts_act_conv_supported(C.byref(g)) == 1, (case, variant)
        for name in ("la", "lb", "filt"):
            keep[name] = p[name].to(DEV)
        if how == "two":
            keep["act"] = torch.full_like(keep["A"], float("nan"))
            act_ptr = keep["act"].data_ptr() + AGUARD * ld["lda"] * es
            ok(lib, lib.itts_snake_aa_fwd(act_ptr, g.A, keep["filt"].data_ptr(), keep["filt"].data_ptr(), keep["la"].data_ptr(),
                                          keep["lb"].data_ptr(), B, Cin, T, L.BF16, 1, stream()), "snake_aa_fwd")
            sync()
            g.A = act_ptr
            ok(lib, lib.itts_gemm(C.byref(g), stream()), "gemm")
        else:
            ok(lib, lib.itts_act_conv(C.byref(g), keep["la"].data_ptr(), keep["lb"].data_ptr(), keep["filt"].data_ptr(), stream()), "act_conv")
    else:
        if variant == "lda":
            assert lib.itts_act_conv_supported(C.byref(g)) == 0  # the fused form stages dense rows only
        ok(lib, lib.itts_gemm(C.byref(g), stream()), "gemm")
    sync()
    after = keep["C"].cpu()
    stored = torch.zeros(after.shape, dtype=torch.bool)
    stored[T:T + B * T, :N] = True
    assert torch.equal(after.view(torch.int16)[~stored], before[~stored]), (case, variant, "guard rows or pad columns were written")
    out = after[T:T + B * T, :N]
    assert bool(torch.isfinite(out.float()).all()), (case, variant, "non-finite output")
    return out.reshape(B, T, N).transpose(1, 2).contiguous()


MEASURED = {}  # table line -> the four figures


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [f"{k:<52s} elem/bound {r['elem']:6.3f}   rms ratio whole {r['whole']:6.4f}  item {r['item']:6.4f}  band {r['band']:6.4f}"
             for k, r in sorted(MEASURED.items())]
    for half in HALF:
        for form in ("act", "plain"):
            sub = [r for k, r in MEASURED.items() if k.startswith(f"{half} {form} ")]
            if sub:
                lines.append(f"{half} {form} largest: elem/bound {max(r['elem'] for r in sub):.3f} (limit 1), rms ratio "
                             f"{max(r['rms'] for r in sub):.4f} (limit {RMS_LIMIT})")
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "conv_lds_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def check_numbers(fx, got, tag=""):
    rep = judge(fx, got)
    line = f"{fx['half']} {'act' if fx['fused'] else 'plain'} {case_id(fx['case'])} {fx['variant']}{tag}"
    MEASURED[line] = rep
    print(line, rep)
    assert rep["elem"] <= 1.0, (line, rep)
    assert rep["whole"] <= RMS_LIMIT and rep["item"] <= RMS_LIMIT and rep["band"] <= RMS_LIMIT, (line, rep)


# ---- the tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("form", ("act", "plain"))
@pytest.mark.parametrize("half", tuple(HALF))
def test_conv_lds_vs_fp64(half, form, case):
    """Both bounds for every epilogue variant of the case; the misaligned-bias run has the bits of the aligned one."""
    lib, fused = L.load(half), form == "act"
    got = {}
    for variant in variants_of(case, fused):
        fx = fixture(case, variant, half, fused)
        got[variant] = call(lib, fx)
        check_numbers(fx, got[variant])
    if "bias4" in got:
        assert torch.equal(got["bias4"].view(torch.int16), got["amp"].view(torch.int16))
    if "ld" in got:  # the leading dimensions move the operands, not the numbers
        assert torch.equal(got["ld"].view(torch.int16), got["amp"].view(torch.int16))
    if "lda" in got:
        assert torch.equal(got["lda"].view(torch.int16), got["amp"].view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("half", tuple(HALF))
def test_conv_lds_act_wide_alpha_beta(half):
    """log_alpha, log_beta drawn from [-1.5, 1.5]: sines up to 4.5 radians per unit input, gains up to 4.5 on sin^2."""
    fx = fixture(CASES[WIDE], "amp", half, True, True)
    check_numbers(fx, call(L.load(half), fx), " wide")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("half", tuple(HALF))
def test_conv_lds_act_bit_exact_properties(half, case):
    lib = L.load(half)
    fx = fixture(case, "amp", half, True)
    bits = lambda t: t.view(torch.int16)  # noqa: E731
    one = call(lib, fx)
    assert torch.equal(bits(one), bits(call(lib, fx))), "two runs differ"
    assert torch.equal(bits(one), bits(call(lib, fx, how="two"))), "fused != itts_snake_aa_fwd then itts_gemm"
    assert torch.equal(bits(one), bits(call(lib, fx, inplace=True))), "ADD == C differs from a separate ADD buffer"
    for b in range(case[0] if case[0] > 1 else 0):
        assert torch.equal(bits(one[b:b + 1]), bits(call(lib, fx, item=b))), f"item {b} alone differs"
