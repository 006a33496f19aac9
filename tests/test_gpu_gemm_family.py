"""Operator-level tests of the shift-GEMM family, one kernel at a time, through itts_gemm_family (include/itts_hip.h): the vector-ALU
kernel (family 0), gemm_mfma under each of its instantiations (family 1), gemm_glds (2) and gemm_p8 in both geometries, with the
scalar branch of its epilogue and with an explicit K split (3) - at the smallest shapes that reach each path, far below the tile
counts at which the selector sends a shape to them.  Both builds of the library (16-bit type bf16 / IEEE half); operands are rounded
to the build's 16-bit torch dtype, inputs come from itts_hip.prng.

Reference: fp64 torch on the CPU from the same rounded operands - conv1d with explicit zero or reflect padding (even k: the extra
row goes to the right), conv_transpose1d, the nearest-upsampled conv - then the GemmArgs epilogue in its documented order (bias,
act, scale / shift, act2, + R, * alpha, + beta * ADD): `exact`.  `floor` (16-bit output) is `exact` rounded to the 16-bit type.

Bounds, all computed here from the reference, never from a kernel:
  per element  |got - exact| <= (K + 8) * 2^-24 * Sigma + h * |exact| + 1e-6, K = taps * Cin,
               Sigma = |alpha| * (S + |bias| + |R|) + |beta * ADD| with S the fp64 convolution of |A| with |W| (the worst case of fp32
               accumulation in any order), h = 2^-8 (bf16) / 2^-11 (f16) / 2^-23 (fp32 output): the rounding of the output.
               relu and tanh are 1-Lipschitz and the scales lie in (0.5, 1), so the chain keeps the bound.  NewGELU and SiLU: the
               device uses x / (1 + __expf(-2u)) (act_apply_fast, p8_finish8) and x / (1 + __expf(-x)) (act_apply); those formulas
               are evaluated in fp32 numpy over the case's pre-activations against fp64 and 4 x the largest error (times |alpha|)
               is allowed on top - __expf is not numpy's exp.
  RMS ratio    16-bit output: rms(got - exact) <= 1.25 * rms(floor - exact) over the whole output, per batch item and over the
               edge band of each item (the first and last pad + 16 rows).
tests/test_gemm_family_api.py runs an fp32 model of the operation (model_fp32 below), right and wrong, against both on the CPU.
The measured maxima are printed and, where ITTS_TEST_OUT names a directory, written to gemm_family_ops.txt there (committed as
profiles/gemm_family_ops.txt).

Bit-exact relations: two runs agree; item b of a B-item call = that item alone under the same family and variant (wherever the
family's rule takes the item alone: gemm_glds needs 256 rows, so only its 2 x 256-row case has it); itts_gemm_family(args,
itts_gemm_which(args), 0) = itts_gemm(args) on one shape per family that the selector routes there.  A K split is held to the bounds
of the unsplit call, not to its bits.

Every call: itts_gemm_family_supported is asked first (a variant it refuses is launched nevertheless, once, to see the entry refuse
it on the host); the output lives inside a NaN-filled buffer (guard rows before and after, pad columns where ldc > N) whose guard
bits have to survive, everything stored has to be finite; A has NaN rows before its first and after its last item, W a NaN row
behind its last (phase), R and ADD NaN pad columns, bias / scale / shift a NaN behind N; after the launch the stream is synchronised
and a device error ends the session.

The planner's case (1, 300, 768, 256, 3, 1): nk = 36 K-tiles in 2 tiles.  gemm_ksplit_plan starts from 8 splits, kper = ceil(36 / 8)
= 5, and keeps them: 7 * 5 = 35 < 36, so the last split owns one K-tile (the shortest pipeline there is) and the other seven own
five.  (Seven splits would be 6 K-tiles each with the seventh starting at K-tile 36, i.e. empty - the planner's loop exists to avoid
exactly that.)  The test asserts 8."""
import collections
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from itts_hip import lib as L
from itts_hip import pack, prng

DEV = "cuda:0"
HALF = {"bf16": (torch.bfloat16, 2.0 ** -8), "f16": (torch.float16, 2.0 ** -11)}  # torch dtype, h of the 16-bit output
H32 = 2.0 ** -23
RMS_LIMIT = 1.25
GUARD = 24  # NaN rows around A and C

# kind "conv": (B, T, Cin, N, k, dilation, padding, in_up) - T output rows per item; "convT": d is the stride u, k the kernel length
Case = collections.namedtuple("Case", "kind B T Cin N k d pad up")


def conv(B, T, Cin, N, k, d, pad, up=1):
    return Case("conv", B, T, Cin, N, k, d, pad, up)


def convT(B, T, Cin, N, k, u):
    return Case("convT", B, T, Cin, N, k, u, "z", 1)


def case_id(c):
    return f"{c.kind}{c.B}x{c.T}x{c.Cin}x{c.N}k{c.k}d{c.d}{c.pad[0]}" + (f"up{c.up}" if c.up > 1 else "")


def geom(c):
    """The GemmArgs geometry of a case"""
    if c.kind == "convT":
        u, p = c.d, (c.k - c.d) // 2
        return dict(M=c.B * c.T, T=c.T, taps=c.k // u, dil=-1, pad_left=0, pad_mode=0, in_up=1, nphase=u,
                    phase_shift=[(ph + p) // u for ph in range(u)], Tin=c.T, Tout=c.T * u, K=(c.k // u) * c.Cin, band=p + 16)
    pl = c.d * (c.k - 1) // 2
    return dict(M=c.B * c.T, T=c.T, taps=c.k, dil=c.d, pad_left=pl, pad_mode=1 if c.pad == "reflect" else 0, in_up=c.up, nphase=1,
                phase_shift=[0], Tin=c.T // c.up, Tout=c.T, K=c.k * c.Cin, band=pl + 16)


# ---- family 1: tile | depth << 4 | nbuf << 8 -----------------------------------------------------------------------------------
def mfma_variant(tile, depth, nbuf=1):
    return tile | depth << 4 | nbuf << 8


TILES = {1: "128x128", 2: "128x64", 3: "64x64", 4: "128x32"}
PRODUCTION = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 4), (4, 1))  # (tile, depth) of the six instantiations dispatch() can pick, NBUF = 1


def variant_id(v):
    return "own" if v == 0 else f"{TILES[v & 15]}d{(v >> 4) & 15}" + ("nbuf2" if v >> 8 == 2 else "")


F1_PLUS = conv(2, 70, 24, 40, 3, 2, "reflect")  # partial chunk, N tail, item boundary inside a tile
F1_ODD = conv(3, 50, 40, 72, 5, 3, "z")         # two chunks per tap, one partial; odd chunk count
F1_TINY = conv(1, 16, 8, 16, 1, 1, "z")         # M = 16 and one 8-channel chunk: npair = 1
F1_WIDE = conv(1, 130, 96, 136, 3, 1, "z")      # second row tile holds 2 rows, second 128-wide column tile 8 columns
# (case, layout): layout "ld" = lda = Cin + 8, ldc = N + 3
F1_CASES = ((F1_TINY, ""), (F1_PLUS, ""), (F1_ODD, ""), (conv(2, 33, 64, 1, 7, 1, "z"), ""), (F1_WIDE, ""), (F1_WIDE, "ld"),
            (conv(2, 64, 32, 48, 3, 1, "z", 2), ""),  # nearest-upsampled source rows
            (convT(2, 19, 64, 32, 8, 4), ""),         # polyphase nphase = 4
            # ... and both at N = 64, where the forced 128-row and 64x64 tiles take them too (below it only 128x32 does)
            (conv(2, 64, 32, 64, 3, 1, "z", 2), ""), (convT(2, 19, 64, 64, 8, 4), ""))
# the instantiations only an A/B switch reaches, so that they are not silently broken; and F1_TINY under ring depths 2 and 4 of the
# one tile that takes N = 16 (npair = 1 < DEPTH: the forced 64x64 / 128-row tiles keep dispatch()'s N >= 64 condition)
F1_AB = tuple((F1_ODD, mfma_variant(t, d, 2)) for t, d in PRODUCTION) + ((F1_ODD, mfma_variant(3, 1)), (F1_ODD, mfma_variant(3, 2)),
                                                                          (F1_TINY, mfma_variant(4, 2)), (F1_TINY, mfma_variant(4, 4)))

F2_PLUS = conv(2, 150, 64, 128, 3, 2, "z")  # nk = 3, M = 300: item boundary inside tile 1, 44 live rows in tile 2
F2_ITEMS = conv(2, 256, 64, 64, 3, 1, "z")  # two items of one row tile each: the one shape whose items the gate takes alone
F2_CASES = (conv(1, 256, 64, 64, 1, 1, "z"),        # nk = 1, BN = 64, one tile
            F2_PLUS,
            conv(3, 100, 128, 192, 2, 1, "z"),      # even k: asymmetric padding; BN = 64 x 3; two stages per tap
            conv(2, 129, 64, 72, 7, 3, "reflect"),  # N tail in a 128-wide tile; reflect at both ends of both items inside one tile
            conv(1, 260, 192, 320, 3, 1, "z"),      # three stages per tap; last column tile 64 wide
            F2_ITEMS)

P8_WIDE_PLUS = conv(3, 100, 64, 256, 4, 1, "z")    # nk = 4, the minimum; three items in two row tiles
P8_ODD = conv(2, 150, 64, 256, 5, 2, "reflect")    # nk = 5, odd
P8_TALL_PLUS = conv(2, 300, 64, 192, 4, 1, "z")    # 512 x 128 geometry, N = 192: half-empty column tile
F3_CASES = (P8_WIDE_PLUS, P8_ODD,
            conv(1, 300, 128, 512, 3, 1, "z"),       # two K-tiles per tap; two column tiles
            conv(1, 257, 256, 256, 1, 1, "z"),       # one live row in the second row tile
            convT(2, 40, 128, 256, 8, 4),            # four phases, nk = 4
            P8_TALL_PLUS,
            conv(1, 520, 128, 384, 3, 5, "reflect"),  # 8 live rows in the second row tile
            conv(3, 171, 64, 320, 7, 1, "z"),        # odd nk; last column tile 64 wide
            convT(2, 40, 128, 192, 8, 4))            # polyphase on the half-empty column tile
# the cases that also run the full chain (16-bit and fp32 output) and NewGELU; F1_ODD because the forced 128-row and 64x64 tiles do
# not take F1_PLUS (N = 40)
PLUS = (F1_PLUS, F1_ODD, F2_PLUS, P8_WIDE_PLUS, P8_TALL_PLUS)  # ("gelu" / "silu": act, + R, * 0.5)
# scalar branch of p8_finish8 (and, last, a dense R: the default layout pads R by 8 columns, both stay on the vector branch)
P8_SCALAR = ("ldc4", "c8", "bias1", "rdense")
# explicit K splits: (case, S)
KSPLITS = ((P8_WIDE_PLUS, 4),                               # nk = 4: one K-tile per split
           (P8_ODD, 2),                                     # nk = 5: splits of 3 and 2
           (conv(2, 150, 128, 256, 5, 1, "z"), 4),          # nk = 10: splits of 3, 3, 3 and 1, starting mid-tap
           (conv(2, 300, 128, 192, 5, 1, "z"), 4))          # ... on the 512 x 128 geometry
PLANNER = conv(1, 300, 768, 256, 3, 1, "z")                 # nk = 36 in 2 tiles: the planner's own 8 splits, the last of one K-tile
PLANNER_SPLITS = 8


def epilogues_of(case):
    return ("bias",) + (("chain", "chain32", "gelu", "silu") if case in PLUS else ())


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
def inputs(case, half):
    """Everything a call of this case may read, channels-first as torch wants it, rounded to the 16-bit type where the device holds it
    in 16 bits (fp32 outputs take R and ADD as the same values in fp32)."""
    tdt, tag, gm = HALF[half][0], case_id(case), geom(case)
    wshape = (case.Cin, case.N, case.k) if case.kind == "convT" else (case.N, case.Cin, case.k)
    return dict(x=rnd(f"gf.x{tag}", (case.B, case.Cin, gm["Tin"]), 1.5).to(tdt), w=rnd(f"gf.w{tag}", wshape, 1.0 / np.sqrt(gm["K"])).to(tdt),
                bias=rnd(f"gf.b{tag}", (case.B, case.N), 0.1), res=rnd(f"gf.r{tag}", (case.B, case.N, gm["Tout"])).to(tdt),
                run=rnd(f"gf.s{tag}", (case.B, case.N, gm["Tout"])).to(tdt), scale=0.75 + rnd(f"gf.sc{tag}", (case.N,), 0.1),
                shift=rnd(f"gf.sh{tag}", (case.N,), 0.1))


def operation(x, w, case):
    """The contraction of a case on [B, Cin, Tin] -> [B, N, Tout], in x's precision"""
    if case.kind == "convT":
        return F.conv_transpose1d(x, w, None, stride=case.d, padding=(case.k - case.d) // 2)
    if case.up > 1:
        x = x.repeat_interleave(case.up, dim=2)
    pl = case.d * (case.k - 1) // 2
    pads = (pl, case.d * (case.k - 1) - pl)
    x = F.pad(x, pads, mode="reflect") if case.pad == "reflect" else F.pad(x, pads)
    return F.conv1d(x, w, None, dilation=case.d)


def epilogue_terms(epi):
    """general branch (relu, scale / shift, tanh), fast-form activation ("gelu" / "silu" / None), R, alpha, beta (0 = no ADD), fp32 output"""
    if epi == "bias":
        return False, None, False, 1.0, 0.0, False
    if epi in ("gelu", "silu"):
        return False, epi, True, 0.5, 0.0, False
    return True, None, True, 1.0 / 3.0, 0.5, epi == "chain32"


def gelu_new(v):
    return 0.5 * v * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v)))


def gelu_device_fp32(x):
    """act_apply_fast / p8_finish8 in fp32 numpy: x / (1 + exp(-2 u)), u = 0.79788456f * (x + 0.044715f * x^3)"""
    x = x.astype(np.float32)
    u = np.float32(0.7978845608028654) * (x + np.float32(0.044715) * x * x * x)
    return x / (np.float32(1.0) + np.exp(np.float32(-2.0) * u, dtype=np.float32))


def silu_device_fp32(x):
    """act_apply(ACT_SILU) in fp32 numpy: x / (1 + exp(-x))"""
    x = x.astype(np.float32)
    return x / (np.float32(1.0) + np.exp(-x, dtype=np.float32))


FAST = {"gelu": (gelu_new, gelu_device_fp32, L.ACT_GELU_NEW), "silu": (F.silu, silu_device_fp32, L.ACT_SILU)}  # fp64 form, device form, code


def epilogue(v, p, epi):
    """GemmArgs' epilogue on v [B, N, Tout] in v's own precision"""
    general, fast, has_r, alpha, beta, _ = epilogue_terms(epi)
    cast = lambda t: t.to(v.dtype)  # noqa: E731
    v = v + cast(p["bias"])[:, :, None]
    if general:
        v = torch.tanh(torch.relu(v) * cast(p["scale"])[None, :, None] + cast(p["shift"])[None, :, None])
    if fast:
        v = FAST[fast][0](v)
    if has_r:
        v = v + cast(p["res"])
    v = v * torch.tensor(alpha, dtype=torch.float32).to(v.dtype)  # (the kernel's alpha and beta are fp32 numbers)
    if beta:
        v = v + torch.tensor(beta, dtype=torch.float32).to(v.dtype) * cast(p["run"])
    return v


@functools.lru_cache(maxsize=None)
def fixture(case, epi, half):
    """inputs, `exact`, `floor` (16-bit output) and the per-element bound of one (case, epilogue, build); never modified"""
    tdt, h16 = HALF[half]
    p, gm = inputs(case, half), geom(case)
    general, fast, has_r, alpha, beta, out32 = epilogue_terms(epi)
    alpha, beta = float(torch.tensor(alpha, dtype=torch.float32)), float(torch.tensor(beta, dtype=torch.float32))
    x64, w64 = p["x"].double(), p["w"].double()
    pre = operation(x64, w64, case)
    exact = epilogue(pre, p, epi)
    S = operation(x64.abs(), w64.abs(), case)
    sigma = abs(alpha) * (S + p["bias"].double().abs()[:, :, None] + (p["res"].double().abs() if has_r else 0.0))
    if beta:
        sigma = sigma + (beta * p["run"].double()).abs()
    h = H32 if out32 else h16
    bound = (gm["K"] + 8) * 2.0 ** -24 * sigma + h * exact.abs() + 1e-6
    act_term = 0.0
    if fast:
        z = pre + p["bias"].double()[:, :, None]
        act_term = 4.0 * float(np.abs(FAST[fast][1](z.numpy()).astype(np.float64) - FAST[fast][0](z).numpy()).max())
        bound = bound + abs(alpha) * act_term
    return dict(case=case, epi=epi, half=half, p=p, exact=exact, floor=None if out32 else exact.to(tdt).double(), bound=bound,
                out32=out32, act_term=act_term)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def judge(fx, got):
    """got [B, N, Tout] against the bounds -> the largest per-element error over its bound, the largest RMS ratio of each kind (16-bit)"""
    exact, floor = fx["exact"], fx["floor"]
    got = got.double()
    elem = float("inf") if not bool(torch.isfinite(got).all()) else float(((got - exact).abs() / fx["bound"]).max())
    out = dict(elem=elem, whole=0.0, item=0.0, band=0.0, rms=0.0, act=fx["act_term"], out32=fx["floor"] is None)
    if floor is None:
        return out
    band = geom(fx["case"])["band"]
    e, f = got - exact, floor - exact
    ratio = lambda a, b: float("inf") if not np.isfinite(rms(a)) else rms(a) / rms(b)  # noqa: E731
    out["whole"] = ratio(e, f)
    out["item"] = max(ratio(e[b], f[b]) for b in range(e.shape[0]))
    out["band"] = max(ratio(torch.cat([e[b, :, :band], e[b, :, -band:]], 1), torch.cat([f[b, :, :band], f[b, :, -band:]], 1))
                      for b in range(e.shape[0]))
    out["rms"] = max(out["whole"], out["item"], out["band"])
    return out


def passes(rep):
    return rep["elem"] <= 1.0 and rep["rms"] <= RMS_LIMIT


def packed_w(p, case):
    """W as the device holds it: [nphase * N, taps * Cin] (fp32 values of the 16-bit weights)"""
    w = p["w"].float().numpy()
    if case.kind == "convT":
        return torch.from_numpy(pack.convT_w(w, case.d, (case.k - case.d) // 2)).reshape(case.d * case.N, -1)
    return torch.from_numpy(pack.conv_w(w))


def model_fp32(fx, plant=None):
    """The operation as the kernels state it - C[m, n] = sum over (tap, c) of A[row(m, tap), c] * W[n, tap * Cin + c], row = t +
    phase_shift + tap * dil - pad_left inside the item, zero or reflected outside it, source row / in_up - with fp32 products and sums,
    the epilogue in fp32 and one rounding of the output.  plant: an error of the kind a wrong kernel would make."""
    case, p, gm = fx["case"], fx["p"], geom(fx["case"])
    tdt = torch.float32 if fx["out32"] else HALF[fx["half"]][0]
    B, T, Tin, Cin, N, taps = case.B, gm["T"], gm["Tin"], case.Cin, case.N, gm["taps"]
    A = p["x"].float().transpose(1, 2).reshape(B * Tin, Cin)
    W = packed_w(p, case).clone()
    shifts = list(gm["phase_shift"])
    if plant == "phase_shift":
        shifts[-1] += 1
    if plant == "drop8":  # the last 8 channels of the last tap
        W[:, -8:] = 0.0
    t = torch.arange(T)
    out = torch.empty(B, T, gm["nphase"], N)
    for ph in range(gm["nphase"]):
        cols = torch.zeros(B, T, taps * Cin)
        for tap in range(taps):
            ts = t + shifts[ph] + tap * gm["dil"] - gm["pad_left"]
            if gm["pad_mode"] == 1:
                left = ts < 0
                ts = torch.where(ts < 0, -ts, ts)
                ts = torch.where(ts >= T, 2 * (T - 1) - ts, ts)
                live = ~left if plant == "zero_pad" else torch.ones_like(left)  # zero instead of reflect padding at the left end
            else:
                live = (ts >= 0) & (ts < T)
            for b in range(B):
                rows = b * Tin + ts.clamp(0, T - 1) // gm["in_up"]
                blk = A[rows] * live[:, None]
                if plant == "neighbour" and b > 0:  # the row in front of the item comes from the item before it
                    first = (t + shifts[ph] + tap * gm["dil"] - gm["pad_left"]) == -1
                    blk = torch.where(first[:, None], A[b * Tin - 1][None, :], blk)
                cols[b, :, tap * Cin:(tap + 1) * Cin] = blk
        Wp = W[ph * N:(ph + 1) * N]
        acc = cols @ Wp.T
        if plant == "twice":  # the last 64-channel K-tile of a split counted twice
            lo = max(taps * Cin - 64, 0)
            acc = acc + cols[:, :, lo:] @ Wp[:, lo:].T
        out[:, :, ph] = acc
    v = out.reshape(B, T * gm["nphase"], N).transpose(1, 2)
    return epilogue(v, p, fx["epi"]).to(tdt)


PLANTS = ("zero_pad", "neighbour", "phase_shift", "drop8", "twice")


def plant_applies(case, plant):
    return (plant != "zero_pad" or case.pad == "reflect") and (plant != "neighbour" or case.B > 1)


# ---- one call -----------------------------------------------------------------------------------------------------------------
def rows_last(t, ld, dtype, before=0, after=0):
    """[B, C, T] -> the [before + B * T + after, ld] buffer (CPU): NaN guard rows, NaN pad columns"""
    B, Cc, T = t.shape
    buf = torch.full((before + B * T + after, ld), float("nan"), dtype=dtype)
    buf[before:before + B * T, :Cc] = t.transpose(1, 2).reshape(B * T, Cc).to(dtype)
    return buf


def phase_rows(t, case):
    """[B, N, Tout] -> [B, nphase * N, T]: the column layout of C, R and ADD (column phase * N + n of row t)"""
    gm = geom(case)
    B, N, _ = t.shape
    return t.reshape(B, N, gm["T"], gm["nphase"]).permute(0, 3, 1, 2).reshape(B, gm["nphase"] * N, gm["T"])


def build_args(fx, keep, layout="", item=None):
    """The argument block of one call and, in keep, every device buffer it points to.  layout: "" = dense A and C, R padded by 8 and
    ADD by 16 columns; "ld" lda = Cin + 8, ldc = N + 3; "ldc4" ldc = N + 4; "c8" C 8 bytes past a 16-byte boundary; "bias1"
    bias_bstride = N + 1; "rdense" ldr = N."""
    case, epi, p = fx["case"], fx["epi"], fx["p"]
    gm = geom(case)
    tdt = HALF[fx["half"]][0]
    cdt = torch.float32 if fx["out32"] else tdt
    es = 4 if fx["out32"] else 2
    sel = slice(None) if item is None else slice(item, item + 1)
    x, bias, res, run = p["x"][sel], p["bias"][sel], p["res"][sel], p["run"][sel]
    B = x.shape[0]
    M, NN = B * gm["T"], case.N * gm["nphase"]
    general, fast, has_r, alpha, beta, _ = epilogue_terms(epi)
    lda = case.Cin + (8 if layout == "ld" else 0)
    ldc = NN + (3 if layout == "ld" else 4 if layout == "ldc4" else 0)
    coff = 8 // es if layout == "c8" else 0  # elements
    keep["A"] = rows_last(x, lda, tdt, GUARD, GUARD).to(DEV)
    keep["W"] = torch.cat([packed_w(p, case).to(tdt), torch.full((1, gm["K"]), float("nan"), dtype=tdt)]).to(DEV)
    keep["C"] = torch.full((coff + (GUARD + M + GUARD) * ldc + 8,), float("nan"), dtype=cdt).to(DEV)
    g = L.GemmArgs()
    g.A, g.W = keep["A"].data_ptr() + GUARD * lda * 2, keep["W"].data_ptr()
    g.C = keep["C"].data_ptr() + (coff + GUARD * ldc) * es
    g.M, g.N, g.Cin, g.taps, g.T, g.dil, g.pad_left, g.pad_mode = M, case.N, case.Cin, gm["taps"], gm["T"], gm["dil"], gm["pad_left"], gm["pad_mode"]
    g.in_up, g.nphase, g.lda, g.ldc, g.alpha, g.beta = gm["in_up"], gm["nphase"], lda, ldc, alpha, beta
    for i, s in enumerate(gm["phase_shift"]):
        g.phase_shift[i] = s
    g.dtype_a = g.dtype_w = L.BF16
    g.dtype_c = L.F32 if fx["out32"] else L.BF16
    bstride = case.N + (1 if layout == "bias1" else 0)
    brows = torch.full((B, bstride), float("nan"))
    brows[:, :case.N] = bias
    keep["bias"] = torch.cat([brows.reshape(-1), torch.full((1,), float("nan"))]).to(DEV)
    g.bias, g.bias_bstride = keep["bias"].data_ptr(), bstride
    nan1 = torch.full((1,), float("nan"))
    if general:
        keep["scale"], keep["shift"] = torch.cat([p["scale"], nan1]).to(DEV), torch.cat([p["shift"], nan1]).to(DEV)
        g.act, g.scale, g.shift, g.act2 = L.ACT_RELU, keep["scale"].data_ptr(), keep["shift"].data_ptr(), L.ACT_TANH
    if fast:
        g.act = FAST[fast][2]
    if has_r:
        g.ldr = NN + (0 if layout == "rdense" else 8)
        keep["R"] = rows_last(phase_rows(res, case), g.ldr, cdt).to(DEV)
        g.R = keep["R"].data_ptr()
    if beta:
        g.ldadd = NN + 16
        keep["ADD"] = rows_last(phase_rows(run, case), g.ldadd, cdt).to(DEV)
        g.ADD = keep["ADD"].data_ptr()
    return g, dict(B=B, M=M, NN=NN, ldc=ldc, coff=coff)


def call(lib, fx, family, variant=0, ksplit=1, layout="", item=None, entry="family"):
    """One launch of the case on one family -> the stored output [B, N, Tout] on the CPU.  entry: "family" = itts_gemm_family, "gemm" =
    itts_gemm (the selector has to answer `family`), "ws" = itts_gemm_ws with a 64 MiB workspace (the planner has to answer `ksplit`).
    item: that batch item alone."""
    case = fx["case"]
    gm = geom(case)
    keep = {}
    g, d = build_args(fx, keep, layout, item)
    before = keep["C"].cpu().view(torch.int32 if fx["out32"] else torch.int16).clone()
    tag = (case_id(case), fx["epi"], family, variant_id(variant), ksplit, layout, item, entry)
    ws_bytes = 0
    if entry == "ws":
        keep["ws"] = torch.full((64 << 18,), float("nan"), dtype=torch.float32, device=DEV)
        ws_bytes = 64 << 20
        assert lib.itts_gemm_which(C.byref(g)) == 1 and lib.itts_gemm_ksplit(C.byref(g), ws_bytes) == ksplit, tag
        ok(lib, lib.itts_gemm_ws(C.byref(g), keep["ws"].data_ptr(), ws_bytes, stream()), "gemm_ws")
    elif entry == "gemm":
        assert lib.itts_gemm_which(C.byref(g)) == family, tag
        ok(lib, lib.itts_gemm(C.byref(g), stream()), "gemm")
    else:
        if ksplit > 1:
            ws_bytes = ksplit * d["M"] * case.N * 4
            keep["ws"] = torch.full((ws_bytes // 4 + 4,), float("nan"), dtype=torch.float32, device=DEV)
        assert lib.itts_gemm_family_supported(C.byref(g), family, variant, ksplit, ws_bytes) == 1, tag
        ok(lib, lib.itts_gemm_family(C.byref(g), family, variant, ksplit, keep["ws"].data_ptr() if ksplit > 1 else None, ws_bytes, stream()),
           "gemm_family")
    sync()
    after = keep["C"].cpu()
    stored = torch.zeros(after.shape, dtype=torch.bool)
    lo = d["coff"] + GUARD * d["ldc"]
    stored[lo:lo + d["M"] * d["ldc"]].view(d["M"], d["ldc"])[:, :d["NN"]] = True
    assert torch.equal(after.view(before.dtype)[~stored], before[~stored]), (tag, "guard rows or pad columns were written")
    if ksplit > 1 and entry == "family":
        assert bool(torch.isnan(keep["ws"][ws_bytes // 4:]).all().cpu()), (tag, "the workspace was written behind its end")
    out = after[lo:lo + d["M"] * d["ldc"]].view(d["M"], d["ldc"])[:, :d["NN"]]
    assert bool(torch.isfinite(out.float()).all()), (tag, "non-finite output")
    # [M, nphase * N] -> [B, N, Tout]
    return out.reshape(d["B"], gm["T"] * gm["nphase"], case.N).transpose(1, 2).contiguous()


def refused(lib, fx, family, variant):
    """A variant the rule does not take: itts_gemm_family_supported says 0 and the entry refuses on the host (no launch, no HIP call)"""
    keep = {}
    g, _ = build_args(fx, keep)
    assert lib.itts_gemm_family_supported(C.byref(g), family, variant, 1, 0) == 0
    assert lib.itts_gemm_family(C.byref(g), family, variant, 1, None, 0, stream()) == -1
    assert lib.itts_last_error().startswith(b"itts_gemm_family: ")
    sync()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


MEASURED = {}  # table line -> the figures


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [f"{k:<72s} elem/bound {r['elem']:6.3f}   rms ratio whole {r['whole']:6.4f}  item {r['item']:6.4f}  band {r['band']:6.4f}"
             + (f"   act term {r['act']:.2e}" if r["act"] else "") for k, r in sorted(MEASURED.items())]
    for group in sorted({k.split(" | ")[0] for k in MEASURED}):
        sub = [r for k, r in MEASURED.items() if k.split(" | ")[0] == group]
        lines.append(f"{group} largest over {len(sub)} runs: elem/bound {max(r['elem'] for r in sub):.3f} (limit 1; fp32 output alone "
                     f"{max([r['elem'] for r in sub if r['out32']], default=0.0):.4f}), rms ratio {max(r['rms'] for r in sub):.4f} "
                     f"(limit {RMS_LIMIT}), act term {max(r['act'] for r in sub):.2e}")
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "gemm_family_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def check_numbers(fx, got, group, tag=""):
    """group: "<build> family <f> <variant>", the unit the profile reports maxima for"""
    rep = judge(fx, got)
    line = f"{group} | {case_id(fx['case'])} {fx['epi']}{tag}"
    MEASURED[line] = rep
    print(line, rep)
    assert rep["elem"] <= 1.0, (line, rep)
    assert rep["whole"] <= RMS_LIMIT and rep["item"] <= RMS_LIMIT and rep["band"] <= RMS_LIMIT, (line, rep)


def items_alone(lib, fx, whole, family, variant=0):
    """item b of the B-item call = that item alone, wherever the family takes the item alone; -> how many were compared"""
    n = 0
    for b in range(fx["case"].B if fx["case"].B > 1 else 0):
        g, _ = build_args(fx, {}, "", b)
        if lib.itts_gemm_family_supported(C.byref(g), family, variant, 1, 0) == 1:
            assert torch.equal(bits(whole[b:b + 1]), bits(call(lib, fx, family, variant, item=b))), (case_id(fx["case"]), f"item {b} alone differs")
            n += 1
    return n


# ---- the tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,layout", F1_CASES, ids=lambda v: case_id(v) if isinstance(v, Case) else v or "dense")
@pytest.mark.parametrize("td", PRODUCTION, ids=lambda td: variant_id(mfma_variant(*td)))
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_mfma_vs_fp64(half, td, case, layout):
    """gemm_mfma under each production instantiation: both bounds for every epilogue of the case, two runs agree, items alone.  The
    128x128, 128x64 and 64x64 tiles are refused below N = 64, as dispatch() does not take them there."""
    lib, variant = L.load(half), mfma_variant(*td)
    if td[0] != 4 and case.N < 64:
        refused(lib, fixture(case, "bias", half), 1, variant)
        return
    for epi in epilogues_of(case):
        fx = fixture(case, epi, half)
        got = call(lib, fx, 1, variant, layout=layout)
        check_numbers(fx, got, f"{half} family 1 {variant_id(variant)}", " " + layout if layout else "")
        if epi == "bias":
            assert torch.equal(bits(got), bits(call(lib, fx, 1, variant, layout=layout))), "two runs differ"
            if layout:  # the leading dimensions move the operands, not the numbers
                assert torch.equal(bits(got), bits(call(lib, fx, 1, variant)))
            else:
                assert items_alone(lib, fx, got, 1, variant) == (case.B if case.B > 1 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", F1_AB, ids=lambda v: case_id(v) if isinstance(v, Case) else variant_id(v))
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_mfma_ab_instantiations(half, case, variant):
    """NBUF = 2 and the ring depths only ITTS_GEMM_DEPTH reaches; a ring deeper than the K loop is long (npair = 1 < DEPTH)."""
    lib, fx = L.load(half), fixture(case, "bias", half)
    got = call(lib, fx, 1, variant)
    check_numbers(fx, got, f"{half} family 1 {variant_id(variant)}")
    assert torch.equal(bits(got), bits(call(lib, fx, 1, variant))), "two runs differ"
    items_alone(lib, fx, got, 1, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_simple_and_own_pick_vs_fp64(half):
    """Family 0 (the vector-ALU kernel) and family 1 with variant 0 (dispatch()'s own pick) against the same references.  (The vector
    kernel evaluates NewGELU with tanhf, act_apply: the bound with the fast form's allowance holds it too.)"""
    lib = L.load(half)
    for case in (F1_PLUS, convT(2, 19, 64, 32, 8, 4)):
        for epi in epilogues_of(case):
            fx = fixture(case, epi, half)
            for family in (0, 1):
                check_numbers(fx, call(lib, fx, family), f"{half} family {family} own")


@pytest.mark.gpu
@pytest.mark.parametrize("case", F2_CASES, ids=case_id)
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_glds_vs_fp64(half, case):
    lib = L.load(half)
    for epi in epilogues_of(case):
        fx = fixture(case, epi, half)
        got = call(lib, fx, 2)
        check_numbers(fx, got, f"{half} family 2 own")
        if epi == "bias":
            assert torch.equal(bits(got), bits(call(lib, fx, 2))), "two runs differ"
            assert items_alone(lib, fx, got, 2) == (2 if case == F2_ITEMS else 0)  # the rule needs 256 rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", F3_CASES, ids=case_id)
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_p8_vs_fp64(half, case):
    lib = L.load(half)
    for epi in epilogues_of(case):
        fx = fixture(case, epi, half)
        got = call(lib, fx, 3)
        check_numbers(fx, got, f"{half} family 3 {'256x256' if case.N % 256 == 0 else '512x128'}")
        if epi == "bias":
            assert torch.equal(bits(got), bits(call(lib, fx, 3))), "two runs differ"
            assert items_alone(lib, fx, got, 3) == (case.B if case.B > 1 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", P8_SCALAR)
@pytest.mark.parametrize("case", (P8_WIDE_PLUS, P8_TALL_PLUS), ids=case_id)
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_p8_scalar_epilogue(half, case, layout):
    """The scalar branch of p8_finish8 (ldc % 8 != 0, C off its 16-byte boundary, a misaligned bias row), and R on a dense row next to
    the padded one of every other test, against the references of the vector branch."""
    lib = L.load(half)
    for epi in ("bias", "chain", "chain32") if layout != "rdense" else ("chain", "chain32"):
        fx = fixture(case, epi, half)
        check_numbers(fx, call(lib, fx, 3, layout=layout), f"{half} family 3 {'256x256' if case.N % 256 == 0 else '512x128'}", " " + layout)


@pytest.mark.gpu
@pytest.mark.parametrize("case,S", KSPLITS, ids=lambda v: case_id(v) if isinstance(v, Case) else f"S{v}")
@pytest.mark.parametrize("epi", ("bias", "chain32"))
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_p8_explicit_ksplit(half, epi, case, S):
    """A K split is held to the bounds of the unsplit call (its sums are added in another order: not to its bits); two runs agree."""
    lib, fx = L.load(half), fixture(case, epi, half)
    got = call(lib, fx, 3, ksplit=S)
    check_numbers(fx, got, f"{half} family 3 ksplit", f" S{S}")
    check_numbers(fx, call(lib, fx, 3), f"{half} family 3 {'256x256' if case.N % 256 == 0 else '512x128'}")
    assert torch.equal(bits(got), bits(call(lib, fx, 3, ksplit=S))), "two runs differ"


@pytest.mark.gpu
@pytest.mark.parametrize("half", tuple(HALF))
def test_gemm_ws_planner_splits(half):
    """itts_gemm_ws on the stage-0 AMP conv at batch 1: the planner's own 8 splits (seven of 5 K-tiles, the last of 1; see the module
    docstring), held to the bounds."""
    lib, fx = L.load(half), fixture(PLANNER, "bias", half)
    check_numbers(fx, call(lib, fx, 3, ksplit=PLANNER_SPLITS, entry="ws"), f"{half} family 3 ksplit", " planner")
    check_numbers(fx, call(lib, fx, 3, ksplit=PLANNER_SPLITS), f"{half} family 3 ksplit", f" S{PLANNER_SPLITS}")


# one shape per family that the selector itself sends there (tests/test_gemm_selector.py pins them): Cin = 12, the mfma epilogue
# shape, the glds epilogue shape (257 tiles), N = 192 at 200 tiles of 512 x 128
ROUTED = ((0, conv(2, 64, 12, 64, 3, 1, "z")), (1, F1_PLUS), (2, conv(2, 16400, 128, 72, 9, 1, "z")), (3, conv(1, 51200, 64, 192, 4, 1, "z")))


@pytest.mark.gpu
@pytest.mark.parametrize("family,case", ROUTED, ids=lambda v: case_id(v) if isinstance(v, Case) else f"family{v}")
def test_gemm_family_entry_is_the_production_path(family, case):
    """itts_gemm_family(args, itts_gemm_which(args), 0) has the bits of itts_gemm(args).  (Bits only: no fp64 reference at these sizes.)"""
    lib = L.load()
    fx = dict(case=case, epi="bias", half="bf16", p=inputs(case, "bf16"), out32=False)
    assert torch.equal(bits(call(lib, fx, family, entry="gemm")), bits(call(lib, fx, family)))
