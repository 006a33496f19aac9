"""Operator-level tests of the row-wise / elementwise kernels (csrc/elementwise.hip) and the two small kernels of
csrc/model_vocoder.hip that feed the DVAE encoder, through the C ABI: itts_rowop, itts_layernorm, itts_transpose.

Inputs come from itts_hip/prng.py on the CPU.  Every reference is a torch functional op (or a plain formula) in fp64 on the CPU from
the SAME rounded inputs: F.layer_norm, F.normalize, F.glu, F.gelu (erf), F.conv1d(groups = C), F.conv2d(stride 2) + ReLU, and plain
formulas for the column statistics and the pooling (tests/test_rowop_api.py cross-checks three of them against an independent
spelling, without a GPU).

Poison and sentinels, every call: what the operation must not read holds NaN - the row past `rows`, the gap D .. ldx, the trailing
mel row / column a stride-2 window never reaches, the other batch item of a depthwise conv, the v third of relpos_pack's qkv (the
argmin's stray reads would win instead: -1e30) - so a stray read shows in the result and nothing leaves an allocation.  The output
holds NaN where the call stores and a sentinel where it must not (the row past `rows`, the gap D .. ldy): the result has to be
finite and the sentinels intact.

Bounds.  Exact operations are compared bit for bit.  fp32 output: relerr of tests/test_gpu_ops.py (largest error over largest
reference) <= max(2e-5, 4 * E32) - 2e-5 is the project's class for fp32 results, E32 the relerr of the same formula evaluated by torch
in fp32 on the CPU against the fp64 reference on the same inputs (what fp32 arithmetic of the formula costs without any kernel; it is
computed here, never from the kernel's output), 4 for another summation order and device intrinsics.  bf16 output, per element:
|got - ref| <= 2^-7 |ref| + fp32_bound * max|ref| (one bf16 ulp: 7 stored mantissa bits, a correctly rounded value may land on the
neighbour where the fp32 value sits near a tie).  The mean and the deviation halves of col_mean_std / asp_pool are judged apart, each
against its own largest reference (the stricter reading: a column of mean 1e3 must not hide a wrong deviation of 1).

The measured maxima, the E32 values and the bounds are printed and, where ITTS_TEST_OUT names a directory, written to
elementwise_ops.txt there (committed as profiles/elementwise_ops.txt).

gather_add and tanh_rows of elementwise.hip have no caller in csrc/ and no entry here."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from itts_hip import lib as L
from itts_hip import prng

DEV = "cuda:0"
NAN = float("nan")
SENT = 776.0  # exact in bf16
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {"f32": L.F32, "bf16": L.BF16}
PAIRS = [("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16"), ("bf16", "f32")]
EPS = 1e-5


def rnd(name, shape, std=1.0):
    return torch.from_numpy(prng.tensor(name, 11, shape, std=std))


def relerr(a, b):  # tests/test_gpu_ops.py
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


# ---- references: one spelling, evaluated in fp64 (the reference) and in fp32 (E32) -----------------------------------------------
def ref_layernorm(x, g, b, act, dt, eps=EPS):
    o = F.layer_norm(x.to(dt), (x.shape[-1],), None if g is None else g.to(dt), None if b is None else b.to(dt), eps)
    return F.silu(o) if act == L.ACT_SILU else o


def ref_rmsnorm_unit(x, g, dt):
    return F.normalize(x.to(dt), dim=-1, eps=1e-12) * math.sqrt(x.shape[-1]) * g.to(dt)


def ref_glu(x, dt):
    return F.glu(x.to(dt), dim=-1)


def ref_geglu(x, dt):
    a, gate = x.to(dt).chunk(2, dim=-1)
    return F.gelu(gate) * a


def ref_dwconv(x, w, bias, dt):
    """x [B, T, C], w [C, k], zero padding (k - 1) / 2 -> [B, T, C]"""
    k = w.shape[1]
    o = F.conv1d(x.to(dt).transpose(1, 2), w.to(dt)[:, None, :], None if bias is None else bias.to(dt), padding=(k - 1) // 2,
                 groups=x.shape[2])
    return o.transpose(1, 2)


def ref_conv2d_sub2(mel, w, bias, dt):
    """mel [B, F, idim], w [odim, 3, 3] -> [B, F', odim, f']: per time row (c, f') c-major"""
    o = F.relu(F.conv2d(mel.to(dt)[:, None], w.to(dt)[:, None], bias.to(dt), stride=2))
    return o.permute(0, 2, 1, 3)


def ref_col_stats(x, dt):
    """x [B, T, C] -> mean [B, C], population std [B, C] clamped at sqrt(1e-12)"""
    x = x.to(dt)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, var.clamp_min(1e-12).sqrt()


def ref_asp_pool(lg, x, bs, bsh, dt):
    """logits, x [B, T, C]; bs, bsh [2 C] -> BN(weighted mean) [B, C], BN(weighted std) [B, C]"""
    lg, x, bs, bsh = lg.to(dt), x.to(dt), bs.to(dt), bsh.to(dt)
    Cn = x.shape[2]
    wgt = torch.softmax(lg, dim=1)
    mean = (wgt * x).sum(1)
    var = (wgt * (x - mean[:, None]) ** 2).sum(1)
    return mean * bs[:Cn] + bsh[:Cn], var.clamp_min(1e-12).sqrt() * bs[Cn:] + bsh[Cn:]


def ref_scale_cols_add(x, sc, res, dt):
    o = x.to(dt) * sc.to(dt)[:, None, :]
    return o if res is None else o + res.to(dt)


# ---- calls, poison, sentinels -----------------------------------------------------------------------------------------------------
def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    """Wait for the launch; a device fault ends the session there (nothing more is started on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


def ptr(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def rowop(lib, op, **kw):
    a = L.RowopArgs()
    for k, v in kw.items():
        setattr(a, k, ptr(v))
    L.check(lib.itts_rowop(L.ROWOP[op], C.byref(a), stream()), op)
    sync()


def poisoned(data, ld=None, fill=NAN):
    """data [rows, D] -> device [rows + 1, ld]: `fill` in the gap D .. ld and in the row past the data"""
    rows, D = data.shape
    buf = torch.full((rows + 1, ld or D), fill, dtype=data.dtype)
    buf[:rows, :D] = data
    return buf.to(DEV)


class Out:
    """[rows + 1, ld] on the device: NaN in [:rows, :store] (what the call stores), the sentinel elsewhere"""

    def __init__(self, rows, D, ld, dtype, store=None):
        self.rows, self.D = rows, D
        self.host = torch.full((rows + 1, ld), SENT, dtype=dtype)
        self.mask = torch.zeros(rows + 1, ld, dtype=torch.bool)
        self.mask[:rows, :(store or D)] = True
        self.host[self.mask] = NAN
        self.dev = self.host.to(DEV)

    def result(self, what):
        got = self.dev.cpu()
        assert torch.equal(got[~self.mask], self.host[~self.mask]), (what, "stored outside the output")
        assert bool(torch.isfinite(got[self.mask].float()).all()), (what, "non-finite output")
        return got[:self.rows, :self.D]


MEASURED = {}  # "op dtype" -> [max relerr, max E32, bound, worst share of the per-element bound or None]


def judge(line, got, ref64, ref32, what):
    """fp32 output: relerr <= max(2e-5, 4 E32); bf16 output: per element 2^-7 |ref| + that * max|ref|"""
    ref64 = ref64.double()
    e32 = relerr(ref32, ref64)
    fb = max(2e-5, 4 * e32)
    e = relerr(got, ref64)
    m = MEASURED.setdefault(line, [0.0, 0.0, 0.0, None])
    m[0], m[1], m[2] = max(m[0], e), max(m[1], e32), max(m[2], fb)
    if got.dtype == torch.float32:
        print(f"{line} {what}: relerr {e:.3e}  E32 {e32:.3e}  bound {fb:.3e}")
        assert e <= fb, (line, what, e, fb)
        return
    err = (got.double() - ref64).abs()
    allow = 2.0 ** -7 * ref64.abs() + fb * (ref64.abs().max() + 1e-12)  # relerr's own denominator: a call whose only output is 5e-44 has no scale
    share = float((err / allow.clamp_min(1e-300)).max())
    m[3] = max(m[3] or 0.0, share)
    print(f"{line} {what}: relerr {e:.3e}  E32 {e32:.3e}  per-element bound 2^-7|ref| + {fb:.3e} max|ref|, worst share {share:.3f}")
    assert bool((err <= allow).all()), (line, what, share)


def exact(line, got, want, what):
    MEASURED.setdefault(line, "bit-exact")
    assert got.dtype == want.dtype and torch.equal(got, want), (line, what)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = []
    for k, m in sorted(MEASURED.items()):
        if m == "bit-exact":
            lines.append(f"{k:<34s} bit-exact")
        elif m[3] is None:
            lines.append(f"{k:<34s} max relerr {m[0]:9.3e}   E32 {m[1]:9.3e}   bound {m[2]:9.3e}")
        else:
            lines.append(f"{k:<34s} max relerr {m[0]:9.3e}   E32 {m[1]:9.3e}   bound per element 2^-7|ref| + {m[2]:9.3e} max|ref| "
                         f"(worst share {m[3]:.3f})")
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "elementwise_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- layernorm -----------------------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 4, 5, 9)  # four rows per block
LN_D_VEC = (4, 252, 256, 260, 512, 1020, 1024, 1280, 2044, 2048)  # 1, 2, 4, 5, 8 chunks of 256, ragged last chunks, the D limit
LN_D_SCALAR = (1, 63, 65, 130, 2052)
LN_ACTS = (L.ACT_NONE, L.ACT_SILU)  # what engine_core.cpp's Engine::ln is handed (model_cond.cpp: conv_norm runs SiLU)


@functools.lru_cache(maxsize=None)
def ln_pool(D, ti, affine, act):
    """9 rows: row 0 has a large mean (3 n + 50), row 1 is constant (variance 0: the output is beta, or 0), the rest are noise"""
    x = rnd(f"ew.ln.x{D}", (9, D))
    x[0] = 3 * x[0] + 50
    x[1] = 1.5  # D * 1.5 is exact in fp32: the mean is exact, the deviations are exactly 0
    x = x.to(TD[ti])
    g = rnd(f"ew.ln.g{D}", (D,)) * 0.2 + 1 if affine else None
    b = rnd(f"ew.ln.b{D}", (D,)) * 0.1 if affine else None
    return x, g, b, ref_layernorm(x, g, b, act, torch.float64), ref_layernorm(x, g, b, act, torch.float32)


def ln_call(lib, D, ti, to, affine, act, sel, ldx, ldy, x_off=0, entry="rowop"):
    """LayerNorm of the pool rows `sel`; x_off: elements the x pointer is moved by (the buffer grows in front, NaN there)"""
    x, g, b, r64, r32 = ln_pool(D, ti, affine, act)
    rows = len(sel)
    xd = poisoned(x[list(sel)], ldx)
    if x_off:
        xd = torch.cat([torch.full((x_off,), NAN, dtype=xd.dtype, device=DEV), xd.flatten()])
    gd, bd = (poisoned(g[None]), poisoned(b[None])) if affine else (None, None)
    y = Out(rows, D, ldy, TD[to])
    if entry == "rowop":
        rowop(lib, "layernorm", y=y.dev, x=xd.data_ptr() + x_off * xd.element_size(), w=gd, b=bd, dtype_x=CODE[ti], dtype_y=CODE[to],
              rows=rows, D=D, ldx=ldx, ldy=ldy, act=act, eps=EPS)
    else:
        assert ldx == D and ldy == D and act == L.ACT_NONE
        L.check(lib.itts_layernorm(y.dev.data_ptr(), CODE[to], xd.data_ptr(), CODE[ti], ptr(gd), ptr(bd), rows, D, EPS, stream()), "layernorm")
        sync()
    what = (D, ti, to, affine, act, tuple(sel), ldx, ldy, x_off, entry)
    return y.result(what), r64[list(sel)], r32[list(sel)], what


def ln_sels(rows):
    return [range(rows)] if rows > 1 else [[0], [1]]  # one row: the large-mean row, then the constant row


@pytest.mark.gpu
@pytest.mark.parametrize("ti,to", PAIRS)
def test_layernorm_vector_path(lib, ti, to):
    for D in LN_D_VEC:
        for affine in (0, 1):
            for act in LN_ACTS:
                for pad in (0, 4):
                    for rows in LN_ROWS:
                        for sel in ln_sels(rows):
                            got, r64, r32, what = ln_call(lib, D, ti, to, affine, act, sel, D + pad, D + pad)
                            judge(f"layernorm vec {ti}->{to}", got, r64, r32, what)


@pytest.mark.gpu
@pytest.mark.parametrize("ti,to", PAIRS)
def test_itts_layernorm_entry(lib, ti, to):
    for affine in (0, 1):
        got, r64, r32, what = ln_call(lib, 260, ti, to, affine, L.ACT_NONE, range(5), 260, 260, entry="itts_layernorm")
        judge(f"itts_layernorm {ti}->{to}", got, r64, r32, what)


@pytest.mark.gpu
@pytest.mark.parametrize("ti,to", PAIRS)
def test_layernorm_scalar_path(lib, ti, to):
    for D in LN_D_SCALAR:  # D % 4 != 0 or D > 2048; ldx = D + 1
        for affine in (0, 1):
            for act in LN_ACTS:
                for rows in (1, 5):
                    for sel in ln_sels(rows):
                        got, r64, r32, what = ln_call(lib, D, ti, to, affine, act, sel, D + 1, D + 1)
                        judge(f"layernorm scalar {ti}->{to}", got, r64, r32, what)
    # D % 4 == 0 with the x pointer moved by 4 bytes: the gate must take the scalar kernel; the aligned call of the same problem runs
    # the vector kernel, and both are held to the same reference
    for D in (256, 1280):
        for affine in (0, 1):
            off = 4 // TD[ti].itemsize
            got, r64, r32, what = ln_call(lib, D, ti, to, affine, L.ACT_NONE, range(5), D, D, x_off=off)
            judge(f"layernorm scalar {ti}->{to}", got, r64, r32, what)
            got, r64, r32, what = ln_call(lib, D, ti, to, affine, L.ACT_NONE, range(5), D, D)
            judge(f"layernorm vec {ti}->{to}", got, r64, r32, what)


# ---- rmsnorm_unit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ti", ("f32", "bf16"))
def test_rmsnorm_unit(lib, ti):
    for D in (64, 130, 512, 1280):
        x = rnd(f"ew.rms.x{D}", (5, D))
        x[1] = 0  # |x| = 0: under the 1e-12 clamp the row is 0, not NaN
        x = x.to(TD[ti])
        g = rnd(f"ew.rms.g{D}", (D,)) * 0.2 + 1
        r64, r32 = ref_rmsnorm_unit(x, g, torch.float64), ref_rmsnorm_unit(x, g, torch.float32)
        for sel in ([0], [1], range(5)):
            y = Out(len(sel), D, D, torch.float32)
            rowop(lib, "rmsnorm_unit", y=y.dev, x=poisoned(x[list(sel)]), w=poisoned(g[None]), dtype_x=CODE[ti], dtype_y=L.F32, rows=len(sel), D=D)
            got = y.result((D, ti, tuple(sel)))
            if 1 in sel:
                assert bool((got[list(sel).index(1)] == 0).all())
            if list(sel) != [1]:
                judge(f"rmsnorm_unit {ti}->f32", got, r64[list(sel)], r32[list(sel)], (D, tuple(sel)))


# ---- glu / geglu ---------------------------------------------------------------------------------------------------------------------
GATES = (30.0, -30.0, 100.0, -100.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_glu(lib, dt):
    for Cn in (1, 64, 257):
        x = rnd(f"ew.glu.x{Cn}", (7, 2 * Cn)) * 2
        for r in range(7):
            x[r, Cn] = GATES[r % 4]  # gate column 0 of row r
        if Cn >= 4:
            x[0, Cn:Cn + 4] = torch.tensor(GATES)
        x = x.to(TD[dt])
        r64, r32 = ref_glu(x, torch.float64), ref_glu(x, torch.float32)
        for sel in ([0], [1], [2], [3], range(7)):  # one row: each of the four gate values in turn
            sel = list(sel)
            y = Out(len(sel), Cn, Cn, TD[dt])
            rowop(lib, "glu", y=y.dev, x=poisoned(x[sel]), dtype_x=CODE[dt], dtype_y=CODE[dt], rows=len(sel), D=Cn)
            got = y.result((Cn, dt, sel))
            judge(f"glu {dt}", got, r64[sel], r32[sel], (Cn, sel))
            a, gate = x[sel][:, :Cn], x[sel][:, Cn:]
            assert torch.equal(got[gate == 100], a[gate == 100]) and bool((got[gate == -100] == 0).all()), (Cn, dt, sel)  # the limits
            assert torch.equal(got[gate == 30], a[gate == 30])  # 1 + e^-30 is 1 in fp32


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_geglu(lib, dt):
    for inner in (5, 64, 1365):
        x = (rnd(f"ew.geglu.x{inner}", (3, 2 * inner)) * 2).to(TD[dt])
        r64, r32 = ref_geglu(x, torch.float64), ref_geglu(x, torch.float32)
        for ldy in (inner, inner + 3, (inner + 31) // 32 * 32):
            y = Out(3, inner, ldy, TD[dt], store=ldy)  # the call stores the whole row: the tail [inner, ldy) is zero-filled
            rowop(lib, "geglu", y=y.dev, x=poisoned(x), dtype_x=CODE[dt], dtype_y=CODE[dt], rows=3, D=inner, ldy=ldy)
            got = y.result((inner, dt, ldy))
            judge(f"geglu {dt}", got, r64, r32, (inner, ldy))
            tail = y.dev.cpu()[:3, inner:]
            assert bool((tail == 0).all()), (inner, dt, ldy, "tail not zero")


# ---- dwconv --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dw_pool(T, Cn, k, has_bias, dt):
    x = rnd(f"ew.dw.x{T}.{Cn}", (2, T, Cn)).to(TD[dt])
    w = rnd(f"ew.dw.w{Cn}.{k}", (Cn, k)) * 0.5
    b = rnd(f"ew.dw.b{Cn}", (Cn,)) if has_bias else None
    return x, w, b, ref_dwconv(x, w, b, torch.float64), ref_dwconv(x, w, b, torch.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("k", (15, 3))
def test_dwconv(lib, dt, k):
    pad = (k - 1) // 2
    for T in (1, 7, 14, 15, 16, 40):  # T < k clips both sides at once
        for Cn in (1, 64, 65):
            for has_bias in (0, 1):
                x, w, b, r64, r32 = dw_pool(T, Cn, k, has_bias, dt)
                wd, bd = w.to(DEV), (b.to(DEV) if has_bias else None)
                # B = 1: item 0 alone; B = 2: one item under test, the other one NaN throughout (its edge rows are what a missing
                # clip reads).  `pad` NaN rows in front of and behind the tensor: a missing clip stays inside the allocation.
                for B, item in ((1, 0), (2, 0), (2, 1)):
                    buf = torch.full((pad + B * T + pad, Cn), NAN, dtype=TD[dt])
                    buf[pad + item * T:pad + (item + 1) * T] = x[item]
                    buf = buf.to(DEV)
                    y = Out(B * T, Cn, Cn, TD[dt])
                    rowop(lib, "dwconv", y=y.dev, x=buf.data_ptr() + pad * Cn * buf.element_size(), w=wd, b=bd, dtype_x=CODE[dt],
                          dtype_y=CODE[dt], B=B, T=T, D=Cn, k=k)
                    got = y.dev.cpu()
                    assert bool((got[B * T:] == SENT).all()), (T, Cn, k, B, item)
                    got = got[item * T:(item + 1) * T]
                    assert bool(torch.isfinite(got.float()).all()), (T, Cn, k, has_bias, B, item, "read across an item's edge")
                    judge(f"dwconv {dt}", got, r64[item], r32[item], (T, Cn, k, has_bias, B, item))


# ---- conv2d_sub2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_conv2d_sub2(lib, dt):
    for B in (1, 2):
        for Fn in (3, 4, 5, 9, 50):
            for idim in (3, 4, 100):
                Fo, fo = (Fn - 3) // 2 + 1, (idim - 3) // 2 + 1
                mel = rnd(f"ew.c2.m{B}.{Fn}.{idim}", (B, Fn, idim)).to(TD[dt])
                poison = mel.clone()  # what a stride-2 window never reaches: the last row of an even F, the last column of an even idim
                if Fn % 2 == 0:
                    poison[:, -1, :] = NAN
                if idim % 2 == 0:
                    poison[:, :, -1] = NAN
                md = poisoned(poison.reshape(B * Fn, idim))
                for odim in (1, 8):
                    w, b = rnd(f"ew.c2.w{odim}", (odim, 3, 3)) * 0.4, rnd(f"ew.c2.b{odim}", (odim,)) * 0.5
                    r64, r32 = ref_conv2d_sub2(mel, w, b, torch.float64), ref_conv2d_sub2(mel, w, b, torch.float32)
                    y = Out(B * Fo, odim * fo, odim * fo, TD[dt])
                    rowop(lib, "conv2d_sub2", y=y.dev, x=md, w=w.to(DEV), b=b.to(DEV), dtype_x=CODE[dt], dtype_y=CODE[dt], B=B, T=Fn,
                          D=idim, N=odim)
                    got = y.result((B, Fn, idim, odim, dt))
                    judge(f"conv2d_sub2 {dt}", got, r64.reshape(B * Fo, odim * fo), r32.reshape(B * Fo, odim * fo), (B, Fn, idim, odim))


# ---- exact ops: transpose, cast_copy, copy_rows, add_strided, pair_rows ----------------------------------------------------------------
def flat_in(t, fill=NAN):
    return torch.cat([t.flatten(), torch.full((8,), fill, dtype=t.dtype)]).to(DEV)


def flat_out(n, dtype):
    host = torch.cat([torch.full((n,), NAN, dtype=dtype), torch.full((8,), SENT, dtype=dtype)])
    return host.to(DEV)


def flat_result(yd, n, what):
    got = yd.cpu()
    assert bool((got[n:] == SENT).all()), (what, "stored past the output")
    return got[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_itts_transpose(lib, dt):
    for B in (1, 3):
        for R, Cn in ((1, 1), (31, 33), (32, 32), (33, 65), (100, 7)):
            x = rnd(f"ew.tr.{B}.{R}.{Cn}", (B, R, Cn)).to(TD[dt])
            xd, yd = flat_in(x), flat_out(B * R * Cn, TD[dt])
            L.check(lib.itts_transpose(yd.data_ptr(), xd.data_ptr(), B, R, Cn, CODE[dt], stream()), "transpose")
            sync()
            got = flat_result(yd, B * R * Cn, (B, R, Cn, dt)).reshape(B, Cn, R)
            exact(f"itts_transpose {dt}", got, x.transpose(1, 2).contiguous(), (B, R, Cn))


@pytest.mark.gpu
@pytest.mark.parametrize("ti,to", PAIRS)
def test_cast_copy(lib, ti, to):
    rows, D = 3, 259  # n = 777: three blocks of 256, the last one ragged
    x = rnd("ew.cast.x", (rows, D)) * 3
    # fp32 values on a bf16 tie (round to nearest even goes down, then up), just off a tie, and the signs
    x[0, :6] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, -0.0])
    x = x.to(TD[ti])
    yd = flat_out(rows * D, TD[to])
    rowop(lib, "cast_copy", y=yd, x=flat_in(x), dtype_x=CODE[ti], dtype_y=CODE[to], rows=rows, D=D)
    got = flat_result(yd, rows * D, (ti, to)).reshape(rows, D)
    exact(f"cast_copy {ti}->{to}", got, x.to(TD[to]), (ti, to))
    if (ti, to) == ("f32", "bf16"):
        assert got[0, :3].float().tolist() == [1.0, 1 + 2.0 ** -6, -1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_copy_rows_and_add_strided(lib, dt):
    rows, D = 5, 259
    x = rnd("ew.copy.x", (rows, D)).to(TD[dt])
    y = Out(rows, D, D + 5, TD[dt])
    rowop(lib, "copy_rows", y=y.dev, x=poisoned(x, D + 3), dtype_x=CODE[dt], dtype_y=CODE[dt], rows=rows, D=D, ldx=D + 3, ldy=D + 5)
    exact(f"copy_rows {dt}", y.result(("copy_rows", dt)), x, dt)
    # the Res2Net loop of model_vocoder.hip: slice j of x [M, C] + slice j - 1 of y [M, C] -> a dense [M, hc] buffer (an output
    # stride below the input strides); the other slices hold NaN
    M, hc, j = 7, 65, 2
    Cn = 4 * hc
    a, b = rnd("ew.add.a", (M, hc)).to(TD[dt]), rnd("ew.add.b", (M, hc)).to(TD[dt])
    xa, xb = torch.full((M + 1, Cn), NAN, dtype=TD[dt]), torch.full((M + 1, Cn), NAN, dtype=TD[dt])
    xa[:M, j * hc:(j + 1) * hc], xb[:M, (j - 1) * hc:j * hc] = a, b
    xa, xb = xa.to(DEV), xb.to(DEV)
    es = xa.element_size()
    want = (a.float() + b.float()).to(TD[dt])  # one IEEE add; bf16: the fp32 sum, one rounding
    for ldy in (hc, hc + 3):
        y = Out(M, hc, ldy, TD[dt])
        rowop(lib, "add_strided", y=y.dev, x=xa.data_ptr() + j * hc * es, x2=xb.data_ptr() + (j - 1) * hc * es, dtype_x=CODE[dt],
              dtype_y=CODE[dt], rows=M, D=hc, ldx=Cn, ld2=Cn, ldy=ldy)
        exact(f"add_strided {dt}", y.result(("add_strided", dt, ldy)), want, (dt, ldy))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_pair_rows(lib, dt):
    for Tin in (1, 2, 5):
        for Cn in (1, 100):
            B, Tout = 2, (Tin + 1) // 2
            x = rnd(f"ew.pair.{Tin}.{Cn}", (B, Tin, Cn)).to(TD[dt])
            want = torch.zeros(B, 2 * Tout, Cn, dtype=TD[dt])
            want[:, :Tin] = x  # zero fill at odd Tin
            y = Out(B * Tout, 2 * Cn, 2 * Cn, TD[dt])
            rowop(lib, "pair_rows", y=y.dev, x=poisoned(x.reshape(B * Tin, Cn)), dtype_x=CODE[dt], dtype_y=CODE[dt], B=B, T=Tin, D=Cn)
            exact(f"pair_rows {dt}", y.result((Tin, Cn, dt)), want.reshape(B * Tout, 2 * Cn), (Tin, Cn))


# ---- column statistics, SE gate, attentive pooling --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_col_mean_and_col_mean_std(lib, dt):
    for B in (1, 3):
        for T in (1, 2, 257):
            for Cn in (1, 64, 300):
                x = rnd(f"ew.col.{B}.{T}.{Cn}", (B, T, Cn))
                x[:, :, 0] += 1e3  # mean 1e3, std 1: E[x^2] - mean^2 in fp32 would lose the deviation
                x = x.to(TD[dt])
                (m64, s64), (m32, s32) = ref_col_stats(x, torch.float64), ref_col_stats(x, torch.float32)
                if T == 1:
                    assert bool(((s64 - 1e-6).abs() < 1e-18).all())  # sqrt of the 1e-12 clamp
                for ldx in (Cn, Cn + 8):
                    xd = poisoned(x.reshape(B * T, Cn), ldx)
                    y = Out(B, Cn, Cn, torch.float32)
                    rowop(lib, "col_mean", y=y.dev, x=xd, dtype_x=CODE[dt], dtype_y=L.F32, B=B, T=T, D=Cn, ldx=ldx)
                    judge(f"col_mean {dt}->f32", y.result((B, T, Cn, ldx)), m64, m32, (B, T, Cn, ldx))
                    y = Out(B, 2 * Cn, 2 * Cn, torch.float32)
                    rowop(lib, "col_mean_std", y=y.dev, x=xd, dtype_x=CODE[dt], dtype_y=L.F32, B=B, T=T, D=Cn, ldx=ldx)
                    got = y.result((B, T, Cn, ldx))
                    judge(f"col_mean_std mean {dt}->f32", got[:, :Cn], m64, m32, (B, T, Cn, ldx))
                    judge(f"col_mean_std std {dt}->f32", got[:, Cn:], s64, s32, (B, T, Cn, ldx))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_scale_cols_add(lib, dt):
    B, T, Cn = 2, 5, 67
    x, res = rnd("ew.sca.x", (B, T, Cn)).to(TD[dt]), rnd("ew.sca.r", (B, T, Cn)).to(TD[dt])
    sc = rnd("ew.sca.s", (B, Cn)) * 0.3 + 0.5  # one gate row per batch item, the two differ
    scd = poisoned(sc)
    scd = torch.cat([scd, torch.full((B * T, Cn), NAN, device=DEV)])  # a gate indexed by row instead of by item reads NaN, in bounds
    for has_res in (0, 1):
        r64 = ref_scale_cols_add(x, sc, res if has_res else None, torch.float64).reshape(B * T, Cn)
        r32 = ref_scale_cols_add(x, sc, res if has_res else None, torch.float32).reshape(B * T, Cn)
        y = Out(B * T, Cn, Cn + 3, TD[dt])
        rowop(lib, "scale_cols_add", y=y.dev, x=poisoned(x.reshape(B * T, Cn), Cn + 1), w=scd,
              x2=poisoned(res.reshape(B * T, Cn), Cn + 2) if has_res else None, dtype_x=CODE[dt], dtype_y=CODE[dt], B=B, T=T, D=Cn,
              ldx=Cn + 1, ldy=Cn + 3, ld2=Cn + 2)
        judge(f"scale_cols_add {dt}", y.result((dt, has_res)), r64, r32, has_res)


def asp_inputs(B, T, Cn, dt):
    """Per item two special columns (one when C = 1): logits spanning -40 .. 40, and a column that is one-hot in effect (one logit 60
    above the rest: the weighted variance is below the 1e-12 clamp).  Returns logits, x, and the (item, column) of the one-hot ones."""
    lg, x = rnd(f"ew.asp.l{B}.{T}.{Cn}", (B, T, Cn)) * 2, rnd(f"ew.asp.x{B}.{T}.{Cn}", (B, T, Cn))
    onehot = []
    for b in range(B):
        span_c, hot_c = (b % 2, 1 - b % 2) if Cn > 1 else ((0, None) if b == 0 else (None, 0))
        if span_c is not None:
            lg[b, :, span_c] = torch.linspace(-40, 40, T) if T > 1 else 40.0
        if hot_c is not None:
            lg[b, T // 2, hot_c] += 60
            onehot.append((b, hot_c))
    return lg.to(TD[dt]), x.to(TD[dt]), onehot


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_asp_pool(lib, dt):
    B = 2
    for T in (1, 3, 200):
        for Cn in (1, 64, 130):
            lg, x, onehot = asp_inputs(B, T, Cn, dt)
            bs, bsh = rnd(f"ew.asp.bs{Cn}", (2 * Cn,)) * 0.2 + 1, rnd(f"ew.asp.bh{Cn}", (2 * Cn,)) * 0.1
            (m64, s64), (m32, s32) = ref_asp_pool(lg, x, bs, bsh, torch.float64), ref_asp_pool(lg, x, bs, bsh, torch.float32)
            y = Out(B, 2 * Cn, 2 * Cn, torch.float32)
            rowop(lib, "asp_pool", y=y.dev, x=poisoned(lg.reshape(B * T, Cn)), x2=poisoned(x.reshape(B * T, Cn)), w=poisoned(bs[None]),
                  b=poisoned(bsh[None]), dtype_x=CODE[dt], dtype_y=L.F32, B=B, T=T, D=Cn)
            got = y.result((T, Cn, dt))
            judge(f"asp_pool mean {dt}->f32", got[:, :Cn], m64, m32, (T, Cn))
            judge(f"asp_pool std {dt}->f32", got[:, Cn:], s64, s32, (T, Cn))
            for b, c in onehot:
                # sd = 1e-6 (sqrt of the clamp) times the BN scale: the BN shift is at most 0.2, its fp32 ulp 1.5e-8, so the scaled
                # deviation is recovered within 1e-7 of 1e-6
                sd = (float(got[b, Cn + c]) - float(bsh[Cn + c])) / float(bs[Cn + c])
                assert abs(sd - 1e-6) < 1e-7, (T, Cn, dt, b, c, sd)


# ---- relpos_pack ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_relpos_pack(lib, dt):
    for T in (1, 5):
        for H in (1, 2, 8):
            for dk in (4, 64):
                D = H * dk
                qkv, p = rnd(f"ew.rp.qkv{T}.{H}.{dk}", (T, 3 * D)).to(TD[dt]), rnd(f"ew.rp.p{T}.{H}.{dk}", (T, D)).to(TD[dt])
                bu, bv = rnd(f"ew.rp.u{D}", (D,)), rnd(f"ew.rp.v{D}", (D,))
                poison = qkv.clone()
                poison[:, 2 * D:] = NAN  # the v third is not this kernel's
                qc, kc = Out(T, 2 * D, 2 * D, TD[dt]), Out(T, 2 * D, 2 * D, TD[dt])
                rowop(lib, "relpos_pack", y=qc.dev, y2=kc.dev, x=poisoned(poison), x2=poisoned(p), w=poisoned(bu[None]), b=poisoned(bv[None]),
                      dtype_x=CODE[dt], dtype_y=CODE[dt], T=T, N=H, D=dk)
                gq, gk = qc.result((T, H, dk, dt)).reshape(T, H, 2, dk), kc.result((T, H, dk, dt)).reshape(T, H, 2, dk)
                q, k = qkv[:, :D].reshape(T, H, dk), qkv[:, D:2 * D].reshape(T, H, dk)
                exact(f"relpos_pack k|p {dt}", gk, torch.stack([k, p.reshape(T, H, dk)], 2), (T, H, dk))
                sums = [q.to(t) + torch.stack([bu, bv]).reshape(2, 1, H, dk).to(t) for t in (torch.float64, torch.float32)]  # [2, T, H, dk]
                if dt == "f32":  # one IEEE add
                    exact("relpos_pack q+u|q+v f32", gq, sums[1].permute(1, 2, 0, 3).contiguous(), (T, H, dk))
                else:
                    judge("relpos_pack q+u|q+v bf16", gq, sums[0].permute(1, 2, 0, 3), sums[1].permute(1, 2, 0, 3), (T, H, dk))


# ---- dvae_argmin ---------------------------------------------------------------------------------------------------------------------
# positions that share the minimum: the same thread in two iterations, two lanes of a wave, two waves, n >= 256 only, the last index
TIES = ((300, 44), (10, 3), (200, 70), (700, 1000, 4000), (8191, 257, 256), (513, 2, 258, 66), (256, 0))


def argmin_case(N):
    """dots [rows, N], esq [N] on a coarse grid (esq: multiples of 2^-5 in [0, 512); dots: multiples of 2^-6, |.| < 256, < 1024 at a tie), so
    esq - 2 dots is exact in fp32 and every row is compared; 3 random rows, then one row per tie set that fits N with two positions."""
    esq = torch.from_numpy(prng.randint(f"ew.am.e{N}", 11, N, 0, 1 << 14)).double() * 2.0 ** -5
    rows = [torch.from_numpy(prng.randint(f"ew.am.d{N}.{r}", 11, N, -(1 << 14), 1 << 14)).double() * 2.0 ** -6 for r in range(3)]
    for pos in TIES:
        pos = [n for n in pos if n < N]
        if len(pos) >= 2:
            d = rows[len(rows) % 3].clone()
            d[pos] = (esq[pos] + 1000.0) / 2  # esq - 2 dots = -1000 there; every other entry is above 0 - 2 * 256
            rows.append(d)
    return torch.stack(rows), esq


@pytest.mark.gpu
def test_dvae_argmin(lib):
    for N in (1, 66, 255, 256, 257, 8192):
        dots, esq = argmin_case(N)
        R = dots.shape[0]
        dist64 = esq[None] - 2 * dots
        dist32 = esq.float()[None] - 2 * dots.float()
        assert torch.equal(dist32.double(), dist64) and torch.equal(dots.float().double(), dots)  # exact in fp32: no row is set aside
        want = torch.from_numpy(np.argmin(dist64.numpy(), axis=1)).int()  # numpy: the first occurrence
        # a stray read past N (or past the rows) would win the comparison
        dd = poisoned(dots.float(), fill=1e30)
        ed = torch.cat([esq.float(), torch.full((8,), -1e30)]).to(DEV)
        codes = torch.full((R + 1,), -7, dtype=torch.int32).to(DEV)
        rowop(lib, "dvae_argmin", y=codes, x=dd, b=ed, dtype_x=L.F32, dtype_y=L.F32, rows=R, N=N)
        got = codes.cpu()
        assert int(got[R]) == -7
        exact("dvae_argmin codes", got[:R], want, (N, got.tolist(), want.tolist()))
