"""GPU: the segment operators of the packed vocoder through the C ABI, in both builds of the library and (where the padded-batch
tests have it) in fp32: itts_snake_aa_fwd_seg (csrc/snake.hip snake_aa_lds_seg_kernel / snake_aa_seg_kernel), itts_act_conv_seg
(csrc/conv_lds.hip conv_lds_seg_kernel) and itts_seg_bias_mask (csrc/elementwise.hip seg_bias_mask_kernel).

A pack is one [rows, C] tensor whose sentences lie back to back: sentence b owns rows [off[b] * mul, off[b + 1] * mul), the first
len[b] * mul of them are signal.  Around the pack lie NaN sentinel rows; the gaps of every source hold NaN (a read there shows).

Segment activation.  C = 24 (one tile as wide as the tensor), 96 (48-channel slabs), 192 (64-channel slabs) take the LDS-tiled kernel,
C = 12 the register-window kernel.  Eight sentences of 1, 5, 6, 7 (shorter than, equal to and just past the 6-row FIR window),
TT - 1, TT, TT + 1 and 2 TT + 3 rows (TT the time tile of the kernel for that C), capacities alternately exactly len + gap and 5 rows
more.  Signal rows are, bit for bit, itts_snake_aa_fwd (layout 1) on the sentence cut out; the rest of a capacity is exactly zero;
the sentinels keep their bits; two runs agree; and with a table of ONE middle sentence nothing outside its capacity - its
NaN-filled neighbours included - is written.

itts_act_conv_seg.  Shapes, inputs, the "amp" epilogue and the rules are those of tests/test_gpu_conv_lds.py (cases 0, 2, 3, 4 of its
table; its helpers are imported, the file is not changed).  Four sentences cut from the case's items, of T, 1, 37 and BM + 3 rows (BM
the fused form's tile), each capacity its length + the convolution's reach (k - 1) * dil, every second one 5 rows more.
  * bit for bit on every signal row: itts_snake_aa_fwd_seg into a scratch tensor, then itts_gemm (family 4, plain form) on the WHOLE
    pack as one item - the taps that leave a sentence read zeros of a gap there, and zeros by construction here; two runs agree;
  * against fp64 on the sentence CUT OUT (Activation1d in fp64 with its replicate padding at the sentence's own ends, the zero-padded
    convolution of len rows, the epilogue): that file's per-element bound and its RMS ratio 1.25 against the floor;
  * a table of one middle sentence leaves its neighbours' rows of C untouched.

itts_seg_bias_mask.  Exact against the torch expression (x.float() + bias[b]).to(dtype) on signal rows, zeros in the gaps, other rows
untouched: 16-byte rows (fp32 C = 8, 16-bit C = 24), 4-byte (fp32 C = 6 and C = 1, the waveform) and 2-byte (16-bit C = 12) forms,
with and without a bias."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_conv_lds as T
import test_gpu_snake_len as S
from itts_hip import lib as L
from itts_hip import pack, prng
from oracle import vocoder as ovoc

DEV = "cuda:0"
GUARD = 8
FORMS = S.FORMS
stream, sync, ok, bits = S.stream, S.sync, S.ok, S.bits


def table(lens, gap, extra=5):
    """offsets with capacities alternately exactly len + gap and `extra` rows more"""
    off = [0]
    for b, n in enumerate(lens):
        off.append(off[-1] + n + gap + (extra if b % 2 else 0))
    return off


def ints(v):
    """-> (the int32 array, which the caller keeps alive over the call; its pointer)"""
    a = np.asarray(v, dtype=np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


# ---- segment activation -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("Cn", S.CHANNELS)
@pytest.mark.parametrize("form", tuple(FORMS))
def test_snake_seg_rows_equal_the_cut_sentence_bit_for_bit(form, Cn):
    half, dt, tdt = FORMS[form]
    lib = L.load(half)
    TT = S.time_tile(Cn)
    lens = (1, 5, 6, 7, TT - 1, TT, TT + 1, 2 * TT + 3)
    gap = 3
    off = table(lens, gap)
    rows = off[-1]
    x = torch.from_numpy(prng.tensor(f"snake_seg.x{Cn}", 5, (len(lens), max(lens), Cn), std=1.5)).to(tdt)
    la = torch.from_numpy(prng.tensor(f"snake_seg.a{Cn}", 5, (Cn,), std=0.4)).to(DEV)
    lb = torch.from_numpy(prng.tensor(f"snake_seg.b{Cn}", 5, (Cn,), std=0.4)).to(DEV)
    filt = ovoc.kaiser_sinc_filter12().to(DEV)
    src = torch.full((GUARD + rows + GUARD, Cn), float("nan"), dtype=tdt)
    for b, n in enumerate(lens):
        src[GUARD + off[b]:GUARD + off[b] + n] = x[b, :n]
    src = src.to(DEV)
    skip = GUARD * Cn * src.element_size()

    def run(off_sub, lens_sub):
        dst = torch.full((GUARD + rows + GUARD, Cn), float("nan"), dtype=tdt, device=DEV)
        off_a, off_p = ints(off_sub)
        len_a, len_p = ints(lens_sub)
        ok(lib, lib.itts_snake_aa_fwd_seg(dst.data_ptr() + skip, src.data_ptr() + skip, filt.data_ptr(), filt.data_ptr(), la.data_ptr(),
                                          lb.data_ptr(), Cn, off_p, len_p, len(lens_sub), 1, dt, stream()), "snake_aa_fwd_seg")
        sync()
        return dst.cpu()

    nan_bits = bits(torch.full((1, Cn), float("nan"), dtype=tdt))[0]
    one, two = run(off, lens), run(off, lens)
    assert torch.equal(bits(one), bits(two)), "two runs differ"
    for g in (one[:GUARD], one[-GUARD:]):
        assert bool((bits(g) == nan_bits).all()), "sentinel rows written"
    body = one[GUARD:GUARD + rows]
    for b, n in enumerate(lens):
        cut = x[b, :n].contiguous().to(DEV)
        ref = torch.full((n, Cn), float("nan"), dtype=tdt, device=DEV)
        ok(lib, lib.itts_snake_aa_fwd(ref.data_ptr(), cut.data_ptr(), filt.data_ptr(), filt.data_ptr(), la.data_ptr(), lb.data_ptr(),
                                      1, Cn, n, dt, 1, stream()), "snake_aa_fwd")
        sync()
        ref = ref.cpu()
        assert bool(torch.isfinite(ref.float()).all())
        assert torch.equal(bits(body[off[b]:off[b] + n]), bits(ref)), (form, Cn, b, n, "signal rows differ from the cut sentence")
        assert bool((bits(body[off[b] + n:off[b + 1]]) == 0).all()), (form, Cn, b, n, "gap not zero")
    # one middle sentence as its own table (off[0] > 0): its capacity as above, every other row - its neighbours' - untouched
    for b in (4, 7):
        alone = run(off[b:b + 2], lens[b:b + 1])[GUARD:GUARD + rows]
        assert torch.equal(bits(alone[off[b]:off[b + 1]]), bits(body[off[b]:off[b + 1]])), (form, Cn, b)
        assert bool((bits(alone[:off[b]]) == nan_bits).all()) and bool((bits(alone[off[b + 1]:]) == nan_bits).all()), (form, Cn, b, "a neighbour was written")


@pytest.mark.gpu
def test_snake_seg_mul_scales_the_table():
    """mul: offsets and lengths are in units of mul rows (the up-sampling between the latent frames and this tensor)"""
    lib = L.load("bf16")
    Cn, mul, lens, gap = 24, 7, (1, 100, 33, 50), 2
    off = table(lens, gap)
    x = torch.from_numpy(prng.tensor("snake_seg.mul", 5, (off[-1] * mul, Cn), std=1.5)).to(torch.bfloat16).to(DEV)
    la = torch.zeros(Cn, device=DEV)
    filt = ovoc.kaiser_sinc_filter12().to(DEV)
    out = []
    for o, ln, m in ((off, lens, mul), ([v * mul for v in off], [n * mul for n in lens], 1)):
        dst = torch.full_like(x, float("nan"))
        off_a, off_p = ints(o)
        len_a, len_p = ints(ln)
        ok(lib, lib.itts_snake_aa_fwd_seg(dst.data_ptr(), x.data_ptr(), filt.data_ptr(), filt.data_ptr(), la.data_ptr(), la.data_ptr(), Cn,
                                          off_p, len_p, len(lens), m, L.BF16, stream()), "snake_aa_fwd_seg")
        sync()
        out.append(dst.cpu())
    assert torch.equal(bits(out[0]), bits(out[1]))
    for b, n in enumerate(lens):
        lo = off[b] * mul
        assert bool((bits(out[0][lo + n * mul:off[b + 1] * mul]) == 0).all()) and bool((out[0][lo:lo + n * mul].float().abs().sum(1) > 0).all())


# ---- fused activation + conv --------------------------------------------------------------------------------------------------------
CASES = tuple(T.CASES[i] for i in (0, 2, 3, 4))
VARIANT = "amp"


def sentences(case):
    """(item, length) of the four sentences and the table of the pack"""
    Bn, Tn, k, dil = case[0], case[1], case[4], case[5]
    bm = 256 if case[3] <= 32 else 128
    lens = (Tn, 1, 37, min(bm + 3, Tn))
    items = tuple(i % Bn for i in range(4))
    return items, lens, table(lens, (k - 1) * dil)


@functools.lru_cache(maxsize=None)
def reference(case, half, item, n):
    """exact, floor and the per-element bound of item `item` cut to n rows, with bias row 0 ([1, N, n]); never modified"""
    tdt, ulp = T.HALF[half]
    p = T.inputs(case, half)
    q = dict(p, bias=p["bias"][0:1], res=p["res"][item:item + 1, :, :n], run=p["run"][item:item + 1, :, :n])
    a64 = ovoc.activation1d(p["x"][item:item + 1, :, :n].double(), p["la"].double(), p["lb"].double(), p["filt"].double())
    w64 = p["w"].double()
    alpha = float(torch.tensor(T.epilogue_terms(VARIANT)[3], dtype=torch.float32))
    exact = T.epilogue(T.conv(a64, w64, case), q, VARIANT)
    floor = T.epilogue(T.conv(a64.to(tdt).double(), w64, case), q, VARIANT).to(tdt).double()
    Sabs = T.conv(a64.abs(), w64.abs(), case)
    return dict(case=case, exact=exact, floor=floor, bound=ulp * abs(alpha) * Sabs + 0.5 * ulp * exact.abs() + 1e-6)


def packed(t_items, items, lens, off, ld, tdt, fill):
    """[B, C, T] items -> the [GUARD.. + off[-1] + ..GUARD, ld] pack on the device: sentence j = item items[j] cut to lens[j] rows"""
    Cc = t_items.shape[1]
    buf = torch.full((T.AGUARD + off[-1] + T.AGUARD, ld), float("nan"), dtype=tdt)
    buf[T.AGUARD:T.AGUARD + off[-1], :Cc] = fill
    for j, (b, n) in enumerate(zip(items, lens)):
        buf[T.AGUARD + off[j]:T.AGUARD + off[j] + n, :Cc] = t_items[b, :, :n].transpose(0, 1).to(tdt)
    return buf.to(DEV)


def conv_call(lib, case, half, how, only=None):
    """One launch sequence over the pack -> the whole C buffer on the CPU ([AGUARD + rows + AGUARD, N]).  how: "fused" =
    itts_act_conv_seg; "two" = itts_snake_aa_fwd_seg into a scratch tensor, then itts_gemm on the pack as one item.  only: a table of
    that one sentence."""
    Cin, N, k, dil = case[2:6]
    tdt = T.HALF[half][0]
    p = T.inputs(case, half)
    items, lens, off = sentences(case)
    rows, es = off[-1], 2
    keep = dict(A=packed(p["x"], items, lens, off, Cin, tdt, float("nan")),
                W=torch.cat([torch.from_numpy(pack.conv_w(p["w"].float().numpy())).to(tdt), torch.full((1, k * Cin), float("nan"), dtype=tdt)]).to(DEV),
                C=torch.full((T.AGUARD + rows + T.AGUARD, N), float("nan"), dtype=tdt, device=DEV),
                bias=p["bias"][0].contiguous().to(DEV), R=packed(p["res"], items, lens, off, N, tdt, 0.0),
                ADD=packed(p["run"], items, lens, off, N, tdt, 0.0), la=p["la"].to(DEV), lb=p["lb"].to(DEV), filt=p["filt"].to(DEV))
    g = L.GemmArgs()
    g.A, g.W, g.C = keep["A"].data_ptr() + T.AGUARD * Cin * es, keep["W"].data_ptr(), keep["C"].data_ptr() + T.AGUARD * N * es
    g.M, g.N, g.Cin, g.taps, g.T, g.dil, g.pad_left, g.pad_mode, g.in_up, g.nphase = rows, N, Cin, k, rows, dil, T.pad_left_of(case), 0, 1, 1
    g.lda, g.ldc, g.alpha, g.beta = Cin, N, 1.0 / 3.0, 1.0
    g.dtype_a = g.dtype_w = g.dtype_c = L.BF16
    g.bias, g.bias_bstride = keep["bias"].data_ptr(), 0
    g.R, g.ldr, g.ADD, g.ldadd = keep["R"].data_ptr() + T.AGUARD * N * es, N, keep["ADD"].data_ptr() + T.AGUARD * N * es, N
    assert lib.itts_gemm_which(C.byref(g)) == 4 and lib.itts_gemm_which_pinned_conv(C.byref(g)) == 4, case
    o, ln = (off, lens) if only is None else (off[only:only + 2], lens[only:only + 1])
    off_a, off_p = ints(o)
    len_a, len_p = ints(ln)
    if how == "two":
        keep["act"] = torch.full_like(keep["A"], float("nan"))
        act_ptr = keep["act"].data_ptr() + T.AGUARD * Cin * es
        T.ok(lib, lib.itts_snake_aa_fwd_seg(act_ptr, g.A, keep["filt"].data_ptr(), keep["filt"].data_ptr(), keep["la"].data_ptr(),
                                            keep["lb"].data_ptr(), Cin, off_p, len_p, len(ln), 1, L.BF16, T.stream()), "snake_aa_fwd_seg")
        T.sync()
        g.A = act_ptr
        T.ok(lib, lib.itts_gemm(C.byref(g), T.stream()), "gemm")
    else:
        T.ok(lib, lib.itts_act_conv_seg(C.byref(g), keep["la"].data_ptr(), keep["lb"].data_ptr(), keep["filt"].data_ptr(), off_p, len_p,
                                        len(ln), 1, T.stream()), "act_conv_seg")
    T.sync()
    return keep["C"].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=T.case_id)
@pytest.mark.parametrize("half", tuple(T.HALF))
def test_act_conv_seg(half, case):
    lib = L.load(half)
    b16 = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    items, lens, off = sentences(case)
    N, G = case[3], T.AGUARD
    nan_bits = b16(torch.full((1, N), float("nan"), dtype=T.HALF[half][0]))[0]
    one, again, two = conv_call(lib, case, half, "fused"), conv_call(lib, case, half, "fused"), conv_call(lib, case, half, "two")
    for buf in (one, again, two):
        assert bool((b16(buf[:G]) == nan_bits).all()) and bool((b16(buf[G + off[-1]:]) == nan_bits).all()), (case, "sentinel rows written")
    failures = []
    for j, (b, n) in enumerate(zip(items, lens)):
        sig = slice(G + off[j], G + off[j] + n)
        assert bool(torch.isfinite(one[sig].float()).all()), (case, j, "non-finite output")
        assert torch.equal(b16(one[sig]), b16(again[sig])), (case, j, "two runs differ")
        assert torch.equal(b16(one[sig]), b16(two[sig])), (case, j, "fused != itts_snake_aa_fwd_seg then itts_gemm on the pack")
        rep = T.judge(reference(case, half, b, n), one[sig].transpose(0, 1)[None])
        print(f"{half} {T.case_id(case)} sentence {j} (item {b}, len {n})", rep)
        if not (rep["elem"] <= 1.0 and rep["rms"] <= T.RMS_LIMIT):
            failures.append((j, rep))
    assert not failures, failures
    j = 2  # a middle sentence as its own table: nothing outside its capacity is stored
    alone = conv_call(lib, case, half, "fused", only=j)
    lo, hi = G + off[j], G + off[j + 1]
    assert torch.equal(b16(alone[lo:lo + lens[j]]), b16(one[lo:lo + lens[j]])), (case, "the sentence alone differs")
    assert bool((b16(alone[:lo]) == nan_bits).all()) and bool((b16(alone[hi:]) == nan_bits).all()), (case, "a neighbour was written")


# ---- bias + mask ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,Cn", [("fp32", 8), ("fp32", 6), ("fp32", 1), ("bf16", 24), ("bf16", 12), ("f16", 24), ("f16", 12)])
def test_seg_bias_mask_is_exact(form, Cn):
    half, dt, tdt = FORMS[form]
    lib = L.load(half)
    lens, mul, gap = (5, 12, 1, 9, 300), 4, 2
    off = table(lens, gap)
    rows = off[-1] * mul
    x = torch.from_numpy(prng.tensor(f"seg_mask.x{Cn}", 5, (GUARD + rows + GUARD, Cn), std=1.5)).to(tdt)
    bias = torch.from_numpy(prng.tensor(f"seg_mask.b{Cn}", 5, (len(lens), Cn), std=0.7))
    off_a, off_p = ints(off)
    len_a, len_p = ints(lens)
    skip = GUARD * Cn * x.element_size()
    for with_bias in (True, False):
        want = x.clone()
        for b, n in enumerate(lens):
            lo = GUARD + off[b] * mul
            if with_bias:
                want[lo:lo + n * mul] = (x[lo:lo + n * mul].float() + bias[b]).to(tdt)
            want[lo + n * mul:GUARD + off[b + 1] * mul] = 0
        dev, bdev = x.to(DEV), bias.to(DEV)
        ok(lib, lib.itts_seg_bias_mask(dev.data_ptr() + skip, bdev.data_ptr() if with_bias else None, Cn, off_p, len_p, len(lens), mul, dt,
                                       stream()), "seg_bias_mask")
        sync()
        assert torch.equal(bits(dev.cpu()), bits(want)), (form, Cn, with_bias)
    # one middle sentence as its own table: the others keep their bits
    dev = x.to(DEV)
    off_a, off_p = ints(off[1:3])
    len_a, len_p = ints(lens[1:2])
    ok(lib, lib.itts_seg_bias_mask(dev.data_ptr() + skip, None, Cn, off_p, len_p, 1, mul, dt, stream()), "seg_bias_mask")
    sync()
    want = x.clone()
    want[GUARD + (off[1] + lens[1]) * mul:GUARD + off[2] * mul] = 0
    assert torch.equal(bits(dev.cpu()), bits(want)), (form, Cn, "one sentence")
