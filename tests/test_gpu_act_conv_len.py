"""GPU: the fused Activation1d convolution over a padded ragged batch (itts_act_conv_len; csrc/conv_lds.hip conv_lds_rag_kernel), through
the C ABI, in both builds of the library.  Shapes, inputs, epilogue ("amp": bias, residual, alpha = 1/3, running sum) and the rules
are those of tests/test_gpu_conv_lds.py (cases 0, 2, 3 and 4 of its table; its helpers are imported, the file is not changed).

Per-item lengths run over T, 256, 1 and one value whose last row lies in the right halo of the first tile (a single-tile case: T - 1),
each value at every item position.  A holds NaN behind every item's length: the fused form must not read there.

  * bit for bit: itts_act_conv_len = itts_snake_aa_fwd_len into a scratch tensor, then itts_gemm (family 4, plain form) on it, for the
    rows < len of every item - the property the fused form already has for whole items; two runs agree;
  * against fp64: the first len rows of every item against that file's two bounds, with the item CUT to len rows as the exact signal
    (Activation1d in fp64 with its replicate padding at row len - 1, the zero-padded convolution of len rows, the epilogue): the
    per-element bound, and the RMS ratio 1.25 against the floor (whole, per item, edge band) - per item, whatever its length.
The measured maxima are printed and, where ITTS_TEST_OUT names a directory, written to act_conv_len_ops.txt there."""
import ctypes as C
import functools
import os

import pytest
import torch

import test_gpu_conv_lds as T
from itts_hip import lib as L
from itts_hip import pack
from oracle import vocoder as ovoc

DEV = T.DEV
CASES = tuple(T.CASES[i] for i in (0, 2, 3, 4))
VARIANT = "amp"


def act_tile(case):
    """rows per workgroup of the fused form (conv_lds.hip conv_lds: by N)"""
    return 256 if case[3] <= 32 else 128


def length_sets(case):
    B, Tn, k, dil = case[0], case[1], case[4], case[5]
    bm = act_tile(case)
    pad_right = (k - 1) * dil - T.pad_left_of(case)
    halo = bm + 1 + pad_right // 2 if bm < Tn else Tn - 1  # its last row, halo - 1, lies in [bm, bm + pad_right)
    assert halo <= Tn and (bm >= Tn or bm <= halo - 1 < bm + pad_right)
    values = (Tn, 256, 1, halo)
    return tuple(tuple(values[(s + i) % 4] for i in range(B)) for s in range(4))


@functools.lru_cache(maxsize=None)
def reference(case, half, b, n):
    """exact, floor and the per-element bound of item b cut to n rows ([1, N, n]); never modified"""
    tdt, ulp = T.HALF[half]
    p = T.inputs(case, half)
    q = dict(p, bias=p["bias"][b:b + 1], res=p["res"][b:b + 1, :, :n], run=p["run"][b:b + 1, :, :n])
    a64 = ovoc.activation1d(p["x"][b:b + 1, :, :n].double(), p["la"].double(), p["lb"].double(), p["filt"].double())
    w64 = p["w"].double()
    alpha = float(torch.tensor(T.epilogue_terms(VARIANT)[3], dtype=torch.float32))
    exact = T.epilogue(T.conv(a64, w64, case), q, VARIANT)
    floor = T.epilogue(T.conv(a64.to(tdt).double(), w64, case), q, VARIANT).to(tdt).double()
    S = T.conv(a64.abs(), w64.abs(), case)
    return dict(case=case, exact=exact, floor=floor, bound=ulp * abs(alpha) * S + 0.5 * ulp * exact.abs() + 1e-6)


def call(lib, case, half, lens, how):
    """One launch sequence -> the stored output [B, N, T] on the CPU.  how: "fused" = itts_act_conv_len; "two" = itts_snake_aa_fwd_len
    into a scratch tensor, then itts_gemm on it."""
    Bn, Tn, Cin, N, k, dil = case[:6]
    tdt = T.HALF[half][0]
    p = T.inputs(case, half)
    es = 2
    x = p["x"].clone()
    for b, n in enumerate(lens):
        x[b, :, n:] = float("nan")
    keep = dict(A=T.channels_last(x, Cin, tdt, T.AGUARD, T.AGUARD),
                W=torch.cat([torch.from_numpy(pack.conv_w(p["w"].float().numpy())).to(tdt),
                             torch.full((1, k * Cin), float("nan"), dtype=tdt)]).to(DEV),
                C=torch.full((Tn + Bn * Tn + Tn, N), float("nan"), dtype=tdt, device=DEV),
                bias=p["bias"].reshape(-1).to(DEV), R=T.channels_last(p["res"], N, tdt), ADD=T.channels_last(p["run"], N, tdt),
                la=p["la"].to(DEV), lb=p["lb"].to(DEV), filt=p["filt"].to(DEV),
                lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    before = keep["C"].cpu().view(torch.int16).clone()
    g = L.GemmArgs()
    g.A, g.W, g.C = keep["A"].data_ptr() + T.AGUARD * Cin * es, keep["W"].data_ptr(), keep["C"].data_ptr() + Tn * N * es
    g.M, g.N, g.Cin, g.taps, g.T, g.dil, g.pad_left, g.pad_mode, g.in_up, g.nphase = Bn * Tn, N, Cin, k, Tn, dil, T.pad_left_of(case), 0, 1, 1
    g.lda, g.ldc, g.alpha, g.beta = Cin, N, 1.0 / 3.0, 1.0
    g.dtype_a = g.dtype_w = g.dtype_c = L.BF16
    g.bias, g.bias_bstride, g.R, g.ldr, g.ADD, g.ldadd = keep["bias"].data_ptr(), N, keep["R"].data_ptr(), N, keep["ADD"].data_ptr(), N
    assert lib.itts_gemm_which(C.byref(g)) == 4 and lib.itts_act_conv_supported(C.byref(g)) == 1, case
    if how == "two":
        keep["act"] = torch.full_like(keep["A"], float("nan"))
        act_ptr = keep["act"].data_ptr() + T.AGUARD * Cin * es
        T.ok(lib, lib.itts_snake_aa_fwd_len(act_ptr, g.A, keep["filt"].data_ptr(), keep["filt"].data_ptr(), keep["la"].data_ptr(),
                                            keep["lb"].data_ptr(), Bn, Cin, Tn, keep["lens"].data_ptr(), 1, L.BF16, T.stream()), "snake_aa_fwd_len")
        T.sync()
        g.A = act_ptr
        T.ok(lib, lib.itts_gemm(C.byref(g), T.stream()), "gemm")
    else:
        T.ok(lib, lib.itts_act_conv_len(C.byref(g), keep["la"].data_ptr(), keep["lb"].data_ptr(), keep["filt"].data_ptr(),
                                        keep["lens"].data_ptr(), 1, T.stream()), "act_conv_len")
    T.sync()
    after = keep["C"].cpu()
    stored = torch.zeros(after.shape, dtype=torch.bool)
    stored[Tn:Tn + Bn * Tn] = True
    assert torch.equal(after.view(torch.int16)[~stored], before[~stored]), (case, lens, "guard rows were written")
    out = after[Tn:Tn + Bn * Tn].reshape(Bn, Tn, N).transpose(1, 2).contiguous()
    for b, n in enumerate(lens):
        assert bool(torch.isfinite(out[b, :, :n].float()).all()), (case, lens, b, "non-finite output")
    return out


MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [f"{k:<44s} elem/bound {r['elem']:6.3f}   rms ratio whole {r['whole']:6.4f}  band {r['band']:6.4f}" for k, r in sorted(MEASURED.items())]
    for half in T.HALF:
        sub = [r for k, r in MEASURED.items() if k.startswith(half + " ")]
        if sub:
            lines.append(f"{half} largest: elem/bound {max(r['elem'] for r in sub):.3f} (limit 1), rms ratio {max(r['rms'] for r in sub):.4f} "
                         f"(limit {T.RMS_LIMIT})")
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "act_conv_len_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=T.case_id)
@pytest.mark.parametrize("half", tuple(T.HALF))
def test_act_conv_len(half, case):
    lib = L.load(half)
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    failures = []
    for lens in length_sets(case):
        one = call(lib, case, half, lens, "fused")
        again = call(lib, case, half, lens, "fused")
        two = call(lib, case, half, lens, "two")
        for b, n in enumerate(lens):
            assert torch.equal(bits(one[b, :, :n]), bits(again[b, :, :n])), (lens, b, "two runs differ")
            assert torch.equal(bits(one[b, :, :n]), bits(two[b, :, :n])), (lens, b, "fused != itts_snake_aa_fwd_len then itts_gemm")
            rep = T.judge(reference(case, half, b, n), one[b:b + 1, :, :n])
            line = f"{half} {T.case_id(case)} item {b} len {n}"
            MEASURED[line] = max((MEASURED.get(line), rep), key=lambda r: r["rms"] if r else -1.0)
            print(line, rep)
            if not (rep["elem"] <= 1.0 and rep["rms"] <= T.RMS_LIMIT):
                failures.append((line, rep))
    assert not failures, failures
