"""No GPU: the public surface of itts_gemm_family / itts_gemm_family_supported (header, both builds of the library, lib.py), what the
entry refuses on the host - it runs the named kernel family or nothing, never another family - and its structural rules against a
restatement of them over a grid of shapes.  One valid argument block on host memory, then one field at a time made invalid: each is
refused with ITTS_E_INVALID and the entry's own message (a HIP call would answer ITTS_E_HIP or touch the block's host pointers), and
itts_gemm_family_supported says 0 for it.  (pre_alpha / pre_beta / pre_filt are not part of itts_gemm_args: that refusal of
gemm_family_refusal cannot be reached through the C ABI.)  The bounds of tests/test_gpu_gemm_family.py are exercised here on its fp32
model of the operation, right and with errors planted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_gemm_selector as S
import test_gpu_gemm_family as T
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HOST = np.zeros(4096, dtype=np.float32)
P = (_HOST.ctypes.data + 63) // 64 * 64  # the matrix-core families want 16-byte aligned operands
# a block every family 0 - 3 takes: 512 rows in two items, K = 3 * 64, N = 256
VALID = dict(A=P, W=P, C=P, M=512, N=256, Cin=64, taps=4, lda=64, ldc=256, T=256, dil=1, pad_left=1, pad_mode=0, in_up=1, nphase=1,
             bias=P, bias_bstride=256, R=P, ldr=256, alpha=1.0 / 3.0, ADD=P, ldadd=256, beta=1.0, dtype_a=L.BF16, dtype_w=L.BF16,
             dtype_c=L.BF16, force_simple=0)
WS = 64 << 20


def block(**kw):
    g = L.GemmArgs()
    for k, v in dict(VALID, **kw).items():
        setattr(g, k, v)
    return g


def refused(lib, family=1, variant=0, ksplit=1, ws=None, ws_bytes=0, ask=True, **kw):
    g = block(**kw)
    st = lib.itts_gemm_family(C.byref(g), family, variant, ksplit, ws, ws_bytes, None)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(b"itts_gemm_family: "), (kw, family, variant, ksplit, st, msg)  # ITTS_E_INVALID, the entry's own message
    if ask and (ws is None or ksplit <= 1):  # (the workspace pointer is not part of the question itts_gemm_family_supported answers)
        assert lib.itts_gemm_family_supported(C.byref(g), family, variant, ksplit, ws_bytes) == 0, (kw, family, variant, ksplit)
    return msg


def test_gemm_family_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+itts_gemm_family\s*\(\s*const\s+itts_gemm_args\s*\*\s*\w+\s*,\s*int\s+family\s*,\s*int\s+variant\s*,\s*int\s+ksplit\s*,"
                     r"\s*void\s*\*\s*ws\s*,\s*size_t\s+ws_bytes\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_gemm_family_supported\s*\(\s*const\s+itts_gemm_args\s*\*\s*\w+\s*,\s*int\s+family\s*,\s*int\s+variant\s*,"
                     r"\s*int\s+ksplit\s*,\s*size_t\s+ws_bytes\s*\)\s*;", h)
    assert {"itts_gemm_family", "itts_gemm_family_supported"} <= set(L.exported_symbols())
    for half in ("bf16", "f16"):
        lib = L.load(half)
        assert lib.itts_gemm_family.restype is L.i32 and len(lib.itts_gemm_family.argtypes) == 7
        assert lib.itts_gemm_family_supported.restype is L.i32 and len(lib.itts_gemm_family_supported.argtypes) == 5
        assert lib.itts_abi_version() == 4  # an addition: the ABI version stays


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_gemm_family_refuses_on_the_host_what_the_family_cannot_run(half):
    lib = L.load(half)
    g = block()
    for family in range(4):
        assert lib.itts_gemm_family_supported(C.byref(g), family, 0, 1, 0) == 1, family  # the block itself is valid
    assert lib.itts_gemm_family(None, 1, 0, 1, None, 0, None) == -1 and b"itts_gemm_family: null args" in lib.itts_last_error()
    assert lib.itts_gemm_family_supported(None, 1, 0, 1, 0) == 0
    for family in range(4):
        for k in ("A", "W", "C"):
            assert b"null pointer" in refused(lib, family, **{k: None})
        assert b"bad leading dims" in refused(lib, family, lda=56)
        assert b"bad leading dims" in refused(lib, family, ldc=248)
        assert b"bad leading dims" in refused(lib, family, nphase=2)  # ldc < N * nphase
        assert b"multiple of T" in refused(lib, family, T=200)
        assert b"bad phase/upsample" in refused(lib, family, nphase=9, ldc=9 * 256)
        for k in ("M", "N", "Cin", "taps"):
            assert b"bad dims" in refused(lib, family, **{k: 0}), k
        assert b"ksplit < 1" in refused(lib, family, ksplit=0)
    for family in (-1, 4, 5, 99):  # family 4 is itts_gemm / itts_act_conv
        assert b"unknown family" in refused(lib, family)
    for family in (0, 2, 3):
        assert b"unknown variant" in refused(lib, family, T.mfma_variant(1, 1))
        if family != 3:
            assert b"only family 3 splits K" in refused(lib, family, ksplit=2, ws=P, ws_bytes=WS)
    assert b"only family 3 splits K" in refused(lib, 1, ksplit=2, ws=P, ws_bytes=WS)
    assert b"force_simple" in refused(lib, 1, force_simple=1)
    assert lib.itts_gemm_family_supported(C.byref(block(force_simple=1)), 0, 0, 1, 0) == 1
    # dtypes: the matrix-core families take the 16-bit type (C also fp32), the vector kernel its six combinations
    for family in (1, 2, 3):
        for k, bads in (("dtype_a", (L.F32, L.F16, L.FP8, -1)), ("dtype_w", (L.F32, L.F16, L.FP8, -1)), ("dtype_c", (L.F16, L.FP8, -1))):
            for bad in bads:
                assert b"dtype" in refused(lib, family, **{k: bad}), (family, k, bad)
        assert lib.itts_gemm_family_supported(C.byref(block(dtype_c=L.F32)), family, 0, 1, 0) == 1
        for kw in (dict(lda=68), dict(A=P + 2), dict(W=P + 8)):
            assert b"operands" in refused(lib, family, **kw), (family, kw)
    assert b"dtype" in refused(lib, 0, dtype_a=L.BF16, dtype_w=L.F32)
    assert b"dtype" in refused(lib, 0, dtype_c=L.FP8)
    for kw in (dict(dtype_a=L.F32, dtype_w=L.F32, dtype_c=L.F32), dict(dtype_a=L.F32), dict(dtype_a=L.F32, dtype_c=L.F32), dict(lda=68), dict(A=P + 2)):
        assert lib.itts_gemm_family_supported(C.byref(block(**kw)), 0, 0, 1, 0) == 1, kw
    # the variants of family 1
    for tile, depth in T.PRODUCTION:
        for nbuf in (1, 2):
            assert lib.itts_gemm_family_supported(C.byref(g), 1, T.mfma_variant(tile, depth, nbuf), 1, 0) == 1
    for bad in (-1, 1, 5 | 1 << 4 | 1 << 8, 1 | 3 << 4 | 1 << 8, 1 | 1 << 4, 1 | 1 << 4 | 3 << 8, 1 << 4 | 1 << 8, 1 | 8 << 4 | 1 << 8, 1 | 1 << 4 | 1 << 8 | 1 << 12):
        assert b"unknown variant" in refused(lib, 1, bad), bad
    for tile in (1, 2, 3):  # dispatch()'s own condition on the forced tiles
        assert b"N >= 64" in refused(lib, 1, T.mfma_variant(tile, 2), N=48, ldc=48)
        assert lib.itts_gemm_family_supported(C.byref(block(N=64, ldc=64)), 1, T.mfma_variant(tile, 2), 1, 0) == 1
    assert lib.itts_gemm_family_supported(C.byref(block(N=48, ldc=48)), 1, T.mfma_variant(4, 2), 1, 0) == 1
    # shapes
    assert b"gemm_mfma needs" in refused(lib, 1, Cin=68, lda=72)
    assert b"gemm_mfma needs" in refused(lib, 1, M=15, T=15)
    for kw in (dict(Cin=96, lda=96), dict(in_up=2), dict(nphase=2, ldc=512), dict(N=56), dict(M=255, T=255)):
        assert b"gemm_glds needs" in refused(lib, 2, **kw), kw
    for kw in (dict(Cin=96, lda=96), dict(in_up=2), dict(N=128), dict(N=224), dict(taps=3)):
        assert b"gemm_p8 needs" in refused(lib, 3, **kw), kw
    # the K split: gemm_p8's own condition and the workspace
    assert lib.itts_gemm_family_supported(C.byref(g), 3, 0, 4, 4 * 512 * 256 * 4) == 1  # nk = 4: one K-tile each
    assert b"shorter than" in refused(lib, 3, ksplit=4, ws=P, ws_bytes=4 * 512 * 256 * 4 - 1)
    assert b"needs a workspace" in refused(lib, 3, ksplit=4, ws=None, ws_bytes=WS, ask=False)
    assert b"16-byte aligned" in refused(lib, 3, ksplit=4, ws=P + 8, ws_bytes=WS)
    assert b"a K-tile for every split" in refused(lib, 3, ksplit=5, ws=P, ws_bytes=WS)       # nk = 4
    assert b"a K-tile for every split" in refused(lib, 3, ksplit=4, ws=P, ws_bytes=WS, taps=5)  # kper = 2: the fourth split starts at 6 > 5
    assert lib.itts_gemm_family_supported(C.byref(block(taps=5)), 3, 0, 3, WS) == 1
    assert b"a K-tile for every split" in refused(lib, 3, ksplit=2, ws=P, ws_bytes=WS, nphase=2, ldc=512)


def rules(f):
    """The three structural rules, restated: (gemm_mfma_supported, gemm_glds_can_run, gemm_p8_tiles > 0) of a field dict"""
    ok = f["lda"] % 8 == 0 and f["lda"] >= f["Cin"] and f["ldc"] >= f["N"] * f["nphase"] and f["M"] % f["T"] == 0 and f["T"] % f["in_up"] == 0
    lds = ok and f["Cin"] % 64 == 0 and f["in_up"] == 1
    return (ok and f["Cin"] % 8 == 0 and f["M"] >= 16,
            lds and f["nphase"] == 1 and f["N"] >= 64 and f["M"] >= 256,
            lds and f["N"] >= 192 and f["N"] % 64 == 0 and f["taps"] * f["Cin"] >= 256)


def test_gemm_family_supported_is_the_structural_rule():
    lib = L.load()
    n = [0, 0, 0]
    for T_ in (8, 15, 16, 100, 255, 256, 300):
        for B in (1, 2):
            for N in (1, 32, 63, 64, 72, 128, 191, 192, 200, 256, 320):
                for Cin in (8, 12, 24, 64, 96, 128):
                    for taps in (1, 3, 4):
                        for in_up, nphase, lda_pad in ((1, 1, 0), (1, 1, 4), (1, 1, 8), (2, 1, 0), (1, 4, 0)):
                            if T_ % in_up:
                                continue
                            f = dict(M=B * T_, T=T_, N=N, Cin=Cin, taps=taps, lda=Cin + lda_pad, ldc=N * nphase, in_up=in_up, nphase=nphase, dil=1)
                            g = block(bias_bstride=N, ldr=N * nphase, ldadd=N * nphase, **f)
                            want = rules(f)
                            got = tuple(lib.itts_gemm_family_supported(C.byref(g), fam, 0, 1, 0) == 1 for fam in (1, 2, 3))
                            assert got == want, (f, got, want)
                            assert lib.itts_gemm_family_supported(C.byref(g), 0, 0, 1, 0) == 1, f
                            for i in range(3):
                                n[i] += got[i]
    assert min(n) > 50, n  # the grid reaches every rule from both sides


@pytest.mark.parametrize("mode", list(S.MODES))
def test_the_family_the_selector_names_is_supported(monkeypatch, mode):
    """Every row of the test_gemm_selector shape list, under every switch: the family itts_gemm_which names runs by name too (family 4
    has no entry here: it is refused), with the planner's split where it plans one."""
    lib = L.load()
    for k in S.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in S.MODES[mode].items():
        monkeypatch.setenv(k, v)
    for nm, fields in S.shapes():
        g = S.gemm_args(fields)
        fam = lib.itts_gemm_which(C.byref(g))
        # ("f32 weights only", 16-bit A with fp32 W: the selector answers 0 and gemm_simple has no such instantiation - itts_gemm fails too)
        assert lib.itts_gemm_family_supported(C.byref(g), fam, 0, 1, 0) == (0 if fam == 4 or nm == "f32 weights only" else 1), (nm, fam)
        split = lib.itts_gemm_ksplit(C.byref(g), WS)
        if split > 1:
            assert lib.itts_gemm_family_supported(C.byref(g), 3, 0, split, WS) == 1, (nm, split)


def test_every_gpu_case_is_one_its_family_takes():
    """The case tables of tests/test_gpu_gemm_family.py against the host rules, on a host-memory block: what the GPU tests launch is
    supported, what they expect to be refused is refused; the routed shapes go where the selector table says; the planner's case
    gets the planner's 8 splits."""
    lib = L.load()

    def args(case, **kw):
        gm = T.geom(case)
        NN = case.N * gm["nphase"]
        g = block(M=gm["M"], T=gm["T"], N=case.N, Cin=case.Cin, taps=gm["taps"], dil=gm["dil"], pad_left=gm["pad_left"], pad_mode=gm["pad_mode"],
                  in_up=gm["in_up"], nphase=gm["nphase"], **dict(dict(lda=case.Cin, ldc=NN, ldr=NN + 8, ldadd=NN + 16, bias_bstride=case.N), **kw))
        for i, s in enumerate(gm["phase_shift"]):
            g.phase_shift[i] = s
        return g

    for case, layout in T.F1_CASES:
        kw = dict(lda=case.Cin + 8, ldc=case.N + 3) if layout else {}
        for td in T.PRODUCTION:
            want = 0 if td[0] != 4 and case.N < 64 else 1
            assert lib.itts_gemm_family_supported(C.byref(args(case, **kw)), 1, T.mfma_variant(*td), 1, 0) == want, (case, td)
        assert sum(td[0] == 4 or case.N >= 64 for td in T.PRODUCTION) >= 1
    for case, variant in T.F1_AB:
        assert lib.itts_gemm_family_supported(C.byref(args(case)), 1, variant, 1, 0) == 1, (case, variant)
    for case in T.F2_CASES:
        assert lib.itts_gemm_family_supported(C.byref(args(case)), 2, 0, 1, 0) == 1, case
        assert lib.itts_gemm_which(C.byref(args(case))) != 2  # ... far below where the selector sends it
    for case in T.F3_CASES:
        assert lib.itts_gemm_family_supported(C.byref(args(case)), 3, 0, 1, 0) == 1, case
        assert lib.itts_gemm_which(C.byref(args(case))) != 3
    for case in (T.P8_WIDE_PLUS, T.P8_TALL_PLUS):
        for kw in (dict(ldc=case.N + 4), dict(C=P + 8), dict(bias_bstride=case.N + 1), dict(ldr=case.N)):
            assert lib.itts_gemm_family_supported(C.byref(args(case, **kw)), 3, 0, 1, 0) == 1, (case, kw)
    for case, split in T.KSPLITS:
        gm = T.geom(case)
        assert lib.itts_gemm_family_supported(C.byref(args(case)), 3, 0, split, split * gm["M"] * case.N * 4) == 1, (case, split)
    nk = {(c.Cin // 64) * c.k: s for c, s in T.KSPLITS}
    assert nk == {4: 4, 5: 2, 10: 4}  # one K-tile per split; 3 + 2; 3 + 3 + 3 + 1
    for family, case in T.ROUTED:
        assert lib.itts_gemm_which(C.byref(args(case, ldr=case.N, ldadd=case.N))) == family, case
    g = args(T.PLANNER)
    assert lib.itts_gemm_ksplit(C.byref(g), WS) == T.PLANNER_SPLITS == 8 and lib.itts_gemm_family_supported(C.byref(g), 3, 0, 8, WS) == 1
    # ... 36 K-tiles: kper = 5, the last split owns K-tile 35 alone; nine splits of kper 4 would fit too, the planner stops at 8
    assert 7 * -(-36 // 8) == 35 < 36


# ---- the checks of tests/test_gpu_gemm_family.py on a CPU model of the operation, right and wrong ------------------------------
MODEL_CASES = (T.F1_PLUS, T.F2_PLUS, T.P8_WIDE_PLUS, T.conv(2, 129, 64, 72, 7, 3, "reflect"), T.convT(2, 19, 64, 32, 8, 4))


@pytest.mark.parametrize("half", tuple(T.HALF))
@pytest.mark.parametrize("case", MODEL_CASES, ids=T.case_id)
def test_the_bounds_pass_an_fp32_model_and_catch_planted_errors(case, half):
    """An fp32-arithmetic model of the operation (fp32 products and sums, the epilogue in fp32, one rounding of the output) stays
    inside both bounds under every epilogue of the case; the same model with zero instead of reflect padding at one end, one row of
    the neighbouring batch item admitted at an item boundary, phase_shift off by one, the last 8 channels of the last tap dropped,
    or the last K-tile counted twice is caught by at least one of them.  The fp32 evaluation uses under one per cent of the bound
    where the output is fp32; the 16-bit floor stays inside the whole bound (0.99 of it at most) and the right model sits on it."""
    for epi in T.epilogues_of(case):
        fx = T.fixture(case, epi, half)
        rep = T.judge(fx, T.model_fp32(fx))
        print(T.case_id(case), epi, half, rep)
        assert T.passes(rep), (epi, rep)
        if fx["floor"] is not None:
            assert float(((fx["floor"] - fx["exact"]).abs() / fx["bound"]).max()) <= 1.0  # a perfect kernel is inside the bound
            assert 0.9 <= rep["whole"] <= 1.1, rep                                         # ... and the right model sits at the floor
        planted = 0
        for plant in T.PLANTS:
            if T.plant_applies(case, plant):
                bad = T.judge(fx, T.model_fp32(fx, plant))
                assert not T.passes(bad), (epi, plant, bad)
                planted += 1
        assert planted >= 3
