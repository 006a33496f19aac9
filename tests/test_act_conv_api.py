"""No GPU: the public surface of itts_act_conv / itts_act_conv_supported (header, both builds of the library, lib.py) and what the
entry refuses on the host - it runs the convolution with Activation1d fused into it (csrc/conv_lds.hip ACT) or not at all.  One
valid argument block on host memory, then one field at a time made invalid: each is refused with ITTS_E_INVALID and the entry's
own message (a HIP call would answer ITTS_E_HIP or touch the block's host pointers), and itts_act_conv_supported says 0 for it.
The CPU model of the kernel that tests/test_gpu_conv_lds.py keeps for its bounds is exercised here too, with errors planted."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_conv_lds as T
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HOST = np.zeros(4096, dtype=np.float32)
P = (_HOST.ctypes.data + 63) // 64 * 64  # the selector wants 16-byte aligned operands
VALID = dict(A=P, W=P, C=P, M=512, N=24, Cin=24, taps=3, lda=24, ldc=24, T=256, dil=1, pad_left=1, pad_mode=0, in_up=1, nphase=1,
             bias=P, bias_bstride=24, R=P, ldr=24, alpha=1.0 / 3.0, ADD=P, ldadd=24, beta=1.0, dtype_a=L.BF16, dtype_w=L.BF16,
             dtype_c=L.BF16, force_simple=0)


def block(**kw):
    g = L.GemmArgs()
    for k, v in dict(VALID, **kw).items():
        setattr(g, k, v)
    return g


def refused(lib, la=P, lb=P, filt=P, **kw):
    g = block(**kw)
    st = lib.itts_act_conv(C.byref(g), la, lb, filt, None)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(b"itts_act_conv: "), (kw, st, msg)  # ITTS_E_INVALID, the entry's own message
    if la and lb and filt:  # (the parameter vectors are not part of the question itts_act_conv_supported answers)
        assert lib.itts_act_conv_supported(C.byref(g)) == 0, kw
    return msg


def test_act_conv_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+itts_act_conv\s*\(\s*const\s+itts_gemm_args\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*log_alpha\s*,\s*const\s+float"
                     r"\s*\*\s*log_beta\s*,\s*const\s+float\s*\*\s*filt12\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_act_conv_supported\s*\(\s*const\s+itts_gemm_args\s*\*\s*\w+\s*\)\s*;", h)
    assert {"itts_act_conv", "itts_act_conv_supported"} <= set(L.exported_symbols())
    for half in ("bf16", "f16"):
        lib = L.load(half)
        assert lib.itts_act_conv.restype is L.i32 and len(lib.itts_act_conv.argtypes) == 5
        assert lib.itts_act_conv_supported.restype is L.i32 and len(lib.itts_act_conv_supported.argtypes) == 1
        assert lib.itts_abi_version() == 4  # an addition: the ABI version stays


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_act_conv_refuses_on_the_host_what_it_cannot_run_fused(half, monkeypatch):
    lib = L.load(half)
    for env in ("ITTS_NO_CONV_LDS", "ITTS_NO_CONV_ACT"):
        monkeypatch.delenv(env, raising=False)
    g = block()
    assert lib.itts_gemm_which(C.byref(g)) == 4 and lib.itts_act_conv_supported(C.byref(g)) == 1  # the block itself is valid
    assert lib.itts_act_conv(None, P, P, P, None) == -1 and b"itts_act_conv: null args" in lib.itts_last_error()
    assert lib.itts_act_conv_supported(None) == 0
    for k in ("A", "W", "C"):
        assert b"null pointer" in refused(lib, **{k: None})
    for k in ("la", "lb", "filt"):
        assert b"null pointer" in refused(lib, **{k: None})
    assert b"force_simple" in refused(lib, force_simple=1)
    for k in ("dtype_a", "dtype_w", "dtype_c"):
        for bad in (L.F32, L.F16, L.FP8, -1):
            assert b"dtype" in refused(lib, **{k: bad}), (k, bad)
    assert b"lda != Cin" in refused(lib, lda=32)
    assert b"lda != Cin" in refused(lib, lda=16)
    shapes = (dict(T=255, M=510), dict(T=0), dict(M=500), dict(Cin=104, lda=104), dict(Cin=8, lda=8), dict(Cin=20, lda=20), dict(N=20),
              dict(N=104, ldc=104, ldr=104, ldadd=104), dict(pad_mode=1), dict(taps=2), dict(taps=1), dict(taps=3, dil=33),
              dict(taps=11, dil=7), dict(nphase=2), dict(in_up=2), dict(ldc=28), dict(ldr=28), dict(ldadd=28), dict(A=P + 2), dict(W=P + 4),
              dict(C=P + 8), dict(R=P + 2), dict(ADD=P + 2))
    for kw in shapes:
        assert b"itts_gemm_which != 4" in refused(lib, **kw), kw
        assert lib.itts_gemm_which(C.byref(block(**kw))) != 4
    # the halo limit itself: (taps - 1) * dil = 64 runs, 68 does not
    assert lib.itts_act_conv_supported(C.byref(block(taps=5, dil=16, Cin=32, lda=32, N=32, ldc=32, ldr=32, ldadd=32, T=300, M=300))) == 1
    assert b"itts_gemm_which != 4" in refused(lib, taps=5, dil=17, Cin=32, lda=32, N=32, ldc=32, ldr=32, ldadd=32, T=300, M=300)
    # gate-accepted forms beyond the vocoder's own: N != Cin, no epilogue operands, leading dimensions beyond the row (C, R, ADD)
    for kw in (dict(N=40, ldc=40, ldr=40, ldadd=40, Cin=16, lda=16), dict(bias=None, R=None, ADD=None), dict(ldc=32, ldr=32, ldadd=40),
               dict(N=8, Cin=96, lda=96), dict(Cin=88, lda=88, N=96, ldc=96, ldr=96, ldadd=96), dict(pad_left=0), dict(pad_left=2)):
        assert lib.itts_act_conv_supported(C.byref(block(**kw))) == 1, kw
    # the two switches, read per call
    monkeypatch.setenv("ITTS_NO_CONV_ACT", "1")
    assert lib.itts_gemm_which(C.byref(g)) == 4  # the plain form still runs there
    assert b"ITTS_NO_CONV_ACT" in refused(lib)
    monkeypatch.delenv("ITTS_NO_CONV_ACT")
    assert lib.itts_act_conv_supported(C.byref(g)) == 1
    monkeypatch.setenv("ITTS_NO_CONV_LDS", "1")
    assert lib.itts_gemm_which(C.byref(g)) != 4
    assert b"itts_gemm_which != 4" in refused(lib)
    monkeypatch.delenv("ITTS_NO_CONV_LDS")
    assert lib.itts_act_conv_supported(C.byref(g)) == 1


def test_every_gpu_case_is_one_the_selector_takes():
    """The case table of tests/test_gpu_conv_lds.py against the host rule: every case and variant runs fused, lda = Cin + 8 is
    taken by the plain form only, dilation 17 at five taps by neither."""
    lib = L.load()
    for case in T.CASES:
        B, Tn, Cin, N, k, dil = case[:6]
        for variant in T.variants_of(case, False):
            ld = T.leading_dims(case, variant)
            g = block(M=B * Tn, T=Tn, Cin=Cin, N=N, taps=k, dil=dil, pad_left=T.pad_left_of(case), bias_bstride=N, **ld)
            fused = ld["lda"] == Cin
            assert lib.itts_gemm_which(C.byref(g)) == 4 and lib.itts_act_conv_supported(C.byref(g)) == (1 if fused else 0), (case, variant)
    assert lib.itts_act_conv_supported(C.byref(block(M=300, T=300, Cin=32, lda=32, N=32, ldc=32, ldr=32, ldadd=32, taps=5, dil=17))) == 0


# ---- the checks of tests/test_gpu_conv_lds.py on a CPU model of the kernel, right and wrong ------------------------------------------
MODEL_CASES = ((2, 256, 24, 24, 3, 1), (1, 257, 24, 24, 11, 5), (1, 256, 16, 40, 3, 5))


@pytest.mark.parametrize("case", MODEL_CASES)
def test_the_bounds_pass_an_fp32_model_and_catch_planted_errors(case):
    """An fp32-arithmetic model of the fused kernel (activation in fp32, rounded to bf16, fp32 products and sums, one rounding of the
    output) stays inside both bounds; the same model with a wrong clamp (zero instead of replicate padding of the activation's
    input), a halo shifted by one row, one channel using its neighbour's alpha, or a pad channel left unzeroed (a NaN under a
    weight of zero: the result is not finite) is caught by at least one of them."""
    half = "bf16"
    fx = T.fixture(case, "amp", half, True)
    good = T.model_fp32(fx)
    rep = T.judge(fx, good)
    assert rep["elem"] <= 1.0 and rep["rms"] <= T.RMS_LIMIT, rep
    for plant in ("zero_pad", "halo_shift", "neighbour_alpha", "pad_channel"):
        bad = T.judge(fx, T.model_fp32(fx, plant))
        assert bad["elem"] > 1.0 or bad["rms"] > T.RMS_LIMIT, (plant, bad)
