"""No GPU: the public surface of the ragged-batch vocoder (itts_bigvgan_ragged, itts_snake_aa_fwd_len, itts_act_conv_len,
itts_zero_tail_rows; header, both builds of the library, lib.py, the Python switches) and what the entries refuse on the host.
One valid argument block on host memory, then one field at a time made invalid: each is refused with ITTS_E_INVALID and the entry's
own message - a HIP call would answer ITTS_E_HIP here, or touch host pointers as if they were device memory.

An engine cannot be created without a device, so of itts_bigvgan_ragged only the null engine is refused here; its other refusals
(null pointers, B outside [1, max_batch], a length of 0 or above T) are in tests/test_gpu_ragged_vocoder.py, on a real engine."""
import ctypes as C
import inspect
import os
import re

import pytest

import test_act_conv_api as A
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = ("bf16", "f16")
P = A.P  # aligned host memory: never read, every call below is refused first
E_INVALID = -1


def test_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+itts_bigvgan_ragged\s*\(\s*itts_engine\s*\*\s*e\s*,\s*const\s+void\s*\*\s*latent\s*,\s*const\s+float\s*\*\s*spk\s*,"
                     r"\s*int\s+B\s*,\s*int\s+T\s*,\s*const\s+int32_t\s*\*\s*lens_host\s*,\s*float\s*\*\s*wav_out\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_snake_aa_fwd_len\s*\(\s*void\s*\*\s*dst\s*,\s*const\s+void\s*\*\s*src\s*,\s*const\s+float\s*\*\s*up12\s*,"
                     r"\s*const\s+float\s*\*\s*down12\s*,\s*const\s+float\s*\*\s*log_alpha\s*,\s*const\s+float\s*\*\s*log_beta\s*,\s*int\s+B\s*,"
                     r"\s*int\s+C\s*,\s*int\s+T\s*,\s*const\s+int\s*\*\s*lens_dev\s*,\s*int\s+mul\s*,\s*int\s+dtype\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_act_conv_len\s*\(\s*const\s+itts_gemm_args\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*log_alpha\s*,\s*const\s+float"
                     r"\s*\*\s*log_beta\s*,\s*const\s+float\s*\*\s*filt12\s*,\s*const\s+int\s*\*\s*lens_dev\s*,\s*int\s+mul\s*,\s*itts_stream\s+\w+\s*\)"
                     r"\s*;", h)
    assert re.search(r"\bint\s+itts_zero_tail_rows\s*\(\s*void\s*\*\s*x\s*,\s*int\s+B\s*,\s*int\s+T\s*,\s*int\s+C\s*,\s*const\s+int\s*\*\s*lens_dev\s*,"
                     r"\s*int\s+mul\s*,\s*int\s+dtype\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    for name, nargs in (("itts_bigvgan_ragged", 8), ("itts_snake_aa_fwd_len", 13), ("itts_act_conv_len", 7), ("itts_zero_tail_rows", 8)):
        assert name in L.exported_symbols()
        for half in HALVES:
            fn = getattr(L.load(half), name)
            assert callable(fn) and len(fn.argtypes) == nargs and fn.restype is L.i32
    for half in HALVES:
        assert L.load(half).itts_abi_version() == 4  # additions: the ABI version stays


def test_python_switches(monkeypatch):
    from itts_hip import engine as ieng

    sig = inspect.signature(ieng.Engine.bigvgan_grouped).parameters
    assert list(sig) == ["self", "lats", "spk", "ragged", "max_pad"] and sig["ragged"].default is False
    assert list(inspect.signature(ieng.Engine.bigvgan_ragged).parameters) == ["self", "lats", "spk"]
    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["ragged_vocoder"].default is False
    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav"]).ragged_vocoder is False
    assert p.parse_args(["hello", "-v", "voice.wav", "--ragged-vocoder"]).ragged_vocoder is True


def refused(lib, status, entry):
    msg = lib.itts_last_error()
    assert status == E_INVALID and msg.startswith(entry.encode() + b": "), (entry, status, msg)
    return msg


@pytest.mark.parametrize("half", HALVES)
def test_snake_len_and_zero_tail_refuse_on_the_host(half):
    lib = L.load(half)
    ok = dict(dst=P, src=P, up12=P, down12=P, log_alpha=P, log_beta=P, B=4, C=24, T=700, lens_dev=P, mul=1, dtype=L.BF16)

    def snake(**kw):
        a = dict(ok, **kw)
        return lib.itts_snake_aa_fwd_len(a["dst"], a["src"], a["up12"], a["down12"], a["log_alpha"], a["log_beta"], a["B"], a["C"], a["T"],
                                         a["lens_dev"], a["mul"], a["dtype"], None)

    for k in ("dst", "src", "up12", "down12", "log_alpha", "log_beta", "lens_dev"):
        assert b"null pointer" in refused(lib, snake(**{k: None}), "itts_snake_aa_fwd_len"), k
    for bad in (0, -3):
        assert b"mul < 1" in refused(lib, snake(mul=bad), "itts_snake_aa_fwd_len")
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(T=0)):
        assert b">= 1" in refused(lib, snake(**kw), "itts_snake_aa_fwd_len"), kw
    for bad in (L.FP8, 2, -1):
        assert b"dtype" in refused(lib, snake(dtype=bad), "itts_snake_aa_fwd_len"), bad

    okz = dict(x=P, B=4, T=700, C=24, lens_dev=P, mul=1, dtype=L.BF16)

    def ztail(**kw):
        a = dict(okz, **kw)
        return lib.itts_zero_tail_rows(a["x"], a["B"], a["T"], a["C"], a["lens_dev"], a["mul"], a["dtype"], None)

    for k in ("x", "lens_dev"):
        assert b"null pointer" in refused(lib, ztail(**{k: None}), "itts_zero_tail_rows"), k
    for bad in (0, -1):
        assert b"mul < 1" in refused(lib, ztail(mul=bad), "itts_zero_tail_rows")
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(C=0)):
        refused(lib, ztail(**kw), "itts_zero_tail_rows")
    for bad in (L.F16, L.FP8, -1):
        assert b"dtype" in refused(lib, ztail(dtype=bad), "itts_zero_tail_rows"), bad


@pytest.mark.parametrize("half", HALVES)
def test_act_conv_len_refuses_what_act_conv_refuses_and_its_own(half, monkeypatch):
    lib = L.load(half)
    for env in ("ITTS_NO_CONV_LDS", "ITTS_NO_CONV_ACT"):
        monkeypatch.delenv(env, raising=False)

    def call(la=P, lb=P, filt=P, lens=P, mul=1, **kw):
        g = A.block(**kw)
        return lib.itts_act_conv_len(C.byref(g), la, lb, filt, lens, mul, None)

    assert lib.itts_act_conv_supported(C.byref(A.block())) == 1  # the block itself is valid
    assert b"null args" in refused(lib, lib.itts_act_conv_len(None, P, P, P, P, 1, None), "itts_act_conv_len")
    assert b"null pointer" in refused(lib, call(lens=None), "itts_act_conv_len")
    for bad in (0, -2):
        assert b"mul < 1" in refused(lib, call(mul=bad), "itts_act_conv_len")
    # ... and the refusals of itts_act_conv, with its reasons
    for k in ("A", "W", "C"):
        assert b"null pointer" in refused(lib, call(**{k: None}), "itts_act_conv_len")
    for k in ("la", "lb", "filt"):
        assert b"null pointer" in refused(lib, call(**{k: None}), "itts_act_conv_len")
    assert b"force_simple" in refused(lib, call(force_simple=1), "itts_act_conv_len")
    for k in ("dtype_a", "dtype_w", "dtype_c"):
        assert b"dtype" in refused(lib, call(**{k: L.F32}), "itts_act_conv_len")
    assert b"lda != Cin" in refused(lib, call(lda=32), "itts_act_conv_len")
    for kw in (dict(T=255, M=510), dict(Cin=104, lda=104), dict(N=20), dict(pad_mode=1), dict(taps=2), dict(taps=3, dil=33), dict(nphase=2),
               dict(in_up=2), dict(ldc=28), dict(A=P + 2)):
        assert b"itts_gemm_which != 4" in refused(lib, call(**kw), "itts_act_conv_len"), kw
    monkeypatch.setenv("ITTS_NO_CONV_ACT", "1")
    assert b"ITTS_NO_CONV_ACT" in refused(lib, call(), "itts_act_conv_len")


@pytest.mark.parametrize("half", HALVES)
def test_bigvgan_ragged_refuses_a_null_engine(half):
    lib = L.load(half)
    assert b"null engine" in refused(lib, lib.itts_bigvgan_ragged(None, P, P, 2, 8, P, P, None), "itts_bigvgan_ragged")
