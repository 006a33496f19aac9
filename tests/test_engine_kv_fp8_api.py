"""No GPU: the public surface of the opt-in "fp8 K/V cache on the persistent decode engine" switch - the C entry point (declared in
the header, exported by both builds of the library, bound in lib.py, a status for a NULL engine), the Python options and the
command-line flag.  All of it is an addition: the ABI version stays."""
import inspect
import os
import re

import pytest

from itts_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "itts_gpt_set_engine_kv_fp8"


def test_engine_kv_fp8_entry_point():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", f.read())
    assert NAME in lib.exported_symbols()
    for half in ("bf16", "f16"):
        l = lib.load(half)
        fn = getattr(l, NAME)
        assert callable(fn) and fn.restype is lib.i32 and len(fn.argtypes) == 2
        assert l.itts_abi_version() == 4  # an addition: the ABI version stays
        for on in (0, 1):
            assert fn(None, on) < 0  # a NULL engine: a status, not a crash
        assert b"null engine" in l.itts_last_error()


def test_engine_kv_fp8_python_options():
    from itts_hip import engine as ieng

    p = inspect.signature(ieng.Engine.set_engine_kv_fp8).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    b = inspect.signature(ieng.build_engine).parameters
    assert b["engine_kv_fp8"].default is False and b["kv_fp8"].default is False

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["engine_kv_fp8"].default is False
    # a mode of the fp8 cache: refused without it, before anything touches a device or a checkpoint
    with pytest.raises(ValueError, match="engine_kv_fp8=True needs kv_fp8=True"):
        IndexTTS(model_dir="/nonexistent", cfg=object(), engine_kv_fp8=True)
    with pytest.raises(ValueError, match="engine_kv_fp8=True needs kv_fp8=True"):
        IndexTTS(model_dir="/nonexistent", cfg=object(), engine_kv_fp8=True, kv_fp8=False, gpt_fp8=True)


def test_engine_kv_fp8_command_line_flag():
    from indextts import cli

    p = cli.build_parser()
    a = p.parse_args(["hello", "-v", "voice.wav"])
    assert a.engine_kv_fp8 is False and a.kv_fp8 is False
    a = p.parse_args(["hello", "-v", "voice.wav", "--kv-fp8"])
    assert a.kv_fp8 is True and a.engine_kv_fp8 is False  # the fp8 cache alone keeps today's behaviour
    a = p.parse_args(["hello", "-v", "voice.wav", "--kv-fp8", "--engine-kv-fp8"])
    assert a.kv_fp8 is True and a.engine_kv_fp8 is True
