"""No GPU: the public surface of the opt-in fp8 (e4m3) K/V cache - the two C entry points (declared in the header, exported by both
builds of the library, bound in lib.py), the dtype code, the Python options and the command-line flag."""
import inspect
import os
import re

from itts_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        return f.read()


def test_kv_fp8_entry_points():
    h = header()
    assert re.search(r"\bint\s+itts_gpt_set_kv_fp8\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_kv_scatter\s*\(\s*void\s*\*\s*kc\s*,\s*void\s*\*\s*vc\s*,\s*const\s+void\s*\*\s*qkv\s*,\s*int\s+B\s*,\s*int\s+S\s*,"
                     r"\s*int\s+H\s*,\s*int\s+dh\s*,\s*int\s+Smax\s*,\s*int\s+tq\s*,\s*int\s+tc\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"^#define\s+ITTS_FP8\s+4\b", h, re.M) and lib.FP8 == 4
    for name in ("itts_gpt_set_kv_fp8", "itts_kv_scatter"):
        assert name in lib.exported_symbols()
        for half in ("bf16", "f16"):
            fn = getattr(lib.load(half), name)
            assert callable(fn) and fn.argtypes is not None and fn.restype is lib.i32
    assert len(lib.load().itts_kv_scatter.argtypes) == 11 and len(lib.load().itts_gpt_set_kv_fp8.argtypes) == 2
    for half in ("bf16", "f16"):
        assert lib.load(half).itts_abi_version() == 4  # additions: the ABI version stays


def test_kv_fp8_python_options():
    from itts_hip import engine as ieng

    p = inspect.signature(ieng.Engine.set_kv_fp8).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True
    assert inspect.signature(ieng.build_engine).parameters["kv_fp8"].default is False

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["kv_fp8"].default is False

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav", "--kv-fp8"]).kv_fp8 is True
    a = p.parse_args(["hello", "-v", "voice.wav"])
    assert a.kv_fp8 is False and a.gpt_fp8 is False
    a = p.parse_args(["hello", "-v", "voice.wav", "--kv-fp8", "--gpt-fp8"])
    assert a.kv_fp8 is True and a.gpt_fp8 is True
