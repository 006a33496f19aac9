"""No GPU: the public surface of the fp8 mode of the persistent decode engine - the C entry point (exported by both builds of
the library and declared in the header), the Python options and the command-line flag."""
import inspect
import os
import re

from itts_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_fp8_public_surface():
    assert "itts_gpt_set_engine_fp8" in lib.exported_symbols()
    for half in ("bf16", "f16"):
        assert callable(getattr(lib.load(half), "itts_gpt_set_engine_fp8"))
    assert lib.load().itts_abi_version() == 4  # an addition: the ABI version stays
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        assert re.search(r"\bint\s+itts_gpt_set_engine_fp8\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", f.read())

    from itts_hip import engine as ieng

    assert "on" in inspect.signature(ieng.Engine.set_engine_fp8).parameters
    assert inspect.signature(ieng.build_engine).parameters["engine_fp8"].default is False

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["gpt_fp8"].default is False

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav", "--gpt-fp8"]).gpt_fp8 is True
    assert p.parse_args(["hello", "-v", "voice.wav"]).gpt_fp8 is False
