"""No GPU: the public surface of the opt-in grouped cache attention under beams - the C entry points (header, both builds, lib.py, a
status for a NULL engine), the Python options and the command-line flag.  Additions: the ABI version stays."""
import inspect
import os
import re

import pytest

from itts_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_attn_entry_points():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+itts_gpt_set_group_attn\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+itts_gpt_group_attn_used\s*\(\s*itts_engine\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+itts_decode_attn_group\s*\(\s*void\s*\*\s*ctx\s*,[^;]*const\s+uint8_t\s*\*\s*anc\s*,\s*int\s+nb\s*,[^;]*\)\s*;", hdr)
    for half in ("bf16", "f16"):
        l = lib.load(half)
        assert l.itts_abi_version() == 4
        for name, nargs in (("itts_gpt_set_group_attn", 2), ("itts_gpt_group_attn_used", 1), ("itts_decode_attn_group", 17)):
            fn = getattr(l, name)
            assert name in lib.exported_symbols() and fn.restype is lib.i32 and len(fn.argtypes) == nargs
        assert l.itts_gpt_set_group_attn(None, 1) < 0 and b"null engine" in l.itts_last_error()  # a status, not a crash
        assert l.itts_gpt_group_attn_used(None) == -1


def test_group_attn_python_options_and_flag():
    from indextts import cli
    from indextts.infer import IndexTTS
    from itts_hip import engine as ieng

    p = inspect.signature(ieng.Engine.set_group_attn).parameters
    assert list(p) == ["self", "on"] and p["on"].default is True and callable(ieng.Engine.group_attn_used)
    assert inspect.signature(ieng.build_engine).parameters["group_attn"].default is False
    assert inspect.signature(IndexTTS.__init__).parameters["group_attn"].default is False
    with pytest.raises(ValueError, match="group_attn=True needs is_fp16=True"):  # before anything touches a device or a checkpoint
        IndexTTS(model_dir="/nonexistent", cfg=object(), group_attn=True, is_fp16=False)
    parser = cli.build_parser()
    assert parser.parse_args(["hello", "-v", "voice.wav"]).group_attn is False
    assert parser.parse_args(["hello", "-v", "voice.wav", "--group-attn"]).group_attn is True
