"""No GPU: the grouped fp8-cache attention's two C entry points, the entry's refusals before any launch, the Python options, the flag."""
import inspect
import os
import re

import numpy as np
import pytest

from itts_hip import lib


def test_entry_points():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "itts_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+itts_gpt_set_group_attn_kv_fp8\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+itts_decode_attn_group_kv8\s*\(\s*void\s*\*\s*ctx\s*,[^;]*const\s+uint8_t\s*\*\s*anc\s*,\s*int\s+nb\s*,[^;]*\)\s*;", hdr)
    for half in ("bf16", "f16"):
        l = lib.load(half)
        for name, nargs in (("itts_gpt_set_group_attn_kv_fp8", 2), ("itts_decode_attn_group_kv8", 17)):
            fn = getattr(l, name)
            assert name in lib.exported_symbols() and fn.restype is lib.i32 and len(fn.argtypes) == nargs
        assert l.itts_gpt_set_group_attn_kv_fp8(None, 1) < 0 and b"null engine" in l.itts_last_error()  # a status, not a crash


def test_entry_refuses_what_the_kernel_does_not_have():
    l, hp = lib.load(), np.zeros(64, dtype=np.float32).ctypes.data
    h, f, e = lib.BF16, lib.F32, lib.FP8  # (to, tc, dh, B, anc, nb, message)
    cases = [(h, h, 64, 6, hp, 3, b"the cache must be the fp8 (e4m3) type"), (h, f, 64, 6, hp, 3, b"the cache must be the fp8 (e4m3) type"),
             (f, e, 64, 6, hp, 3, b"ctx must be the 16-bit type"), (h, e, 32, 6, hp, 3, b"head dim must be 64"),
             (h, e, 64, 6, hp, 1, b"needs 2 <= nb <= 16"), (h, e, 64, 34, hp, 17, b"needs 2 <= nb <= 16"),
             (h, e, 64, 7, hp, 3, b"B must be a multiple of nb"), (h, e, 64, 6, None, 3, b"the beam ancestry is missing")]
    for to, tc, dh, B, anc, nb, msg in cases:
        st = l.itts_decode_attn_group_kv8(hp, to, hp, hp, hp, hp, hp, hp, B, 3, dh, 128, tc, 0, anc, nb, None)
        assert st != 0 and b"decode_attn_group_kv8" in l.itts_last_error() and msg in l.itts_last_error(), (to, tc, dh, B, nb, st, l.itts_last_error())
    st = l.itts_decode_attn_group_kv8(None, h, hp, hp, hp, hp, hp, hp, 6, 3, 64, 128, e, 0, hp, 3, None)
    assert st != 0 and b"itts_decode_attn_group_kv8: bad arguments" in l.itts_last_error()


def test_python_options_and_flag():
    from indextts import cli
    from indextts.infer import IndexTTS
    from itts_hip import engine as ieng

    assert inspect.signature(ieng.Engine.set_group_attn_kv_fp8).parameters["on"].default is True
    assert inspect.signature(ieng.build_engine).parameters["group_attn_kv_fp8"].default is False
    assert inspect.signature(IndexTTS.__init__).parameters["group_attn_kv_fp8"].default is False
    for kw in (dict(group_attn=True), dict(kv_fp8=True), dict()):  # before anything touches a device or a checkpoint
        with pytest.raises(ValueError, match="group_attn_kv_fp8=True needs group_attn=True and kv_fp8=True"):
            IndexTTS(model_dir="/nonexistent", cfg=object(), group_attn_kv_fp8=True, **kw)
    parser = cli.build_parser()
    assert parser.parse_args(["hello", "-v", "voice.wav"]).group_attn_kv_fp8 is False
    assert parser.parse_args(["hello", "-v", "voice.wav", "--group-attn-kv-fp8"]).group_attn_kv_fp8 is True
