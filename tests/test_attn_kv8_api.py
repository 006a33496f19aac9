"""No GPU: the e4m3 cache attention's three C entry points, the operator entry's refusals before any launch, the Python options, the
flag.  (An engine object needs a device: that ITTS_ATTN_KV8=0 overrides the setter is checked in tests/test_gpu_attn_kv8_engine.py.)"""
import inspect
import os
import re

import numpy as np
import pytest

from itts_hip import lib


def test_entry_points():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "itts_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+itts_gpt_set_attn_kv8\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+itts_gpt_attn_kv8_used\s*\(\s*itts_engine\s*\*\s*\w*\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+itts_decode_attn_kv8\s*\(\s*void\s*\*\s*ctx\s*,[^;]*const\s+uint8_t\s*\*\s*anc\s*,\s*int\s+nb\s*,[^;]*\)\s*;", hdr)
    for half in ("bf16", "f16"):
        l = lib.load(half)
        for name, nargs in (("itts_gpt_set_attn_kv8", 2), ("itts_gpt_attn_kv8_used", 1), ("itts_decode_attn_kv8", 17)):
            fn = getattr(l, name)
            assert name in lib.exported_symbols() and fn.restype is lib.i32 and len(fn.argtypes) == nargs
        assert l.itts_gpt_set_attn_kv8(None, 1) < 0 and b"null engine" in l.itts_last_error() and l.itts_gpt_attn_kv8_used(None) == -1


def test_entry_refuses_what_the_kernel_does_not_have():
    l, buf = lib.load(), np.zeros(64, dtype=np.float32)
    hp = buf.ctypes.data + buf.ctypes.data % 16  # (numpy aligns to 8 at least) 16-byte aligned host memory that nothing reads
    h, f, e = lib.BF16, lib.F32, lib.FP8  # (to, tc, dh, B, kc, tiled, anc, nb, message)
    cases = [(h, h, 64, 6, hp, 0, None, 1, b"the cache must be the fp8 (e4m3) type"), (f, f, 64, 6, hp, 0, None, 1, b"the cache must be the fp8 (e4m3) type"),
             (h, e, 32, 6, hp, 0, None, 1, b"head dim must be 64"), (h, e, 64, 6, hp + 8, 0, None, 1, b"16-byte aligned"),
             (f, e, 64, 6, hp, 1, None, 1, b"tiled ctx is 16-bit only"), (h, e, 64, 6, hp, 0, hp, 0, b"1 <= nb <= 16"),
             (h, e, 64, 34, hp, 0, hp, 17, b"1 <= nb <= 16"), (h, e, 64, 7, hp, 0, hp, 3, b"B to be a multiple of")]
    for to, tc, dh, B, kc, tiled, anc, nb, msg in cases:
        st = l.itts_decode_attn_kv8(hp, to, hp, kc, hp, hp, hp, hp, B, 3, dh, 128, tc, tiled, anc, nb, None)
        assert st != 0 and b"decode_attn_kv8" in l.itts_last_error() and msg in l.itts_last_error(), (to, tc, dh, B, nb, st, l.itts_last_error())
    for null in range(7):  # ctx, qkv, kc, vc, len, kv_start, prefix
        p = [hp] * 7
        p[null] = None
        st = l.itts_decode_attn_kv8(p[0], h, p[1], p[2], p[3], p[4], p[5], p[6], 6, 3, 64, 128, e, 0, None, 1, None)
        assert st != 0 and b"itts_decode_attn_kv8: bad arguments" in l.itts_last_error(), null


def test_python_options_and_flag():
    from indextts import cli
    from indextts.infer import IndexTTS
    from itts_hip import engine as ieng
    for fn, name, default in ((ieng.Engine.set_attn_kv8, "on", True), (ieng.build_engine, "attn_kv8", False), (IndexTTS.__init__, "attn_kv8", False)):
        assert inspect.signature(fn).parameters[name].default is default
    with pytest.raises(ValueError, match="attn_kv8=True needs kv_fp8=True"):  # before anything touches a device or a checkpoint
        IndexTTS(model_dir="/nonexistent", cfg=object(), attn_kv8=True)
    parser = cli.build_parser()
    assert parser.parse_args(["hello", "-v", "voice.wav"]).attn_kv8 is False and parser.parse_args(["hello", "-v", "voice.wav", "--attn-kv8"]).attn_kv8 is True
