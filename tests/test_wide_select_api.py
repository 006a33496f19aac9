"""No GPU: the three C entry points of the sort-free whole-vocabulary samplers, the operator entries' refusals before any device
call, the Python options, the flag.  (An engine object needs a device: that ITTS_WIDE_SELECT overrides the setter in both
directions is checked in tests/test_gpu_wide_select_engine.py.)"""
import inspect
import os
import re

import numpy as np
import pytest

from itts_hip import lib


def test_entry_points():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "itts_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint\s+itts_gpt_set_wide_select\s*\(\s*itts_engine\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", hdr)
    for half in ("bf16", "f16"):
        l = lib.load(half)
        for name, twin in (("itts_sample_rows_select", "itts_sample_rows"), ("itts_beam_sample_rows_select", "itts_beam_sample_rows")):
            fn, old = getattr(l, name), getattr(l, twin)
            assert name in lib.exported_symbols() and fn.restype is lib.i32 and list(fn.argtypes) == list(old.argtypes)
            assert len(fn.argtypes) == (17 if twin == "itts_sample_rows" else 25)
        assert l.itts_gpt_set_wide_select.restype is lib.i32 and len(l.itts_gpt_set_wide_select.argtypes) == 2
        assert l.itts_gpt_set_wide_select(None, 1) < 0 and b"null engine" in l.itts_last_error()
        assert l.itts_abi_version() == 4


@pytest.mark.parametrize("twin", [0, 1])
def test_entries_refuse_what_their_twins_refuse(twin):
    """Host memory that nothing reads: every case is refused before any device call, by name."""
    l, hp = lib.load(), np.zeros(64, dtype=np.float32).ctypes.data
    name = ("itts_sample_rows", "itts_sample_rows_select")[twin]
    ok = [hp, hp, hp, None, 1, 1024, 1.0, 5, 0, 0, 0, 0.8, 1.0, hp, hp, 1024 + 16, None]
    for at, bad in ((0, None), (1, None), (2, None), (13, None), (14, None), (4, 0), (5, 0), (7, -1), (7, 1024), (14, hp + 2), (15, 1039)):
        a = list(ok)
        a[at] = bad
        assert getattr(l, name)(*a) == -1 and l.itts_last_error().startswith(name.encode() + b": bad arguments"), (at, bad)
    name = ("itts_beam_sample_rows", "itts_beam_sample_rows_select")[twin]
    ok = [hp, hp, hp, hp, hp, hp, 4, 2, hp, 1, 3, 1025, 1.0, 5, 0, 6, 1, 0, 0, 0.8, 1.0, hp, hp, (3 * 1026 + 1) * 4, None]
    for at, bad in ((0, None), (3, None), (4, None), (8, None), (21, None), (22, None), (9, 0), (7, -1), (5, None), (6, 1), (22, hp + 2),
                    (10, 1), (10, 11), (11, 1), (11, 16385), (13, 1025), (15, -1), (16, 1025), (19, 0.0), (20, 0.0), (23, 3 * 1026 * 4)):
        a = list(ok)
        a[at] = bad
        assert getattr(l, name)(*a) == -1 and l.itts_last_error().startswith(name.encode() + b": "), (at, bad)


def test_python_options_and_flag():
    from indextts import cli
    from indextts.infer import IndexTTS
    from itts_hip import engine as ieng
    for fn, name, default in ((ieng.Engine.set_wide_select, "on", True), (ieng.build_engine, "wide_select", False),
                              (IndexTTS.__init__, "wide_select", False)):
        assert inspect.signature(fn).parameters[name].default is default
    parser = cli.build_parser()
    assert [parser.parse_args(["hello", "-v", "voice.wav"] + f).wide_select for f in ([], ["--wide-select"])] == [False, True]
