"""No GPU: the grouped attention's key split - its C entry points, the entry's refusals before any launch, the rule, the Python options."""
import inspect

import numpy as np
import pytest

from itts_hip import lib


def test_entry_points_and_rule():
    for half in ("bf16", "f16"):
        l = lib.load(half)
        for name, nargs in (("itts_decode_attn_group_split", 20), ("itts_gpt_set_group_attn_split", 2), ("itts_group_attn_split_rule", 2)):
            fn = getattr(l, name)
            assert name in lib.exported_symbols() and fn.restype is lib.i32 and len(fn.argtypes) == nargs
        assert l.itts_gpt_set_group_attn_split(None, 1) < 0 and b"null engine" in l.itts_last_error()  # a status, not a crash
        for H in (1, 3, 16, 20):
            for items in range(1, 140):
                ns = l.itts_group_attn_split_rule(H, items)
                assert 1 <= ns <= 8 and (ns == 1 or H * items < 128), (H, items, ns)


def test_entry_refuses_what_the_kernel_does_not_have():
    l, hp = lib.load(), np.zeros(64, dtype=np.float32).ctypes.data
    h, f, e = lib.BF16, lib.F32, lib.FP8  # (tc, dh, B, nb, nsplit, part_o, part_ml, message)
    cases = [(h, 64, 6, 3, 1, hp, hp, b"needs 2 <= nsplit <= 8"), (h, 64, 6, 3, 9, hp, hp, b"needs 2 <= nsplit <= 8"),
             (h, 64, 6, 3, 2, None, hp, b"the partial workspaces are missing"), (h, 64, 6, 3, 2, hp, None, b"the partial workspaces are missing"),
             (e, 64, 6, 3, 2, hp, hp, b"the cache must be the 16-bit type"), (f, 64, 6, 3, 2, hp, hp, b"the cache must be the 16-bit type"),
             (h, 32, 6, 3, 2, hp, hp, b"head dim must be 64"), (h, 64, 7, 3, 2, hp, hp, b"B must be a multiple of nb")]
    for tc, dh, B, nb, ns, po, pml, msg in cases:
        st = l.itts_decode_attn_group_split(hp, h, hp, hp, hp, hp, hp, hp, B, 3, dh, 128, tc, 0, hp, nb, ns, po, pml, None)
        assert st != 0 and b"decode_attn_group_split" in l.itts_last_error() and msg in l.itts_last_error(), (tc, dh, B, nb, ns, st, l.itts_last_error())
    st = l.itts_decode_attn_group_split(None, h, hp, hp, hp, hp, hp, hp, 6, 3, 64, 128, h, 0, hp, 3, 2, hp, hp, None)
    assert st != 0 and b"itts_decode_attn_group_split: bad arguments" in l.itts_last_error()


def test_python_options_and_flag():
    from indextts import cli
    from indextts.infer import IndexTTS
    from itts_hip import engine as ieng

    assert inspect.signature(ieng.Engine.set_group_attn_split).parameters["n"].default == 1
    assert inspect.signature(ieng.build_engine).parameters["group_attn_split"].default == 0
    assert inspect.signature(IndexTTS.__init__).parameters["group_attn_split"].default == 0
    with pytest.raises(ValueError, match="group_attn_split needs group_attn=True"):  # before anything touches a device or a checkpoint
        IndexTTS(model_dir="/nonexistent", cfg=object(), group_attn_split=1)
    parser = cli.build_parser()
    assert parser.parse_args(["hello", "-v", "voice.wav"]).group_attn_split == 0
    assert parser.parse_args(["hello", "-v", "voice.wav", "--group-attn-split"]).group_attn_split == 1
    assert parser.parse_args(["hello", "-v", "voice.wav", "--group-attn-split", "4"]).group_attn_split == 4
