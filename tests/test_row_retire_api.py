"""No GPU: the public surface of the opt-in row retirement of a batched decode (itts_gpt_retire_rows / itts_gpt_rows, the operator
entry itts_rows_move and the plan itts_retire_plan), the plan against a restatement, and what itts_rows_move refuses before it
touches the device."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from itts_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = ("bf16", "f16")


def header():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        return f.read()


def test_entry_points():
    h = header()
    assert re.search(r"\bint\s+itts_gpt_retire_rows\s*\(\s*itts_engine\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_gpt_rows\s*\(\s*itts_engine\s*\*\s*\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_rows_move\s*\(\s*void\s*\*\s*base\s*,\s*size_t\s+outer_stride\s*,\s*int\s+n_outer\s*,\s*size_t\s+row_stride\s*,"
                     r"\s*size_t\s+chunk_stride\s*,\s*int\s+n_chunks\s*,\s*size_t\s+chunk_bytes\s*,\s*const\s+int\s*\*\s*src_host\s*,"
                     r"\s*const\s+int\s*\*\s*dst_host\s*,\s*int\s+n_moves\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_retire_plan\s*\(\s*const\s+int\s*\*\s*unfinished_host\s*,\s*int\s+B\s*,\s*int\s*\*\s*n_live\s*,"
                     r"\s*int\s*\*\s*src_host\s*,\s*int\s*\*\s*dst_host\s*,\s*int\s*\*\s*n_moves\s*\)\s*;", h)
    for name, nargs in (("itts_gpt_retire_rows", 3), ("itts_gpt_rows", 1), ("itts_rows_move", 11), ("itts_retire_plan", 6)):
        assert name in lib.exported_symbols()
        for half in HALVES:
            fn = getattr(lib.load(half), name)
            assert callable(fn) and len(fn.argtypes) == nargs and fn.restype is lib.i32
    for half in HALVES:
        assert lib.load(half).itts_abi_version() == 4  # additions: the ABI version stays


def test_python_options():
    from itts_hip import engine as ieng

    assert list(inspect.signature(ieng.Engine.retire_rows).parameters) == ["self"]
    assert list(inspect.signature(ieng.Engine.rows).parameters) == ["self"]
    assert inspect.signature(ieng.Engine.generate).parameters["retire_rows"].default is None
    assert "retire_rows" in inspect.signature(ieng.Engine._generate_once).parameters  # passed through the hand-off redo

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["retire_rows"].default is None

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav"]).retire_rows is None
    assert p.parse_args(["hello", "-v", "voice.wav", "--retire-rows", "0.75"]).retire_rows == 0.75


def plan_restated(unf):
    """The plan in ten lines: the live rows at slots >= n go to the dead slots < n, both ascending."""
    live = [b for b, u in enumerate(unf) if u]
    n = len(live)
    src = [b for b in live if b >= n]
    dst = [b for b in range(n) if not unf[b]]
    assert len(src) == len(dst)
    return n, src, dst


def plan(l, unf):
    B = len(unf)
    u = np.ascontiguousarray(unf, dtype=np.int32)
    src, dst = np.full(max(B, 1), -7, np.int32), np.full(max(B, 1), -7, np.int32)
    n, m = C.c_int(-1), C.c_int(-1)
    st = l.itts_retire_plan(u.ctypes.data_as(C.c_void_p), B, C.byref(n), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                            C.byref(m))
    assert st == 0
    assert np.all(src[m.value:] == -7) and np.all(dst[m.value:] == -7)  # nothing written behind the lists
    return n.value, src[: m.value].tolist(), dst[: m.value].tolist()


def check_plan(l, unf):
    n, src, dst = plan(l, unf)
    assert (n, src, dst) == plan_restated(unf), unf
    assert n == sum(1 for u in unf if u) and len(src) == len(dst)
    assert all(s >= n and unf[s] for s in src) and all(d < n and not unf[d] for d in dst)
    assert src == sorted(src) and dst == sorted(dst)
    assert not set(src) & set(dst)


@pytest.mark.parametrize("half", HALVES)
def test_retire_plan_exhaustive_and_seeded(half):
    l = lib.load(half)
    for B in range(1, 11):
        for unf in itertools.product((0, 1), repeat=B):
            check_plan(l, unf)
    rng = np.random.default_rng(5)
    for B in (64, 128):
        for p in (0.1, 0.5, 0.9):
            for _ in range(20):
                check_plan(l, (rng.random(B) < p).astype(int).tolist())
        check_plan(l, [1] * B)
        check_plan(l, [0] * B)
    check_plan(l, [0, 0, 5, -1])  # any non-zero flag is a live row
    n, m = C.c_int(), C.c_int()
    assert l.itts_retire_plan(None, 4, C.byref(n), None, None, C.byref(m)) == -1  # ITTS_E_INVALID


def move(l, base=0x1000, outer_stride=4096, n_outer=1, row_stride=256, chunk_stride=64, n_chunks=2, chunk_bytes=64, src=(7, 8), dst=(1, 4),
         n_moves=None):
    s, d = np.asarray(src, np.int32), np.asarray(dst, np.int32)
    return l.itts_rows_move(base, outer_stride, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes, s.ctypes.data_as(C.c_void_p),
                            d.ctypes.data_as(C.c_void_p), len(src) if n_moves is None else n_moves, None)


@pytest.mark.parametrize("half", HALVES)
def test_rows_move_refusals(half):
    """Every one of these is refused with ITTS_E_INVALID before any HIP call: the base is not device memory, and no GPU is here."""
    l = lib.load(half)
    E_INVALID = -1
    assert move(l, base=None) == E_INVALID
    assert b"null base" in l.itts_last_error()
    assert move(l, n_outer=-1) == E_INVALID
    assert move(l, n_chunks=-1) == E_INVALID
    assert move(l, n_moves=-1) == E_INVALID
    assert b"negative" in l.itts_last_error()
    many = list(range(129))
    assert move(l, src=[200 + i for i in many], dst=many, row_stride=8, chunk_stride=4, chunk_bytes=4) == E_INVALID
    assert b"128" in l.itts_last_error()
    assert move(l, src=(7, 8), dst=(1, 7)) == E_INVALID  # a row is read and written
    assert b"intersect" in l.itts_last_error()
    assert move(l, src=(3,), dst=(3,)) == E_INVALID
    assert move(l, src=(7, 8), dst=(1, 1)) == E_INVALID  # one destination twice
    assert move(l, chunk_bytes=65) == E_INVALID
    assert b"chunk_bytes > chunk_stride" in l.itts_last_error()
    assert move(l, n_chunks=5) == E_INVALID  # 5 * 64 > 256
    assert b"n_chunks * chunk_stride > row_stride" in l.itts_last_error()
    assert move(l, src=(7, -1), dst=(1, 4)) == E_INVALID
    assert move(l, n_outer=2, outer_stride=8 * 256) == E_INVALID  # row 8 of layer 0 would be row 0 of layer 1
