"""No GPU: the public surface of the opt-in retirement of finished beam groups (itts_gpt_set_retire_beams, the operator entry
itts_rows_gather), what itts_rows_gather refuses before it touches the device, and itts_retire_plan over group-uniform flags:
whole groups move into whole holes and a beam keeps its index inside its group."""
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
E_INVALID = -1


def header():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("half", HALVES)
def test_libraries_export_the_entry_points(half):
    l = lib.load(half)
    for name, nargs in (("itts_gpt_set_retire_beams", 2), ("itts_rows_gather", 9)):
        assert name in lib.exported_symbols()
        fn = getattr(l, name)
        assert callable(fn) and len(fn.argtypes) == nargs and fn.restype is lib.i32
    assert l.itts_abi_version() == 4  # additions: the ABI version stays


def test_header_declares_them():
    h = header()
    assert re.search(r"\bint\s+itts_gpt_set_retire_beams\s*\(\s*itts_engine\s*\*\s*\w+\s*,\s*int\s+on\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_rows_gather\s*\(\s*void\s*\*\s*dst\s*,\s*size_t\s+dst_plane_stride\s*,\s*const\s+void\s*\*\s*src\s*,"
                     r"\s*size_t\s+src_plane_stride\s*,\s*int\s+n_planes\s*,\s*size_t\s+row_bytes\s*,\s*const\s+int\s*\*\s*src_rows_host\s*,"
                     r"\s*int\s+n_rows\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert "ITTS_RETIRE_BEAMS" in h


def test_python_options_default_off():
    from itts_hip import engine as ieng

    assert list(inspect.signature(ieng.Engine.set_retire_beams).parameters) == ["self", "on"]
    assert inspect.signature(ieng.Engine.generate).parameters["retire_beams"].default is None
    assert inspect.signature(ieng.Engine._generate_once).parameters["retire_beams"].default is False  # through the hand-off redo
    assert inspect.signature(ieng.build_engine).parameters["retire_beams"].default is False

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["retire_beams"].default is None

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav"]).retire_beams is None
    assert p.parse_args(["hello", "-v", "voice.wav", "--retire-rows", "0.5", "--retire-beams"]).retire_beams is True


def gather(l, dst=0x100000, dst_plane_stride=0, src=0x200000, src_plane_stride=0, n_planes=1, row_bytes=64, rows=(3, 0, 7), n_rows=None):
    r = np.asarray(() if rows is None else rows, np.int32)
    return l.itts_rows_gather(dst, dst_plane_stride, src, src_plane_stride, n_planes, row_bytes,
                              r.ctypes.data_as(C.c_void_p) if rows is not None else None, len(r) if n_rows is None else n_rows, None)


@pytest.mark.parametrize("half", HALVES)
def test_rows_gather_refusals(half):
    """Every one of these is refused with ITTS_E_INVALID before any HIP call: the pointers are not device memory, and no GPU is
    here.  The addresses below are numbers only."""
    l = lib.load(half)
    assert gather(l, dst=None) == E_INVALID
    assert b"null pointer" in l.itts_last_error()
    assert gather(l, src=None) == E_INVALID
    assert gather(l, rows=None, n_rows=2) == E_INVALID
    assert b"null row list" in l.itts_last_error()
    assert gather(l, n_planes=-1) == E_INVALID
    assert gather(l, n_rows=-1) == E_INVALID
    assert b"negative" in l.itts_last_error()
    assert gather(l, rows=list(range(129)), row_bytes=4) == E_INVALID
    assert b"128" in l.itts_last_error()
    assert gather(l, rows=(3, -1)) == E_INVALID
    assert b"[0, 65536)" in l.itts_last_error()
    assert gather(l, rows=(3, 65536)) == E_INVALID
    assert gather(l, row_bytes=1 << 32) == E_INVALID
    # two destination planes of 3 x 64 bytes, 128 bytes apart: they would overlap each other
    assert gather(l, n_planes=2, dst_plane_stride=128, src_plane_stride=4096) == E_INVALID
    assert b"dst_plane_stride" in l.itts_last_error()
    # overlapping ranges.  In place: row 0 of the source is row 0 of the destination
    assert gather(l, dst=0x200000, rows=(5, 0)) == E_INVALID
    assert b"intersect" in l.itts_last_error()
    # the destination block [src + 1, src + 1 + 3 * 64) reaches one byte into source row 3 (rows 0 .. 2 are not read)
    assert gather(l, dst=0x200000 + 1, rows=(3, 4, 5)) == E_INVALID
    assert b"intersect" in l.itts_last_error()
    assert gather(l, src=0x100000 + 3 * 64 - 1 - 7 * 64, rows=(3, 0, 7)) == E_INVALID  # the first byte of source row 7 is the block's last
    assert b"intersect" in l.itts_last_error()
    # the engine's old half 1 -> new half 1 in ONE launch at 15 -> 9 rows: new rows [9, 18) against the old rows 15 .. 17
    base, row = 0x300000, 77
    live = [15 + r for r in (0, 1, 2, 6, 7, 8, 12, 13, 14)]
    assert gather(l, dst=base + 9 * row, src=base, row_bytes=row, rows=live) == E_INVALID
    assert b"intersect" in l.itts_last_error()
    # the second plane only: source plane 1 begins 32 bytes into destination plane 1 (plane 0 of each is clear of everything)
    assert gather(l, dst=0x400000, dst_plane_stride=4096, src=0x400000 + 1024, src_plane_stride=4096 - 1024 + 32, n_planes=2,
                  rows=(0,)) == E_INVALID
    assert b"intersect" in l.itts_last_error()


@pytest.mark.parametrize("half", HALVES)
def test_rows_gather_accepts_empty_launches(half):
    """Nothing to copy: accepted, and nothing is launched (no GPU is here)."""
    l = lib.load(half)
    assert gather(l, rows=(), n_rows=0) == 0
    assert gather(l, n_planes=0) == 0
    assert gather(l, row_bytes=0) == 0


def plan(l, flags):
    B = len(flags)
    u = np.ascontiguousarray(flags, dtype=np.int32)
    src, dst = np.full(B, -7, np.int32), np.full(B, -7, np.int32)
    n, m = C.c_int(-1), C.c_int(-1)
    assert l.itts_retire_plan(u.ctypes.data_as(C.c_void_p), B, C.byref(n), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                              C.byref(m)) == 0
    return n.value, src[: m.value].tolist(), dst[: m.value].tolist()


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("nb", [2, 3, 10])
def test_retire_plan_moves_whole_groups(half, nb):
    """Every done pattern of up to 6 items, each item's nb rows carrying its flag: the live count is a multiple of nb, every move
    takes (group, q) to (group', q), a group's nb moves are consecutive and go to one hole, and the groups keep their order."""
    l = lib.load(half)
    for items in range(1, 7):
        for done in itertools.product((0, 1), repeat=items):
            flags = [int(not d) for d in done for _ in range(nb)]
            n, src, dst = plan(l, flags)
            live_items = [i for i, d in enumerate(done) if not d]
            assert n == nb * len(live_items) and n % nb == 0 and len(src) % nb == 0
            for i, (s, d) in enumerate(zip(src, dst)):
                assert s % nb == d % nb == i % nb, (done, src, dst)
                assert s // nb == src[i - i % nb] // nb and d // nb == dst[i - i % nb] // nb
                assert not done[s // nb] and done[d // nb] and s >= n > d
            # the layout after the moves: n / nb live groups, contiguous
            slot = list(range(len(flags)))
            for s, d in zip(src, dst):
                slot[d] = s
            after = [slot[j] for j in range(n)]
            assert sorted(a // nb for a in after[::nb]) == live_items
            assert all(after[g * nb + q] == after[g * nb] + q for g in range(n // nb) for q in range(nb))
