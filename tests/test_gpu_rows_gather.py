"""Operator-level tests of rows_gather_kernel (csrc/decode_rows.hip) through the C ABI entry itts_rows_gather: the out-of-place row
gather behind the retirement of finished beam groups - row j of every destination plane takes row src_rows[j] of the same source
plane.

Reference: a numpy gather on a copy of the buffer.  EVERY byte of the buffer has to be equal afterwards: the gathered rows, the
source, the guard bytes in front of and behind the destination block of every plane.  The buffer holds seeded random bytes, so a
copy from a wrong place does not pass by chance.

row_bytes 1920 / 308 / 77 take the 16-, 4- and 1-byte copy unit (1920 = max_gen 480 ids, 77: an ancestry row of an arbitrary
Smax); one plane and two planes with different source and destination plane strides; 1, 9 and 128 rows in an unsorted order; bases
that force the narrower units on a 1920-byte row (in single bytes it spans two 256-thread x 4-unit tiles).  The last test runs the
two launches by which the
engine takes the live half 1 of a [2][rows][row] ping-pong array from base rows_old * row to base rows_new * row."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_gemv import stream, sync

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64  # bytes around each destination plane's block that must stay; a multiple of 16
SRC_ROWS = 160


def lib_of(half):
    if half == "f16" and not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    return L.load(half)


def up(x, unit):
    return (x + unit - 1) // unit * unit


def gather(lib, buf, dst_off, dps, src_off, sps, n_planes, row_bytes, rows):
    r = np.asarray(rows, np.int32)
    st = lib.itts_rows_gather(buf.data_ptr() + dst_off, dps, buf.data_ptr() + src_off, sps, n_planes, row_bytes, r.ctypes.data_as(C.c_void_p),
                              len(r), stream())
    assert st == 0, lib.itts_last_error()


def gather_ref(want, host, dst_off, dps, src_off, sps, n_planes, row_bytes, rows):
    for p in range(n_planes):
        for j, r in enumerate(rows):
            a = src_off + p * sps + r * row_bytes
            b = dst_off + p * dps + j * row_bytes
            want[b:b + row_bytes] = host[a:a + row_bytes]


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("n_planes", [1, 2])
@pytest.mark.parametrize("n_rows", [1, 9, 128])
@pytest.mark.parametrize("row_bytes", [1920, 308, 77])
def test_rows_gather_every_byte(half, n_planes, n_rows, row_bytes):
    lib = lib_of(half)
    unit = 16 if row_bytes % 16 == 0 else 4 if row_bytes % 4 == 0 else 1
    rows = np.random.default_rng(n_rows).permutation(SRC_ROWS)[:n_rows].tolist()  # unsorted, no row twice
    assert n_rows == 1 or rows != sorted(rows)
    # the destination planes: a block of n_rows rows and GUARD bytes on either side of it; the source planes a different stride apart
    dps = up(n_rows * row_bytes, unit) + 2 * GUARD
    sps = SRC_ROWS * row_bytes + 5 * unit
    dst_off = GUARD
    src_off = up(dst_off + n_planes * dps, 16)
    total = src_off + n_planes * sps + GUARD
    host = np.random.default_rng(7).integers(0, 256, total, dtype=np.uint8)
    want = host.copy()
    gather_ref(want, host, dst_off, dps, src_off, sps, n_planes, row_bytes, rows)
    buf = torch.from_numpy(host).to(DEV)
    gather(lib, buf, dst_off, dps, src_off, sps, n_planes, row_bytes, rows)
    sync()
    got = buf.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0]) - dst_off} from the destination"
    assert np.count_nonzero(want != host) > 0.9 * n_planes * n_rows * row_bytes  # (random bytes: 1 in 256 coincides)


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_rows_gather_bases_not_16_byte_aligned(half):
    """row_bytes a multiple of 16, the source base only of 4, then the destination base of nothing: the narrower units take them."""
    lib = lib_of(half)
    row, rows = 1920, [5, 0, 3]
    for shift_d, shift_s in ((0, 4), (1, 0)):
        dst_off, src_off = GUARD + shift_d, 2 * GUARD + 16 + 3 * row + shift_s
        host = np.random.default_rng(9).integers(0, 256, src_off + 8 * row + GUARD, dtype=np.uint8)
        want = host.copy()
        gather_ref(want, host, dst_off, 0, src_off, 0, 1, row, rows)
        buf = torch.from_numpy(host).to(DEV)
        gather(lib, buf, dst_off, 0, src_off, 0, 1, row, rows)
        sync()
        assert np.array_equal(buf.cpu().numpy(), want)


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("row_bytes", [77, 1920])
def test_parity_one_sequence_15_to_9_rows(half, row_bytes):
    """[2][15][row]: 5 groups of 3 beams, groups 0, 2 and 4 live, the live data in half 1 (rows 15 .. 29).  After the retirement
    half 1 is rows [9, 18) - it overlaps the old half 1, where group 0's live rows 15 .. 17 sit, so one launch cannot do it (the
    host check refuses that launch: tests/test_beam_retire_api.py).  The engine's two launches: old half 1 -> [0, 9) of the dead half
    0, then [0, 9) -> [9, 18).  The new half 1 must be the numpy gather of the live rows; nothing outside rows [0, 18) changes."""
    lib = lib_of(half)
    old, new = 15, 9
    live = [g * 3 + q for g in (0, 2, 4) for q in range(3)]
    host = np.random.default_rng(11).integers(0, 256, GUARD + 2 * old * row_bytes + GUARD, dtype=np.uint8)
    arr = host[GUARD:GUARD + 2 * old * row_bytes].reshape(2 * old, row_bytes)
    want_half1 = arr[[old + r for r in live]].copy()
    buf = torch.from_numpy(host).to(DEV)
    gather(lib, buf, GUARD, 0, GUARD, 0, 1, row_bytes, [old + r for r in live])
    gather(lib, buf, GUARD + new * row_bytes, 0, GUARD, 0, 1, row_bytes, list(range(new)))
    sync()
    got = buf.cpu().numpy()
    rows = got[GUARD:GUARD + 2 * old * row_bytes].reshape(2 * old, row_bytes)
    assert np.array_equal(rows[new:2 * new], want_half1)
    assert np.array_equal(rows[:new], want_half1)  # (the staging block)
    assert np.array_equal(rows[2 * new:], arr[2 * new:])
    assert np.array_equal(got[:GUARD], host[:GUARD]) and np.array_equal(got[-GUARD:], host[-GUARD:])
