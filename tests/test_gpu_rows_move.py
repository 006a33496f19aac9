"""Operator-level tests of rows_move_kernel (csrc/decode_rows.hip) through the C ABI entry itts_rows_move: the three-level strided
row copy behind the row retirement of a batched decode.

Reference: a numpy gather on a copy of the buffer.  EVERY byte of the buffer has to be equal afterwards - the copied chunks, the
gaps between chunk_bytes and chunk_stride, the rows that are not a destination, the guard bytes in front of and behind the rows.
The buffer holds seeded random bytes, so a copy from a wrong place does not pass by chance.

Sizes cover the three copy units (16 / 4 / 1 bytes: chunk_bytes 16 and 4096 + 16; 4; 1, 3, 66 and 8194 = a `seen` row), chunks
shorter than, equal to and longer than one 256-thread x 4-unit tile with a ragged tail, one and several chunks and outer blocks,
a cache-shaped case in the three cache element sizes and a base that is 4- but not 16-byte aligned."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_gemv import stream, sync

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 9
MOVES = ((7, 1), (8, 4))
GUARD = 64  # bytes in front of and behind the rows; a multiple of 16, so the alignment of the rows is the allocation's


def lib_of(half):
    if half == "f16" and not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    return L.load(half)


def run_case(lib, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes, moves=MOVES, rows=ROWS, shift=0, seed=3):
    outer_stride = rows * row_stride
    total = GUARD + shift + n_outer * outer_stride + GUARD
    host = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
    want = host.copy()
    off = GUARD + shift
    for o in range(n_outer):
        for s, d in moves:
            for c in range(n_chunks):
                a = off + o * outer_stride + s * row_stride + c * chunk_stride
                b = off + o * outer_stride + d * row_stride + c * chunk_stride
                want[b:b + chunk_bytes] = host[a:a + chunk_bytes]
    buf = torch.from_numpy(host).to(DEV)
    src = np.asarray([m[0] for m in moves], np.int32)
    dst = np.asarray([m[1] for m in moves], np.int32)
    st = lib.itts_rows_move(buf.data_ptr() + off, outer_stride, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes,
                            src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), len(moves), stream())
    assert st == 0, lib.itts_last_error()
    sync()
    got = buf.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0]) - off} from the base"
    return int(np.count_nonzero(want != host))


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("n_outer", [1, 3])
@pytest.mark.parametrize("n_chunks", [1, 3])
@pytest.mark.parametrize("chunk_bytes", [1, 3, 4, 66, 8194, 16, 4096 + 16])
def test_rows_move_every_byte(half, n_outer, n_chunks, chunk_bytes):
    lib = lib_of(half)
    # chunk_stride > chunk_bytes, with the multiple the copy unit of this chunk size needs (16 / 4 / 1), and a row a little longer
    # than its chunks
    unit = 16 if chunk_bytes % 16 == 0 else 4 if chunk_bytes % 4 == 0 else 1
    chunk_stride = chunk_bytes + 3 * unit
    row_stride = n_chunks * chunk_stride + 2 * unit
    changed = run_case(lib, n_outer, row_stride, chunk_stride, n_chunks, chunk_bytes)
    assert changed > 0 or chunk_bytes < 4  # (random bytes: a few bytes can coincide, thousands do not)


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_rows_move_nothing_to_move(half):
    lib = lib_of(half)
    assert run_case(lib, 3, 3 * 80 + 32, 80, 3, 64, moves=()) == 0


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("ces", [1, 2, 4])
def test_rows_move_cache_shaped(half, ces):
    """[2 layers][9 rows][3 heads][Smax 256][dh 64] elements of 1 / 2 / 4 bytes, 77 positions of history: what lies behind them in
    the destination rows stays."""
    lib = lib_of(half)
    H, Smax, dh, pos = 3, 256, 64, 77
    head = Smax * dh * ces
    changed = run_case(lib, 2, H * head, head, H, pos * dh * ces)
    assert changed > 2 * len(MOVES) * H * pos * dh * ces * 0.98


@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_rows_move_base_not_16_byte_aligned(half):
    """Strides and chunk_bytes are multiples of 16, the base only of 4: the 4-byte path has to take it."""
    lib = lib_of(half)
    run_case(lib, 3, 3 * 4128 + 32, 4128, 3, 4096 + 16, shift=4)
    run_case(lib, 1, 3 * 80 + 32, 80, 3, 64, shift=1)  # ... and a base that is not even 4-byte aligned: bytes
