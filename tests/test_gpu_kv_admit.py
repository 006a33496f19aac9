"""Operator-level tests of the two row-admission kernels (csrc/decode_admit.hip) through their C ABI entries.

itts_kv_admit: the k and v thirds of an admission prefill's qkv [n][S][3 * H * dh] go to positions 0 .. S - 1 of chosen rows of
caches [Bcache][H][Smax][dh].  The reference is itts_kv_scatter on the same rows: the admitted rows must hold its bytes, bit for
bit, for every (tq, tc) pair in both libraries, and every other byte of both caches - the rows of the other slots, positions
S .. Smax - 1 of the admitted ones, a guard block behind each cache - must keep its sentinel.  The caches start from a byte
pattern that differs from byte to byte, so a write to a wrong place cannot land on an equal value.

itts_rows_admit: every byte of every state array against a numpy model of rows_admit_kernel, the other slots unchanged."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_gemv import rnd, stream, sync
from test_gpu_kv_scatter import EDGES, PAIRS, half_dtype, tdt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMAX, DH = 256, 64
# H, cache rows, S, the slots (n = their count): ascending, descending, with the last slot; S = 1 (one position), 5, 70 (past one
# 64-lane wave of 16-byte chunks per (row, head) run)
CASES = [(2, 3, 1, [2]), (2, 3, 5, [0, 2]), (2, 3, 70, [2, 0]), (20, 3, 1, [1, 2]), (20, 7, 5, [6, 4, 3, 1, 0]),
         (20, 7, 70, [0, 2, 3, 5, 6]), (20, 7, 70, [3])]


def pattern(nbytes, seed):
    """bytes that differ from their neighbours and from row to row"""
    return torch.from_numpy(((np.arange(nbytes, dtype=np.int64) * 37 + seed * 101 + 11) % 251).astype(np.uint8))


def ints(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("tq,tc", PAIRS)
@pytest.mark.parametrize("H,rows,S,slots", CASES)
def test_kv_admit_equals_kv_scatter(half, tq, tc, H, rows, S, slots):
    if half == "f16" and not os.path.exists(L.LIB_PATH_F16):
        pytest.fail("libitts_hip_f16.so was not built")
    lib = L.load(half)
    hd = half_dtype(lib)
    n, D = len(slots), H * DH
    qkv = rnd(f"kva.{H}.{S}.{n}", (n, S, 3, H, DH))
    qkv[:, :, 1, :, :8] = EDGES
    qkv[:, :, 2, :, :8] = EDGES.flip(0)
    qd = qkv.to(tdt(tq, hd)).reshape(n, S, 3 * D).contiguous().to(DEV)
    ces = tdt(tc, hd).itemsize
    row_bytes = H * SMAX * DH * ces
    guard = SMAX * DH * ces
    sl = np.asarray(slots, dtype=np.int32)
    got, want = [], []
    for which in (0, 1):
        start = pattern(rows * row_bytes + guard, which + 1)
        got.append(start.clone().to(DEV))
        # the reference: itts_kv_scatter over the n rows, on a buffer that starts from the bytes of the slots they go to
        ref = torch.cat([start[s * row_bytes:(s + 1) * row_bytes] for s in slots]).to(DEV)
        want.append((start, ref))
    L.check(lib.itts_kv_scatter(want[0][1].data_ptr(), want[1][1].data_ptr(), qd.data_ptr(), n, S, H, DH, SMAX, tq, tc, stream()),
            "kv_scatter", lib)
    L.check(lib.itts_kv_admit(got[0].data_ptr(), got[1].data_ptr(), qd.data_ptr(), n, S, H, DH, SMAX, rows, tq, tc, ints(sl), stream()),
            "kv_admit", lib)
    sync()
    for name, g, (start, ref) in zip("KV", got, want):
        g, ref = g.cpu(), ref.cpu()
        expect = start.clone()
        for i, s in enumerate(slots):
            expect[s * row_bytes:(s + 1) * row_bytes] = ref[i * row_bytes:(i + 1) * row_bytes]
        assert not torch.equal(expect, start)  # the reference wrote something
        bad = torch.nonzero(g != expect).flatten()
        assert bad.numel() == 0, (name, f"{bad.numel()} bytes differ, the first at {int(bad[0])} "
                                        f"(slot {int(bad[0]) // row_bytes}, position {int(bad[0]) % (SMAX * DH * ces) // (DH * ces)})")


def test_kv_admit_full_heads_fp32_chunks():
    """dh = 4: one 16-byte chunk per run of an fp32 cache (the smallest run the kernel takes)"""
    lib = L.load()
    n, S, H, dh, Smax, rows = 2, 3, 3, 4, 8, 4
    qkv = rnd("kva.small", (n, S, 3 * H * dh)).contiguous().to(DEV)
    sl = np.asarray([3, 1], dtype=np.int32)
    got = [torch.full((rows + 1, H, Smax, dh), 0.75, device=DEV) for _ in range(2)]
    L.check(lib.itts_kv_admit(got[0].data_ptr(), got[1].data_ptr(), qkv.data_ptr(), n, S, H, dh, Smax, rows, L.F32, L.F32, ints(sl),
                              stream()), "kv_admit", lib)
    sync()
    q = qkv.cpu().view(n, S, 3, H, dh)
    for which in (1, 2):
        want = torch.full((rows + 1, H, Smax, dh), 0.75)
        for i, s in enumerate(sl):
            want[s, :, :S] = q[i, :, which].permute(1, 0, 2)
        assert torch.equal(got[which - 1].cpu(), want)


@pytest.mark.parametrize("B,V,mg,slots,with_src", [(3, 37, 5, [2], True), (7, 8194, 32, [6, 0, 3], True), (7, 30, 600, [1, 5], False),
                                                   (12, 1000, 33, [11, 10, 4, 2, 0], True)])
def test_rows_admit_every_byte(B, V, mg, slots, with_src):
    """V above and below max_gen, one and several slots, the last slot; with and without the forced / uniforms sources."""
    lib = L.load()
    n = len(slots)
    rng = np.random.default_rng(B * 1000 + V)
    host = dict(seen=rng.integers(0, 256, (B, V), dtype=np.uint8), unfinished=rng.integers(0, 2, B).astype(np.int32),
                cur_tok=rng.integers(0, V, B).astype(np.int32), len=rng.integers(0, mg, B).astype(np.int32),
                kv_start=rng.integers(0, 40, B).astype(np.int32), ids=rng.integers(0, V, (B, mg)).astype(np.int32),
                forced=rng.integers(-1, V, (B, mg)).astype(np.int32), uniforms=rng.random((mg, B), dtype=np.float32))
    fsrc = rng.integers(-1, V, (n, mg)).astype(np.int32)
    usrc = rng.random((n, mg), dtype=np.float32)
    kvs = rng.integers(0, 40, n).astype(np.int32)
    sl = np.asarray(slots, dtype=np.int32)
    fake, start_tok, stop = 1, V - 2, V - 1
    dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in host.items()}
    fs, us = torch.from_numpy(fsrc).to(DEV), torch.from_numpy(usrc).to(DEV)
    a = L.RowsAdmitArgs(**{k: v.data_ptr() for k, v in dev.items()}, forced_src=fs.data_ptr() if with_src else None,
                        uniforms_src=us.data_ptr() if with_src else None, slots_host=sl.ctypes.data, kv_start_host=kvs.ctypes.data,
                        n=n, B=B, V=V, max_gen=mg, fake_id=fake, start_tok=start_tok, stop=stop)
    L.check(lib.itts_rows_admit(C.byref(a), stream()), "rows_admit", lib)
    sync()
    want = {k: v.copy() for k, v in host.items()}
    for i, s in enumerate(slots):
        want["seen"][s] = 0
        want["seen"][s, [fake, start_tok]] = 1
        want["unfinished"][s], want["cur_tok"][s], want["len"][s], want["kv_start"][s] = 1, start_tok, 0, kvs[i]
        want["ids"][s] = stop
        want["forced"][s] = fsrc[i] if with_src else -1
        if with_src:
            want["uniforms"][:, s] = usrc[i]
    for k, v in want.items():
        g = dev[k].cpu().numpy()
        assert np.array_equal(g.view(np.uint8), v.view(np.uint8)), (k, np.argwhere(g != v)[:4].tolist())
