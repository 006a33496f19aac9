"""Operator-level tests of the prefill's K/V cache write (csrc/decode.hip kv_scatter_kernel) through the C ABI entry
itts_kv_scatter: qkv [B][S][3 * H * dh] -> rows 0 .. S - 1 of each [Smax][dh] block of the caches, rounded to the cache type.

Every (tq, tc) pair the entry accepts - fp32 -> fp32, 16-bit -> 16-bit, fp32 -> fp8, 16-bit -> fp8 - in both libraries.  The written
rows equal torch's cast bit for bit (for the e4m3 cache: x.clamp(-448, 448).to(torch.float8_e4m3fn), round to nearest even after the
clamp, subnormals included); k and v carry the e4m3 ties and edge values and +-500 in their first dims.  Rows S .. Smax - 1 and
the [Smax][dh] guard block behind each cache keep their sentinel bytes.  Refusals are checked on the CPU: a status and a message
before any launch (the host buffer is never read)."""
import os

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_gemv import rnd, stream, sync

DEV = "cuda:0"
# e4m3 (3 mantissa bits, subnormal step 2^-9): 1 + 2^-4 and 1 + 3 * 2^-4 lie midway between two values (nearest even: down, up), 2^-10
# midway between 0 and the smallest subnormal (-> 0), 3 * 2^-10 between 2^-9 and 2^-8 (-> 2^-8); 460 rounds to 448 = the largest
# value, 500 and -1e4 are clamped to it
EDGES = torch.tensor([1 + 2.0 ** -4, -(1 + 3 * 2.0 ** -4), 2.0 ** -10, 3 * 2.0 ** -10, 460.0, 500.0, -500.0, -1e4])
SHAPES = [(2, 5, 3, 64, 9), (1, 4, 3, 64, 4)]  # B, S, H, dh, Smax


def e4m3(x):
    """the cache's rounding: clamp, then torch's round-to-nearest-even cast"""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def test_e4m3_rounding_of_the_edge_values():
    """the fixture itself: what torch's clamp-and-cast gives for the ties and edge values (a plain cast turns 500 into NaN)"""
    got = e4m3(EDGES).float().tolist()
    assert got == [1.0, -1.25, 0.0, 2.0 ** -8, 448.0, 448.0, -448.0, -448.0], got
    assert bool(torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all())
    assert e4m3(torch.zeros(3)).view(torch.uint8).tolist() == [0, 0, 0]  # the zero fill of a fresh cache is +0


def half_dtype(lib):
    return torch.float16 if lib.itts_half_is_f16() else torch.bfloat16


def tdt(code, half):
    return {L.F32: torch.float32, L.BF16: half, L.FP8: torch.float8_e4m3fn}[code]


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


PAIRS = [(L.F32, L.F32), (L.BF16, L.BF16), (L.F32, L.FP8), (L.BF16, L.FP8)]


@pytest.mark.gpu
@pytest.mark.parametrize("half", ["bf16", "f16"])
@pytest.mark.parametrize("tq,tc", PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kv_scatter_bits(half, tq, tc, shape):
    if half == "f16" and not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    lib = L.load(half)
    hd = half_dtype(lib)
    B, S, H, dh, Smax = shape
    D = H * dh
    qkv = rnd(f"kvs.{B}.{S}", (B, S, 3, H, dh))
    qkv[:, :, 1, :, :8] = EDGES
    qkv[:, :, 2, :, :8] = EDGES.flip(0)
    qkv[0, 0, 1, 0, 8:16] = -EDGES  # the other sign of every edge value
    q_in = qkv.to(tdt(tq, hd))  # what the kernel reads (the 16-bit input is itself rounded: +-500 and the ties are exact in it or not,
    src = q_in.float()          # the expectation starts from the values it holds)
    cdt = tdt(tc, hd)
    want_rows = e4m3(src) if tc == L.FP8 else src.to(cdt)  # [B, S, 3, H, dh]
    sent = torch.full((B * H + 1, Smax, dh), 0.75).to(cdt)  # 0.75 is exact in every cache type; the last block is the guard
    caches, wants = [], []
    for which in (1, 2):
        caches.append(sent.clone().to(DEV))
        w = sent.clone()
        w[:B * H].view(B, H, Smax, dh)[:, :, :S] = want_rows[:, :, which].permute(0, 2, 1, 3)
        wants.append(w)
    qd = q_in.reshape(B, S, 3 * D).contiguous().to(DEV)
    L.check(lib.itts_kv_scatter(caches[0].data_ptr(), caches[1].data_ptr(), qd.data_ptr(), B, S, H, dh, Smax, tq, tc, stream()),
            "kv_scatter", lib)
    sync()
    for name, got, want in zip("KV", caches, wants):
        got = got.cpu()
        assert torch.equal(bits(got[B * H]), bits(want[B * H])), (name, "the guard block behind the cache was written")
        g, w = got[:B * H].view(B, H, Smax, dh), want[:B * H].view(B, H, Smax, dh)
        assert torch.equal(bits(g[:, :, S:]), bits(w[:, :, S:])), (name, "rows S .. Smax - 1 were written")
        assert torch.equal(bits(g[:, :, :S]), bits(w[:, :, :S])), (name, "written rows differ from torch's cast")
        if tc == L.FP8:
            assert not bool(((bits(got) & 0x7F) == 0x7F).any()), (name, "a NaN byte in the e4m3 cache")


def test_kv_scatter_refusals():
    """Host only: null pointers, non-positive shapes, S > Smax and type pairs the kernel does not have come back with a status and a
    message before any launch (the host buffer is never read as device memory)."""
    lib = L.load()
    host = np.zeros(64, dtype=np.float32)
    hp = host.ctypes.data
    ok = dict(kc=hp, vc=hp, qkv=hp, B=2, S=5, H=3, dh=64, Smax=9, tq=L.F32, tc=L.FP8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.itts_kv_scatter(a["kc"], a["vc"], a["qkv"], a["B"], a["S"], a["H"], a["dh"], a["Smax"], a["tq"], a["tc"], None)

    for kw in (dict(kc=None), dict(vc=None), dict(qkv=None), dict(B=0), dict(S=0), dict(H=0), dict(dh=0), dict(Smax=0), dict(B=-1),
               dict(S=10), dict(S=5, Smax=4)):
        st = call(**kw)
        assert st != 0 and b"itts_kv_scatter: bad arguments" in lib.itts_last_error(), (kw, st, lib.itts_last_error())
    for tq, tc in ((L.F32, L.BF16), (L.BF16, L.F32), (L.FP8, L.FP8), (L.FP8, L.BF16), (L.F32, L.F16), (L.F16, L.FP8), (2, 2), (L.F32, 7)):
        st = call(tq=tq, tc=tc)
        assert st != 0 and b"itts_kv_scatter: type pair" in lib.itts_last_error(), (tq, tc, st, lib.itts_last_error())
