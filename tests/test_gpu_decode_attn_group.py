"""The grouped cache attention under beams (csrc/decode_attn_group.hip) through itts_decode_attn_group, with the fixture of
tests/test_gpu_decode_attn.py: its `launch` (append to the bit, every other cache byte, guards, NaN / Inf) gets an adapter that forwards
to the grouped entry.  The Call's caches are the PHYSICAL rows (a seed per row, poison outside the item's [kv_start, pos)), beam q's
history is K[base + anc[q][j], h, j]; reference: fp64 softmax over that gathered history plus the row's rounded k / v.  H = 3,
Smax = 300; S at a wave's 32-key tile, the four-wave deal of 128 and one past each; entries at >= pos are 255, the dead parity half
holds another valid ancestry.  Bounds: the existing file's for a 16-bit ctx.  Maxima: decode_attn_group_ops.txt under ITTS_TEST_OUT."""
import os
import types

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_attn import MEASURED, Call, ancestry, ibits, judge, launch

SMAX, H = 300, 3
S_EDGES = [1, 2, 31, 32, 33, 127, 128, 129, 161, 257, 300]
PAIRS = sorted({(S, ks) for S in S_EDGES for ks in (0, 31, 33, S - 1) if ks <= S - 1})
KINDS = ["identity", "trunk", "tail1", "tail5", "tail40", "scattered", "pair"]


def Grouped(lib):  # the grouped entry behind the name `launch` calls: its arguments without the two partial buffers
    return types.SimpleNamespace(itts_last_error=lib.itts_last_error, itts_decode_attn=lambda *a: lib.itts_decode_attn_group(*a[:14], *a[16:]))


def problem(pairs, nb, kind, half=torch.bfloat16):
    """items (S, kv_start) of nb beams -> the Call (its reference replaced by the gathered one), the ancestry table [2][B][Smax].
    Kinds: identity (nb passes per tile), trunk (one random row per position for all beams), tailD (the trunk with the last D
    positions scattered), scattered, pair (two beams share a row, the others differ)"""
    rows = [(S, ks, (S * 2003 + ks) * 64 + q) for S, ks in pairs for q in range(nb)]
    c = Call("bf16", rows, H=H, half=half, Smax=SMAX)
    B, items = c.B, len(pairs)
    scat = ancestry(c, nb, f"dag.{kind}.{nb}.{pairs[0]}")
    lead = scat.view(items, nb, SMAX)[:, :1].expand(-1, nb, -1).reshape(B, SMAX)
    if kind == "identity":
        true = (torch.arange(B) % nb)[:, None].expand(B, SMAX).clone()
    elif kind in ("scattered", "pair"):
        true = scat.clone()
        if kind == "pair":
            true.view(items, nb, SMAX)[:, 1] = true.view(items, nb, SMAX)[:, 0]
    else:  # the trunk, and its last d positions scattered
        true, d = lead.clone(), int(kind[4:] or 0) if kind != "trunk" else 0
        for b in range(B):
            true[b, max(c.pos[b] - d, 0):c.pos[b]] = scat[b, max(c.pos[b] - d, 0):c.pos[b]]
    other = ancestry(c, nb, f"dag.other.{nb}")
    anc = torch.empty(2, B, SMAX, dtype=torch.uint8)
    K, V, j = c.K.double(), c.V.double(), torch.arange(SMAX)
    for b in range(B):
        t = true[b].clone()
        t[c.pos[b]:] = 255
        anc[c.len[b] & 1, b], anc[1 - (c.len[b] & 1), b] = t.to(torch.uint8), other[b].to(torch.uint8)
        src = b // nb * nb + true[b]
        q, vis = c.qkv[b, 0].double() / 8, (j >= c.ks[b]) & (j < c.pos[b])
        sc = torch.einsum("hd,jhd->hj", q, K[src, :, j]).masked_fill(~vis, float("-inf"))
        w = torch.softmax(torch.cat([sc, (q * c.knew[b].double()).sum(-1)[:, None]], 1), -1)
        c.ref[b] = (torch.einsum("hj,jhd->hd", w[:, :-1], V[src, :, j]) + w[:, -1:] * c.vnew[b].double()).reshape(-1)
    return c, anc


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    lines = [f"{k:<36s} max relerr {e:9.3e}   bound {b:.1e}" for k, (e, b) in sorted(MEASURED.items()) if k.startswith("group ")]
    out = os.environ.get("ITTS_TEST_OUT")
    if out and lines:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_attn_group_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb", [2, 3, 4, 10])
def test_group_against_fp64(nb, kind):
    # every (S, kv_start) pair, dealt to launches of three items and of one; the first launch twice: the same bits
    g, i, first = Grouped(L.load()), 0, None
    while i < len(PAIRS):
        n = 3 if (i // 3) % 2 == 0 else 1
        c, anc = problem(PAIRS[i:i + n], nb, kind)
        o = launch(g, c, anc=anc, nb=nb)
        judge(c, o, f"group nb={nb} {kind}")
        if first is None:
            first = launch(g, c, anc=anc, nb=nb)
            assert torch.equal(ibits(first.ctx), ibits(o.ctx)), (nb, kind, "two runs differ")
        i += n


@pytest.mark.gpu
def test_ieee_half_library():
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    c, anc = problem([(257, 33), (129, 0), (32, 31)], 3, "tail5", half=torch.float16)
    judge(c, launch(Grouped(L.load("f16")), c, anc=anc, nb=3), "group nb=3 tail5 [IEEE half]")


@pytest.mark.gpu
@pytest.mark.parametrize("items", [1, 6])
def test_tiled_ctx_and_item_alone(items):
    # ctx in MFMA-fragment tiles (3 and 18 rows) = the row-major ctx; an item alone = that item among the others, bit for bit
    g = Grouped(L.load())
    pairs = [(300, 33), (128, 0), (33, 31), (161, 0), (65, 40), (257, 31)][:items]
    c, anc = problem(pairs, 3, "tail5")
    plain = launch(g, c, anc=anc, nb=3)
    judge(c, plain, "group nb=3 tiled / alone")
    assert torch.equal(ibits(launch(g, c, anc=anc, nb=3, tiled=1).ctx), ibits(plain.ctx)), items
    for it in range(min(items, 3)):
        ca, _ = problem(pairs[it:it + 1], 3, "tail5")
        assert ca.prefix == c.prefix
        alone = launch(g, ca, anc=anc[:, 3 * it:3 * it + 3].contiguous(), nb=3)
        assert torch.equal(ibits(alone.ctx), ibits(plain.ctx[3 * it:3 * it + 3])), (items, it)


def test_entry_refuses_what_the_kernel_does_not_have():
    # host only: every refusal comes back with its message before any launch (the host buffer is never read)
    lib, hp = L.load(), np.zeros(64, dtype=np.float32).ctypes.data
    h, f, e = L.BF16, L.F32, L.FP8  # (to, tc, dh, B, tiled, anc, nb, message)
    cases = [(h, h, 32, 6, 0, hp, 3, b"head dim must be 64"), (h, h, 64, 7, 0, hp, 3, b"B must be a multiple of nb"),
             (h, h, 64, 6, 0, hp, 1, b"needs 2 <= nb <= 16"), (h, h, 64, 34, 0, hp, 17, b"needs 2 <= nb <= 16"),
             (h, f, 64, 6, 0, hp, 3, b"the cache must be the 16-bit type"), (h, e, 64, 6, 0, hp, 3, b"the cache must be the 16-bit type"),
             (f, h, 64, 6, 0, hp, 3, b"ctx must be the 16-bit type"), (f, h, 64, 6, 1, hp, 3, b"tiled ctx is the 16-bit type only"),
             (h, h, 64, 6, 0, None, 3, b"the beam ancestry is missing")]
    for to, tc, dh, B, tiled, anc, nb, msg in cases:
        st = lib.itts_decode_attn_group(hp, to, hp, hp, hp, hp, hp, hp, B, 3, dh, 128, tc, tiled, anc, nb, None)
        assert st != 0 and msg in lib.itts_last_error(), (to, tc, dh, B, tiled, nb, st, lib.itts_last_error())
    st = lib.itts_decode_attn_group(None, L.BF16, hp, hp, hp, hp, hp, hp, 6, 3, 64, 128, L.BF16, 0, hp, 3, None)
    assert st != 0 and b"itts_decode_attn_group: bad arguments" in lib.itts_last_error()
