"""The grouped cache attention on the e4m3 K/V cache (csrc/decode_attn_group.hip) through itts_decode_attn_group_kv8, with the
fixture of tests/test_gpu_decode_attn_fp8.py (`launch`: append to the byte, other cache bytes, guards, no NaN byte, finite ctx; finite
winning poison) behind an adapter.  The Call's caches are the PHYSICAL rows, beam q's history is K[base + anc[q][j], h, j]; reference:
fp64 softmax over that gathered history from the stored e4m3 values plus the row's rounded k / v.  Unit U = 64 positions; entries at
>= pos are 255, the dead parity half holds another valid ancestry.  Maxima: decode_attn_group_kv8_ops.txt under ITTS_TEST_OUT."""
import os
import types

import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_attn import ancestry
from test_gpu_decode_attn_fp8 import FORMS, MEASURED, Call, bits, judge, launch

SMAX, H, U = 300, 3, 64
PAIRS = sorted({(S, ks) for S in (1, 2, U - 1, U, U + 1, 2 * U + 1, 4 * U - 1, 4 * U, 4 * U + 1, 300) for ks in (0, U - 1, U + 1, S - 1) if ks <= S - 1})
KINDS = ["identity", "trunk", "tail1", "tail5", "tail70", "scattered", "pair"]


def Grouped(lib):  # the new entry behind the names `launch` / `judge` call: its arguments without the two partial buffers
    return types.SimpleNamespace(itts_last_error=lib.itts_last_error, itts_half_is_f16=lib.itts_half_is_f16,
                                 itts_decode_attn=lambda *a: lib.itts_decode_attn_group_kv8(*a[:14], *a[16:]))


def problem(pairs, nb, kind):
    # items (S, kv_start) of nb beams -> the Call (its reference replaced by the gathered one), the ancestry table [2][B][Smax]
    c = Call(FORMS["fp8"], [(S, ks, (S * 2003 + ks) * 64 + q) for S, ks in pairs for q in range(nb)], H=H, Smax=SMAX)
    B, items = c.B, len(pairs)
    scat = ancestry(c, nb, f"dag8.{kind}.{nb}.{pairs[0]}")
    if kind == "identity":
        true = (torch.arange(B) % nb)[:, None].expand(B, SMAX).clone()
    elif kind in ("scattered", "pair"):
        true = scat.clone()
        if kind == "pair":
            true.view(items, nb, SMAX)[:, 1] = true.view(items, nb, SMAX)[:, 0]
    else:
        true, d = scat.view(items, nb, SMAX)[:, :1].expand(-1, nb, -1).reshape(B, SMAX).clone(), int(kind[4:] or 0) if kind != "trunk" else 0
        for b in range(B):
            true[b, max(c.pos[b] - d, 0):c.pos[b]] = scat[b, max(c.pos[b] - d, 0):c.pos[b]]
    other = ancestry(c, nb, f"dag8.other.{nb}")
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
    lines = [f"{k:<36s} max relerr {e:9.3e}   dims 8..63 of a head {t:9.3e}   bound {b:.1e}"
             for k, (e, t, b) in sorted(MEASURED.items()) if k.startswith("group8 ")]
    out = os.environ.get("ITTS_TEST_OUT")
    if out and lines:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_attn_group_kv8_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb", [2, 3, 4, 10])
def test_group_kv8_against_fp64(nb, kind):
    g, i, first = Grouped(L.load()), 0, None
    while i < len(PAIRS):
        n = 3 if (i // 3) % 2 == 0 else 1
        c, anc = problem(PAIRS[i:i + n], nb, kind)
        o = launch(g, c, L.BF16, anc=anc, nb=nb)
        judge(g, c, o, f"group8 nb={nb} {kind}", L.BF16)
        if first is None:
            first = launch(g, c, L.BF16, anc=anc, nb=nb)
            assert torch.equal(bits(first.ctx), bits(o.ctx)), (nb, kind, "two runs differ")
        i += n


@pytest.mark.gpu
def test_ieee_half_library():
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    g, (c, anc) = Grouped(L.load("f16")), problem([(257, 65), (129, 0), (64, 63)], 3, "tail5")
    judge(g, c, launch(g, c, L.BF16, anc=anc, nb=3), "group8 nb=3 tail5 [IEEE half]", L.BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("items", [1, 6])
def test_tiled_ctx_and_item_alone(items):
    g = Grouped(L.load())
    pairs = [(300, 65), (256, 0), (65, 63), (129, 0), (70, 40), (257, 63)][:items]
    c, anc = problem(pairs, 3, "tail5")
    plain = launch(g, c, L.BF16, anc=anc, nb=3)
    judge(g, c, plain, "group8 nb=3 tiled / alone", L.BF16)
    assert torch.equal(bits(launch(g, c, L.BF16, anc=anc, nb=3, tiled=1).ctx), bits(plain.ctx)), items
    for it in range(min(items, 3)):
        ca, _ = problem(pairs[it:it + 1], 3, "tail5")
        assert ca.prefix == c.prefix
        alone = launch(g, ca, L.BF16, anc=anc[:, 3 * it:3 * it + 3].contiguous(), nb=3)
        assert torch.equal(bits(alone.ctx), bits(plain.ctx[3 * it:3 * it + 3])), (items, it)
