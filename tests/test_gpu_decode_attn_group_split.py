"""The grouped cache attention with a key split (csrc/decode_attn_group.hip) through itts_decode_attn_group_split, on the
fixture of tests/test_gpu_decode_attn_group.py (`problem`: physical rows, poison outside [kv_start, pos), fp64 reference over the
gathered history) and the `launch` / `judge` of tests/test_gpu_decode_attn.py (append to the bit, every other cache byte, guards,
NaN / Inf; fp64 agreement at 2^-8 / 2^-10; only the appended key visible -> the rounded v to the bit).  The adapter allocates the
two workspaces with one guard slot behind each.  H = 3, Smax = 300: 0 to 10 tiles, a first tile that is not tile 0, chunk edges,
and at NS = 8 splits with nothing to do."""
import functools
import os

import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_attn import DEV, SENT, ibits, judge, launch
from test_gpu_decode_attn_group import PAIRS, problem

cached = functools.lru_cache(maxsize=None)(lambda pairs, nb, kind, half=torch.bfloat16: problem(list(pairs), nb, kind, half))


class Split:
    """the split entry behind the name `launch` calls; keeps the partials of the last call in .po [NS, B, H, 64] / .pml [NS, B, H, 2]"""

    def __init__(self, lib, ns):
        self.lib, self.ns, self.itts_last_error = lib, ns, lib.itts_last_error

    def itts_decode_attn(self, *a):
        B, H, n = a[8], a[9], self.ns * a[8] * a[9]
        po, pml = torch.full((n + 1, 64), float("nan")), torch.full((n + 1, 2), float("nan"))
        po[n], pml[n] = SENT, SENT
        po, pml = po.to(DEV), pml.to(DEV)
        st = self.lib.itts_decode_attn_group_split(*a[:14], *a[16:18], self.ns, po.data_ptr(), pml.data_ptr(), a[18])
        torch.cuda.synchronize()
        po, pml = po.cpu(), pml.cpu()
        assert bool((po[n] == SENT).all()) and bool((pml[n] == SENT).all()), "the guard slot behind a workspace was written"
        assert st != 0 or not (bool(torch.isnan(po).any()) or bool(torch.isnan(pml).any())), "a (z, b, h) slot was not written"
        self.po, self.pml = po[:n].view(self.ns, B, H, 64), pml[:n].view(self.ns, B, H, 2)
        return st


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["identity", "tail5", "scattered"])
@pytest.mark.parametrize("nb", [2, 3, 10])
@pytest.mark.parametrize("ns", [2, 3, 8])
def test_split_against_fp64(ns, nb, kind):
    # every (S, kv_start) pair, dealt to launches of three items and of one; the first launch twice: the same bits
    g, i, first = Split(L.load(), ns), 0, None
    while i < len(PAIRS):
        n = 3 if (i // 3) % 2 == 0 else 1
        c, anc = cached(tuple(PAIRS[i:i + n]), nb, kind)
        o = launch(g, c, anc=anc, nb=nb)
        judge(c, o, f"group split NS={ns} nb={nb} {kind}")
        if first is None:
            first = launch(g, c, anc=anc, nb=nb)
            assert torch.equal(ibits(first.ctx), ibits(o.ctx)), (ns, nb, kind, "two runs differ")
        i += n


@pytest.mark.gpu
def test_split_without_a_key_writes_minus_inf_zero_zeros():
    # S = 33: one tile of cache keys, so at NS = 8 only split 0 owns any (and, with kv_start = pos, only the appended one)
    g = Split(L.load(), 8)
    c, anc = cached(((33, 0), (33, 31), (33, 32)), 3, "tail5")
    judge(c, launch(g, c, anc=anc, nb=3), "group split NS=8 empty splits")
    m, l = g.pml[..., 0], g.pml[..., 1]
    assert bool((m[1:] == float("-inf")).all()) and bool((l[1:] == 0).all()) and bool((g.po[1:] == 0).all())
    assert bool(torch.isfinite(m[0]).all()) and bool((l[0] >= 1).all())
    assert bool((l[0, 6:] == 1).all()) and torch.equal(g.po[0, 6:].reshape(3, -1), c.vnew[6:].float().reshape(3, -1))  # kv_start = pos


@pytest.mark.gpu
def test_ieee_half_library():
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    c, anc = cached(((257, 33), (129, 0), (32, 31)), 3, "tail5", torch.float16)
    judge(c, launch(Split(L.load("f16"), 3), c, anc=anc, nb=3), "group split NS=3 nb=3 tail5 [IEEE half]")


@pytest.mark.gpu
@pytest.mark.parametrize("items", [1, 6])
def test_tiled_ctx_and_item_alone(items):
    # ctx in MFMA-fragment tiles (3 and 18 rows) = the row-major ctx; an item alone = that item among the others, bit for bit
    g = Split(L.load(), 3)
    pairs = ((300, 33), (128, 0), (33, 31), (161, 0), (65, 40), (257, 31))[:items]
    c, anc = cached(pairs, 3, "tail5")
    plain = launch(g, c, anc=anc, nb=3)
    judge(c, plain, "group split NS=3 tiled / alone")
    assert torch.equal(ibits(launch(g, c, anc=anc, nb=3, tiled=1).ctx), ibits(plain.ctx)), items
    for it in range(min(items, 3)):
        ca, _ = cached(pairs[it:it + 1], 3, "tail5")
        assert ca.prefix == c.prefix
        alone = launch(g, ca, anc=anc[:, 3 * it:3 * it + 3].contiguous(), nb=3)
        assert torch.equal(ibits(alone.ctx), ibits(plain.ctx[3 * it:3 * it + 3])), (items, it)
