"""Operator-level tests of the decode cache attention (csrc/decode_attn.hip decode_attn2_kernel, the per-key arithmetic of
csrc/itts_attn_dev.h) through the C ABI entry itts_decode_attn.

Reference: fp64 torch on the CPU from the SAME rounded inputs.  Per (row, head): q = the step's q (fp32) / 8; the keys
kv_start[b] <= j < pos = prefix[0] + len[b] exactly as the cache stores them, plus this step's k / v rounded to the cache type;
softmax, times V.  q has std 2, K and V std 1 (scores of std 2, as the split fixture of test_gpu_decode_gemv.py).

Poison, not zeros: every cache row outside [kv_start, pos) - the padding, the stale row at pos, every row up to Smax - 1 - holds a K
whose score lies 30 above the largest real score of its (row, head) and V = 1000: admitted with any weight it wrecks the result.
All of it is finite (the kernel's contract, step (e): rows past S are multiplied by p = 0).  Behind each cache lies one more
[Smax][64] block, behind ctx / part_o / part_ml one more row, filled with a sentinel; the test asserts 0 <= kv_start <= pos < Smax
on the host before every launch.

Forms (SLOTS rows per deal / blind rows U / register window W / stream step T), H = 3 unless stated:
  bf16         bf16 cache -> bf16 ctx, 1024 threads       128 / 256 / 768 / 256   Smax 1400
  bf16_f32ctx  bf16 cache -> fp32 ctx                      the same
  f32          fp32 cache -> fp32 ctx                       64 / 128 / 384 / 128   Smax 800
  split        4 x 256 threads, partials                    32 / 256 / 768 / 512   Smax 1400 (chunk u of split sp = rows (4u+sp)*32)
  many_bf16    256 threads, 8 pairs, B = 8, H = 64          32 /  64 / 512 / 128   Smax 700
  many_f32     the same on an fp32 cache                    16 /  32 / 256 /  64   Smax 400
  tiled ctx (bf16 form, B = 3 and 17, Smax 300); the beam ancestry (ANC) on each form with nb = 2, 3, 4.
S = pos + 1 takes 1, 2, SLOTS-1..+1, U-1..+1, W-1..+1, W+T-1..+1, W+2T+7 and Smax where they fit (33, 65, 97 too in the split form),
several in one launch as different len[b]; kv_start takes 0, 1, SLOTS-1..+1, a value past the window and pos.  prefix[0] = 5,
except in a launch that holds a row with pos < 5 (S = 1, 2 and their neighbours in that launch): its prefix[0] is 0.

Per call: (1) the result against fp64 per row - relerr < 2e-5 for fp32 ctx and for the fp64 merge of the split partials, < 2^-8 for
bf16 ctx (one ulp of the largest output: half for the store, the rest for fp32 arithmetic across a tie), 2^-10 for IEEE half; a
split without a visible key holds exactly (-inf, 0, zeros); a row whose only visible key is the appended one returns the rounded v
to the bit (its weight is exp(0) / exp(0)).  (2) The append to the bit: cache row pos = this step's k / v rounded to nearest even
(k and v carry exact ties in their first dims), every other byte of caches and guards unchanged, compared as integers.
(3) Bit-exact relations: bf16 ctx = the fp32 ctx rounded; tiled = row-major; a row alone = that row in a 2-, 3-, 4-row call; two
runs agree; ANC with the identity ancestry = plain; ANC over a scattered history (every position of every beam in a random
physical row of its item, the other parity holding another valid ancestry, entries at >= pos 255) = plain on the gathered cache.
Beams of one item share len, as in a generation (a beam's append may land in a row another beam of a different length reads).
(4) No NaN / Inf.

The measured maxima are printed and, where ITTS_TEST_OUT names a directory, written to decode_attn_ops.txt there (committed as
profiles/decode_attn_ops.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from itts_hip import prng
from test_gpu_decode_gemv import merge_partials, relerr, rnd, stream, sync
from test_gpu_ops import from_tiles

DEV = "cuda:0"
SENT = 777.0
NSPLIT = 4   # csrc/itts_decode.h ATTN_NSPLIT
PREFIX = 5
NPOOL, POOL_ROWS = 4, 1400
# exact ties of the 16-bit roundings in the first dims of the step's k and v: 1 + 2^-8 and 1 + 3 * 2^-8 lie midway between two
# bf16 values (nearest even: down, up), 1 + 2^-11 and 1 + 3 * 2^-11 between two binary16 values
TIES = torch.tensor([1 + 2.0 ** -8, -(1 + 3 * 2.0 ** -8), -(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11])

FORMS = {
    "bf16": dict(tc=L.BF16, to=L.BF16, split=0, SL=128, U=256, W=768, T=256, Smax=1400, B=0, H=3),
    "bf16_f32ctx": dict(tc=L.BF16, to=L.F32, split=0, SL=128, U=256, W=768, T=256, Smax=1400, B=0, H=3),
    "f32": dict(tc=L.F32, to=L.F32, split=0, SL=64, U=128, W=384, T=128, Smax=800, B=0, H=3),
    "split": dict(tc=L.BF16, to=L.F32, split=1, SL=32, U=256, W=768, T=512, Smax=1400, B=0, H=3),
    "many_bf16": dict(tc=L.BF16, to=L.BF16, split=0, SL=32, U=64, W=512, T=128, Smax=700, B=8, H=64),
    "many_f32": dict(tc=L.F32, to=L.F32, split=0, SL=16, U=32, W=256, T=64, Smax=400, B=8, H=64),
}


def s_edges(form):
    f = FORMS[form]
    SL, U, W, T = f["SL"], f["U"], f["W"], f["T"]
    vals = [1, 2, SL - 1, SL, SL + 1, U - 1, U, U + 1, W - 1, W, W + 1, W + T - 1, W + T, W + T + 1, W + 2 * T + 7, f["Smax"]]
    if f["split"]:
        vals += [33, 65, 97]  # only some splits own a key
    return sorted({s for s in vals if s <= f["Smax"]})


def ks_edges(form):
    """(S, kv_start) rows, ordered so that one launch mixes the values"""
    f = FORMS[form]
    SL, U, W, T = f["SL"], f["U"], f["W"], f["T"]
    Sa, Sb = U + 1, min(W + T + 1, f["Smax"])
    return [(Sa, 1), (Sb, SL), (Sa, Sa - 1), (Sb, W + 3), (Sa, SL - 1), (Sb, Sb - 1), (Sa, SL + 1), (Sb, 1), (2, 1), (Sa, SL),
            (W + 1, SL + 1), (SL + 1, SL)]


def deal(rows, B):
    """rows -> launches: B rows each where the form fixes B (the last one filled up with the rows before it), else 4, 3, 2, 1, 4, ..."""
    out, i, n = [], 0, 4
    while i < len(rows):
        k = B or n
        chunk = rows[i:i + k]
        if B and len(chunk) < B:
            chunk = rows[i - (B - len(chunk)):i] + chunk
        out.append(chunk)
        i += k
        n = n - 1 if n > 1 else 4
    return out


def half_of(lib):
    return torch.float16 if lib.itts_half_is_f16() else torch.bfloat16


def tdt(code, half):
    return torch.float32 if code == L.F32 else half


def ibits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- one launch's problem and its fp64 reference (CPU) --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(cdt):
    """a small pool of random [POOL_ROWS][64] blocks, rounded to the cache type and held as fp32 (the CPU is slow in 16-bit types);
    every (row, head) cache is one of them with its rows permuted and its dims signed"""
    return rnd("da.poolk", (NPOOL, POOL_ROWS, 64)).to(cdt).float(), rnd("da.poolv", (NPOOL, POOL_ROWS, 64)).to(cdt).float()


def head_data(seed, h, Smax):
    """Head h of the row problem `seed`, independent of the row it is placed in: the pool blocks and row permutations of its K and
    V cache, their signs [2][64], and the step's q, k, v [3][64]"""
    name = f"da.{seed}.{h}"
    u = prng.uniform(name + ".perm", 5, 2 * POOL_ROWS)
    pk = np.argsort(u[:POOL_ROWS], kind="stable")[:Smax]
    pv = np.argsort(u[POOL_ROWS:], kind="stable")[:Smax]
    sg = np.where(prng.uniform(name + ".sign", 5, 128) < 0, -1.0, 1.0).astype(np.float32).reshape(2, 64)
    blk = prng.randint(name + ".blk", 5, 2, 0, NPOOL)
    qkv = rnd(name + ".qkv", (3, 64))
    qkv[0] *= 2.0
    qkv[1, :4], qkv[2, :4] = TIES, TIES.flip(0)
    return blk, pk, pv, sg, qkv


class Call:
    """One launch: rows = [(S, kv_start, seed)].  Holds the logical caches (poisoned outside [kv_start, pos)), qkv, the fp64
    reference [B, H * 64], the rounded step rows and the masked fp64 scores."""

    def __init__(self, form, rows, H=None, half=torch.bfloat16, Smax=None):
        f = FORMS[form]
        self.form, self.f, self.rows, self.half = form, f, rows, half
        self.B, self.H, self.Smax = len(rows), H or f["H"], Smax or f["Smax"]
        B, H, Smax = self.B, self.H, self.Smax
        self.cdt = cdt = tdt(f["tc"], half)
        self.pos = [S - 1 for S, _, _ in rows]
        self.ks = [ks for _, ks, _ in rows]
        self.prefix = PREFIX if min(self.pos) >= PREFIX else 0
        self.len = [p - self.prefix for p in self.pos]
        blk = np.empty((2, B * H), dtype=np.int64)
        perm = np.empty((2, B * H, Smax), dtype=np.int64)
        sign = np.empty((B * H, 2, 64), dtype=np.float32)
        self.qkv = torch.empty(B, 3, H, 64)
        for b, (_, _, seed) in enumerate(rows):
            for h in range(H):
                blk[:, b * H + h], perm[0, b * H + h], perm[1, b * H + h], sign[b * H + h], self.qkv[b, :, h] = head_data(seed, h, Smax)
        blk, perm, sign = torch.from_numpy(blk), torch.from_numpy(perm), torch.from_numpy(sign)
        pk, pv = pool(cdt)
        # the caches as fp32 holding values of the cache type (signs and permutations keep them so); converted once at the end
        K = (pk[blk[0][:, None], perm[0]] * sign[:, 0, None, :]).view(B, H, Smax, 64)
        V = (pv[blk[1][:, None], perm[1]] * sign[:, 1, None, :]).view(B, H, Smax, 64)
        self.knew, self.vnew = self.qkv[:, 1].to(cdt), self.qkv[:, 2].to(cdt)  # [B, H, 64] as torch rounds: nearest even
        self.ref = torch.empty(B, H * 64, dtype=torch.float64)
        self.scm, self.sown, self.vis = [], [], []
        j = torch.arange(Smax)
        for b in range(B):
            q = self.qkv[b, 0].double()
            vis = (j >= self.ks[b]) & (j < self.pos[b])
            sc = torch.einsum("hd,hjd->hj", q / 8, K[b].double()).masked_fill(~vis, float("-inf"))
            sown = (q / 8 * self.knew[b].double()).sum(-1)
            w = torch.softmax(torch.cat([sc, sown[:, None]], 1), -1)
            self.ref[b] = (torch.einsum("hj,hjd->hd", w[:, :-1], V[b].double()) + w[:, -1:] * self.vnew[b].double()).reshape(-1)
            top = torch.maximum(sc.max(-1).values, sown)  # the largest real score per head
            kp = ((top + 30.0) * 8 / (q * q).sum(-1))[:, None] * q  # (q / 8) . kp = top + 30
            K[b][:, ~vis] = kp.to(cdt).float()[:, None, :]
            V[b][:, ~vis] = 1000.0
            self.scm.append(sc), self.sown.append(sown), self.vis.append(vis)
        assert bool(torch.isfinite(K).all()) and bool(torch.isfinite(self.ref).all())
        self.K, self.V = K.to(cdt), V.to(cdt)

    def qkv_flat(self):
        return self.qkv.reshape(self.B, 3 * self.H * 64).contiguous()

    def owners(self):
        """[B, NSPLIT] bool: does split sp own a visible key (the appended one is split 0's)"""
        j = torch.arange(self.Smax)
        own = torch.stack([torch.stack([(v & ((j // 32) % NSPLIT == sp)).any() for sp in range(NSPLIT)]) for v in self.vis])
        own[:, 0] = True
        return own

    def split_partials_fp64(self):
        """the reference split-wise, with the kernel's dealing of rows to splits: o [B, H, 4, 64], ml [B, H, 2, 4] (fp64)"""
        B, H = self.B, self.H
        o = torch.zeros(B, H, NSPLIT, 64, dtype=torch.float64)
        ml = torch.zeros(B, H, 2, NSPLIT, dtype=torch.float64)
        j = torch.arange(self.Smax)
        for b in range(B):
            for sp in range(NSPLIT):
                mine = self.vis[b] & ((j // 32) % NSPLIT == sp)
                s = self.scm[b].masked_fill(~mine, float("-inf"))
                s = torch.cat([s, self.sown[b][:, None] if sp == 0 else torch.full((H, 1), float("-inf"), dtype=torch.float64)], 1)
                m = s.max(-1).values
                ml[b, :, 0, sp] = m
                if bool(torch.isinf(m).any()):
                    assert bool(torch.isinf(m).all())  # the same rows for every head
                    continue
                e = torch.exp(s - m[:, None])
                ml[b, :, 1, sp] = e.sum(-1)
                v = torch.where(mine[None, :, None], self.V[b].double(), torch.zeros((), dtype=torch.float64))
                o[b, :, sp] = torch.einsum("hj,hjd->hd", e[:, :-1], v) + e[:, -1:] * self.vnew[b].double()
        return o, ml


def seed_of(S, ks, salt=0):
    return (S * 2003 + ks) * 16 + salt


def mk(form, pairs, salt=0, **kw):
    return Call(form, [(S, ks, seed_of(S, ks, salt)) for S, ks in pairs], **kw)


# ---- the launch ---------------------------------------------------------------------------------------------------------------
def guarded(t, rows_shape):
    """[n, ...] -> device tensor [n + 1, ...], the last entry the sentinel"""
    return torch.cat([t, torch.full((1,) + tuple(rows_shape), SENT, dtype=t.dtype)]).contiguous().to(DEV)


class Out:
    pass


def launch(lib, c, to=None, tiled=0, anc=None, nb=1, phys=None):
    """One itts_decode_attn call on Call c (phys: the physical caches of an ancestry, instead of the logical ones).  Checks the
    host precondition before, and after: the append to the bit, every other cache byte, the guards, NaN / Inf."""
    f, B, H, Smax, cdt = c.f, c.B, c.H, c.Smax, c.cdt
    D = H * 64
    for b in range(B):
        assert 0 <= c.ks[b] <= c.pos[b] < Smax, (c.form, b, c.ks[b], c.pos[b], Smax)  # the kernel cannot check it
    assert anc is None or (tuple(anc.shape) == (2, B, Smax) and anc.dtype == torch.uint8 and B % nb == 0)
    Kl, Vl = phys if phys is not None else (c.K, c.V)
    kd, vd = guarded(Kl.view(B * H, Smax, 64), (Smax, 64)), guarded(Vl.view(B * H, Smax, 64), (Smax, 64))
    want_k, want_v = kd.clone(), vd.clone()
    for b in range(B):
        want_k[b * H:(b + 1) * H, c.pos[b]] = c.knew[b].to(DEV)
        want_v[b * H:(b + 1) * H, c.pos[b]] = c.vnew[b].to(DEV)
    qkv = c.qkv_flat().to(DEV)
    ln = torch.tensor(c.len, dtype=torch.int32, device=DEV)
    ks = torch.tensor(c.ks, dtype=torch.int32, device=DEV)
    pre = torch.tensor([c.prefix], dtype=torch.int32, device=DEV)
    ancd = anc.contiguous().to(DEV) if anc is not None else None
    to = f["to"] if to is None else to
    odt = tdt(to, c.half)
    ctx = po = pml = None
    if f["split"]:
        po = torch.full((B + 1, H, NSPLIT, 64), float("nan"))
        pml = torch.full((B + 1, H, 2, NSPLIT), float("nan"))
        po[B], pml[B] = SENT, SENT
        po, pml = po.to(DEV), pml.to(DEV)
    elif tiled:
        BT = (B + 15) // 16
        full = torch.full((BT * 16, D), SENT, dtype=odt)
        full[:B] = float("nan")
        ctx = torch.cat([full.view(BT, 16, D // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1), torch.full((D,), SENT, dtype=odt)]).to(DEV)
    else:
        ctx = torch.full((B + 1, D), float("nan"), dtype=odt)
        ctx[B] = SENT
        ctx = ctx.to(DEV)
    L.check(lib.itts_decode_attn(ctx.data_ptr() if ctx is not None else None, to, qkv.data_ptr(), kd.data_ptr(), vd.data_ptr(),
                                 ln.data_ptr(), ks.data_ptr(), pre.data_ptr(), B, H, 64, Smax, f["tc"], tiled,
                                 po.data_ptr() if po is not None else None, pml.data_ptr() if pml is not None else None,
                                 ancd.data_ptr() if ancd is not None else None, nb, stream()), "decode_attn", lib)
    sync()
    what = (c.form, c.rows, "anc" if anc is not None else "", nb)
    # (2) the append, bit for bit, and every other byte of the caches and their guards
    for name, got, want in (("K", kd, want_k), ("V", vd, want_v)):
        if not torch.equal(ibits(got), ibits(want)):
            for b in range(B):
                assert torch.equal(ibits(got[b * H:(b + 1) * H, c.pos[b]]), ibits(want[b * H:(b + 1) * H, c.pos[b]])), \
                    what + (f"{name} cache row pos of row {b} is not this step's rounded row",)
            assert bool((got[B * H] == SENT).all()), what + (f"the guard block behind the {name} cache was written",)
            assert False, what + (f"{name} cache bytes other than the appended rows changed",)
    o = Out()
    if f["split"]:
        po, pml = po.cpu(), pml.cpu()
        assert bool((po[B] == SENT).all()) and bool((pml[B] == SENT).all()), what + ("partials past B were written",)
        o.o, o.ml = po[:B], pml[:B]
        assert not bool(torch.isnan(o.o).any()) and not bool(torch.isnan(o.ml).any()), what
        assert bool(torch.isfinite(o.o).all()) and bool(torch.isfinite(o.ml[:, :, 1]).all()), what
        own = c.owners()  # a split that owns no visible key: exactly (-inf, 0, 0 .. 0)
        for b in range(B):
            for sp in range(NSPLIT):
                if not own[b, sp]:
                    assert bool((o.ml[b, :, 0, sp] == float("-inf")).all()) and bool((o.ml[b, :, 1, sp] == 0).all()) and \
                        bool((o.o[b, :, sp] == 0).all()), what + (f"row {b} split {sp} owns no key",)
                else:
                    assert bool(torch.isfinite(o.ml[b, :, 0, sp]).all()), what + (f"row {b} split {sp} owns a key",)
        o.merged = merge_partials(o.o, o.ml)
        assert bool(torch.isfinite(o.merged).all()), what
        return o
    ctx = ctx.cpu()
    if tiled:
        BT = (B + 15) // 16
        assert bool((ctx[BT * 16 * D:] == SENT).all()), what + ("the guard behind the tiled ctx was written",)
        rows = from_tiles(ctx[:BT * 16 * D], BT * 16, D)
        assert bool((rows[B:] == SENT).all()), what + ("padding rows of the last tile were written",)
        o.ctx = rows[:B].contiguous()
    else:
        assert bool((ctx[B] == SENT).all()), what + ("the row behind ctx was written",)
        o.ctx = ctx[:B]
    assert bool(torch.isfinite(o.ctx.float()).all()), what + ("NaN / Inf in ctx",)
    return o


def bound_of(c, to=None):
    to = c.f["to"] if to is None else to
    if c.f["split"] or to == L.F32:
        return 2e-5
    return 2.0 ** -10 if c.half == torch.float16 else 2.0 ** -8


MEASURED = {}  # table line -> (max relerr, bound)


def judge(c, o, line, to=None):
    """(1) the result of every row against fp64, and the rows whose only visible key is the appended one to the bit"""
    bound = bound_of(c, to)
    got = o.merged if c.f["split"] else o.ctx
    worst = 0.0
    for b in range(c.B):
        e = relerr(got[b], c.ref[b])
        print(f"decode_attn {line} S={c.pos[b] + 1} kv_start={c.ks[b]} row {b} of {c.B}: relerr {e:.3e} (bound {bound:.1e})")
        worst = max(worst, e)
        if c.ks[b] == c.pos[b] and not c.f["split"]:
            want = c.vnew[b].reshape(-1).to(got.dtype)
            assert torch.equal(ibits(got[b].contiguous()), ibits(want)), (line, c.rows[b], "only the appended key is visible: ctx = rounded v")
    MEASURED[line] = (max(worst, MEASURED.get(line, (0.0, bound))[0]), bound)
    assert worst < bound, (line, c.rows, worst)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [f"{k:<36s} max relerr {e:9.3e}   bound {b:.1e}" for k, (e, b) in sorted(MEASURED.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_attn_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- CPU: the fixture, the case lists, the refusals -----------------------------------------------------------------------
def test_split_reference_merges_to_the_unsplit_reference():
    """The fixture itself: the fp64 reference computed split-wise, rows dealt to the four splits as the kernel deals them (chunk u
    of split sp = rows (4u + sp) * 32 .., the appended key in split 0), merges to the unsplit reference; splits without a visible
    key occur and hold (-inf, 0, zeros)."""
    c = mk("split", [(33, 0), (97, 40), (1281, 771), (769, 5)])
    o, ml = c.split_partials_fp64()
    assert relerr(merge_partials(o, ml), c.ref) < 1e-12
    own = c.owners()
    assert own[0].tolist() == [True, False, False, False] and own[1].tolist() == [True, True, True, False]
    assert own[2].all() and own[3].all()
    empty = torch.isinf(ml[:, :, 0])
    assert torch.equal(empty, ~own[:, None, :].expand_as(empty))
    assert bool((ml[:, :, 1][empty] == 0).all()) and bool((o[empty] == 0).all())
    # poison: outside [kv_start, pos) every K scores 30 above the largest real score, V = 1000
    b, h = 1, 2
    sc = (c.qkv[b, 0, h].double() / 8 * c.K[b, h].double()).sum(-1)
    top = max(float(c.scm[b][h].max()), float(c.sown[b][h]))
    bad = sc[~c.vis[b]]
    assert bad.numel() == c.Smax - (96 - 40) and float(bad.min()) > top + 29 and float(bad.max()) < top + 31
    assert bool((c.V[b, h][~c.vis[b]] == 1000).all()) and float(c.V[b, h][c.vis[b]].abs().max()) < 2


def test_case_lists_cover_the_edges():
    for form, f in FORMS.items():
        S = s_edges(form)
        for v in (1, 2, f["SL"], f["U"] + 1, f["W"], f["W"] + 1, f["W"] + f["T"] + 1, f["Smax"]):
            assert v in S, (form, v)
        assert (f["W"] + 2 * f["T"] + 7 in S) == (form in ("bf16", "bf16_f32ctx", "f32", "many_f32"))  # what fits under Smax
        for Sv, ks in ks_edges(form):
            assert 0 <= ks <= Sv - 1 < f["Smax"], (form, Sv, ks)
        assert any(ks > f["W"] for _, ks in ks_edges(form)) and any(ks == Sv - 1 for Sv, ks in ks_edges(form))
    assert [len(x) for x in deal(list(range(11)), 0)] == [4, 3, 2, 1, 1] and [len(x) for x in deal(list(range(11)), 8)] == [8, 8]


def test_entry_refuses_what_the_kernel_does_not_have(lib):
    """Host only: every refusal comes back with a message before any launch (the host buffer is never read)."""
    host = np.zeros(64, dtype=np.float32)
    hp = host.ctypes.data
    #            to      tc      dh  B   ctx_tiled part_o part_ml anc  nb  message
    cases = [(L.BF16, L.BF16, 32, 2, 0, None, None, None, 1, b"head dim must be 64"),
             (L.BF16, L.F32, 64, 2, 0, hp, hp, None, 1, b"split form needs both partial buffers and a bf16 cache"),
             (L.BF16, L.BF16, 64, 2, 0, hp, None, None, 1, b"split form needs both partial buffers and a bf16 cache"),
             (L.F32, L.BF16, 64, 2, 1, None, None, None, 1, b"tiled ctx is bf16 only"),
             (L.BF16, L.F32, 64, 2, 0, None, None, None, 1, b"dtype combination"),
             (L.BF16, L.BF16, 64, 3, 0, None, None, hp, 2, b"beam ancestry needs B to be a multiple"),
             (L.BF16, L.BF16, 64, 17, 0, None, None, hp, 17, b"beam ancestry needs B to be a multiple")]
    for to, tc, dh, B, tiled, po, pml, anc, nb, msg in cases:
        st = lib.itts_decode_attn(hp, to, hp, hp, hp, hp, hp, hp, B, 3, dh, 128, tc, tiled, po, pml, anc, nb, None)
        assert st != 0 and msg in lib.itts_last_error(), (to, tc, dh, B, tiled, nb, st, lib.itts_last_error())
    # what the wrapper itself sees: null pointers, empty shapes, no output at all
    for args in ((hp, None, hp, hp, hp, hp, hp, 2, 3, 128), (hp, hp, None, hp, hp, hp, hp, 2, 3, 128), (hp, hp, hp, None, hp, hp, hp, 2, 3, 128),
                 (hp, hp, hp, hp, None, hp, hp, 2, 3, 128), (hp, hp, hp, hp, hp, None, hp, 2, 3, 128), (hp, hp, hp, hp, hp, hp, None, 2, 3, 128),
                 (None, hp, hp, hp, hp, hp, hp, 2, 3, 128), (hp, hp, hp, hp, hp, hp, hp, 0, 3, 128), (hp, hp, hp, hp, hp, hp, hp, 2, 0, 128),
                 (hp, hp, hp, hp, hp, hp, hp, 2, 3, 0)):
        ctx, qkv, kc, vc, ln, ks, pre, B, H, Smax = args
        st = lib.itts_decode_attn(ctx, L.BF16, qkv, kc, vc, ln, ks, pre, B, H, 64, Smax, L.BF16, 0, None, None, None, 1, None)
        assert st != 0 and b"itts_decode_attn: bad arguments" in lib.itts_last_error(), args


# ---- GPU: every form at the edges of S and of kv_start ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["S", "kv_start"])
@pytest.mark.parametrize("form", list(FORMS))
def test_form_against_fp64(lib, form, kind):
    f = FORMS[form]
    rows = [(S, 0) for S in s_edges(form)] if kind == "S" else ks_edges(form)
    first = None
    for pairs in deal(rows, f["B"]):
        c = mk(form, pairs)
        o = launch(lib, c)
        judge(c, o, f"{form} {kind} edges")
        if form == "bf16":  # (3) the fp32 ctx of the same call, rounded, is the bf16 ctx: both store the same o / L
            o32 = launch(lib, c, to=L.F32)
            assert torch.equal(ibits(o32.ctx.to(torch.bfloat16)), ibits(o.ctx)), (form, pairs, "bf16 ctx != rounded fp32 ctx")
        if first is None:
            first = (c, o)
    c, o = first  # (3) two runs agree
    again = launch(lib, c)
    if f["split"]:
        assert torch.equal(ibits(again.o), ibits(o.o)) and torch.equal(ibits(again.ml), ibits(o.ml)), (form, c.rows)
    else:
        assert torch.equal(ibits(again.ctx), ibits(o.ctx)), (form, c.rows)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["bf16", "bf16_f32ctx", "f32", "split"])
def test_row_alone_equals_row_in_a_batch(lib, form):
    """(3) the same (row, head) problem in row 0 alone and in row r of a 2-, 3- and 4-row call: the same bits"""
    f = FORMS[form]
    pairs = [(f["W"] + 1, 3), (f["U"], 0), (f["W"] + f["T"] + 2, f["SL"] + 1), (2, 0)]
    key = (lambda o: (ibits(o.o), ibits(o.ml))) if f["split"] else (lambda o: (ibits(o.ctx),))
    alone = []
    for p in pairs:
        c = mk(form, [p])
        o = launch(lib, c)
        judge(c, o, f"{form} rows alone")
        alone.append(key(o))
    for B in (2, 3, 4):
        c = mk(form, pairs[:B])
        o = launch(lib, c)
        judge(c, o, f"{form} rows alone")
        for r in range(B):
            for got, want in zip(key(o), alone[r]):
                assert torch.equal(got[r], want[0]), (form, f"row {r} alone differs from row {r} of {B}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 17])
def test_tiled_ctx(lib, B):
    """(3) ctx in MFMA-fragment tiles, un-tiled, is the row-major ctx of the same problem; padding rows of the last tile stay"""
    S = [1, 2, 127, 128, 129, 255, 256, 257, 300, 64, 200, 299, 5, 131, 290, 33, 250]
    ks = [0, 1, 0, 127, 3, 254, 0, 129, 1, 63, 128, 0, 2, 0, 270, 32, 249]
    c = mk("bf16", list(zip(S[:B], ks[:B])), Smax=300)
    plain = launch(lib, c)
    judge(c, plain, "bf16 tiled ctx")
    tiled = launch(lib, c, tiled=1)
    assert torch.equal(ibits(tiled.ctx), ibits(plain.ctx)), B


# ---- GPU: the beam ancestry ---------------------------------------------------------------------------------------------------
def ancestry(c, nb, name):
    """A scattered history: per item and position a random permutation of its nb beams says in which physical row each beam's
    logical row lies -> [B, Smax]"""
    anc = torch.empty(c.B, c.Smax, dtype=torch.int64)
    for it in range(c.B // nb):
        perm = np.argsort(prng.uniform(f"{name}.{it}", 5, c.Smax * nb).reshape(c.Smax, nb), axis=1, kind="stable")
        anc[it * nb:(it + 1) * nb] = torch.from_numpy(perm.T.copy())
    return anc


def scattered(c, nb, anc):
    """the physical caches in which every beam's logical rows lie where `anc` says"""
    B, H, Smax = c.B, c.H, c.Smax
    src = (torch.arange(B)[:, None] // nb) * nb + anc  # [B, Smax] physical row of (beam, position)
    R = src[:, None, :].expand(B, H, Smax)
    Hh = torch.arange(H)[None, :, None].expand(B, H, Smax)
    J = torch.arange(Smax)[None, None, :].expand(B, H, Smax)
    Kp, Vp = torch.empty_like(c.K), torch.empty_like(c.V)
    Kp[R, Hh, J], Vp[R, Hh, J] = c.K, c.V
    return Kp, Vp


ANC_CASES = [(form, nb) for form in FORMS for nb in (2, 3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,nb", ANC_CASES)
def test_ancestry_gather(lib, form, nb):
    """(3) ANC with the identity ancestry = the plain form; ANC over a scattered history = the plain form on the gathered cache.
    The append lands in the beam's own physical row whatever the ancestry says (checked by launch)."""
    f = FORMS[form]
    B = {2: 8, 3: 9, 4: 8}[nb] if f["B"] else {2: 4, 3: 3, 4: 4}[nb]
    items = B // nb
    Ss = [f["W"] + 3, f["W"] + f["T"] + 2, f["U"] + 2, f["SL"] + 1]
    Ss = Ss[nb - 3:nb - 2] if items == 1 else Ss[:items]
    kss = [0, 5, 1, f["SL"] - 1]
    c = mk(form, [(Ss[b // nb], kss[(b % nb) % 4]) for b in range(B)], salt=nb, H=f["H"])
    key = (lambda o: (ibits(o.o), ibits(o.ml))) if f["split"] else (lambda o: (ibits(o.ctx),))
    plain = launch(lib, c)
    judge(c, plain, f"{form} ancestry")
    ident = (torch.arange(B) % nb).to(torch.uint8)[None, :, None].expand(2, B, c.Smax).contiguous()
    o = launch(lib, c, anc=ident, nb=nb)
    for got, want in zip(key(o), key(plain)):
        assert torch.equal(got, want), (form, nb, "identity ancestry != plain")
    true, other = ancestry(c, nb, f"da.anc.{form}.{nb}"), ancestry(c, nb, f"da.anc2.{form}.{nb}")
    phys = scattered(c, nb, true)
    assert not torch.equal(true, other)
    anc = torch.empty(2, B, c.Smax, dtype=torch.uint8)
    for b in range(B):
        t = true[b].clone()
        t[c.pos[b]:] = 255  # the kernel clamps what it reads there
        anc[c.len[b] & 1, b], anc[1 - (c.len[b] & 1), b] = t.to(torch.uint8), other[b].to(torch.uint8)
    o = launch(lib, c, anc=anc, nb=nb, phys=phys)
    for got, want in zip(key(o), key(plain)):
        assert torch.equal(got, want), (form, nb, "scattered ancestry != plain on the gathered cache")


def test_ancestry_cases_have_odd_and_even_len():
    par = set()
    for form, nb in ANC_CASES:
        f = FORMS[form]
        items = ({2: 8, 3: 9, 4: 8}[nb] if f["B"] else {2: 4, 3: 3, 4: 4}[nb]) // nb
        Ss = [f["W"] + 3, f["W"] + f["T"] + 2, f["U"] + 2, f["SL"] + 1]
        for S in (Ss[nb - 3:nb - 2] if items == 1 else Ss[:items]):
            assert S <= f["Smax"]
            par.add((form, (S - 1 - PREFIX) & 1))
    assert par == {(form, p) for form in FORMS for p in (0, 1)}


# ---- GPU: the IEEE-half library -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["bf16", "split"])
def test_ieee_half_library(form):
    """the same sources with binary16 as the 16-bit type: float16 caches, 2^-10 for the half ctx"""
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    lib16 = L.load("f16")
    f = FORMS[form]
    c = mk(form, [(f["W"] + f["T"] + 1, f["SL"] + 1), (f["W"], 0), (f["U"] + 1, f["U"]), (2, 0)], half=torch.float16)
    assert c.cdt == torch.float16 and half_of(lib16) == torch.float16
    o = launch(lib16, c)
    judge(c, o, f"{form} [IEEE half]")
    if not f["split"]:
        assert o.ctx.dtype == torch.float16


# ---- GPU: producer into consumer ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_split_partials_into_the_projection_gemv(lib):
    """The split form's partials, as the kernel wrote them, through prologue 3 of itts_gemv_bf16 (accumulate, bias) against the fp64
    chain attention -> bf16 -> matmul, at the GEMV file's bound for that prologue: the layout of part_o / part_ml held to a number."""
    H, N = 8, 37
    K = H * 64
    w = (rnd("da.w", (N, K)) * 0.05).to(torch.bfloat16)
    bias, y0 = rnd("da.b", (N,)), rnd("da.y", (4, N))
    pairs = [(769, 3), (700, 0), (1283, 40), (33, 0)]  # both sides of the window, a row with three empty splits
    for B in (1, 2, 3, 4):
        c = mk("split", pairs[:B], H=H)
        assert int(lib.itts_gemv_which(B, N, K, 3, 1, 0, 0)) >= 0
        o = launch(lib, c)
        judge(c, o, "split H=8 (producer)")
        po, pml = o.o.contiguous().to(DEV), o.ml.contiguous().to(DEV)
        wd, bd = w.to(DEV), bias.to(DEV)
        y = torch.cat([y0[:B], torch.full((1, N), SENT)]).to(DEV)
        L.check(lib.itts_gemv_bf16(y.data_ptr(), 0, None, 1, wd.data_ptr(), bd.data_ptr(), B, N, K, L.ACT_NONE, 1, 3, None, None,
                                   po.data_ptr(), pml.data_ptr(), None, None, stream()), "gemv_bf16")
        sync()
        y = y.cpu()
        assert bool((y[B] == SENT).all()) and bool(torch.isfinite(y).all())
        ref = c.ref.to(torch.bfloat16).double() @ w.double().T + bias.double() + y0[:B].double()
        e = relerr(y[:B], ref)
        print(f"split attention -> gemv_bf16 prologue 3, B={B}: relerr {e:.3e} (bound 2e-03)")
        MEASURED["split -> gemv_bf16 prologue 3"] = (max(e, MEASURED.get("split -> gemv_bf16 prologue 3", (0.0, 2e-3))[0]), 2e-3)
        assert e < 2e-3, (B, e)
