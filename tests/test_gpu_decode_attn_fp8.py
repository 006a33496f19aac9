"""Operator-level tests of the decode cache attention on an fp8 (OCP e4m3, no scale) K/V cache: csrc/decode_attn.hip
decode_attn2_kernel<fp8_t, ..> with CacheVec<fp8_t> of csrc/itts_attn_dev.h, through the C ABI entry itts_decode_attn with
tc = ITTS_FP8.  The problem class, the case lists and the helpers are those of tests/test_gpu_decode_attn.py (head_data, deal,
s_edges / ks_edges, ancestry, scattered), rebuilt around a 1-byte cache.

Reference: fp64 torch on the CPU from the SAME rounded inputs - the keys kv_start[b] <= j < pos exactly as the cache stores them
(e4m3 values), plus this step's k / v rounded as the cache rounds: x.clamp(-448, 448).to(torch.float8_e4m3fn), i.e. clamp, then
round to nearest even, subnormals included.  K and V hold e4m3 values (std 1, rounded with that expression); q has std 2.  The
step's k carries 1 + 2^-4, -(1 + 3 * 2^-4), 2^-10, 3 * 2^-10, 500, -1e4 in its first six dims (v the same, reversed): the two
ties, the two subnormal ties, a value past the largest and one far past it.  Dims 4 and 5 of q (which meet the +-448 those last
two become) are scaled by 2^-6, so that the appended key's score moves by a few units instead of deciding every softmax.

Poison, not zeros: every cache row outside [kv_start, pos) holds a K which, AFTER rounding to e4m3, still scores at least 20 above
the largest real score of its (row, head) (asserted on the host) and V = 448, the largest e4m3 value.  All of it is finite.
Behind each cache lies one more [Smax][64] block of sentinel bytes, behind ctx one more row.

Forms (SLOTS / blind rows U / register window W / stream step T) - CacheVec<fp8_t> is VEC 8, LPK 8, the 16-bit mapping, so the
edges are those of the bf16 forms:
  fp8          e4m3 cache -> 16-bit ctx, 1024 threads, H = 3     128 / 256 / 768 / 256   Smax 1400
  fp8_f32ctx   e4m3 cache -> fp32 ctx                             the same
  many_fp8     256 threads, 8 pairs, B = 8, H = 64                 32 /  64 / 512 / 128   Smax 700

Per call: (1) every row against fp64: relerr < 2e-5 for fp32 ctx, < 2^-8 for bf16 ctx, < 2^-10 for binary16 ctx (the bounds of
tests/test_gpu_decode_attn.py: the reference uses the stored values, so the cache type costs nothing).  The +-448 of the step's v
enter the row maximum that relerr divides by, so the same bounds (for a 16-bit ctx plus the fp32 bound: there the largest element
itself may sit at a tie of the store) are also asserted over dims 8 .. 63 of every head alone, which hold no edge value (a
stricter check; both figures are printed).  A row whose only visible key is the appended one returns the rounded
v to the bit (a value that rounds to -0 returns as +0: e4m3 flushes |x| < 2^-10 to a signed zero, and the sum starts at +0).  (2) The append to the byte: cache row pos = torch's clamp-and-cast of this step's k / v, every other byte of the
caches and guards unchanged, compared as uint8.  (3) Exact relations: the fp8 form = the 16-bit form of the same library on caches
holding the same values with the step's k / v pre-rounded to e4m3 (ctx bits identical, fp32 and 16-bit ctx, both thread counts);
16-bit ctx = the fp32 ctx rounded; tiled = row-major; a row alone = that row in a 2-, 3-, 4-row call; two runs agree; ANC with the
identity ancestry = plain; ANC over a scattered history = plain on the gathered cache.  (4) No NaN / Inf, no NaN byte in a cache.

The measured maxima are printed and, where ITTS_TEST_OUT names a directory, written to decode_attn_fp8_ops.txt there (committed
as profiles/decode_attn_fp8_ops.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_attn import (NPOOL, POOL_ROWS, PREFIX, SENT, ancestry, deal, head_data, ks_edges, s_edges, scattered,
                                  seed_of)
from test_gpu_decode_gemv import relerr, rnd, stream, sync
from test_gpu_ops import from_tiles

DEV = "cuda:0"
EDGES = torch.tensor([1 + 2.0 ** -4, -(1 + 3 * 2.0 ** -4), 2.0 ** -10, 3 * 2.0 ** -10, 500.0, -1e4])
EDGES_ROUNDED = [1.0, -1.25, 0.0, 2.0 ** -8, 448.0, -448.0]  # torch's clamp-and-cast of EDGES
GUARD_BYTE = 0x5A  # the sentinel of the guard block behind an e4m3 cache (SENT = 777 is not an e4m3 value)

FORMS = {
    "fp8": dict(to=L.BF16, SL=128, U=256, W=768, T=256, Smax=1400, B=0, H=3, like="bf16"),
    "fp8_f32ctx": dict(to=L.F32, SL=128, U=256, W=768, T=256, Smax=1400, B=0, H=3, like="bf16_f32ctx"),
    "many_fp8": dict(to=L.BF16, SL=32, U=64, W=512, T=128, Smax=700, B=8, H=64, like="many_bf16"),
}


def e4m3(x):
    """the cache's rounding, as fp32 values: clamp to the finite range, then torch's round-to-nearest-even cast"""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def half_of(lib):
    return torch.float16 if lib.itts_half_is_f16() else torch.bfloat16


def tdt(code, half):
    return {L.F32: torch.float32, L.BF16: half, L.FP8: torch.float8_e4m3fn}[code]


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- one launch's problem and its fp64 reference (CPU) --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool():
    """random [POOL_ROWS][64] blocks rounded to e4m3, held as fp32; every (row, head) cache is one of them, rows permuted, dims
    signed (e4m3 is sign-symmetric: the values stay e4m3 values)"""
    return e4m3(rnd("da8.poolk", (NPOOL, POOL_ROWS, 64))), e4m3(rnd("da8.poolv", (NPOOL, POOL_ROWS, 64)))


class Call:
    """One launch: rows = [(S, kv_start, seed)].  K, V [B, H, Smax, 64]: the logical caches as fp32 holding e4m3 values (poisoned
    outside [kv_start, pos)); qkv the step's q, k, v (fp32, unrounded); knew / vnew the step's rows as the cache rounds them;
    ref [B, H * 64] fp64."""

    def __init__(self, f, rows, H=None, Smax=None):
        self.f, self.rows = f, rows
        self.B, self.H, self.Smax = len(rows), H or f["H"], Smax or f["Smax"]
        B, H, Smax = self.B, self.H, self.Smax
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
        self.qkv[:, 0, :, 4:6] *= 2.0 ** -6
        self.qkv[:, 1, :, :6] = EDGES
        self.qkv[:, 2, :, :6] = EDGES.flip(0)
        blk, perm, sign = torch.from_numpy(blk), torch.from_numpy(perm), torch.from_numpy(sign)
        pk, pv = pool()
        K = (pk[blk[0][:, None], perm[0]] * sign[:, 0, None, :]).view(B, H, Smax, 64)
        V = (pv[blk[1][:, None], perm[1]] * sign[:, 1, None, :]).view(B, H, Smax, 64)
        self.knew, self.vnew = e4m3(self.qkv[:, 1]), e4m3(self.qkv[:, 2])  # [B, H, 64]
        self.ref = torch.empty(B, H * 64, dtype=torch.float64)
        self.vis, self.margin = [], float("inf")
        j = torch.arange(Smax)
        for b in range(B):
            q = self.qkv[b, 0].double()
            vis = (j >= self.ks[b]) & (j < self.pos[b])
            sc = torch.einsum("hd,hjd->hj", q / 8, K[b].double()).masked_fill(~vis, float("-inf"))
            sown = (q / 8 * self.knew[b].double()).sum(-1)
            w = torch.softmax(torch.cat([sc, sown[:, None]], 1), -1)
            self.ref[b] = (torch.einsum("hj,hjd->hd", w[:, :-1], V[b].double()) + w[:, -1:] * self.vnew[b].double()).reshape(-1)
            top = torch.maximum(sc.max(-1).values, sown)  # the largest real score per head
            kp = e4m3(((top + 30.0) * 8 / (q * q).sum(-1))[:, None] * q)  # (q / 8) . kp = top + 30 before the rounding
            self.margin = min(self.margin, float(((q / 8 * kp.double()).sum(-1) - top).min()))  # ... and this much after it
            K[b][:, ~vis] = kp[:, None, :]
            V[b][:, ~vis] = 448.0
            self.vis.append(vis)
        # the host assertions of the fixture: the poison key still wins by 20 after its rounding, every value is an e4m3 value
        assert self.margin >= 20.0, (rows, self.margin)
        assert bool(torch.isfinite(self.ref).all()) and torch.equal(e4m3(K), K) and torch.equal(e4m3(V), V)
        self.K, self.V = K, V

    def qkv_flat(self, rounded):
        """[B, 3 * H * 64]; rounded: k and v pre-rounded to e4m3, so that a 16-bit cache's own rounding is the identity"""
        q = self.qkv.clone()
        if rounded:
            q[:, 1], q[:, 2] = self.knew, self.vnew
        return q.reshape(self.B, 3 * self.H * 64).contiguous()


@functools.lru_cache(maxsize=None)
def cached_call(like, rows, H, Smax):
    return Call(FORMS[like], list(rows), H=H, Smax=Smax)


def mk(form, pairs, salt=0, H=None, Smax=None):
    """the problems depend on the shape numbers only: forms of equal shape (fp8 / fp8_f32ctx) share them, computed once"""
    f = FORMS[form]
    rows = tuple((S, ks, seed_of(S, ks, salt)) for S, ks in pairs)
    if f["B"]:  # (used once each, and large)
        return Call(f, list(rows), H=H, Smax=Smax)
    return cached_call("fp8", rows, H or f["H"], Smax or f["Smax"])


# ---- the launch ---------------------------------------------------------------------------------------------------------------
class Out:
    pass


def cache_dev(t, cdt):
    """[n, Smax, 64] fp32 values -> (device bytes [n + 1, Smax, 64 * size] with the guard block last, host copy)"""
    body = bits(t.to(cdt))
    if cdt == torch.float8_e4m3fn:
        guard = torch.full((1,) + tuple(body.shape[1:]), GUARD_BYTE, dtype=torch.uint8)
    else:
        guard = bits(torch.full((1,) + tuple(t.shape[1:]), SENT).to(cdt))
    host = torch.cat([body, guard]).contiguous()
    return host.to(DEV), host


def launch(lib, c, to, tc=L.FP8, tiled=0, anc=None, nb=1, phys=None):
    """One itts_decode_attn call on Call c with the caches held as type tc (the e4m3 cache, or the library's 16-bit type holding
    the same values - then with the step's k / v pre-rounded).  Checks the host precondition before, and after: the append to the
    byte, every other cache byte, the guards, NaN / Inf."""
    B, H, Smax = c.B, c.H, c.Smax
    D = H * 64
    half = half_of(lib)
    cdt = tdt(tc, half)
    for b in range(B):
        assert 0 <= c.ks[b] <= c.pos[b] < Smax, (b, c.ks[b], c.pos[b], Smax)  # the kernel cannot check it
    assert anc is None or (tuple(anc.shape) == (2, B, Smax) and anc.dtype == torch.uint8 and B % nb == 0)
    Kl, Vl = phys if phys is not None else (c.K, c.V)
    kd, k0 = cache_dev(Kl.view(B * H, Smax, 64), cdt)
    vd, v0 = cache_dev(Vl.view(B * H, Smax, 64), cdt)
    want_k, want_v = k0.clone(), v0.clone()
    for b in range(B):
        want_k[b * H:(b + 1) * H, c.pos[b]] = bits(c.knew[b].to(cdt))
        want_v[b * H:(b + 1) * H, c.pos[b]] = bits(c.vnew[b].to(cdt))
    assert kd.data_ptr() % 8 == 0 and vd.data_ptr() % 8 == 0
    qkv = c.qkv_flat(rounded=tc != L.FP8).to(DEV)
    ln = torch.tensor(c.len, dtype=torch.int32, device=DEV)
    ks = torch.tensor(c.ks, dtype=torch.int32, device=DEV)
    pre = torch.tensor([c.prefix], dtype=torch.int32, device=DEV)
    ancd = anc.contiguous().to(DEV) if anc is not None else None
    odt = tdt(to, half)
    if tiled:
        BT = (B + 15) // 16
        full = torch.full((BT * 16, D), SENT, dtype=odt)
        full[:B] = float("nan")
        ctx = torch.cat([full.view(BT, 16, D // 32, 4, 8).permute(2, 0, 3, 1, 4).reshape(-1), torch.full((D,), SENT, dtype=odt)]).to(DEV)
    else:
        ctx = torch.full((B + 1, D), float("nan"), dtype=odt)
        ctx[B] = SENT
        ctx = ctx.to(DEV)
    L.check(lib.itts_decode_attn(ctx.data_ptr(), to, qkv.data_ptr(), kd.data_ptr(), vd.data_ptr(), ln.data_ptr(), ks.data_ptr(),
                                 pre.data_ptr(), B, H, 64, Smax, tc, tiled, None, None,
                                 ancd.data_ptr() if ancd is not None else None, nb, stream()), "decode_attn", lib)
    sync()
    what = (c.rows, tc, to, "anc" if anc is not None else "", nb)
    # (2) the append, byte for byte, and every other byte of the caches and their guards
    for name, got, want in (("K", kd.cpu(), want_k), ("V", vd.cpu(), want_v)):
        if not torch.equal(got, want):
            for b in range(B):
                assert torch.equal(got[b * H:(b + 1) * H, c.pos[b]], want[b * H:(b + 1) * H, c.pos[b]]), \
                    what + (f"{name} cache row pos of row {b} is not torch's clamp-and-cast of this step's row",)
            assert torch.equal(got[B * H], want[B * H]), what + (f"the guard block behind the {name} cache was written",)
            assert False, what + (f"{name} cache bytes other than the appended rows changed",)
        if tc == L.FP8:  # (4) no NaN byte
            assert not bool(((got[:B * H] & 0x7F) == 0x7F).any()), what + (f"a NaN byte in the {name} cache",)
    o = Out()
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


def bound_of(lib, to):
    if to == L.F32:
        return 2e-5
    return 2.0 ** -10 if half_of(lib) == torch.float16 else 2.0 ** -8


MEASURED = {}  # table line -> (max relerr per row, max relerr over the plain dims of a head, bound)


def judge(lib, c, o, line, to):
    """(1) every row against fp64 - as a whole and over dims 8 .. 63 of every head, which hold no edge value - and the rows whose
    only visible key is the appended one to the bit"""
    bound = bound_of(lib, to)
    worst = worst_t = 0.0
    for b in range(c.B):
        e = relerr(o.ctx[b], c.ref[b])
        got_t, ref_t = o.ctx[b].view(c.H, 64)[:, 8:], c.ref[b].view(c.H, 64)[:, 8:]
        et = max(relerr(got_t[h], ref_t[h]) for h in range(c.H))
        print(f"decode_attn {line} S={c.pos[b] + 1} kv_start={c.ks[b]} row {b} of {c.B}: relerr {e:.3e}, dims 8..63 per head {et:.3e} "
              f"(bound {bound:.1e})")
        worst, worst_t = max(worst, e), max(worst_t, et)
        if c.ks[b] == c.pos[b]:
            want = (c.vnew[b].reshape(-1) + 0.0).to(o.ctx.dtype)  # (the accumulator starts at +0: a -0 of the rounded v comes out as +0)
            assert torch.equal(bits(o.ctx[b]), bits(want)), (line, c.rows[b], "only the appended key is visible: ctx = rounded v")
    old = MEASURED.get(line, (0.0, 0.0, bound))
    MEASURED[line] = (max(worst, old[0]), max(worst_t, old[1]), bound)
    assert worst < bound, (line, c.rows, worst)
    # per head the largest element itself may sit at a tie of the 16-bit store: half an ulp (<= the row bound) plus the fp32 bound
    assert worst_t < (bound if to == L.F32 else bound + 2e-5), (line, c.rows, worst_t, "dims 8 .. 63")


def same_as_16bit(lib, c, o, to, what, **kw):
    """(3) the 16-bit form of the same library on caches holding the same values, k / v pre-rounded: the same ctx bits"""
    o16 = launch(lib, c, to, tc=L.BF16, **kw)
    assert torch.equal(bits(o16.ctx), bits(o.ctx)), what + ("the fp8 form differs from the 16-bit form on the same values",)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = [f"{k:<36s} max relerr {e:9.3e}   dims 8..63 of a head {t:9.3e}   bound {b:.1e}" for k, (e, t, b) in sorted(MEASURED.items())]
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "decode_attn_fp8_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- CPU: the fixture, the case lists, the refusals -----------------------------------------------------------------------
def test_fixture_ties_and_poison():
    """The fixture itself: torch's clamp-and-cast of the ties and edge values (a cast alone turns 500 into NaN); the step rows carry
    them; the poison key, after its rounding to e4m3, scores at least 20 above the largest real score; the poison V is 448."""
    assert e4m3(EDGES).tolist() == EDGES_ROUNDED
    assert e4m3(torch.tensor([460.0, 2.0 ** -9, -(2.0 ** -10)])).tolist() == [448.0, 2.0 ** -9, -0.0]
    assert bool(torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all())
    assert torch.zeros(4).to(torch.float8_e4m3fn).view(torch.uint8).tolist() == [0] * 4  # a zero-filled cache holds +0
    c = mk("fp8", [(97, 40), (1281, 771), (2, 1)])
    assert c.margin >= 20.0 and c.prefix == 0
    assert c.knew[:, :, :6].unique(dim=0).shape[0] == 1 and c.knew[0, 0, :6].tolist() == EDGES_ROUNDED
    assert c.vnew[1, 2, :6].tolist() == EDGES_ROUNDED[::-1]
    b, h = 0, 2
    q = c.qkv[b, 0, h].double() / 8
    sc = (q * c.K[b, h].double()).sum(-1)
    top = max(float(sc[c.vis[b]].max()), float((q * c.knew[b, h].double()).sum()))
    bad = sc[~c.vis[b]]
    assert bad.numel() == c.Smax - (96 - 40) and float(bad.min()) >= top + 20 and float(bad.max()) < top + 40
    assert bool((c.V[b, h][~c.vis[b]] == 448).all()) and float(c.V[b, h][c.vis[b]].abs().max()) < 8
    assert float(c.qkv[:, 0].std()) > 1.8  # q keeps std 2 but for the two scaled dims


def test_case_lists_cover_the_edges():
    for form, f in FORMS.items():
        S = s_edges(f["like"])
        for v in (1, 2, f["SL"], f["U"] + 1, f["W"], f["W"] + 1, f["W"] + f["T"] + 1, f["Smax"]):
            assert v in S, (form, v)
        for Sv, ks in ks_edges(f["like"]):
            assert 0 <= ks <= Sv - 1 < f["Smax"], (form, Sv, ks)
        assert any(ks == Sv - 1 for Sv, ks in ks_edges(f["like"]))


def test_entry_refuses_what_the_fp8_cache_does_not_have(lib):
    """Host only: the split form with an fp8 cache, and an fp8 cache with dh = 32, come back with a status and a message before any
    launch (the host buffer is never read)."""
    host = np.zeros(64, dtype=np.float32)
    hp = host.ctypes.data
    for to in (L.BF16, L.F32):
        st = lib.itts_decode_attn(hp, to, hp, hp, hp, hp, hp, hp, 2, 3, 64, 128, L.FP8, 0, hp, hp, None, 1, None)
        msg = lib.itts_last_error()
        assert st != 0 and b"split form" in msg and b"fp8" in msg, (st, msg)
    st = lib.itts_decode_attn(None, L.BF16, hp, hp, hp, hp, hp, hp, 2, 3, 64, 128, L.FP8, 0, hp, None, None, 1, None)
    assert st != 0 and b"fp8" in lib.itts_last_error()
    st = lib.itts_decode_attn(hp, L.BF16, hp, hp, hp, hp, hp, hp, 2, 3, 32, 128, L.FP8, 0, None, None, None, 1, None)
    assert st != 0 and b"head dim must be 64" in lib.itts_last_error(), (st, lib.itts_last_error())
    # the fp32 cache's message stays what it was
    st = lib.itts_decode_attn(hp, L.BF16, hp, hp, hp, hp, hp, hp, 2, 3, 64, 128, L.F32, 0, hp, hp, None, 1, None)
    assert st != 0 and b"split form needs both partial buffers and a bf16 cache" in lib.itts_last_error()


# ---- GPU: every form at the edges of S and of kv_start ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["S", "kv_start"])
@pytest.mark.parametrize("form", list(FORMS))
def test_form_against_fp64(lib, form, kind):
    f = FORMS[form]
    rows = [(S, 0) for S in s_edges(f["like"])] if kind == "S" else ks_edges(f["like"])
    first = None
    for pairs in deal(rows, f["B"]):
        c = mk(form, pairs)
        o = launch(lib, c, f["to"])
        judge(lib, c, o, f"{form} {kind} edges", f["to"])
        same_as_16bit(lib, c, o, f["to"], (form, pairs))
        if f["to"] == L.BF16:  # (3) the fp32 ctx of the same call, rounded, is the 16-bit ctx: both store the same o / L
            o32 = launch(lib, c, L.F32)
            assert torch.equal(bits(o32.ctx.to(half_of(lib))), bits(o.ctx)), (form, pairs, "16-bit ctx != rounded fp32 ctx")
            if form == "many_fp8":
                same_as_16bit(lib, c, o32, L.F32, (form, pairs, "fp32 ctx"))
        if first is None:
            first = (c, o)
    c, o = first  # (3) two runs agree
    again = launch(lib, c, f["to"])
    assert torch.equal(bits(again.ctx), bits(o.ctx)), (form, c.rows)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["fp8", "fp8_f32ctx"])
def test_row_alone_equals_row_in_a_batch(lib, form):
    """(3) the same (row, head) problem in row 0 alone and in row r of a 2-, 3- and 4-row call: the same bits"""
    f = FORMS[form]
    pairs = [(f["W"] + 1, 3), (f["U"], 0), (f["W"] + f["T"] + 2, f["SL"] + 1), (2, 0)]
    alone = []
    for p in pairs:
        c = mk(form, [p])
        o = launch(lib, c, f["to"])
        judge(lib, c, o, f"{form} rows alone", f["to"])
        alone.append(bits(o.ctx))
    for B in (2, 3, 4):
        c = mk(form, pairs[:B])
        o = launch(lib, c, f["to"])
        judge(lib, c, o, f"{form} rows alone", f["to"])
        for r in range(B):
            assert torch.equal(bits(o.ctx)[r], alone[r][0]), (form, f"row {r} alone differs from row {r} of {B}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 17])
def test_tiled_ctx(lib, B):
    """(3) ctx in MFMA-fragment tiles, un-tiled, is the row-major ctx of the same problem; padding rows of the last tile stay"""
    S = [1, 2, 127, 128, 129, 255, 256, 257, 300, 64, 200, 299, 5, 131, 290, 33, 250]
    ks = [0, 1, 0, 127, 3, 254, 0, 129, 1, 63, 128, 0, 2, 0, 270, 32, 249]
    c = mk("fp8", list(zip(S[:B], ks[:B])), Smax=300)
    plain = launch(lib, c, L.BF16)
    judge(lib, c, plain, "fp8 tiled ctx", L.BF16)
    tiled = launch(lib, c, L.BF16, tiled=1)
    assert torch.equal(bits(tiled.ctx), bits(plain.ctx)), B
    same_as_16bit(lib, c, tiled, L.BF16, ("tiled", B), tiled=1)


# ---- GPU: the beam ancestry over byte-sized blocks ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,nb", [(form, nb) for form in ("fp8", "many_fp8") for nb in (2, 3, 4)])
def test_ancestry_gather(lib, form, nb):
    """(3) ANC with the identity ancestry = the plain form; ANC over a scattered history = the plain form on the gathered cache.
    The append lands in the beam's own physical row whatever the ancestry says (checked by launch)."""
    f = FORMS[form]
    B = {2: 8, 3: 9, 4: 8}[nb] if f["B"] else {2: 4, 3: 3, 4: 4}[nb]
    items = B // nb
    Ss = [f["W"] + 3, f["W"] + f["T"] + 2, f["U"] + 2, f["SL"] + 1]
    Ss = Ss[nb - 3:nb - 2] if items == 1 else Ss[:items]
    kss = [0, 5, 1, f["SL"] - 1]
    c = mk(form, [(Ss[b // nb], kss[(b % nb) % 4]) for b in range(B)], salt=nb)
    plain = launch(lib, c, f["to"])
    judge(lib, c, plain, f"{form} ancestry", f["to"])
    ident = (torch.arange(B) % nb).to(torch.uint8)[None, :, None].expand(2, B, c.Smax).contiguous()
    o = launch(lib, c, f["to"], anc=ident, nb=nb)
    assert torch.equal(bits(o.ctx), bits(plain.ctx)), (form, nb, "identity ancestry != plain")
    true, other = ancestry(c, nb, f"da8.anc.{form}.{nb}"), ancestry(c, nb, f"da8.anc2.{form}.{nb}")
    phys = scattered(c, nb, true)
    assert not torch.equal(true, other)
    anc = torch.empty(2, B, c.Smax, dtype=torch.uint8)
    for b in range(B):
        t = true[b].clone()
        t[c.pos[b]:] = 255  # the kernel clamps what it reads there
        anc[c.len[b] & 1, b], anc[1 - (c.len[b] & 1), b] = t.to(torch.uint8), other[b].to(torch.uint8)
    o = launch(lib, c, f["to"], anc=anc, nb=nb, phys=phys)
    assert torch.equal(bits(o.ctx), bits(plain.ctx)), (form, nb, "scattered ancestry != plain on the gathered cache")
    same_as_16bit(lib, c, o, f["to"], (form, nb, "scattered ancestry"), anc=anc, nb=nb, phys=phys)


# ---- GPU: the IEEE-half library -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ieee_half_library():
    """the same sources with binary16 as the 16-bit type: the e4m3 cache is the same bytes, 2^-10 for the half ctx"""
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    lib16 = L.load("f16")
    f = FORMS["fp8"]
    c = mk("fp8", [(f["W"] + f["T"] + 1, f["SL"] + 1), (f["W"], 0), (f["U"] + 1, f["U"]), (2, 0)])
    assert half_of(lib16) == torch.float16
    o = launch(lib16, c, L.BF16)
    assert o.ctx.dtype == torch.float16
    judge(lib16, c, o, "fp8 [IEEE half]", L.BF16)
    same_as_16bit(lib16, c, o, L.BF16, ("IEEE half",))
    o32 = launch(lib16, c, L.F32)
    assert torch.equal(bits(o32.ctx.to(torch.float16)), bits(o.ctx))
