"""Operator-level tests of the prefill attention, one kernel at a time, through itts_attention_kernel (include/itts_hip.h):
attn_simple_kernel (csrc/attention.hip, vector ALU; kernel 1) in fp32 and in the library's 16-bit type, attn_mfma_kernel<64 | 128>
(csrc/attention_mfma.hip, matrix cores; kernel 2) in the 16-bit type.  Both builds of the library (bf16 / IEEE half); inputs come
from itts_hip.prng and are rounded to the call's torch dtype.  Each kernel is judged against fp64, never against the other.

Reference: fp64 torch on the CPU from the SAME rounded inputs.  Scores q . k * scale (scale = 1/8 everywhere); key j is visible to
query i iff kv_start[b] <= j < Sk and, when causal, j <= i + (Sk - Sq); softmax over the visible keys, times V: `ref`.  Beside it
E[i][d] = sum_j p_ij |v_jd| in fp64, and the same formula evaluated in torch fp32 on the CPU: E32 = max |ref32 - ref| / max E.

Inputs: K and V std 1, q std 2 (1.4 at dqk = 128: scores of std 2); dim 0 of every query is exactly 2.0, so that one key vector
can score high for every query of a head.  "flat": as said.  "ramp": additionally k[j][0] = 4 j, i.e. a score step of 1 per key
(exact in bf16 up to j = 255, so ramp cases keep Sk <= 256): every key beyond the causal diagonal outscores every visible one and the
running maximum rises in every tile.

Poison, finite: every key row j < kv_start[b] and 64 guard rows behind the last item of k and of v hold K = P * e0 with P chosen so
that its score is the largest visible score of the case plus 30, and V = 1000 - admitted with any weight it wrecks the row.  The
fp64 reference of the poisoned and of the unpoisoned tensors is asserted to be the same tensor.  Where a tensor has ld > H * d
(layout "sep": separate q, k, v with ld = H * d + 8) the gap columns hold NaN; layout "fused" is one [rows][H * (2 dqk + dv)] tensor
with the three pointers offset into it, o dense.  o is pre-filled with NaN where the call stores, a sentinel in the ldo gap and in
one row past the end; afterwards the sentinels are intact (as integers) and everything stored is finite.  All reads the tests
arrange stay inside the allocations (the guard rows are part of the tensors); nothing here provokes a refusal or a fault - the
refusals are tests/test_attention_api.py's, on the host.

Bound, per element of every row that has a visible key:
    |got - ref| <= a * E + b * |ref| + fb * max(E)
a = unit roundoff of the type the kernel rounds P to (matrix-core kernel: 2^-8 bf16 / 2^-11 IEEE half; vector kernel: 0 - its P
stays fp32), b = unit roundoff of the stored type (2^-8 / 2^-11 / 0 for fp32), fb = max(2e-5, 4 * E32), the project's fp32 class
(E32 from the CPU formula above, never from a kernel).  Derivation: the kernel's l sums the unrounded p, so the rounded P costs
|sum_j (p~_ij - p_ij) v_jd| / l <= a * sum_j p_ij |v_jd| = a * E; the store rounds once, b * |ref| (to first order); the fp32
arithmetic of scores, exponentials and sums is the fp32 class, relative to the largest E of the call.
A row without a visible key is exactly +0 in every element, compared as integers.

Bit-exact relations, compared as integers, for each kernel: two runs agree; a batch item alone = that item within the batch; one
head alone (H = 1, pointers moved to the head) = that head within the call; rows 0 .. n-1 of a causal Sq = Sk = S call = the causal
Sq = Sk = n call on the first n rows (the prefix property the K/V cache relies on; n = 63, 64, 65 at S = 130); itts_attention =
itts_attention_kernel(..., itts_attention_which(...)).  Before a call that names kernel 2, itts_attention_which is asked.

The measured maxima, E32 and the worst share of the bound per form are printed and, where ITTS_TEST_OUT names a directory, written
to attention_ops.txt there (committed as profiles/attention_ops.txt)."""
import collections
import ctypes as C
import functools
import os

import pytest
import torch

from itts_hip import lib as L
from itts_hip import prng

DEV = "cuda:0"
HALF = {"bf16": (torch.bfloat16, 2.0 ** -8), "f16": (torch.float16, 2.0 ** -11)}  # torch dtype, unit roundoff
SCALE = 0.125
SENT = 777.0
GUARD = 64      # poisoned rows behind the last item of k and of v
FB_FLOOR = 2e-5  # the project's fp32 class
SIMPLE, MFMA = 1, 2
# form -> (kernel, 16-bit storage?)
FORMS = {"mfma": (MFMA, True), "simple16": (SIMPLE, True), "simple32": (SIMPLE, False)}

# kvs: kv_start per item or None (no kv_start array); data "flat" / "ramp"; layout "fused" (Sq == Sk only) / "sep"
Case = collections.namedtuple("Case", "B H Sq Sk dqk dv causal kvs data layout")


def case(B, Sq, Sk, causal, kvs=None, data="flat", layout=None, H=3, dqk=64, dv=64):
    assert kvs is None or len(kvs) == B
    assert data == "flat" or Sk <= 256
    return Case(B, H, Sq, Sk, dqk, dv, causal, kvs, data, layout or ("fused" if Sq == Sk else "sep"))


def case_id(c):
    kv = "" if c.kvs is None else "kv" + "_".join(map(str, c.kvs))
    return f"B{c.B}H{c.H}_{c.Sq}x{c.Sk}_d{c.dqk}_{c.dv}_{'c' if c.causal else 'n'}{kv}_{c.data}_{c.layout}"


def both(*a, **kw):
    return [case(*a, data=d, **kw) for d in ("flat", "ramp")]


# ---- head dim 64, both kernels -------------------------------------------------------------------------------------------------
COMMON = (
    # Sk over the key-tile edges, non-causal, kv_start absent / mixed (Sk - 1: one visible key; Sk: zeros for the whole item)
    [case(2, 17, Sk, 0, kvs) for Sk, kvs in ((1, None), (63, (0, 62)), (64, (1, 64)), (65, (64, 63)), (128, (65, 127)), (129, (128, 1)),
                                             (200, (130, 199)))]
    # causal Sq == Sk (the GPT prefill), fused qkv layout; every Sq edge of the 64-query workgroup and the 16-query wave
    + [case(2, S, S, 1, kvs) for S, kvs in ((16, (0, 1)), (17, (0, 16)), (63, (0, 62)), (64, (1, 63)), (65, (0, 64)))]
    + both(2, 130, 130, 1, (0, 65))       # the last workgroup has whole waves past Sq
    + both(3, 200, 200, 1, (0, 1, 63))
    + both(3, 200, 200, 1, (64, 65, 130))   # whole 64-key tiles without a visible key
    + both(3, 200, 200, 1, (199, 200, 0))   # one visible key; none at all
    + both(3, 130, 130, 1, (129, 130, 64), layout="sep")
    # causal, Sk > Sq and Sk < Sq (there the first 50 rows see no key)
    + both(2, 96, 200, 1, (0, 130)) + both(2, 96, 200, 1, None)
    # Sk - Sq = 1: the last query's last key opens a key tile of its own, so the causal end of the key loop (kend) has to be exact
    + both(2, 64, 65, 1, (0, 3))
    + both(2, 80, 30, 1, (0, 1)) + both(1, 80, 30, 1, None)
    # non-causal cross attention (perceiver): 32 x 290
    + [case(2, 32, 290, 0, None), case(3, 32, 290, 0, (64, 289, 290))]
    + both(2, 64, 256, 0, (63, 255))
)
# ---- matrix-core kernel only: Sq 16 .. 130 are in COMMON; the 128-wide keys of the conformer's rel-pos attention ---------------
MFMA_CASES = COMMON + [case(2, 70, 133, 0, None, dqk=128), case(2, 70, 133, 0, (0, 65), dqk=128), case(2, 65, 65, 1, (0, 3), dqk=128, layout="sep"),
                       case(2, 65, 65, 1, None, dqk=128, layout="fused")]
# ---- vector kernel only: Sq below the matrix-core kernel's 16, the other head dims (conformer on the fp32 engine 128 / 64, the
# micro configuration 64 / 32, idle lanes 32 / 16, no power of two 80 / 48) --------------------------------------------------------
DIMS = ((64, 64), (128, 64), (64, 32), (32, 16), (80, 48))
SIMPLE_CASES = (COMMON + [case(2, S, S, 1, kvs) for S, kvs in ((1, (0, 1)), (15, (0, 14)))] + [case(1, 1, 65, 1, None), case(2, 15, 129, 0, (0, 64))]
                + [c for dqk, dv in DIMS[1:] for c in (case(2, 65, 65, 1, (0, 3), dqk=dqk, dv=dv), case(2, 17, 129, 0, (64, 1), dqk=dqk, dv=dv),
                                                       case(2, 65, 65, 1, (0, 64), "ramp", "sep", dqk=dqk, dv=dv))])
PREFIX_CASE = case(2, 130, 130, 1, (0, 3))
PREFIX_N = (63, 64, 65)


def cases_of(form):
    return MFMA_CASES if form == "mfma" else SIMPLE_CASES


def rnd(name, shape, std=1.0):
    return torch.from_numpy(prng.tensor(name, 5, shape, std=std))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    """Wait for the launch; a device fault ends the session there (nothing more is started on a faulted GPU)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


def ok(lib, status, what):
    """A refused call fails the test; a HIP error ends the session like a fault seen at the synchronisation."""
    if status == -2:  # ITTS_E_HIP
        pytest.exit(f"HIP error in {what}, nothing more is launched: {lib.itts_last_error()}", returncode=3)
    L.check(status, what, lib)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- inputs and references (CPU) -----------------------------------------------------------------------------------------------
def visible(c, Sq=None, Sk=None, kvs=None):
    """[B, 1, Sq, Sk] bool"""
    Sq, Sk = Sq or c.Sq, Sk or c.Sk
    kvs = (c.kvs or (0,) * c.B) if kvs is None else kvs
    j, i = torch.arange(Sk)[None, :], torch.arange(Sq)[:, None]
    vis = torch.ones(len(kvs), 1, Sq, Sk, dtype=torch.bool)
    if c.causal:
        vis &= (j <= i + (Sk - Sq))[None, None]
    return vis & (j[None, None] >= torch.tensor(kvs).view(-1, 1, 1, 1))


def attend(q, k, v, vis, dt):
    """q [B, Sq, H, dqk], k [B, Sk, H, dqk], v [B, Sk, H, dv] -> (out, E, masked scores) in dtype dt; rows without a visible key are 0"""
    s = torch.einsum("bihd,bjhd->bhij", q.to(dt), k.to(dt)) * SCALE
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = p.sum(-1, keepdim=True)
    p = p / torch.where(l > 0, l, torch.ones_like(l))
    return torch.einsum("bhij,bjhd->bihd", p, v.to(dt)), torch.einsum("bhij,bjhd->bihd", p, v.to(dt).abs()), s


@functools.lru_cache(maxsize=None)
def fixture(c, tdt):
    """The problem of a case in torch dtype tdt: rounded inputs (held in tdt, poisoned), the fp64 reference, E, E32, the rows that see a key"""
    name = "attn." + case_id(c)
    q = rnd(name + ".q", (c.B, c.Sq, c.H, c.dqk), 1.4 if c.dqk == 128 else 2.0)
    k = rnd(name + ".k", (c.B, c.Sk, c.H, c.dqk))
    v = rnd(name + ".v", (c.B, c.Sk, c.H, c.dv))
    q[..., 0] = 2.0
    if c.data == "ramp":
        k[..., 0] = 4.0 * torch.arange(c.Sk, dtype=torch.float32)[None, :, None]
    q, k, v = q.to(tdt), k.to(tdt), v.to(tdt)
    if c.data == "ramp":
        assert torch.equal(k[0, :, 0, 0].double(), 4.0 * torch.arange(c.Sk, dtype=torch.float64))
    vis = visible(c)
    ref, E, s = attend(q, k, v, vis, torch.float64)
    ref32, _, _ = attend(q, k, v, vis, torch.float32)
    live = vis.any(-1)[:, 0]  # [B, Sq]
    assert bool(live.any()) and bool(torch.isfinite(ref).all())
    top = float(s[torch.isfinite(s)].max())
    P = torch.tensor((top + 30.0) / (2.0 * SCALE)).to(tdt)  # q[0] = 2: the poison row scores P * 2 * SCALE = top + 30, up to P's rounding
    assert float(P) * 2.0 * SCALE >= top + 29.0 and bool(torch.isfinite(P))
    krow = torch.zeros(c.dqk, dtype=tdt)
    krow[0] = P
    for b in range(c.B):
        n = (c.kvs or (0,) * c.B)[b]
        k[b, :n] = krow
        v[b, :n] = 1000.0
    refp, Ep, _ = attend(q, k, v, vis, torch.float64)
    assert torch.equal(refp, ref) and torch.equal(Ep, E)  # the poison is invisible to the reference
    Emax = float(E[live].max())
    e32 = float((ref32.double() - ref)[live].abs().max()) / Emax
    return dict(case=c, tdt=tdt, q=q, k=k, v=v, krow=krow, ref=ref, E=E, Emax=Emax, e32=e32, live=live)


def bound_share(fx, got, a, b):
    """-> the largest |got - ref| / bound over the rows with a visible key, and the largest error over max E"""
    fb = max(FB_FLOOR, 4.0 * fx["e32"])
    live = fx["live"]
    err = (got.double() - fx["ref"]).abs()[live]
    bound = (a * fx["E"] + b * fx["ref"].abs() + fb * fx["Emax"])[live]
    return float((err / bound).max()), float(err.max()) / fx["Emax"]


def zero_rows_are_plus_zero(fx, got):
    dead = ~fx["live"]
    return not bool(dead.any()) or not bool((bits(got[dead]) != 0).any())


# ---- the launch ----------------------------------------------------------------------------------------------------------------
class Device:
    """The tensors of a fixture on the GPU in the case's layout, with guard rows and NaN gaps"""

    def __init__(self, fx):
        c, tdt = fx["case"], fx["tdt"]
        self.fx, self.c, self.es = fx, c, torch.empty(0, dtype=tdt).element_size()
        wq, wk, wv = c.H * c.dqk, c.H * c.dqk, c.H * c.dv
        nq, nk = c.B * c.Sq, c.B * c.Sk
        kg = fx["krow"].repeat(c.H)
        if c.layout == "fused":
            assert c.Sq == c.Sk
            ld = wq + wk + wv
            t = torch.full((nk + GUARD, ld), float("nan"), dtype=tdt)  # the q part of the guard rows is never read
            t[:nq, :wq] = fx["q"].reshape(nq, wq)
            t[:nk, wq:wq + wk] = fx["k"].reshape(nk, wk)
            t[:nk, wq + wk:] = fx["v"].reshape(nk, wv)
            t[nk:, wq:wq + wk] = kg
            t[nk:, wq + wk:] = 1000.0
            self.t = t.to(DEV)
            base = self.t.data_ptr()
            self.q, self.k, self.v = base, base + wq * self.es, base + (wq + wk) * self.es
            self.ldq = self.ldk = self.ldv = ld
            self.ldo = wv
        else:
            tq = torch.full((nq, wq + 8), float("nan"), dtype=tdt)
            tq[:, :wq] = fx["q"].reshape(nq, wq)
            tk = torch.full((nk + GUARD, wk + 8), float("nan"), dtype=tdt)
            tk[:nk, :wk] = fx["k"].reshape(nk, wk)
            tk[nk:, :wk] = kg
            tv = torch.full((nk + GUARD, wv + 8), float("nan"), dtype=tdt)
            tv[:nk, :wv] = fx["v"].reshape(nk, wv)
            tv[nk:, :wv] = 1000.0
            self.tq, self.tk, self.tv = tq.to(DEV), tk.to(DEV), tv.to(DEV)
            self.q, self.k, self.v = self.tq.data_ptr(), self.tk.data_ptr(), self.tv.data_ptr()
            self.ldq, self.ldk, self.ldv, self.ldo = wq + 8, wk + 8, wv + 8, wv + 8
        self.kvs = None if c.kvs is None else torch.tensor(c.kvs, dtype=torch.int32).to(DEV)

    def args(self, b0=0, B=None, h0=0, H=None, n=None):
        """The arguments of itts_attention_which for items b0 .. b0 + B - 1, heads h0 .. h0 + H - 1 (pointers moved there); n: the causal
        Sq = Sk = n call on the first n rows of one item"""
        c, es = self.c, self.es
        B, H = B or c.B - b0, H or c.H - h0
        Sq, Sk = (n, n) if n else (c.Sq, c.Sk)
        assert 0 <= b0 and b0 + B <= c.B and 0 <= h0 and h0 + H <= c.H and 1 <= Sq <= c.Sq and 1 <= Sk <= c.Sk and (n is None or B == 1)
        q = self.q + (b0 * c.Sq * self.ldq + h0 * c.dqk) * es
        k = self.k + (b0 * c.Sk * self.ldk + h0 * c.dqk) * es
        v = self.v + (b0 * c.Sk * self.ldv + h0 * c.dv) * es
        kvs = None if self.kvs is None else self.kvs.data_ptr() + 4 * b0
        dt = L.F32 if self.fx["tdt"] == torch.float32 else L.BF16
        return (q, k, v, B, H, Sq, Sk, c.dqk, c.dv, self.ldq, self.ldk, self.ldv, self.ldo, SCALE, c.causal, kvs, dt)

    def run(self, lib, kernel, entry="kernel", **part):
        """entry "kernel": itts_attention_kernel(kernel; None = the one itts_attention_which names), "attention": itts_attention.
        -> ([B, Sq, H, dv] on the CPU, after the sentinel and finiteness checks; what itts_attention_which said)"""
        c, tdt = self.c, self.fx["tdt"]
        args = self.args(**part)
        B, H, Sq = args[3], args[4], args[5]
        w = H * c.dv
        o = torch.full((B * Sq + 1, self.ldo), SENT, dtype=tdt)
        o[:B * Sq, :w] = float("nan")
        before = bits(o).clone()
        od = o.to(DEV)
        which = lib.itts_attention_which(*args)
        assert which in (SIMPLE, MFMA), (case_id(c), which, lib.itts_last_error())
        if kernel == MFMA:  # asked before the kernel is named; every case of the matrix-core tables is one its rule takes
            assert which == MFMA or os.environ.get("ITTS_ATTN_SIMPLE") is not None, (case_id(c), which)
        if entry == "attention":
            ok(lib, lib.itts_attention(od.data_ptr(), *args, stream()), "itts_attention")
        else:
            ok(lib, lib.itts_attention_kernel(od.data_ptr(), *args, which if kernel is None else kernel, stream()), "itts_attention_kernel")
        sync()
        got = od.cpu()
        stored = torch.zeros(o.shape, dtype=torch.bool)
        stored[:B * Sq, :w] = True
        assert torch.equal(bits(got)[~stored], before[~stored]), (case_id(c), "a sentinel was overwritten")
        out = got[:B * Sq, :w]
        assert bool(torch.isfinite(out).all()), (case_id(c), "NaN / Inf or an element never stored")
        return out.reshape(B, Sq, H, c.dv), which


MEASURED = {}  # "<build> <form>" -> list of (case id, share, err / max E, e32)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = []
    for group in sorted(MEASURED):
        lines += [f"{group:<14s} | {cid:<52s} err/bound {s:6.3f}   err/maxE {e:9.3e}   E32 {e32:9.3e}" for cid, s, e, e32 in MEASURED[group]]
    for group in sorted(MEASURED):
        rows = MEASURED[group]
        lines.append(f"{group} largest over {len(rows)} cases: err/bound {max(r[1] for r in rows):.3f} (limit 1), err/maxE {max(r[2] for r in rows):.3e}, "
                     f"E32 {max(r[3] for r in rows):.3e}")
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "attention_ops.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def roundoffs(form, half):
    """(a, b) of the bound"""
    u = HALF[half][1]
    return (u if form == "mfma" else 0.0), (u if FORMS[form][1] else 0.0)


def fixture_of(c, form, half):
    return fixture(c, HALF[half][0] if FORMS[form][1] else torch.float32)


def check_vs_fp64(fx, got, form, half):
    c = fx["case"]
    a, b = roundoffs(form, half)
    share, err = bound_share(fx, got, a, b)
    MEASURED.setdefault(f"{half} {form}", []).append((case_id(c), share, err, fx["e32"]))
    print(f"{half} {form} {case_id(c)}: err/bound {share:.3f} err/maxE {err:.3e} E32 {fx['e32']:.3e}")
    assert zero_rows_are_plus_zero(fx, got), (case_id(c), "a row without a visible key is not +0")
    assert share <= 1.0, (case_id(c), form, half, share, err, fx["e32"])


# ---- the tests ----------------------------------------------------------------------------------------------------------------
ALL = [(form, c) for form in FORMS for c in cases_of(form)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,c", ALL, ids=lambda v: v if isinstance(v, str) else case_id(v))
@pytest.mark.parametrize("half", tuple(HALF))
def test_attention_kernel_vs_fp64(half, form, c):
    """One kernel on one case: the bound against fp64 and exact zeros; two runs agree; every item alone and every head alone equal
    their part of the whole call; where the dispatcher takes this kernel for the call, itts_attention gives the same bits."""
    lib = L.load(half)
    kernel = FORMS[form][0]
    fx = fixture_of(c, form, half)
    dev = Device(fx)
    got, which = dev.run(lib, kernel)
    check_vs_fp64(fx, got, form, half)
    again, _ = dev.run(lib, kernel)
    assert torch.equal(bits(got), bits(again)), "two runs differ"
    for b in range(c.B if c.B > 1 else 0):
        alone, _ = dev.run(lib, kernel, b0=b, B=1)
        assert torch.equal(bits(alone), bits(got[b:b + 1])), f"item {b} alone differs"
    for h in range(c.H):
        alone, _ = dev.run(lib, kernel, h0=h, H=1)
        assert torch.equal(bits(alone), bits(got[:, :, h:h + 1])), f"head {h} alone differs"
    if which == kernel:
        entry, _ = dev.run(lib, kernel, entry="attention")
        assert torch.equal(bits(entry), bits(got)), "itts_attention differs from the kernel it dispatches to"


@pytest.mark.gpu
@pytest.mark.parametrize("form", tuple(FORMS))
@pytest.mark.parametrize("half", tuple(HALF))
def test_attention_causal_prefix_property(half, form):
    """Rows 0 .. n-1 of the causal S x S call = the causal n x n call on the first n rows, to the bit (what the K/V cache relies on),
    for n on both sides of the 64-key tile, per item (the second one left-padded)."""
    lib = L.load(half)
    kernel = FORMS[form][0]
    c = PREFIX_CASE
    dev = Device(fixture_of(c, form, half))
    whole, _ = dev.run(lib, kernel)
    for n in PREFIX_N:
        for b in range(c.B):
            part, _ = dev.run(lib, kernel, b0=b, B=1, n=n)
            assert torch.equal(bits(part), bits(whole[b:b + 1, :n])), (n, b)


DISPATCHED = (("simple16", case(2, 15, 15, 1, (0, 14))), ("simple16", case(2, 16, 16, 1, (0, 1))), ("simple16", case(2, 17, 129, 0, (64, 1), dv=32)),
              ("simple16", case(2, 70, 133, 0, None, dqk=128)), ("simple32", case(2, 65, 65, 1, (0, 64))), ("simple16", case(3, 200, 200, 1, (64, 65, 130))))


@pytest.mark.gpu
@pytest.mark.parametrize("half", tuple(HALF))
def test_itts_attention_is_the_kernel_which_names(half):
    """itts_attention = itts_attention_kernel(..., itts_attention_which(...)) to the bit, on calls the dispatcher sends to either kernel
    (unless ITTS_ATTN_SIMPLE keeps it on the vector kernel)."""
    lib = L.load(half)
    seen = set()
    for form, c in DISPATCHED:
        dev = Device(fixture_of(c, form, half))
        entry, which = dev.run(lib, None, entry="attention")
        named, _ = dev.run(lib, None)
        assert torch.equal(bits(entry), bits(named)), (case_id(c), which)
        seen.add(which)
    assert seen == ({SIMPLE} if os.environ.get("ITTS_ATTN_SIMPLE") is not None else {SIMPLE, MFMA})
