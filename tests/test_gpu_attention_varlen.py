"""Operator-level tests of the packed (variable-length) causal attention, one kernel at a time, through itts_attention_varlen
(include/itts_hip.h): attn_varlen_simple_kernel (csrc/attention_varlen.hip, vector ALU; kernel 1) in fp32 and in the library's 16-bit
type, attn_varlen_mfma_kernel (matrix cores; kernel 2) in the 16-bit type.  Both builds of the library.  The reference, the bound, the
roundoffs, the integer comparison and the poison scheme are those of tests/test_gpu_attention.py, imported from there, not restated:
fp64 torch on the CPU from the SAME rounded inputs, per sequence; |got - ref| <= a * E + b * |ref| + fb * max E with that file's a / b /
fb (max E and E32 per sequence).  Every query sees itself, so no row is without a visible key.

Sequence b owns rows [off[b], off[b + 1]) of q, k, v, o.  Inputs per sequence as in that file: K and V std 1, q std 2 with dim 0 exactly
2.0; "ramp": k[j][0] = 4 j with j the position in its OWN sequence (lengths <= 256), so every key past the diagonal outscores every
visible one.  Layout "fused": one [rows][H * (2 * 64 + 64)] tensor with three offset pointers (the engine's qkv), o dense; "sep":
separate tensors with ld = H * d + 8 and NaN in the gap columns, o with a gap too.  64 poison rows (K = P * e0 scoring the largest
visible score + 30, V = 1000) lie in front of the first and behind the last sequence of every call, in k and in v; o is pre-filled with
NaN where the call stores and a sentinel in the ldo gap and in one row past the end, which have to be intact afterwards, compared as
integers; everything stored has to be finite.  All reads stay inside the allocations; nothing here provokes a refusal or a fault -
the refusals are tests/test_packed_latent_api.py's, on the host.

Bit-exact relations, compared as integers, for each kernel: two runs agree; each sequence ALONE (nseq = 1, a copy of its rows between
the poison rows) = that sequence in the packed call; the sequences in a permuted order; one head alone; the first n rows of a
length-130 sequence = the length-n sequence (n = 63, 64, 65); itts_attention_varlen's dispatcher = the kernel
itts_attention_varlen_which names; and the anchor: each sequence = itts_attention_kernel(B = 1, Sq = Sk = len, causal = 1, kv_start =
NULL) of the same family on its rows, for every length that entry takes (its matrix-core rule needs Sq >= 16).

The measured shares of the bound are printed and, where ITTS_TEST_OUT names a directory, appended to packed_latent.txt there."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_attention as T
from itts_hip import lib as L

DEV = T.DEV
H, D = 3, 64
LENSETS = ((1,), (16,), (64,), (65,), (15, 16, 17), (63, 64, 65), (1, 129, 64, 130), (200, 1, 1, 1, 70), tuple(1 + (7 * i) % 37 for i in range(128)))
LAYOUTS = ("fused", "sep")
DATA = ("flat", "ramp")


def set_id(lens):
    return "n128" if len(lens) == 128 else "L" + "_".join(map(str, lens))


def tdt_of(form, half):
    return T.HALF[half][0] if T.FORMS[form][1] else torch.float32


@functools.lru_cache(maxsize=None)
def seq_data(tag, n, data, tdt):
    """One sequence: rounded q, k, v [n, H, 64] and what the bound needs of its fp64 reference (T.bound_share reads ref, E, Emax, e32, live)"""
    q = T.rnd(tag + ".q", (1, n, H, D), 2.0)
    k = T.rnd(tag + ".k", (1, n, H, D))
    v = T.rnd(tag + ".v", (1, n, H, D))
    q[..., 0] = 2.0
    if data == "ramp":
        assert n <= 256
        k[..., 0] = 4.0 * torch.arange(n, dtype=torch.float32)[None, :, None]
    q, k, v = q.to(tdt), k.to(tdt), v.to(tdt)
    j, i = torch.arange(n)[None, :], torch.arange(n)[:, None]
    vis = (j <= i)[None, None]
    ref, E, s = T.attend(q, k, v, vis, torch.float64)
    ref32, _, _ = T.attend(q, k, v, vis, torch.float32)
    live = torch.ones(1, n, dtype=torch.bool)
    Emax = float(E.max())
    e32 = float((ref32.double() - ref).abs().max()) / Emax
    assert bool(torch.isfinite(ref).all())
    return dict(q=q[0], k=k[0], v=v[0], ref=ref, E=E, Emax=Emax, e32=e32, live=live, top=float(s[torch.isfinite(s)].max()))


@functools.lru_cache(maxsize=None)
def problem(lens, data, tdt):
    """The sequences of a length set and the poison key row of the call (T.fixture's rule: the largest visible score + 30)"""
    seqs = [seq_data(f"varlen.{set_id(lens)}.{i}", n, data, tdt) for i, n in enumerate(lens)]
    return seqs, poison_row(seqs, tdt)


def poison_row(seqs, tdt):
    top = max(s["top"] for s in seqs)
    P = torch.tensor((top + 30.0) / (2.0 * T.SCALE)).to(tdt)
    assert float(P) * 2.0 * T.SCALE >= top + 29.0 and bool(torch.isfinite(P))
    krow = torch.zeros(D, dtype=tdt)
    krow[0] = P
    return krow


class Packed:
    """Sequences back to back on the GPU in a layout, T.GUARD poison rows in front of the first and behind the last one (k, v)"""

    def __init__(self, seqs, krow, tdt, layout):
        self.tdt, self.es = tdt, torch.empty(0, dtype=tdt).element_size()
        self.lens = [int(s["q"].shape[0]) for s in seqs]
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        n, G, w = int(self.off[-1]), T.GUARD, H * D
        self.n = n
        q = torch.cat([s["q"] for s in seqs]).reshape(n, w)
        k = torch.cat([s["k"] for s in seqs]).reshape(n, w)
        v = torch.cat([s["v"] for s in seqs]).reshape(n, w)
        kg = krow.repeat(H)
        nan = float("nan")
        if layout == "fused":
            ld = 3 * w
            t = torch.full((n + 2 * G, ld), nan, dtype=tdt)  # the q part of the guard rows is never read
            t[G:G + n, :w], t[G:G + n, w:2 * w], t[G:G + n, 2 * w:] = q, k, v
            for rows in (slice(0, G), slice(G + n, None)):
                t[rows, w:2 * w] = kg
                t[rows, 2 * w:] = 1000.0
            self.t = t.to(DEV)
            base = self.t.data_ptr() + G * ld * self.es
            self.q, self.k, self.v = base, base + w * self.es, base + 2 * w * self.es
            self.ldq = self.ldk = self.ldv = ld
            self.ldo = w
        else:
            ld = w + 8
            tq = torch.full((n, ld), nan, dtype=tdt)
            tq[:, :w] = q
            tk = torch.full((n + 2 * G, ld), nan, dtype=tdt)
            tv = torch.full((n + 2 * G, ld), nan, dtype=tdt)
            tk[G:G + n, :w], tv[G:G + n, :w] = k, v
            for rows in (slice(0, G), slice(G + n, None)):
                tk[rows, :w] = kg
                tv[rows, :w] = 1000.0
            self.tq, self.tk, self.tv = tq.to(DEV), tk.to(DEV), tv.to(DEV)
            self.q, self.k, self.v = self.tq.data_ptr(), self.tk.data_ptr() + G * ld * self.es, self.tv.data_ptr() + G * ld * self.es
            self.ldq = self.ldk = self.ldv = self.ldo = ld
        self.dt = L.F32 if tdt == torch.float32 else L.BF16

    def _out(self, rows, heads):
        o = torch.full((rows + 1, self.ldo), T.SENT, dtype=self.tdt)
        o[:rows, :heads * D] = float("nan")
        return o, T.bits(o).clone()

    def _check(self, od, before, rows, heads, what):
        got = od.cpu()
        stored = torch.zeros(got.shape, dtype=torch.bool)
        stored[:rows, :heads * D] = True
        assert torch.equal(T.bits(got)[~stored], before[~stored]), (what, "a sentinel was overwritten")
        out = got[:rows, :heads * D]
        assert bool(torch.isfinite(out).all()), (what, "NaN / Inf or an element never stored")
        return out.reshape(rows, heads, D)

    def run(self, lib, kernel, h0=0, heads=H):
        """itts_attention_varlen(kernel) on heads h0 .. h0 + heads - 1 -> ([rows, heads, 64] on the CPU after the sentinel and
        finiteness checks, what itts_attention_varlen_which said for kernel 0)"""
        o, before = self._out(self.n, heads)
        od = o.to(DEV)
        sh = h0 * D * self.es
        args = (self.q + sh, self.k + sh, self.v + sh, self.off.ctypes.data_as(C.c_void_p), len(self.lens), heads, D, D, self.ldq, self.ldk, self.ldv,
                self.ldo, T.SCALE, self.dt)
        which = lib.itts_attention_varlen_which(*args, 0)
        assert which in (T.SIMPLE, T.MFMA), (which, lib.itts_last_error())
        assert lib.itts_attention_varlen_which(*args, kernel) == (kernel or which), (kernel, lib.itts_last_error())  # the call is one the entry takes
        T.ok(lib, lib.itts_attention_varlen(od.data_ptr(), *args, kernel, T.stream()), "itts_attention_varlen")
        T.sync()
        return self._check(od, before, self.n, heads, ("varlen", kernel, self.lens)), which

    def run_old(self, lib, kernel, b):
        """itts_attention_kernel(B = 1, Sq = Sk = len, causal, no kv_start) of the same family on sequence b's rows of these tensors"""
        n, r0 = self.lens[b], int(self.off[b])
        o, before = self._out(n, H)
        od = o.to(DEV)
        args = (self.q + r0 * self.ldq * self.es, self.k + r0 * self.ldk * self.es, self.v + r0 * self.ldv * self.es, 1, H, n, n, D, D,
                self.ldq, self.ldk, self.ldv, self.ldo, T.SCALE, 1, None, self.dt)
        T.ok(lib, lib.itts_attention_kernel(od.data_ptr(), *args, kernel, T.stream()), "itts_attention_kernel")
        T.sync()
        return self._check(od, before, n, H, ("old", kernel, n))


MEASURED = {}  # "<build> <form>" -> list of (case id, share, err / max E, e32)


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    if not MEASURED:
        return
    lines = ["tests/test_gpu_attention_varlen.py: largest share of the fp64 bound over the sequences of each call (limit 1)"]
    for group in sorted(MEASURED):
        rows = MEASURED[group]
        lines += [f"{group:<14s} | {cid:<28s} err/bound {s:6.3f}   err/maxE {e:9.3e}   E32 {e32:9.3e}" for cid, s, e, e32 in rows]
        lines.append(f"{group} largest over {len(rows)} calls: err/bound {max(r[1] for r in rows):.3f} (limit 1), err/maxE {max(r[2] for r in rows):.3e}")
    print("\n" + "\n".join(lines))
    out = os.environ.get("ITTS_TEST_OUT")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "packed_latent.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


def split(p, got):
    return [got[int(p.off[b]):int(p.off[b + 1])] for b in range(len(p.lens))]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("lens", LENSETS, ids=set_id)
@pytest.mark.parametrize("form", tuple(T.FORMS))
@pytest.mark.parametrize("half", tuple(T.HALF))
def test_varlen_kernel(half, form, lens, data, layout):
    """One kernel on one length set: every sequence inside the fp64 bound; two runs agree; every sequence alone, the permuted order and
    every head alone give the bits of the packed call; the dispatcher gives the bits of the kernel it names; every sequence has the bits
    of the existing kernel of the family at B = 1."""
    lib = L.load(half)
    kernel = T.FORMS[form][0]
    tdt = tdt_of(form, half)
    seqs, krow = problem(lens, data, tdt)
    p = Packed(seqs, krow, tdt, layout)
    got, which = p.run(lib, kernel)
    parts = split(p, got)
    a, b = T.roundoffs(form, half)
    share, err, e32 = 0.0, 0.0, 0.0
    for s, g in zip(seqs, parts):
        sh, er = T.bound_share(s, g[None], a, b)
        share, err, e32 = max(share, sh), max(err, er), max(e32, s["e32"])
    cid = f"{set_id(lens)}_{data}_{layout}"
    MEASURED.setdefault(f"{half} {form}", []).append((cid, share, err, e32))
    print(f"{half} {form} {cid}: err/bound {share:.3f} err/maxE {err:.3e} E32 {e32:.3e}")
    assert share <= 1.0, (cid, form, half, share, err, e32)
    again, _ = p.run(lib, kernel)
    assert torch.equal(T.bits(got), T.bits(again)), "two runs differ"
    for i, s in enumerate(seqs):  # alone: nseq = 1, its rows between the poison rows
        alone, _ = Packed([s], krow, tdt, layout).run(lib, kernel)
        assert torch.equal(T.bits(alone), T.bits(parts[i])), f"sequence {i} (length {lens[i]}) alone differs"
    if len(lens) > 1:
        perm = list(reversed(range(len(lens)))) if len(lens) < 4 else [(5 * i + 3) % len(lens) for i in range(len(lens))] if len(lens) == 128 else \
            list(np.roll(np.arange(len(lens)), 2))
        assert sorted(perm) == list(range(len(lens))) and perm != list(range(len(lens)))
        pp = Packed([seqs[i] for i in perm], krow, tdt, layout)
        for j, part in enumerate(split(pp, pp.run(lib, kernel)[0])):
            assert torch.equal(T.bits(part), T.bits(parts[perm[j]])), f"sequence {perm[j]} differs in the permuted order"
    for h in range(H):
        alone, _ = p.run(lib, kernel, h0=h, heads=1)
        assert torch.equal(T.bits(alone), T.bits(got[:, h:h + 1])), f"head {h} alone differs"
    if which == kernel:
        entry, _ = p.run(lib, 0)
        assert torch.equal(T.bits(entry), T.bits(got)), "the dispatcher differs from the kernel it names"
    for i, n in enumerate(lens):  # the anchor: the existing kernel of the family on this sequence alone
        if kernel == T.MFMA and n < 16:
            continue  # attention_mfma's rule needs Sq >= 16 (include/itts_hip.h); the new kernel has no such rule
        assert torch.equal(T.bits(p.run_old(lib, kernel, i)), T.bits(parts[i])), f"sequence {i} (length {n}) differs from itts_attention_kernel at B = 1"


@pytest.mark.gpu
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("form", tuple(T.FORMS))
@pytest.mark.parametrize("half", tuple(T.HALF))
def test_varlen_prefix_property(half, form, data):
    """Rows 0 .. n-1 of a length-130 sequence = the length-n sequence made of its first n rows, to the bit, for n on both sides of the
    64-key tile; the 130-row sequence lies behind a companion."""
    lib = L.load(half)
    kernel = T.FORMS[form][0]
    tdt = tdt_of(form, half)
    s130 = seq_data("varlen.prefix.130", 130, data, tdt)
    comp = seq_data("varlen.prefix.comp", 17, data, tdt)
    krow = poison_row([s130, comp], tdt)
    p = Packed([comp, s130], krow, tdt, "fused")
    whole = split(p, p.run(lib, kernel)[0])[1]
    for n in T.PREFIX_N:
        cut = dict(q=s130["q"][:n], k=s130["k"][:n], v=s130["v"][:n])
        part, _ = Packed([cut], krow, tdt, "fused").run(lib, kernel)
        assert torch.equal(T.bits(part), T.bits(whole[:n])), n


@pytest.mark.gpu
@pytest.mark.parametrize("half", tuple(T.HALF))
def test_the_dispatcher_is_the_kernel_which_names(half):
    """kernel 0 = the kernel itts_attention_varlen_which names, to the bit, on calls the dispatcher sends to either kernel (unless
    ITTS_ATTN_SIMPLE keeps it on the vector kernel) - and a 1-row companion does not move the others to another kernel."""
    lib = L.load(half)
    seen = set()
    for form, lens, layout in (("simple32", (15, 16, 17), "fused"), ("mfma", (15, 16, 17), "fused"), ("mfma", (200, 1, 1, 1, 70), "sep"), ("mfma", (1,), "fused")):
        tdt = tdt_of(form, half)
        seqs, krow = problem(lens, "flat", tdt)
        p = Packed(seqs, krow, tdt, layout)
        entry, which = p.run(lib, 0)
        named, _ = p.run(lib, which)
        assert torch.equal(T.bits(entry), T.bits(named)), (form, lens, which)
        assert which == (T.SIMPLE if form == "simple32" or os.environ.get("ITTS_ATTN_SIMPLE") is not None else T.MFMA), (form, lens, which)
        seen.add(which)
    assert seen == ({T.SIMPLE} if os.environ.get("ITTS_ATTN_SIMPLE") is not None else {T.SIMPLE, T.MFMA})
