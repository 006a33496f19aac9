"""Operator-level tests of the attention for APPENDED rows, one kernel at a time, through itts_attention_append and
itts_kv_rows_append (include/itts_hip.h; csrc/attention_append.hip): attn_append_simple_kernel (kernel 1) in fp32 (dqk 32, dv 16) and in
the library's 16-bit type (dqk = dv = 64), attn_append_mfma_kernel (kernel 2) in the 16-bit type.  Both builds of the library.

Three sequences share every launch and advance unevenly over four calls:
    A, 130 rows: 0 -> 17 (a start inside a tile), 17 -> 64 (an end on a tile edge), 64 -> 65 (one row on the edge), 65 -> 130 (two tiles)
    B,  63 rows: one append from empty
    C,   1 row : appended in the first call, n_new = 0 in the other three
Each sequence owns a block of one K/V history tensor (rows of k | v, ld = H * (dqk + dv)); before every call the rows of its block
behind its new end are filled with NaN, then itts_kv_rows_append copies the chunk's k / v into [pos0, pos0 + n_new) and
itts_attention_append runs.  The chunk's o has one spare row behind every sequence's rows and an ldo gap, all holding a sentinel.

Asserted: every delivered row equals, as raw bits, the row itts_attention_varlen of the SAME kernel number gives in one pass over the
three complete sequences; every o element outside the appended ranges keeps the sentinel (compared as integers); everything stored is
finite; after the last call the history holds the complete k and v, bit for bit.  Against fp64: the delivered rows, put together per
sequence, lie inside the bound of tests/test_gpu_attention.py with that file's a / b / fb - the bars tests/test_gpu_attention_varlen.py
uses for the varlen kernels (imported, not restated; the arithmetic is the same).

The refusals are made on the host before any HIP call; they are asked of itts_attention_append_which (the same check, no launch), and
the two that cannot reach a launch whatever the check does (a null pointer, nseq = 0) of itts_attention_append as well."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_attention as T
from itts_hip import lib as L

DEV = T.DEV
H = 2
LENS = (130, 63, 1)
CAPS = (136, 63, 4)  # history rows per block: B's block ends where B ends
# per call: (pos0, n_new) of A, B, C
CALLS = (((0, 17), (0, 63), (0, 1)), ((17, 47), (63, 0), (1, 0)), ((64, 1), (63, 0), (1, 0)), ((65, 65), (63, 0), (1, 0)))
# form -> (kernel, dqk, dv, 16-bit storage?)
SHAPES = {"mfma": (T.MFMA, 64, 64, True), "simple16": (T.SIMPLE, 64, 64, True), "simple32": (T.SIMPLE, 32, 16, False)}
CASES = [(half, form) for half in T.HALF for form in SHAPES]


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def problem(form, half):
    """The three sequences: rounded q, k, v [n, H, d] and what T.bound_share reads of their fp64 reference"""
    _, dqk, dv, half16 = SHAPES[form]
    tdt = T.HALF[half][0] if half16 else torch.float32
    seqs = []
    for i, n in enumerate(LENS):
        tag = f"append.{form}.{i}"
        q, k, v = T.rnd(tag + ".q", (1, n, H, dqk), 2.0), T.rnd(tag + ".k", (1, n, H, dqk)), T.rnd(tag + ".v", (1, n, H, dv))
        q[..., 0] = 2.0
        q, k, v = q.to(tdt), k.to(tdt), v.to(tdt)
        vis = (torch.arange(n)[None, :] <= torch.arange(n)[:, None])[None, None]
        ref, E, _ = T.attend(q, k, v, vis, torch.float64)
        ref32, _, _ = T.attend(q, k, v, vis, torch.float32)
        Emax = float(E.max())
        seqs.append(dict(q=q[0], k=k[0], v=v[0], ref=ref, E=E, Emax=Emax, e32=float((ref32.double() - ref).abs().max()) / Emax,
                         live=torch.ones(1, n, dtype=torch.bool)))
    return seqs, tdt


def run_case(lib, form, half):
    """-> (delivered rows per sequence [n, H, dv] on the CPU, the complete varlen pass per sequence, the final history, the complete k | v)"""
    kernel, dqk, dv, _ = SHAPES[form]
    seqs, tdt = problem(form, half)
    dt = L.F32 if tdt == torch.float32 else L.BF16
    es = torch.empty(0, dtype=tdt).element_size()
    wq, wv = H * dqk, H * dv
    ld = 2 * wq + wv
    # ---- the complete sequences, packed: the reference bits (itts_attention_varlen of the same kernel number) ----
    n_all = sum(LENS)
    off = i32(np.concatenate([[0], np.cumsum(LENS)]))
    qkv = torch.cat([torch.cat([s["q"].reshape(-1, wq), s["k"].reshape(-1, wq), s["v"].reshape(-1, wv)], 1) for s in seqs]).to(DEV)
    full = torch.full((n_all, wv), float("nan"), dtype=tdt, device=DEV)
    base = qkv.data_ptr()
    T.ok(lib, lib.itts_attention_varlen(full.data_ptr(), base, base + wq * es, base + 2 * wq * es, ptr(off), len(LENS), H, dqk, dv, ld, ld, ld, wv,
                                        T.SCALE, dt, kernel, T.stream()), "itts_attention_varlen")
    T.sync()
    full = full.cpu()
    assert bool(torch.isfinite(full).all())
    # ---- the history: block b = rows [kv_off[b], kv_off[b + 1]) of k | v ----
    ldh = wq + wv
    kv_off = i32(np.concatenate([[0], np.cumsum(CAPS)]))
    hist = torch.full((int(kv_off[-1]), ldh), float("nan"), dtype=tdt, device=DEV)
    hk, hv = hist.data_ptr(), hist.data_ptr() + wq * es
    ldo = wv + 8
    got = [torch.full((n, wv), float("nan"), dtype=tdt) for n in LENS]
    for call in CALLS:
        pos0, n_new = i32([c[0] for c in call]), i32([c[1] for c in call])
        q_off = i32(np.concatenate([[0], np.cumsum(n_new + 1)]))  # one spare row behind every sequence's rows
        rows = int(q_off[-1])
        chunk = torch.full((rows, ld), float("nan"), dtype=tdt)
        for b, (p0, n) in enumerate(call):
            chunk[int(q_off[b]):int(q_off[b]) + n] = qkv[int(off[b]) + p0:int(off[b]) + p0 + n].cpu()
        chunk = chunk.to(DEV)
        o = torch.full((rows + 1, ldo), T.SENT, dtype=tdt)
        stored = torch.zeros(o.shape, dtype=torch.bool)
        for b, (p0, n) in enumerate(call):
            stored[int(q_off[b]):int(q_off[b]) + n, :wv] = True
            hist[int(kv_off[b]) + p0 + n:int(kv_off[b + 1])] = float("nan")  # whatever lies behind the new end is poison
        o[stored] = float("nan")
        before = T.bits(o).clone()
        od = o.to(DEV)
        cb = chunk.data_ptr()
        tabs = (ptr(q_off), ptr(kv_off), ptr(pos0), ptr(n_new), len(LENS))
        T.ok(lib, lib.itts_kv_rows_append(hk, hv, cb + wq * es, cb + 2 * wq * es, *tabs, ld, ldh, ldh, wq, wv, dt, T.stream()), "itts_kv_rows_append")
        args = (cb, hk, hv, *tabs, H, dqk, dv, ld, ldh, ldh, ldo, T.SCALE, dt)
        which = lib.itts_attention_append_which(*args, 0)
        assert which in (T.SIMPLE, T.MFMA), (which, lib.itts_last_error())
        assert lib.itts_attention_append_which(*args, kernel) == kernel, lib.itts_last_error()  # the call is one the entry takes
        T.ok(lib, lib.itts_attention_append(od.data_ptr(), *args, kernel, T.stream()), "itts_attention_append")
        T.sync()
        out = od.cpu()
        assert torch.equal(T.bits(out)[~stored], before[~stored]), (form, half, call, "an o element outside the appended ranges was written")
        assert bool(torch.isfinite(out[stored]).all()), (form, half, call, "NaN / Inf or an element never stored")
        for b, (p0, n) in enumerate(call):
            got[b][p0:p0 + n] = out[int(q_off[b]):int(q_off[b]) + n, :wv]
    kv_full = qkv[:, wq:].cpu()
    return seqs, got, [full[int(off[b]):int(off[b + 1])] for b in range(len(LENS))], hist.cpu(), kv_off, [kv_full[int(off[b]):int(off[b + 1])] for b in range(len(LENS))]


@pytest.mark.gpu
@pytest.mark.parametrize("half,form", CASES, ids=[f"{h}-{f}" for h, f in CASES])
def test_appended_rows_have_the_bits_of_the_complete_pass(half, form):
    lib = L.load(half)
    _, _, dv, _ = SHAPES[form]
    seqs, got, full, hist, kv_off, kv_full = run_case(lib, form, half)
    a, b = T.roundoffs("mfma" if form == "mfma" else "simple16" if SHAPES[form][3] else "simple32", half)
    for i, n in enumerate(LENS):
        assert bool(torch.isfinite(got[i]).all()), f"sequence {i}: a row was never delivered"
        assert torch.equal(T.bits(got[i]), T.bits(full[i])), f"sequence {i} (length {n}) differs from itts_attention_varlen over the complete sequences"
        assert torch.equal(T.bits(hist[int(kv_off[i]):int(kv_off[i]) + n]), T.bits(kv_full[i])), f"sequence {i}: the history is not its k | v"
        share, err = T.bound_share(seqs[i], got[i].reshape(1, n, H, dv), a, b)
        print(f"{half} {form} sequence {i}: err/bound {share:.3f} err/maxE {err:.3e} E32 {seqs[i]['e32']:.3e}")
        assert share <= 1.0, (half, form, i, share, err)


@pytest.mark.gpu
@pytest.mark.parametrize("half", tuple(T.HALF))
def test_the_dispatcher_is_the_kernel_which_names(half):
    """kernel 0 = itts_attention_varlen's rule: the matrix-core kernel for the 16-bit type at dqk = dv = 64, the vector kernel in fp32"""
    import os
    lib = L.load(half)
    fake = 0x10000
    tabs = (ptr(i32([0, 4])), ptr(i32([0, 8])), ptr(i32([2])), ptr(i32([3])), 1)
    simple = os.environ.get("ITTS_ATTN_SIMPLE") is not None
    assert lib.itts_attention_append_which(fake, fake, fake, *tabs, H, 64, 64, 384, 256, 256, 128, T.SCALE, L.BF16, 0) == (T.SIMPLE if simple else T.MFMA)
    assert lib.itts_attention_append_which(fake, fake, fake, *tabs, H, 32, 16, 160, 96, 96, 32, T.SCALE, L.F32, 0) == T.SIMPLE


# ---- refusals: host only, before any HIP call (they need no GPU) --------------------------------------------------------------------
def which(lib, *, q=0x10000, k=0x20000, v=0x30000, q_off=(0, 4), kv_off=(0, 8), pos0=(2,), n_new=(3,), nseq=1, dqk=64, dv=64, dt=None, kernel=0,
          tabs=None):
    dt = L.BF16 if dt is None else dt
    arrays = tabs or (ptr(i32(q_off)), ptr(i32(kv_off)), ptr(i32(pos0)), ptr(i32(n_new)))
    return lib.itts_attention_append_which(q, k, v, *arrays, nseq, H, dqk, dv, 3 * H * dqk, H * (dqk + dv), H * (dqk + dv), H * dv, T.SCALE, dt, kernel)


def refused(lib, status, entry="itts_attention_append_which"):
    msg = lib.itts_last_error().decode()
    assert status == -1 and msg.startswith(entry + ": "), (status, msg)
    return msg


@pytest.mark.parametrize("half", tuple(T.HALF))
def test_refusals_are_made_on_the_host(half):
    lib = L.load(half)
    assert which(lib) in (T.SIMPLE, T.MFMA)  # the call the refusals below are one step away from
    refused(lib, which(lib, q=None))
    refused(lib, which(lib, k=None))
    refused(lib, which(lib, v=None))
    refused(lib, which(lib, tabs=(None, ptr(i32([0, 8])), ptr(i32([2])), ptr(i32([3])))))
    big = i32(np.arange(131))
    assert "nseq" in refused(lib, which(lib, nseq=0))
    assert "nseq" in refused(lib, which(lib, nseq=129, tabs=(ptr(big), ptr(big), ptr(big), ptr(big))))
    assert "n_new" in refused(lib, which(lib, n_new=(-1,)))
    assert "pos0" in refused(lib, which(lib, pos0=(-1,)))
    assert "history block" in refused(lib, which(lib, pos0=(6,), n_new=(3,)))
    assert which(lib, pos0=(5,), n_new=(3,)) in (T.SIMPLE, T.MFMA)  # ... and up to the block's end is fine
    assert "rows of q" in refused(lib, which(lib, n_new=(5,), pos0=(0,)))
    assert "attn_append_mfma" in refused(lib, which(lib, dt=L.F32, kernel=2))
    assert "kernel" in refused(lib, which(lib, kernel=3))
    assert "head dims" in refused(lib, which(lib, dqk=129, dt=L.F32))
    # the launching entry: the same check (only calls that cannot reach a launch whatever it answers)
    tabs = (ptr(i32([0, 4])), ptr(i32([0, 8])), ptr(i32([2])), ptr(i32([3])))
    st = lib.itts_attention_append(None, None, None, None, *tabs, 1, H, 64, 64, 384, 256, 256, 128, T.SCALE, L.BF16, 0, None)
    refused(lib, st, "itts_attention_append")
    st = lib.itts_attention_append(None, None, None, None, *tabs, 0, H, 64, 64, 384, 256, 256, 128, T.SCALE, L.BF16, 0, None)
    refused(lib, st, "itts_attention_append")
    st = lib.itts_kv_rows_append(None, None, None, None, *tabs, 1, 384, 256, 256, 128, 128, L.BF16, None)
    refused(lib, st, "itts_kv_rows_append")
