"""No GPU: the public surface of the batched decode projections (itts_skinny_gemm, itts_skinny_gemm_fp8, itts_skinny_gemm_supported,
itts_retile_weights_fp8, itts_ln_rows_bf16: header, both builds of the library, lib.py); what the entries refuse on the host - one
valid call on host memory, then one argument at a time made invalid: each is refused with ITTS_E_INVALID and a message that begins
with the entry's own name (a HIP call would answer ITTS_E_HIP or touch the host pointers), and itts_skinny_gemm_supported says 0 for
every refused shape (it takes no pointers: the null-pointer refusals are the entries' alone).  The case tables of
tests/test_gpu_skinny.py are held against itts_skinny_gemm_supported and against the launcher's rule restated here, so that every
instantiation it can pick occurs; the tests' own helpers against the index formulas; and the bounds are exercised on an fp32
emulation of the operation in the kernel's summation order, right and with errors planted."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_skinny as T
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HOST = np.zeros(4096, dtype=np.float32)
P = (_HOST.ctypes.data + 63) // 64 * 64
GELU = L.ACT_GELU_NEW
# a split-free 20-row projection, and a LayerNorm of 5 rows
VALID = dict(Y=P, ybf=0, X=P, W=P, W8t=None, wscale=P, bias=P, B=20, N=96, K=256, act=0, acc=0, ksplit=1, partial=None, layout=0)
VALID_LN = dict(y=P, x=P, gamma=None, beta=None, rows=5, D=64, eps=1e-5, passes=1, partial=None, nsplit=0, pbias=None, tiled=0)


def supported(lib, fp8, **kw):
    a = dict(VALID, **kw)
    return lib.itts_skinny_gemm_supported(a["ybf"], a["B"], a["N"], a["K"], a["act"], a["acc"], a["ksplit"], a["layout"], fp8)


def call(lib, fp8, **kw):
    a = dict(VALID, **kw)
    tail = (a["bias"], a["B"], a["N"], a["K"], a["act"], a["acc"], a["ksplit"], a["partial"], a["layout"], None)
    if fp8:
        return lib.itts_skinny_gemm_fp8(a["Y"], a["ybf"], a["X"], a["W"], a["W8t"], a["wscale"], *tail), b"itts_skinny_gemm_fp8: "
    return lib.itts_skinny_gemm(a["Y"], a["ybf"], a["X"], a["W"], *tail), b"itts_skinny_gemm: "


def refused(lib, entries=(0, 1), ask=True, **kw):
    """Both entries (0: bf16 weights, 1: fp8) refuse the call on the host, and the selector says 0 -> the messages"""
    msgs = []
    for fp8 in entries:
        st, name = call(lib, fp8, **kw)
        msg = lib.itts_last_error()
        assert st == -1 and msg.startswith(name), (kw, fp8, st, msg)  # ITTS_E_INVALID, before any HIP call
        if ask:
            assert supported(lib, fp8, **kw) == 0, (kw, fp8)
        msgs.append(msg)
    return b" | ".join(msgs)


def ln_refused(lib, **kw):
    a = dict(VALID_LN, **kw)
    st = lib.itts_ln_rows_bf16(a["y"], a["x"], a["gamma"], a["beta"], a["rows"], a["D"], a["eps"], a["passes"], a["partial"], a["nsplit"], a["pbias"],
                               a["tiled"], None)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(b"itts_ln_rows_bf16: "), (kw, st, msg)
    return msg


def test_skinny_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    shape = r"int\s+B\s*,\s*int\s+N\s*,\s*int\s+K\s*,\s*int\s+act\s*,\s*int\s+accumulate\s*,\s*int\s+ksplit\s*,"
    assert re.search(r"\bint\s+itts_skinny_gemm_fp8\s*\(\s*void\s*\*\s*Y\s*,\s*int\s+y_bf16\s*,\s*const\s+void\s*\*\s*X\s*,\s*const\s+void\s*\*\s*W8\s*,"
                     r"\s*const\s+void\s*\*\s*W8t\s*,\s*const\s+float\s*\*\s*wscale\s*,\s*const\s+float\s*\*\s*bias\s*,\s*" + shape +
                     r"\s*float\s*\*\s*partial\s*,\s*int\s+layout\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_skinny_gemm_supported\s*\(\s*int\s+y_bf16\s*,\s*" + shape + r"\s*int\s+layout\s*,\s*int\s+fp8\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_retile_weights_fp8\s*\(\s*void\s*\*\s*dst\s*,\s*const\s+void\s*\*\s*src\s*,\s*int\s+N\s*,\s*int\s+K\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert {"itts_skinny_gemm_fp8", "itts_skinny_gemm_supported", "itts_retile_weights_fp8"} <= set(L.exported_symbols())
    for half in ("bf16", "f16"):
        lib = L.load(half)
        assert len(lib.itts_skinny_gemm_fp8.argtypes) == len(lib.itts_skinny_gemm.argtypes) + 2 and lib.itts_skinny_gemm_fp8.restype is L.i32
        assert len(lib.itts_skinny_gemm_supported.argtypes) == 9 and lib.itts_skinny_gemm_supported.restype is L.i32
        assert lib.itts_retile_weights_fp8.argtypes == lib.itts_retile_weights.argtypes
        assert lib.itts_abi_version() == 4  # additions: the ABI version stays


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_skinny_entries_refuse_on_the_host(half):
    lib = L.load(half)
    assert supported(lib, 0) == 1 and supported(lib, 1) == 1  # the call itself is valid (W8t may be null)
    for k in ("X", "W", "Y"):
        assert b"null pointer" in refused(lib, ask=False, **{k: None}), k
    assert b"null pointer" in refused(lib, entries=(1,), ask=False, wscale=None)
    assert supported(lib, 0, ksplit=2) == 1 and b"partial" in refused(lib, ask=False, ksplit=2)  # ksplit > 1 without partial
    for kw in (dict(B=0), dict(B=-3), dict(N=0), dict(N=-1), dict(K=0), dict(K=-32), dict(ksplit=0), dict(ksplit=-1, partial=P)):
        assert b"non-positive" in refused(lib, **kw), kw
    for kw in (dict(B=129), dict(K=48), dict(K=16), dict(ksplit=9, partial=P),   # K / 32 = 8 k-steps
               dict(ksplit=2, partial=P, act=GELU), dict(acc=1, ybf=1),
               dict(layout=8, B=17), dict(layout=8, B=9, K=1312), dict(layout=8, B=9, ksplit=2, partial=P),
               dict(layout=16 | 1, B=17), dict(layout=16 | 1, B=9, ksplit=2, partial=P), dict(layout=8 | 16, B=9), dict(layout=32),
               dict(ybf=1, layout=2, N=40), dict(ybf=1, layout=3, N=40), dict(ybf=1, layout=8 | 2, B=9, N=40)):  # a tiled bf16 Y needs N % 32 == 0
        assert b"unsupported shape" in refused(lib, **kw), kw
    # each of them next to a call that is taken
    for kw in (dict(B=128), dict(K=32), dict(ksplit=8, partial=P), dict(ksplit=2, partial=P), dict(acc=1), dict(ybf=1), dict(layout=8, B=16),
               dict(layout=8, B=9, K=1280), dict(layout=16 | 1, B=16), dict(ybf=1, layout=2, N=64), dict(ybf=1, N=40), dict(layout=2, N=40),
               dict(layout=3, ybf=1), dict(act=GELU)):
        assert supported(lib, 0, **kw) == 1 and supported(lib, 1, **kw) == 1, kw
    # layout bit 2 is the bf16 entry's: the fp8 entry says tiled by W8t
    assert supported(lib, 0, layout=4) == 1 and b"bit 2" in refused(lib, entries=(1,), layout=4)


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_ln_rows_bf16_refuses_on_the_host(half):
    lib = L.load(half)
    assert b"gamma / beta" in ln_refused(lib, gamma=P) and b"gamma / beta" in ln_refused(lib, beta=P)
    for kw in (dict(y=None), dict(x=None)):
        assert b"null pointer" in ln_refused(lib, **kw)
    for kw in (dict(rows=0), dict(D=0), dict(D=-64), dict(D=2080)):
        assert b"D <= 2048" in ln_refused(lib, **kw), kw
    for bad in (0, 3):
        assert b"passes" in ln_refused(lib, passes=bad)
    for kw in (dict(nsplit=9, partial=P), dict(nsplit=1), dict(nsplit=-1, partial=P)):
        assert b"splits" in ln_refused(lib, **kw), kw
    assert b"D % 32" in ln_refused(lib, tiled=1, D=40)


# ---- the case tables of tests/test_gpu_skinny.py against the launcher's rule -----------------------------------------------------
def instantiation(form, B, N, K, S, layout):
    """skinny_mfma / launch_skinny / launch_skinny16 of csrc/decode_mfma.hip: the template arguments picked for a call"""
    bt, tiles = T.bt_of(B), (N + 15) // 16
    assert bt == {1: 1, 2: 2, 3: 4, 4: 4}.get((B + 15) // 16, 8)
    if layout & 8:
        return ("prologue", 1, 2 if tiles >= 300 else 1, 5, form)
    if layout & 16:
        return ("half", 1, 1, 20 if K // 32 > 8 * 5 else 5, form)
    return ("plain", bt, 2 if tiles * S >= 300 and bt <= 4 else 1, 5, form)


def test_every_gpu_case_is_supported_and_every_instantiation_occurs():
    lib = L.load()
    calls = T.planned_calls()
    seen = set()
    for form, ybf, B, N, K, gelu, acc, S, layout in calls:
        fp8 = int(form.startswith("fp8"))
        assert lib.itts_skinny_gemm_supported(ybf, B, N, K, GELU if gelu else 0, acc, S, layout, fp8) == 1, (form, ybf, B, N, K, gelu, acc, S, layout)
        assert N * K * (1 if fp8 else 2) <= 1 << 20 and B <= 128  # weights of about a megabyte at the most
        seen.add(instantiation(form, B, N, K, S, layout))
    want = {("plain", bt, nt, 5, f) for bt in (1, 2, 4, 8) for nt in (1, 2) if not (bt == 8 and nt == 2) for f in T.FORMS}
    want |= {("prologue", 1, nt, 5, f) for nt in (1, 2) for f in T.FORMS} | {("half", 1, 1, su, f) for su in (5, 20) for f in T.FORMS}
    assert seen == want, (want - seen, seen - want)
    # every (row-tile template, weight form, X layout) triple, every K, every mode per family, every B
    plain = [(B, K, fam, xt, mode, bias) for B, K, fam, xt, mode, bias in T.PLAIN_CASES]
    assert {(T.bt_of(B), fam, xt) for B, _, fam, xt, _, _ in plain} == {(bt, fam, xt) for bt in (1, 2, 4, 8) for fam in ("bf16", "fp8") for xt in (0, 1)}
    assert {B for B, *_ in plain} == {1, 5, 16, 17, 32, 33, 64, 65, 128}
    assert {(K, fam) for _, K, fam, _, _, _ in plain} == {(K, fam) for K in (32, 224, 288, 1312) for fam in ("bf16", "fp8")}
    assert {(K, xt) for _, K, _, xt, _, _ in plain} == {(K, xt) for K in (32, 224, 288, 1312) for xt in (0, 1)}
    assert {(mode, fam) for _, _, fam, _, mode, _ in plain} == {(m, fam) for m in T.MODES for fam in ("bf16", "fp8")}
    assert {bias for *_, bias in plain} == {True, False}
    assert {(B, N) for B, N, *_ in T.NT2_CASES} >= {(16, 4808), (64, 4808), (128, 4808)}
    lnp = T.LNP_CASES
    assert {B for B, *_ in lnp} == {1, 5, 9, 16} and {K for _, K, *_ in lnp} == {32, 96, 288, 1056, 1280}
    assert {(fam, T.MODES[mode][0]) for _, _, fam, mode, *_ in lnp} == {(fam, y) for fam in ("bf16", "fp8") for y in (0, 1)}
    assert any(yt and T.MODES[mode][0] for _, _, _, mode, yt, _, _ in lnp) and any(off > 100 for *_, off in lnp) and T.LNP_NT2[1] == 4808
    hf = T.HALF_CASES
    assert {B for B, *_ in hf} == {1, 11, 16} and {K for _, K, *_ in hf} == {96, 1280, 1312, 5152} and T.HALF_NS == (8, 40, 72)
    assert {(fam, mode) for _, _, fam, mode, _ in hf} == {(fam, m) for fam in ("bf16", "fp8") for m in ("acc", "f32", "bf16")}
    assert {(K // 32 > 40, fam) for _, K, fam, _, _ in hf} == {(d, fam) for d in (False, True) for fam in ("bf16", "fp8")}
    sp = T.SPLIT_CASES
    assert {(K, S) for _, _, K, S in sp} == {(160, 4), (1280, 3), (5120, 5), (256, 8)} and {B for B, *_ in sp} == {9, 20, 64}
    assert {N for _, N, _, _ in sp} == {96, 128, 616} and (20, 616, 256, 8) in sp
    assert set(T.LN_DS) == {32, 96, 1056, 1280, 1312, 2048} and set(T.LN_ROWS) == {1, 17, 37}
    cf = set(T.LN_CONFIGS)
    assert {c[2] for c in cf} == {0, 1, 3, 8} and (2, 1, 3, 1) in cf and {(c[0], c[1]) for c in cf} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    assert {(c[2] > 0, c[3]) for c in cf} == {(False, 0), (True, 0), (True, 1)}
    assert set(T.RETILE_CASES) == {(8, 32), (66, 96), (4808, 64)}


def test_the_engines_shapes_pass_the_new_gate():
    """GPT width 1280, 20 heads: every bf16 output of the batched step (qkv 3 D, fc 4 D; D itself for completeness) is written tiled
    and has N % 32 == 0; the head writes fp32.  From the dimensions alone - no model runs."""
    lib = L.load()
    D, heads = 1280, 20
    assert D % heads == 0 and D // heads == 64
    for N, K in ((3 * D, D), (4 * D, D), (D, D), (D, 4 * D)):
        assert N % 32 == 0
        for B in (5, 16, 17, 64, 128):
            for fp8 in (0, 1):
                assert lib.itts_skinny_gemm_supported(1, B, N, K, GELU if N == 4 * D else 0, 0, 1, 3, fp8) == 1, (B, N, K)
                if B <= 16 and K == D:  # the LayerNorm prologue writes the same tiled bf16 Y
                    assert lib.itts_skinny_gemm_supported(1, B, N, K, 0, 0, 1, 8 | 2, fp8) == 1, (B, N, K)
    for K, S in ((D, 3), (4 * D, 5)):  # the residual projections: split K, fp32 partial sums
        assert lib.itts_skinny_gemm_supported(0, 64, D, K, 0, 1, S, 1, 1) == 1


# ---- the helpers of tests/test_gpu_skinny.py against the index formulas ----------------------------------------------------------
def test_tile_helpers_follow_the_index_formulas():
    B, K, BT = 37, 96, 3
    x = torch.arange(B * K, dtype=torch.float32).view(B, K) + 1
    t = T.to_tiles(x, BT, -1.0)
    assert t.numel() == BT * 16 * K
    for b in range(B):
        for k in range(K):
            assert t[T.tile_off(b, k, BT)] == x[b, k]
    assert int((t == -1).sum()) == (BT * 16 - B) * K and torch.equal(T.from_tiles(t, B, K), x)
    assert bool((T.from_tiles(t, BT * 16, K)[B:] == -1).all())
    N, K = 40, 96
    w = torch.arange(N * K, dtype=torch.float32).view(N, K) + 1
    wt = T.w_tiles(w)
    for n in range(N):
        for k in range(K):
            assert wt[T.wtile_off(n, k, K)] == w[n, k]
    assert int((wt == 0).sum()) == 8 * K and torch.equal(T.retiled_by_formula(w), wt) and torch.equal(T.from_w_tiles(wt, 48, K)[:N], w)


def test_quantised_weights_round_trip_through_bf16():
    for N, K in ((8, 32), (66, 288), (72, 1312)):
        w = T.weights(N, K)
        _, scale, deq = T.quantize_rows_e4m3(T.rnd(f"sk.w{N}x{K}", (N, K)) * 0.05 * torch.pow(2.0, (torch.arange(N) % 3 - 1).float())[:, None])
        assert torch.equal(w["deq"].float(), deq) and torch.equal(deq.to(torch.bfloat16).float(), deq)  # exact in bf16
        assert torch.equal(torch.exp2(torch.log2(scale).round()), scale) and bool((w["w8"] & 0x7F != 0x7F).all())  # powers of two, no NaN byte
        assert torch.equal(w["w8"].view(torch.float8_e4m3fn).float() * scale[:, None], deq)
        assert bool((scale[1:] != scale[:-1]).all())  # neighbouring rows have different scales: a scale taken from the neighbour shows
    a, b = torch.tensor([1.0, -1.0, 0.0]), torch.tensor([1.0 + 2 ** -23, -1.0 - 2 ** -22, -0.0])
    assert T.ulps(a, a) == 0 and T.ulps(a, b) == 2 and T.ulps(a.bfloat16(), torch.tensor([1.0 + 2 ** -7, -1.0, 0.0]).bfloat16()) == 1


# ---- the bounds on an fp32 emulation of the operation, right and with errors planted ---------------------------------------------
def emulate_sums(x, wq, S=1, plant=None):
    """fp32: per K split, 8 wave partials of interleaved 32-wide k-steps, summed in wave order -> [S, B, N]"""
    x, wq = x.float(), wq.float()
    nks = x.shape[1] // 32
    per = (nks + S - 1) // S
    out = torch.zeros(S, x.shape[0], wq.shape[0])
    for s in range(S):
        steps = range(s * per, min((s + 1) * per, nks))
        waves = []
        for wv in range(8):
            acc = torch.zeros(x.shape[0], wq.shape[0])
            for ks in list(steps)[wv::8]:
                if plant == "k-step" and ks == nks // 2:
                    continue
                acc = acc + x[:, ks * 32:(ks + 1) * 32] @ wq[:, ks * 32:(ks + 1) * 32].T
            waves.append(acc)
        for acc in waves:
            out[s] = out[s] + acc
    return out


def emulate(x, N, K, fam, *, gelu=0, ybf=0, y0=None, plant=None):
    w = T.weights(N, K)
    scale = w["wscale"] if fam == "fp8" else torch.ones(N)
    wq = w["deq"].float() / scale[:, None] if fam == "fp8" else w["w"].float()
    if plant == "row":
        x = torch.cat([x[1:2], x[1:]])  # row 0 takes its neighbour's input
    if plant == "scale":
        scale = torch.roll(scale, 1)
    v = emulate_sums(x, wq, 1, plant)[0]
    v = (v + w["bias"]) * scale if plant == "bias" else v * scale + w["bias"]
    if gelu:
        v = T.gelu_new(v)
    if y0 is not None:
        v = y0 + v
    return v.to(torch.bfloat16).float() if ybf else v


def ln_f32(h):
    """LayerNorm in fp32 about the row's first element, as both kernels take their moments"""
    d = h - h[:, :1]
    md = d.mean(1, keepdim=True)
    var = ((d * d).mean(1, keepdim=True) - md * md).clamp_min(0)
    return (h - (h[:, :1] + md)) * torch.rsqrt(var + 1e-5)


PLANTS = ("k-step", "row", "scale", "bias")


@pytest.mark.parametrize("fam", ("bf16", "fp8"))
def test_the_bounds_pass_an_fp32_emulation_and_catch_planted_errors(fam):
    B, N, K = 5, 40, 224
    plants = PLANTS if fam == "fp8" else PLANTS[:2]  # (the scale is the fp8 kernel's)
    x, y0 = T.x_bf16(K)[:B], T.y0_of(N)[:B]
    checks = []  # (name, bound, emulation(plant), reference)
    checks.append(("fp32 store", T.BOUND_F32, lambda p: emulate(x, N, K, fam, plant=p), T.ref_plain(K, N, fam, 1, 0, 0)[:B]))
    checks.append(("fp32 accumulate", T.BOUND_F32, lambda p: emulate(x, N, K, fam, y0=y0, plant=p), T.ref_plain(K, N, fam, 1, 0, 1)[:B]))
    checks.append(("bf16 gelu", T.BOUND_BF16, lambda p: emulate(x, N, K, fam, gelu=1, ybf=1, plant=p), T.ref_plain(K, N, fam, 1, 1, 0)[:B]))
    h = T.x_f32(K)[:B]
    xn = ln_f32(h).to(torch.bfloat16)
    checks.append(("prologue fp32", T.BOUND_LN_F32, lambda p: emulate(xn, N, K, fam, plant=p), T.ref_prologue(K, N, fam, 1, 0, 0.3)[:B]))
    checks.append(("prologue bf16", T.BOUND_BF16, lambda p: emulate(xn, N, K, fam, ybf=1, plant=p), T.ref_prologue(K, N, fam, 1, 0, 0.3)[:B]))
    # the split-K chain: partial sums, absorbed into the residual stream, LayerNorm of it rounded to bf16
    S, Ks, Ns = 4, 160, 96
    xs, h0, w = T.x_bf16(Ks)[:B], T.y0_of(Ns)[:B] * 2, T.weights(Ns, Ks)
    h_ref = h0.double() + xs.double() @ T.w_ref(Ns, Ks, fam).T + w["bias"].double()

    def chain(p):
        scale = w["wscale"] if fam == "fp8" else torch.ones(Ns)
        wq = w["deq"].float() / scale[:, None] if fam == "fp8" else w["w"].float()
        xx = torch.cat([xs[1:2], xs[1:]]) if p == "row" else xs
        sc = torch.roll(scale, 1) if p == "scale" else scale
        part = emulate_sums(xx, wq, S, p) * sc
        a = w["bias"].clone().expand(B, Ns)
        if p == "bias":
            a = a * sc  # (the bias scaled with the sums)
        for s in range(S):
            a = a + part[s]
        return h0 + a

    checks.append(("residual stream", T.BOUND_RESID, chain, h_ref))
    checks.append(("ln_rows output", T.BOUND_LNROWS, lambda p: ln_f32(chain(p)).to(torch.bfloat16).float(), T.ln_ref(h_ref, None, None, 1)))
    for name, bound, run, ref in checks:
        e = T.relerr(run(None), ref)
        print(f"{fam} {name}: emulation relerr {e:.3e} (bound {bound:.0e})")
        assert e < bound, (name, e)
        for p in plants:
            bad = T.relerr(run(p), ref)
            assert bad > bound, (name, p, bad)
