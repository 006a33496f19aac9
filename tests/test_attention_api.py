"""No GPU: the public surface of itts_attention_kernel / itts_attention_which (header, both builds of the library, lib.py), what the
three attention entries refuse on the host - one valid call on host memory, then one argument at a time made invalid: each is refused
with ITTS_E_INVALID and a message that begins with the entry's own name (a HIP call would answer ITTS_E_HIP or touch the host
pointers), and itts_attention_which says -1 for it - and which kernel itts_attention_which names on a table of supported calls.
A named kernel is never replaced by the other one: what attention_mfma cannot run is refused under kernel 2, not sent to the
vector kernel.  The case tables of tests/test_gpu_attention.py are held against the host rule, and its bound is exercised here on
an fp32 model of the operation (16-bit P where the matrix-core kernel has it), right and with errors planted."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_attention as T
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HOST = np.zeros(4096, dtype=np.float32)
P = (_HOST.ctypes.data + 63) // 64 * 64  # the matrix-core kernel wants 16-byte aligned q, k, v
# the GPT prefill call of the bf16 engine: fused qkv, 3 heads of 64
VALID = dict(o=P, q=P, k=P, v=P, B=2, H=3, Sq=40, Sk=40, dqk=64, dv=64, ldq=576, ldk=576, ldv=576, ldo=192, scale=0.125, causal=1, kv_start=None,
             dtype=L.BF16)
ORDER = ("q", "k", "v", "B", "H", "Sq", "Sk", "dqk", "dv", "ldq", "ldk", "ldv", "ldo", "scale", "causal", "kv_start", "dtype")
NO_SWITCH = os.environ.get("ITTS_ATTN_SIMPLE") is None  # read once per process by the library: with it set the dispatcher never names 2


def call_args(**kw):
    a = dict(VALID, **kw)
    return a["o"], tuple(a[k] for k in ORDER)


def which(lib, **kw):
    return lib.itts_attention_which(*call_args(**kw)[1])


def refused(lib, kernels=(None, 0, 1, 2), ask=True, **kw):
    """Every entry (None: itts_attention) refuses the call: status -1, the entry's own message, itts_attention_which -1; -> the messages"""
    o, args = call_args(**kw)
    msgs = []
    for kernel in kernels:
        if kernel is None:
            st, name = lib.itts_attention(o, *args, None), b"itts_attention: "
        else:
            st, name = lib.itts_attention_kernel(o, *args, kernel, None), b"itts_attention_kernel: "
        msg = lib.itts_last_error()
        assert st == -1 and msg.startswith(name), (kw, kernel, st, msg)  # ITTS_E_INVALID, before any HIP call
        msgs.append(msg)
    if ask:
        assert lib.itts_attention_which(*args) == -1, kw
    return b" | ".join(msgs)


def test_attention_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    common = (r"const\s+void\s*\*\s*q\s*,\s*const\s+void\s*\*\s*k\s*,\s*const\s+void\s*\*\s*v\s*,\s*int\s+B\s*,\s*int\s+H\s*,\s*int\s+Sq\s*,\s*int\s+Sk\s*,"
              r"\s*int\s+dqk\s*,\s*int\s+dv\s*,\s*int\s+ldq\s*,\s*int\s+ldk\s*,\s*int\s+ldv\s*,\s*int\s+ldo\s*,\s*float\s+scale\s*,\s*int\s+causal\s*,"
              r"\s*const\s+int\s*\*\s*kv_start\s*,\s*int\s+dtype\s*")
    assert re.search(r"\bint\s+itts_attention\s*\(\s*void\s*\*\s*o\s*,\s*" + common + r",\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_attention_kernel\s*\(\s*void\s*\*\s*o\s*,\s*" + common + r",\s*int\s+kernel\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_attention_which\s*\(\s*" + common + r"\)\s*;", h)
    assert {"itts_attention", "itts_attention_kernel", "itts_attention_which"} <= set(L.exported_symbols())
    for half in ("bf16", "f16"):
        lib = L.load(half)
        n = len(lib.itts_attention.argtypes)
        assert lib.itts_attention_kernel.restype is L.i32 and len(lib.itts_attention_kernel.argtypes) == n + 1
        assert lib.itts_attention_which.restype is L.i32 and len(lib.itts_attention_which.argtypes) == n - 2
        assert lib.itts_abi_version() == 4  # an addition: the ABI version stays


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_attention_entries_refuse_on_the_host(half):
    lib = L.load(half)
    assert which(lib) == (2 if NO_SWITCH else 1)  # the call itself is valid
    for k in ("q", "k", "v"):
        assert b"null pointer" in refused(lib, **{k: None}), k
    assert b"null pointer" in refused(lib, ask=False, o=None)  # (o is not an argument of itts_attention_which)
    for k in ("B", "H", "Sq", "Sk"):
        for bad in (0, -1):
            assert b"bad dims" in refused(lib, **{k: bad}), (k, bad)
    assert b"65535" in refused(lib, B=65536)
    assert b"65535" in refused(lib, H=65536, ldq=1 << 23, ldk=1 << 23, ldv=1 << 23, ldo=1 << 23)
    assert which(lib, B=65535) in (1, 2) and which(lib, H=65535, ldq=65535 * 192, ldk=65535 * 192, ldv=65535 * 192, ldo=65535 * 64) in (1, 2)
    for bad in (L.F16, L.FP8, 2, 3, -1, 6):
        assert b"dtype" in refused(lib, dtype=bad), bad
    for kw in (dict(dqk=0), dict(dqk=-64), dict(dqk=129, ldq=1024, ldk=1024), dict(dv=0), dict(dv=65, ldv=1024, ldo=1024), dict(dv=128, ldv=1024, ldo=1024)):
        assert b"head dims" in refused(lib, **kw), kw
    for k, least in (("ldq", 192), ("ldk", 192), ("ldv", 192), ("ldo", 192)):
        assert b"leading dims" in refused(lib, **{k: least - 1}), k
        assert b"leading dims" in refused(lib, **{k: 0}), k
        assert which(lib, **dict(dict(ldq=192, ldk=192, ldv=192, ldo=192), **{k: least})) in (1, 2)
    assert b"leading dims" in refused(lib, dqk=128, ldq=383)  # H * dqk = 384
    assert b"leading dims" in refused(lib, dqk=128, ldk=383)
    for bad in (-1, 3, 99):
        assert b"unknown kernel" in refused(lib, kernels=(bad,), ask=False)
    # kernel 2: whatever attention_mfma_supported rejects is refused, the vector kernel does not take its place - and kernels 0 and 1
    # take every one of these calls
    for kw in (dict(dtype=L.F32), dict(Sq=15, causal=0), dict(dqk=32), dict(dqk=96), dict(dv=32), dict(dv=48), dict(ldq=580), dict(ldk=580),
               dict(ldv=580), dict(q=P + 8), dict(k=P + 8), dict(v=P + 2)):
        assert b"attention_mfma needs" in refused(lib, kernels=(2,), ask=False, **kw), kw
        assert which(lib, **kw) == 1, kw


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_attention_which_names_the_dispatchers_kernel(half):
    lib = L.load(half)
    mfma = 2 if NO_SWITCH else 1
    table = ((dict(Sq=15, Sk=15), 1), (dict(Sq=16, Sk=16), mfma),                       # bf16 64 / 64: the matrix-core kernel from 16 queries
             (dict(dqk=128, ldq=384, ldk=384, causal=0), mfma),                          # the conformer's rel-pos attention
             (dict(dv=32), 1), (dict(dv=32, ldv=96, ldo=96), 1),                         # the micro configuration
             (dict(ldk=580), 1), (dict(ldk=584), mfma), (dict(ldq=577), 1), (dict(ldv=582), 1),
             (dict(dtype=L.F32), 1), (dict(dtype=L.F32, Sq=15, Sk=15), 1),
             (dict(q=P + 8), 1), (dict(q=P + 16), mfma), (dict(k=P + 4), 1), (dict(v=P + 8), 1),  # aligned to 8 bytes only
             (dict(o=P + 2, ldo=193), mfma),                                             # o is stored by elements
             (dict(causal=0, Sq=32, Sk=290), mfma), (dict(Sq=1, Sk=65), 1), (dict(Sq=16, Sk=1), mfma),
             (dict(kv_start=P), mfma), (dict(scale=0.0), mfma), (dict(dqk=80, dv=48, ldq=240, ldk=240), 1), (dict(B=1, H=1), mfma))
    for kw, want in table:
        assert which(lib, **kw) == want, (kw, want)


def test_every_gpu_case_is_one_its_kernel_takes():
    """The case tables of tests/test_gpu_attention.py on host memory, in the layouts its Device class builds: the matrix-core cases are
    ones itts_attention_which answers 2 for, whole and for every item alone, head alone and prefix the tests launch; the vector
    kernel's extra cases are ones the dispatcher sends to it in the 16-bit type; the shapes stay within what the issue allows."""
    lib = L.load()

    def args(c, es, B=None, H=None, n=None, off=0):
        wq, wv = c.H * c.dqk, c.H * c.dv
        ld = (2 * wq + wv,) * 3 + (wv,) if c.layout == "fused" else (wq + 8, wq + 8, wv + 8, wv + 8)
        q, k, v = (P + off, P + off + wq * es, P + off + 2 * wq * es) if c.layout == "fused" else (P + off,) * 3
        Sq, Sk = (n, n) if n else (c.Sq, c.Sk)
        return (q, k, v, B or c.B, H or c.H, Sq, Sk, c.dqk, c.dv) + ld + (T.SCALE, c.causal, None, L.F32 if es == 4 else L.BF16)

    for c in T.MFMA_CASES + [T.PREFIX_CASE]:
        assert c.dv == 64 and c.dqk in (64, 128) and c.Sq >= 16
        for kw in (dict(), dict(B=1, off=c.Sq * 16), dict(H=1, off=c.dqk * 2)):
            assert lib.itts_attention_which(*args(c, 2, **kw)) == (2 if NO_SWITCH else 1), (c, kw)
    for n in T.PREFIX_N:
        assert lib.itts_attention_which(*args(T.PREFIX_CASE, 2, B=1, n=n)) == (2 if NO_SWITCH else 1)
    for c in T.SIMPLE_CASES:
        assert lib.itts_attention_which(*args(c, 4)) == 1
        if c not in T.COMMON and c.dqk != 128:
            assert lib.itts_attention_which(*args(c, 2)) == 1, c
    for c in T.MFMA_CASES + T.SIMPLE_CASES:
        assert c.Sq <= 256 and c.Sk <= 320 and c.B <= 3 and c.H == 3 and (c.data == "flat" or c.Sk <= 256)
        assert c.kvs is None or all(0 <= s <= c.Sk for s in c.kvs)
    assert {c.Sk for c in T.COMMON} >= {1, 63, 64, 65, 128, 129, 200} and {c.Sq for c in T.MFMA_CASES} >= {16, 17, 63, 64, 65, 130}
    assert {c.Sq for c in T.SIMPLE_CASES} >= {1, 15, 16, 17, 65} and {(c.dqk, c.dv) for c in T.SIMPLE_CASES} == set(T.DIMS)
    starts = {(s if s < c.Sk - 1 else ("Sk-1" if s == c.Sk - 1 else "Sk")) for c in T.COMMON if c.kvs for s in c.kvs}
    assert starts >= {0, 1, 63, 64, 65, 130, "Sk-1", "Sk"}


# ---- the bound of tests/test_gpu_attention.py on a CPU model of the operation, right and wrong ---------------------------------
def model(fx, form, half, plant=None):
    """fp32 torch arithmetic over whole rows (not the kernels' tile-by-tile online form): scores, exp(s - max), l = the sum of the
    unrounded p, P rounded to the 16-bit type where the matrix-core kernel does, P V / l, one rounding of the output - over keys
    0 .. Sk with key Sk the guard row behind the item (the poison).  plant: "diag" admits the key one past the causal diagonal, "start" the key one before kv_start,
    "tail" row Sk of the partial last tile."""
    c = fx["case"]
    tdt = fx["tdt"]
    q, k, v = fx["q"].float(), fx["k"].float(), fx["v"].float()
    k = torch.cat([k, fx["krow"].float().expand(c.B, 1, c.H, c.dqk)], 1)
    v = torch.cat([v, torch.full((c.B, 1, c.H, c.dv), 1000.0)], 1)
    j, i = torch.arange(c.Sk + 1)[None, :], torch.arange(c.Sq)[:, None]
    kvs = torch.tensor(c.kvs or (0,) * c.B).view(-1, 1, 1, 1)
    vis = (j < c.Sk + int(plant == "tail"))[None, None] & (j[None, None] >= kvs - int(plant == "start"))
    if c.causal:
        vis = vis & (j <= i + (c.Sk - c.Sq) + int(plant == "diag"))[None, None]
    s = (torch.einsum("bihd,bjhd->bhij", q, k) * T.SCALE).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = p.sum(-1, keepdim=True)
    if form == "mfma":
        p = p.to(T.HALF[half][0]).float()
    o = torch.einsum("bhij,bjhd->bihd", p, v) / torch.where(l > 0, l, torch.ones_like(l)).transpose(1, 2)
    return o.to(tdt)


MODEL_CASES = (T.case(2, 65, 65, 1, (0, 64)), T.case(3, 200, 200, 1, (64, 65, 130)), T.case(3, 200, 200, 1, (64, 65, 130), "ramp"),
               T.case(2, 96, 200, 1, (0, 130), "ramp"), T.case(2, 80, 30, 1, (0, 1)), T.case(3, 32, 290, 0, (64, 289, 290)), T.case(2, 17, 129, 0, (128, 1)),
               T.case(2, 70, 133, 0, (0, 65), dqk=128))


@pytest.mark.parametrize("half", tuple(T.HALF))
@pytest.mark.parametrize("form", tuple(T.FORMS))
@pytest.mark.parametrize("c", MODEL_CASES, ids=T.case_id)
def test_the_bound_passes_an_fp32_model_and_catches_planted_errors(c, form, half):
    """The model stays inside the bound and gives exact zeros where no key is visible; with one key admitted that should be masked - one
    past the diagonal, one before kv_start, row Sk - it is caught, on flat data too (a single number per call, the largest error over
    the largest reference, passes those at n visible keys in the hundreds)."""
    fx = T.fixture_of(c, form, half)
    a, b = T.roundoffs(form, half)
    share, err = T.bound_share(fx, model(fx, form, half), a, b)
    print(T.case_id(c), form, half, share, err, fx["e32"])
    assert share <= 1.0 and T.zero_rows_are_plus_zero(fx, model(fx, form, half))
    planted = 0
    for plant in ("diag", "start", "tail"):
        if (plant == "diag" and not c.causal) or (plant == "start" and not (c.kvs and any(c.kvs))) or (plant == "tail" and c.causal):
            continue  # (the causal mask keeps row Sk out by itself)
        bad = model(fx, form, half, plant)
        bad_share, _ = T.bound_share(fx, bad, a, b)
        assert bad_share > 1.0 or not T.zero_rows_are_plus_zero(fx, bad), (plant, bad_share)
        planted += 1
    assert planted >= 1
