"""No GPU: the public surface of itts_rowop (header, both builds of the library, lib.py), what the entry refuses before any device
call, and the fp64 references of tests/test_gpu_elementwise.py against an independent spelling of the same operation."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_elementwise as E
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        return f.read()


def test_rowop_entry_point_header_and_binding():
    h = header()
    assert re.search(r"\bint\s+itts_rowop\s*\(\s*int\s+op\s*,\s*const\s+itts_rowop_args\s*\*\s*\w+\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    # the op codes and the argument block of lib.py are the header's, in the header's order
    enum = re.search(r"enum\s*\{([^}]*ITTS_ROWOP_COUNT[^}]*)\}", h).group(1)
    names = re.findall(r"ITTS_ROWOP_([A-Z0-9_]+)", enum)
    assert names[-1] == "COUNT" and tuple(n.lower() for n in names[:-1]) == L.ROWOPS and "= 0" in enum.split(",")[0]
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*itts_rowop_args\s*;", h).group(1)
    fields = []
    for decl in struct.split(";"):
        decl = decl.strip()
        if decl:
            ctype = "ptr" if "*" in decl else "float" if decl.startswith("float") else "int"
            fields += [(n.strip(), ctype) for n in re.sub(r"^(const\s+)?(void|float|int)\s*\*?", "", decl).split(",")]
    kinds = {L.vp: "ptr", L.f32: "float", L.i32: "int"}
    assert fields == [(n, kinds[t]) for n, t in L.RowopArgs._fields_]
    assert "itts_rowop" in L.exported_symbols()
    for half in ("bf16", "f16"):
        lib = L.load(half)
        assert lib.itts_rowop.restype is L.i32 and len(lib.itts_rowop.argtypes) == 3
        assert lib.itts_abi_version() == 4  # an addition: the ABI version stays


# one valid argument block per op (host memory that a refused call never touches), then one field at a time made invalid
_HOST = np.zeros(64, dtype=np.float32)
P = _HOST.ctypes.data
VALID = {
    "layernorm": dict(y=P, x=P, w=P, b=P, dtype_x=0, dtype_y=1, rows=2, D=8, ldx=8, ldy=8, act=0, eps=1e-5),
    "rmsnorm_unit": dict(y=P, x=P, w=P, dtype_x=1, dtype_y=0, rows=2, D=8),
    "glu": dict(y=P, x=P, dtype_x=0, dtype_y=0, rows=2, D=8),
    "geglu": dict(y=P, x=P, dtype_x=1, dtype_y=1, rows=2, D=8, ldy=8),
    "dwconv": dict(y=P, x=P, w=P, b=None, dtype_x=0, dtype_y=0, B=1, T=4, D=2, k=3),
    "conv2d_sub2": dict(y=P, x=P, w=P, b=P, dtype_x=0, dtype_y=0, B=1, T=3, D=3, N=1),
    "cast_copy": dict(y=P, x=P, dtype_x=0, dtype_y=1, rows=2, D=8),
    "copy_rows": dict(y=P, x=P, dtype_x=0, dtype_y=0, rows=2, D=8, ldx=8, ldy=8),
    "add_strided": dict(y=P, x=P, x2=P, dtype_x=0, dtype_y=0, rows=2, D=8, ldx=8, ld2=8, ldy=8),
    "col_mean": dict(y=P, x=P, dtype_x=1, dtype_y=0, B=1, T=2, D=4, ldx=4),
    "col_mean_std": dict(y=P, x=P, dtype_x=0, dtype_y=0, B=1, T=2, D=4, ldx=4),
    "scale_cols_add": dict(y=P, x=P, w=P, x2=None, dtype_x=0, dtype_y=0, B=1, T=2, D=4, ldx=4, ldy=4),
    "asp_pool": dict(y=P, x=P, x2=P, w=P, b=P, dtype_x=0, dtype_y=0, B=1, T=2, D=4),
    "relpos_pack": dict(y=P, y2=P, x=P, x2=P, w=P, b=P, dtype_x=0, dtype_y=0, T=1, N=1, D=4),
    "dvae_argmin": dict(y=P, x=P, b=P, dtype_x=0, dtype_y=0, rows=1, N=4),
    "pair_rows": dict(y=P, x=P, dtype_x=0, dtype_y=0, B=1, T=2, D=4),
}
OPTIONAL = {("dwconv", "b"), ("scale_cols_add", "x2")}
POINTERS = ("y", "y2", "x", "x2", "w", "b")
DIMS = ("rows", "B", "T", "D", "N", "k")


def refused(lib, op, **kw):
    a = L.RowopArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    st = lib.itts_rowop(op if isinstance(op, int) else L.ROWOP[op], C.byref(a), None)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(b"itts_rowop: "), (op, kw, st, msg)  # ITTS_E_INVALID, the entry's own message
    return msg


def test_every_op_has_a_valid_block():
    assert set(VALID) == set(L.ROWOPS) and len(L.ROWOPS) == 16


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_rowop_refuses_bad_arguments_on_the_host(half):
    lib = L.load(half)
    st = lib.itts_rowop(0, None, None)
    assert st == -1 and b"null args" in lib.itts_last_error()
    for op in (-1, len(L.ROWOPS), 1000):
        assert b"unknown op" in refused(lib, op, **VALID["layernorm"])
    for op, ok in VALID.items():
        for k in ok:
            if k in POINTERS and ok[k] is not None and (op, k) not in OPTIONAL:
                assert b"null pointer" in refused(lib, op, **dict(ok, **{k: None})), (op, k)
            if k in DIMS:
                for bad in (0, -3):
                    refused(lib, op, **dict(ok, **{k: bad}))
            if k in ("ldx", "ldy", "ld2"):
                refused(lib, op, **dict(ok, **{k: ok["D"] - 1}))
        for bad in (dict(dtype_x=2), dict(dtype_x=L.FP8), dict(dtype_y=L.F16), dict(dtype_x=-1, dtype_y=-1)):
            if op == "dvae_argmin" and "dtype_x" not in bad:
                continue  # its output is int32: dtype_y is not read
            assert b"dtype" in refused(lib, op, **dict(ok, **bad)), (op, bad)
    # ops with one element type refuse a mixed pair; the statistics write fp32 only; the argmin reads fp32 only
    for op in ("glu", "geglu", "dwconv", "conv2d_sub2", "copy_rows", "add_strided", "scale_cols_add", "relpos_pack", "pair_rows"):
        assert b"dtype" in refused(lib, op, **dict(VALID[op], dtype_x=0, dtype_y=1))
    for op in ("rmsnorm_unit", "col_mean", "col_mean_std", "asp_pool"):
        assert b"dtype" in refused(lib, op, **dict(VALID[op], dtype_x=1, dtype_y=1))
    assert b"dtype" in refused(lib, "dvae_argmin", **dict(VALID["dvae_argmin"], dtype_x=1))
    for T, D in ((2, 3), (3, 2), (2, 100), (100, 2)):
        assert b"below 3 x 3" in refused(lib, "conv2d_sub2", **dict(VALID["conv2d_sub2"], T=T, D=D))
    assert b"one of w / b alone" in refused(lib, "layernorm", **dict(VALID["layernorm"], b=None))
    assert b"act" in refused(lib, "layernorm", **dict(VALID["layernorm"], act=7))
    refused(lib, "scale_cols_add", **dict(VALID["scale_cols_add"], x2=P, ld2=3))


# ---- the references against an independent spelling ------------------------------------------------------------------------------
def test_dwconv_reference_against_an_explicit_loop():
    B, T, Cn, k = 2, 5, 3, 15  # T < k: both sides clip at once
    x, w, b = E.rnd("api.dw.x", (B, T, Cn)), E.rnd("api.dw.w", (Cn, k)), E.rnd("api.dw.b", (Cn,))
    want = torch.zeros(B, T, Cn, dtype=torch.float64)
    for bi in range(B):
        for t in range(T):
            for c in range(Cn):
                acc = float(b[c])
                for j in range(k):
                    ts = t + j - (k - 1) // 2
                    if 0 <= ts < T:
                        acc += float(w[c, j]) * float(x[bi, ts, c])
                want[bi, t, c] = acc
    assert E.relerr(E.ref_dwconv(x, w, b, torch.float64), want) < 1e-14
    assert E.relerr(E.ref_dwconv(x, w, None, torch.float64), want - b.double()) < 1e-14


def test_conv2d_sub2_reference_against_unfold():
    B, Fn, idim, odim = 2, 6, 7, 3
    mel, w, b = E.rnd("api.c2.m", (B, Fn, idim)), E.rnd("api.c2.w", (odim, 3, 3)), E.rnd("api.c2.b", (odim,))
    Fo, fo = (Fn - 3) // 2 + 1, (idim - 3) // 2 + 1
    win = mel.double().unfold(1, 3, 2).unfold(2, 3, 2)  # [B, F', f', 3, 3]
    assert win.shape == (B, Fo, fo, 3, 3)
    want = torch.einsum("btfad,cad->btcf", win, w.double()) + b.double()[None, None, :, None]  # (c, f') c-major per time row
    got = E.ref_conv2d_sub2(mel, w, b, torch.float64)
    assert got.shape == (B, Fo, odim, fo) and E.relerr(got, want.clamp_min(0)) < 1e-14
    assert bool((got == 0).any()) and bool((got > 0).any())  # the ReLU is at work


def test_asp_pool_reference_against_the_two_step_formula():
    B, T, Cn = 2, 9, 4
    lg, x, onehot = E.asp_inputs(B, T, Cn, "f32")
    bs, bsh = E.rnd("api.asp.s", (2 * Cn,)) * 0.2 + 1, E.rnd("api.asp.h", (2 * Cn,)) * 0.1
    lg64, x64 = lg.double(), x.double()
    e = torch.exp(lg64 - lg64.max(1, keepdim=True).values)  # step one: stable exponentials; step two: moments over their sum
    m0, m1, m2 = e.sum(1), (e * x64).sum(1), (e * x64 * x64).sum(1)
    mean = m1 / m0
    sd = (m2 / m0 - mean * mean).clamp_min(1e-12).sqrt()
    gm, gs = E.ref_asp_pool(lg, x, bs, bsh, torch.float64)
    assert E.relerr(gm, mean * bs[:Cn].double() + bsh[:Cn].double()) < 1e-12
    # E[x^2] - mean^2 cancels: in fp64, at |x| < 2, to 1e-15 of a variance of order 1 -> 1e-12 of the deviation is ample
    assert E.relerr(gs, sd * bs[Cn:].double() + bsh[Cn:].double()) < 1e-12
    for b, c in onehot:  # one-hot in effect: the deviation sits on the clamp
        assert abs(float((gs[b, c] - bsh[Cn + c]) / bs[Cn + c]) - 1e-6) < 1e-9


def test_argmin_fixture_is_exact_in_fp32_and_has_ties():
    for N in (1, 66, 255, 256, 257, 8192):
        dots, esq = E.argmin_case(N)
        d64 = esq[None] - 2 * dots
        assert torch.equal((esq.float()[None] - 2 * dots.float()).double(), d64)
        assert float(dots.abs().max()) < 1024 and float(esq.abs().max()) < 1024
        ties = int(((d64 == d64.min(1, keepdim=True).values).sum(1) > 1).sum())
        assert ties == {1: 0, 66: 1, 255: 3, 256: 3, 257: 4, 8192: 7}[N], (N, ties)
