"""csrc/decode_attn_kv8.hip through itts_decode_attn_kv8, on the fixture of tests/test_gpu_decode_attn_fp8.py behind an adapter (`launch`:
poisoned rows, guards, the append as bytes, no NaN byte; `judge`: fp64 from the stored e4m3 values, 2e-5 fp32 / 2^-8 bf16 / 2^-10 half
ctx, the lone appended key to the bit).  H = 3, Smax 700; R, BLIND, W mirror the kernel's header.  Order-independent relations are
compared as bits.  Trunk / tail5: the physical-cache problems of tests/test_gpu_decode_attn_group_kv8.py (Smax 300); nb = 10 needs 10
rows per call.  Maxima: decode_attn_kv8_ops.txt under ITTS_TEST_OUT (committed as profiles/decode_attn_kv8_ops.txt)."""
import os
import types

import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_attn import ancestry, scattered
from test_gpu_decode_attn_fp8 import MEASURED, bits, half_of, judge, launch, mk
from test_gpu_decode_attn_group_kv8 import problem

R, D, BLIND, H, SMAX = 64, 4, 128, 3, 700
W = D * R
S_EDGES = [1, 2, 16, 17, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1, W + R + 1, 2 * W + 1, 699]
PAIRS = sorted({(S, ks) for S in S_EDGES for ks in (0, 1, 15, 16, 17, 63, 65, S - 2, S - 1) if 0 <= ks <= S - 1}, key=lambda p: p[::-1])
CALLS = [PAIRS[i:i + (3 if i % 4 == 0 else 1)] for i in range(len(PAIRS)) if i % 4 in (0, 3)]  # rows of different S share a call: 3 rows, 1 row, ..


def Kv8(lib):  # the new entry behind the names `launch` / `judge` call: its arguments without the two partial buffers
    return types.SimpleNamespace(itts_last_error=lib.itts_last_error, itts_half_is_f16=lib.itts_half_is_f16,
                                 itts_decode_attn=lambda *a: lib.itts_decode_attn_kv8(*a[:14], *a[16:]))


@pytest.fixture(scope="module", autouse=True)
def measured_table():
    yield
    lines = [f"{k:<36s} max relerr {e:9.3e}   dims 8..63 of a head {t:9.3e}   bound {b:.1e}\n"
             for k, (e, t, b) in sorted(MEASURED.items()) if k.startswith("kv8 ")]
    print("\n" + "".join(lines))
    if os.environ.get("ITTS_TEST_OUT") and lines:
        os.makedirs(os.environ["ITTS_TEST_OUT"], exist_ok=True)
        with open(os.path.join(os.environ["ITTS_TEST_OUT"], "decode_attn_kv8_ops.txt"), "w") as f:
            f.writelines(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["half", "f32", "tiled"])
def test_kv8_against_fp64(form):
    g = Kv8(L.load())
    for n, pairs in enumerate(CALLS):
        c = mk("fp8", pairs, H=H, Smax=SMAX)
        o = launch(g, c, L.BF16)  # 16-bit, row-major: what the other two forms must reproduce
        if form == "half":
            judge(g, c, o, "kv8 16-bit ctx", L.BF16)
            if n < 2:
                assert torch.equal(bits(launch(g, c, L.BF16).ctx), bits(o.ctx)), (pairs, "two runs differ")
        elif form == "f32":
            o32 = launch(g, c, L.F32)
            judge(g, c, o32, "kv8 fp32 ctx", L.F32)
            assert torch.equal(bits(o32.ctx.to(half_of(g))), bits(o.ctx)), (pairs, "16-bit ctx != rounded fp32 ctx")
        else:
            ot = launch(g, c, L.BF16, tiled=1)
            judge(g, c, ot, "kv8 tiled ctx", L.BF16)
            assert torch.equal(bits(ot.ctx), bits(o.ctx)), (pairs, "tiled ctx != row-major ctx")


@pytest.mark.gpu
@pytest.mark.parametrize("half", ["bf16", "f16"])
def test_row_alone_equals_row_in_a_batch(half):
    if half == "f16" and not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    g, pairs = Kv8(L.load(half)), [(W + 1, 3), (BLIND, 0), (W + R + 2, 65), (2, 0)]
    alone = [bits(launch(g, mk("fp8", [p], H=H, Smax=SMAX), L.BF16).ctx) for p in pairs]
    for B in (2, 3, 4):
        c = mk("fp8", pairs[:B], H=H, Smax=SMAX)
        o = launch(g, c, L.BF16)
        judge(g, c, o, f"kv8 rows alone [{half}]", L.BF16)
        assert torch.equal(bits(launch(g, c, L.F32).ctx.to(half_of(g))), bits(o.ctx)), (half, B, "16-bit ctx != rounded fp32 ctx")
        for r in range(B):
            assert torch.equal(bits(o.ctx)[r], alone[r][0]), f"{half}: row {r} alone differs from row {r} of {B}"


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2, 3, 10])
def test_ancestry_identity_and_scattered_equal_plain(nb):
    g, items = Kv8(L.load()), {2: 4, 3: 2, 10: 1}[nb]
    Ss, kss = [699, 2 * W + 1, W + 1, BLIND + 1], [0, 5, 1, 63, 17]
    c = mk("fp8", [(Ss[b // nb], kss[(b % nb) % 5]) for b in range(items * nb)], salt=nb, H=H, Smax=SMAX)
    B, plain = c.B, launch(g, c, L.BF16)
    judge(g, c, plain, f"kv8 nb={nb} identity / scattered", L.BF16)
    ident = (torch.arange(B) % nb).to(torch.uint8)[None, :, None].expand(2, B, SMAX).contiguous()
    assert torch.equal(bits(launch(g, c, L.BF16, anc=ident, nb=nb).ctx), bits(plain.ctx)), (nb, "identity ancestry != plain")
    true, other = ancestry(c, nb, f"dak8.anc.{nb}"), ancestry(c, nb, f"dak8.anc2.{nb}")
    anc = torch.empty(2, B, SMAX, dtype=torch.uint8)
    for b in range(B):
        t = true[b].clone()
        t[c.pos[b]:] = 255  # the kernel clamps what it reads there
        anc[c.len[b] & 1, b], anc[1 - (c.len[b] & 1), b] = t.to(torch.uint8), other[b].to(torch.uint8)
    o = launch(g, c, L.F32, anc=anc, nb=nb, phys=scattered(c, nb, true))  # (the fp32 ctx, rounded: the ANC instantiation of both ctx types)
    assert torch.equal(bits(o.ctx.to(half_of(g))), bits(plain.ctx)), (nb, "scattered ancestry != plain on the gathered cache")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["trunk", "tail5"])
@pytest.mark.parametrize("nb", [2, 3, 10])
def test_ancestry_against_fp64(nb, kind):
    g, (c, anc) = Kv8(L.load()), problem([(300, 65), (W + 1, 0), (BLIND + 1, 17), (R, 63)][:8 // nb or 1], nb, kind)
    o = launch(g, c, L.BF16, anc=anc, nb=nb)
    judge(g, c, o, f"kv8 nb={nb} {kind}", L.BF16)
    assert torch.equal(bits(launch(g, c, L.BF16, anc=anc, nb=nb, tiled=1).ctx), bits(o.ctx)), (nb, kind, "tiled")
