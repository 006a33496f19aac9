"""GPU: the length-aware Activation1d (itts_snake_aa_fwd_len; csrc/snake.hip snake_aa_lds_len_kernel / snake_aa_len_kernel) on a
padded ragged batch, through the C ABI, in both builds of the library and in fp32.

B = 4 items in a [B, 700, C] buffer.  C = 24 (one tile as wide as the tensor), 96 (48-channel slabs), 192 (64-channel slabs) take the
LDS-tiled kernel, C = 12 the register-window kernel.  The lengths run over 1, 5, 6, 7 (shorter than, equal to and just past the
6-row FIR window), TT - 1, TT, TT + 1 (TT the time tile of the kernel for that C, (256 / CT) * 36 rows, or its 32-row chunk) and T.
The source holds NaN behind every item's length and in guard rows around the buffer: a read past an item's end shows.

For every item the first len rows are, bit for bit, what itts_snake_aa_fwd (layout 1) writes for the item cut to len rows; the
rows behind them are exactly zero; the guard rows of the destination keep their bits; a second run writes the same bits."""
import ctypes as C

import pytest
import torch

from itts_hip import lib as L
from itts_hip import prng
from oracle import vocoder as ovoc

DEV = "cuda:0"
B, T, GUARD = 4, 700, 8
CHANNELS = (24, 96, 192, 12)
# (build of the library, dtype code, torch dtype)
FORMS = {"bf16": ("bf16", L.BF16, torch.bfloat16), "f16": ("f16", L.BF16, torch.float16), "fp32": ("bf16", L.F32, torch.float32)}


def time_tile(Cn):
    """rows per workgroup (LDS-tiled kernel, snake.hip launch_snake_lds) or per lane (register-window kernel, C % 8 != 0)"""
    if Cn % 8:
        return 32
    ct = Cn
    if Cn > 64:
        ct = 64
        while Cn % ct:
            ct -= 8
    return (256 // ct) * 36


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


def ok(lib, status, what):
    if status == -2:  # ITTS_E_HIP
        pytest.exit(f"HIP error in {what}, nothing more is launched: {lib.itts_last_error()}", returncode=3)
    L.check(status, what, lib)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", CHANNELS)
@pytest.mark.parametrize("form", tuple(FORMS))
def test_snake_len_rows_equal_the_cut_item_bit_for_bit(form, Cn):
    half, dt, tdt = FORMS[form]
    lib = L.load(half)
    TT = time_tile(Cn)
    assert TT + 1 < T
    all_lens = (1, 5, 6, 7, TT - 1, TT, TT + 1, T)
    x = torch.from_numpy(prng.tensor(f"snake_len.x{Cn}", 5, (B, T, Cn), std=1.5)).to(tdt)
    la = torch.from_numpy(prng.tensor(f"snake_len.a{Cn}", 5, (Cn,), std=0.4)).to(DEV)
    lb = torch.from_numpy(prng.tensor(f"snake_len.b{Cn}", 5, (Cn,), std=0.4)).to(DEV)
    filt = ovoc.kaiser_sinc_filter12().to(DEV)
    for lens in (all_lens[:4], all_lens[4:]):
        src = torch.full((GUARD + B * T + GUARD, Cn), float("nan"), dtype=tdt)
        for b, n in enumerate(lens):
            src[GUARD + b * T:GUARD + b * T + n] = x[b, :n]
        src = src.to(DEV)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
        off = GUARD * Cn * src.element_size()
        runs = []
        for _ in range(2):
            dst = torch.full((GUARD + B * T + GUARD, Cn), float("nan"), dtype=tdt, device=DEV)
            before = bits(dst.cpu()).clone()
            ok(lib, lib.itts_snake_aa_fwd_len(dst.data_ptr() + off, src.data_ptr() + off, filt.data_ptr(), filt.data_ptr(), la.data_ptr(),
                                              lb.data_ptr(), B, Cn, T, lens_dev.data_ptr(), 1, dt, stream()), "snake_aa_fwd_len")
            sync()
            after = dst.cpu()
            assert torch.equal(bits(after)[:GUARD], before[:GUARD]) and torch.equal(bits(after)[-GUARD:], before[-GUARD:]), "guard rows written"
            runs.append(after[GUARD:GUARD + B * T].reshape(B, T, Cn))
        assert torch.equal(bits(runs[0]), bits(runs[1])), "two runs differ"
        for b, n in enumerate(lens):
            cut = x[b, :n].contiguous().to(DEV)
            ref = torch.full((n, Cn), float("nan"), dtype=tdt, device=DEV)
            ok(lib, lib.itts_snake_aa_fwd(ref.data_ptr(), cut.data_ptr(), filt.data_ptr(), filt.data_ptr(), la.data_ptr(), lb.data_ptr(),
                                          1, Cn, n, dt, 1, stream()), "snake_aa_fwd")
            sync()
            ref = ref.cpu()
            assert bool(torch.isfinite(ref.float()).all())
            assert torch.equal(bits(runs[0][b, :n]), bits(ref)), (form, Cn, n, "rows < len differ from the cut item")
            assert bool((bits(runs[0][b, n:]) == 0).all()), (form, Cn, n, "tail not zero")


@pytest.mark.gpu
def test_snake_len_mul_scales_the_lengths():
    """mul: the lengths are in units of mul rows (the up-sampling between the latent frames and this tensor)"""
    lib = L.load("bf16")
    Cn, mul, lens = 24, 7, (1, 100, 33, 50)
    x = torch.from_numpy(prng.tensor("snake_len.mul", 5, (B, T, Cn), std=1.5)).to(torch.bfloat16).to(DEV)
    la = torch.zeros(Cn, device=DEV)
    filt = ovoc.kaiser_sinc_filter12().to(DEV)
    out = []
    for ln, m in ((lens, mul), (tuple(n * mul for n in lens), 1)):
        dst = torch.full_like(x, float("nan"))
        ld = torch.tensor(ln, dtype=torch.int32, device=DEV)
        ok(lib, lib.itts_snake_aa_fwd_len(dst.data_ptr(), x.data_ptr(), filt.data_ptr(), filt.data_ptr(), la.data_ptr(), la.data_ptr(),
                                          B, Cn, T, ld.data_ptr(), m, L.BF16, stream()), "snake_aa_fwd_len")
        sync()
        out.append(dst.cpu())
    assert torch.equal(bits(out[0]), bits(out[1]))
    for b, n in enumerate(lens):
        assert bool((bits(out[0][b, n * mul:]) == 0).all()) and bool((out[0][b, :n * mul].float().abs().sum(1) > 0).all())
