"""GPU, engine level: the opt-in fp8 (e4m3) K/V cache of the GPT decode steps (Engine.set_kv_fp8 / build_engine(kv_fp8=True) /
ITTS_KV_FP8) - the latch at the prefill, the re-zeroing and re-capture when the cache type changes, the byte-sized per-layer
offsets, the launch path at every row count, beams (cache ancestry over byte-sized blocks), fp8 weights on top, both libraries, the
fp32 engine's refusal.  Engines are indextts_1_5() with 3 layers, parts=("gpt",), text length 41, 32 steps: the sizes of
tests/test_gpu_engine_fp8.py.  Every comparison is exact (codes and logits bit for bit): there is no tolerance.

Batch invariance (ITTS_GEMM_KSPLIT=0, the project's batch-invariance mode): a row's results do not depend on the other rows of its
batch within one family of projection kernels - the GEMV family at 1 - 4 rows, the folded-LayerNorm MFMA family at 5 - 16 rows,
the K-split MFMA family above 16.  Across families the summation order differs with the 16-bit cache on the parent commit too
(tests/test_gpu_configs.py bounds it by 3e-2 instead), so rows are compared inside a family: 2, 3, 4 rows against each row's own
1-row run; 6 rows against the same rows in a 9-row batch; 33 rows (33 x 20 heads >= 512: the 256-thread attention form)
against the same rows in a 40-row batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402
from test_gpu_engine_fp8 import CFG, CFG3, TEXT_LEN, run, same_bits, texts  # noqa: E402


@pytest.fixture(scope="module")
def eng():  # the 16-bit cache by default; the tests switch it and switch it back
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def engkv():  # the mode on from construction
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",), kv_fp8=True)


@pytest.fixture(scope="module")
def cond(eng):
    return eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))


@pytest.fixture(autouse=True)
def no_env(monkeypatch):
    monkeypatch.delenv("ITTS_KV_FP8", raising=False)


def ragged(rows, seed):
    """[rows, TEXT_LEN] text ids of different lengths (row 0 full length); row r is the same in every batch size"""
    t = np.full((rows, TEXT_LEN), CFG.gpt.stop_text_token, np.int32)
    for r in range(rows):
        n = TEXT_LEN if r == 0 else 17 + (r * 7) % 24
        t[r, :n] = synth.text_ids(n, seed + r, CFG.gpt.number_text_tokens)
    return t


def gen(e, cond, text, steps=32):
    """default switches: the persistent engine where the step may use it"""
    return run(e, cond, text, steps, no_engine=False)


def test_default_unchanged_and_toggle_on_one_engine_object(eng, engkv, cond):
    text = texts(2, 11)
    off1 = gen(eng, cond, text)
    assert off1[2] == 1  # mode off: the 2-row step is the persistent engine's, as before the mode existed
    eng.set_kv_fp8(True)
    try:
        on1 = gen(eng, cond, text)
        eng.set_kv_fp8(False)
        off2 = gen(eng, cond, text)
        eng.set_kv_fp8(True)
        on2 = gen(eng, cond, text)
    finally:
        eng.set_kv_fp8(False)
    assert on1[2] == 0 and on2[2] == 0 and off2[2] == 1
    assert same_bits(off1, off2), "16-bit cache after an fp8 generation: stale bytes or a stale graph"
    assert not np.array_equal(on1[1], off1[1]), "the fp8 cache did not engage"
    fresh = gen(engkv, cond, text)
    assert fresh[2] == 0
    assert same_bits(on1, fresh), "fp8 cache after a 16-bit generation differs from a fresh fp8 engine: re-zeroing / re-capture"
    assert same_bits(on2, fresh)


def test_environment_overrides_the_setter_at_the_next_prefill(eng, cond, monkeypatch):
    text = texts(2, 11)
    off = gen(eng, cond, text)
    monkeypatch.setenv("ITTS_KV_FP8", "1")  # setter off, environment on
    on = gen(eng, cond, text)
    assert (off[2], on[2]) == (1, 0) and not np.array_equal(on[1], off[1])
    # latched by the prefill: a change in the middle of a generation waits for the next prefill
    eng.debug(engine=True)
    try:
        eng.prefill(cond, text, 32, 10.0, True)
        eng.decode(8)
        monkeypatch.setenv("ITTS_KV_FP8", "0")
        eng.set_kv_fp8(False)
        eng.decode(23)
        mid = eng.fetch(logits=True) + (eng.decode_mode(),)
        eng._exit()
    finally:
        eng.debug()
    assert mid[2] == 0 and same_bits(mid, on)
    eng.set_kv_fp8(True)  # setter on, environment off
    try:
        assert same_bits(gen(eng, cond, text), off)
        monkeypatch.delenv("ITTS_KV_FP8")
        assert same_bits(gen(eng, cond, text), on)
    finally:
        eng.set_kv_fp8(False)
    assert same_bits(gen(eng, cond, text), off)


@pytest.mark.parametrize("rows,within", [(1, 1), (2, 1), (3, 1), (4, 1), (6, 9), (33, 40)])
def test_ragged_rows_do_not_depend_on_their_batch(engkv, cond, monkeypatch, rows, within):
    """within = 1: every row against its own 1-row run; else against the same row of a `within`-row batch of the same kernel
    family (module docstring)"""
    monkeypatch.setenv("ITTS_GEMM_KSPLIT", "0")
    text = ragged(max(rows, within), 31)
    got = gen(engkv, cond, text[:rows])
    assert got[2] == 0 and np.isfinite(got[1]).all()
    if within == 1:
        for r in range(rows):
            one = gen(engkv, cond, text[r:r + 1])
            assert np.array_equal(one[0][0], got[0][r]) and np.array_equal(one[1][0].view(np.uint32), got[1][r].view(np.uint32)), (rows, r)
    else:
        big = gen(engkv, cond, text)
        assert big[2] == 0
        assert np.array_equal(big[0][:rows], got[0]) and np.array_equal(big[1][:rows].view(np.uint32), got[1].view(np.uint32)), rows


@pytest.mark.parametrize("sample", [True, False])
def test_beam_rows_on_the_fp8_cache(engkv, cond, monkeypatch, sample):
    """num_beams = 3 beam-sample and beam search on the fp8 cache (the ancestry gathers byte-sized blocks).  One sentence = 3 rows
    runs on the GEMV family; two sentences = 2 x 3 = 6 rows and three = 9 rows run on the MFMA family, where the launch path's
    projections differ from the 3-row run's in summation order with the 16-bit cache too (module docstring) - so the 6-row batch is
    compared, sentence by sentence, with the 9-row batch, and the 3-row run with itself across a cache-type round trip."""
    monkeypatch.setenv("ITTS_GEMM_KSPLIT", "0")
    n, nb = 48, 3
    text = texts(3, 51)
    u = np.random.default_rng(9).random((n, 3, 2 * nb), dtype=np.float32)
    kw = dict(do_sample=sample, num_beams=nb, top_k=30, top_p=0.8, temperature=1.0, suppress_stop=True)
    one = engkv.generate(cond, text[:1], n, uniforms=np.ascontiguousarray(u[:, :1]), **kw)
    assert engkv.decode_mode() == 0 and one.shape == (1, n)
    two = engkv.generate(cond, text[:2], n, uniforms=np.ascontiguousarray(u[:, :2]), **kw)
    assert engkv.decode_mode() == 0 and two.shape == (2, n)
    three = engkv.generate(cond, text, n, uniforms=u, **kw)
    assert engkv.decode_mode() == 0
    assert np.array_equal(three[:2], two)
    engkv.set_kv_fp8(False)
    try:
        engkv.generate(cond, text[:1], n, uniforms=np.ascontiguousarray(u[:, :1]), **kw)
    finally:
        engkv.set_kv_fp8(True)
    again = engkv.generate(cond, text[:1], n, uniforms=np.ascontiguousarray(u[:, :1]), **kw)
    assert engkv.decode_mode() == 0 and np.array_equal(again, one)


@pytest.mark.parametrize("rows", [2, 20])
def test_with_fp8_weights(cond, rows):
    """fp8 weights and the fp8 cache together: the fp8-weight engine still equals the engine on the dequantised weights bit for bit"""
    text = ragged(rows, 71)
    out = {}
    for mode in ("fp8", "dequant"):
        e = ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8=mode, engine_fp8=True, kv_fp8=True)
        out[mode] = gen(e, cond, text)
        del e
        torch.cuda.empty_cache()
    assert out["fp8"][2] == 0 and out["dequant"][2] == 0
    assert same_bits(out["fp8"], out["dequant"]), float(np.abs(out["fp8"][1] - out["dequant"][1]).max())


def test_ieee_half_library(cond):
    import os

    from itts_hip import lib as L

    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    text = texts(2, 11)
    e = ieng.build_engine(CFG3, "f16", parts=("gpt",), kv_fp8=True)
    c16 = e.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    on1 = gen(e, c16, text)
    e.set_kv_fp8(False)
    off = gen(e, c16, text)
    e.set_kv_fp8(True)
    on2 = gen(e, c16, text)
    assert on1[2] == 0 and on2[2] == 0
    assert same_bits(on1, on2) and not np.array_equal(on1[1], off[1])
    fresh16 = ieng.build_engine(CFG3, "f16", parts=("gpt",))
    assert same_bits(gen(fresh16, c16, text), off)


def test_fp32_engine_refuses_and_ignores_the_environment(monkeypatch):
    e = ieng.build_engine(CFG3, "fp32", parts=("gpt",))
    with pytest.raises(RuntimeError, match="fp8 .* K/V cache needs a 16-bit engine"):
        e.set_kv_fp8(True)
    c32 = e.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    text = texts(2, 11)
    a = gen(e, c32, text, 16)
    monkeypatch.setenv("ITTS_KV_FP8", "1")
    b = gen(e, c32, text, 16)
    assert same_bits(a, b)
