"""GPU: the persistent decode engine on fp8-e4m3 GPT weights (csrc/decode_engine.hip, decode_engine_kernel<.., W8>; opt-in
through Engine.set_engine_fp8 / ITTS_ENGINE_FP8).

The W8 kernel streams the bytes and per-row power-of-two scales that gemv_bf16_kernel<.., W8> reads and repeats its arithmetic
operation for operation, so against the fp8 launch path codes AND logits are bit-identical (1 - 4 rows: the launch path is
the GEMV there).  Multiplying by a power of two commutes with fp32 rounding, so the fp8 engine also equals the bf16 engine on the
dequantised model bit for bit - the comparison that pins the 5 - 6 row slot map, where the launch path runs on the matrix cores.
Every comparison in this file is exact: there is no tolerance.

Sizes: the engine is compiled for D = 1280, H = 20 and takes 1 - 24 layers; 3 layers is the smallest depth at which the slot
rotation is in steady state (c_attn of block l + 1 is requested during block l).  One case runs all 24 layers."""
import inspect
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import pack, synth  # noqa: E402

CFG = icfg.indextts_1_5()
CFG3 = icfg.indextts_1_5()
CFG3.gpt.layers = 3
TEXT_LEN = 41


@pytest.fixture(scope="module")
def eng8():  # fp8 bytes + scales, opted in: launch path under debug(no_engine=True), engine otherwise
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8="fp8", engine_fp8=True)


@pytest.fixture(scope="module")
def engdq():  # the same quantised model, every kernel reads its bf16 dequantisation
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8="dequant")


@pytest.fixture(scope="module")
def cond(eng8):
    return eng8.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))


def texts(rows, seed, ragged=False):
    """[rows, TEXT_LEN] text ids; ragged: rows of different lengths (stop ids are stripped and left-padded -> kv_start)."""
    if not ragged:
        return np.stack([synth.text_ids(TEXT_LEN, seed + r, CFG.gpt.number_text_tokens) for r in range(rows)]).astype(np.int32)
    t = np.full((rows, TEXT_LEN), CFG.gpt.stop_text_token, np.int32)
    for r, n in enumerate([41, 30, 17, 36, 23, 33][:rows]):
        t[r, :n] = synth.text_ids(n, seed + r, CFG.gpt.number_text_tokens)
    return t


def run(eng, cond, text, steps, no_engine, no_graph=False, chunk=8):
    eng.debug(no_engine=no_engine, engine=not no_engine, no_graph=no_graph)
    try:
        eng.prefill(cond, text, steps, 10.0, True)
        done = 1
        while done < steps:
            n = min(chunk, steps - done)
            eng.decode(n)
            done += n
        codes, lg = eng.fetch(logits=True)
        mode = eng.decode_mode()
        eng._exit()
    finally:
        eng.debug()
    return codes, lg, mode


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_fp8_engine_equals_fp8_launch_path_bitwise(eng8, cond, rows):
    text = texts(rows, 11, ragged=rows == 4)
    ref = run(eng8, cond, text, 32, no_engine=True)
    got = run(eng8, cond, text, 32, no_engine=False)
    assert (ref[2], got[2]) == (0, 1)
    assert same_bits(got, ref), float(np.abs(got[1] - ref[1]).max())
    if rows == 2:  # eager launches of the same kernel (no graph): same bits again
        eager = run(eng8, cond, text, 32, no_engine=False, no_graph=True)
        assert eager[2] == 1 and same_bits(eager, ref)


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 6])
def test_fp8_engine_equals_engine_on_the_dequantised_model(eng8, engdq, cond, rows):
    """Both on the persistent engine: the three slot maps (<= 2, 3 - 4, 5 - 6 rows: half slot B, two-part c_attn) of the W8
    loader against the bf16 loader's, ragged rows."""
    text = texts(rows, 31, ragged=True)
    ref = run(engdq, cond, text, 32, no_engine=False)
    got = run(eng8, cond, text, 32, no_engine=False)
    assert (ref[2], got[2]) == (1, 1)
    assert same_bits(got, ref), float(np.abs(got[1] - ref[1]).max())


@pytest.mark.parametrize("sample", [True, False])
def test_fp8_engine_beam_rows(eng8, cond, sample):
    """1 sentence x 3 beams (the reference's default mode; the head inside the launch, the beam sampler as its own kernels)
    against the fp8 launch path, and 2 x 3 = 6 beam rows on the engine against each sentence's own 3-row run."""
    n, nb = 48, 3
    text = texts(2, 51)
    u = np.random.default_rng(9).random((n, 2, 2 * nb), dtype=np.float32)
    kw = dict(do_sample=sample, num_beams=nb, top_k=30, top_p=0.8, temperature=1.0, suppress_stop=True)
    one, modes = [], []
    for no_engine in (True, False):
        eng8.debug(no_engine=no_engine, engine=not no_engine)
        try:
            one.append(eng8.generate(cond, text[:1], n, uniforms=np.ascontiguousarray(u[:, :1]), **kw))
            modes.append(eng8.decode_mode())
        finally:
            eng8.debug()
    assert modes == [0, 1], modes
    assert one[0].shape == (1, n) and np.array_equal(one[0], one[1])
    eng8.debug(engine=True)
    try:
        both = eng8.generate(cond, text, n, uniforms=u, **kw)
        assert eng8.decode_mode() == 1
        second = eng8.generate(cond, text[1:2], n, uniforms=np.ascontiguousarray(u[:, 1:2]), **kw)
    finally:
        eng8.debug()
    assert np.array_equal(both[0], one[1][0]) and np.array_equal(both[1], second[0])


def test_fp8_engine_full_depth(monkeypatch):
    """24 layers, 2 rows, 64 steps: fp8 engine against the fp8 launch path; then a fresh engine object with ITTS_ENGINE_HEAD=0 -
    the blocks on the engine, the head as its own launch on the fp8 bytes."""
    text = texts(2, 71)
    packed = pack.quantize_gpt_fp8(pack.pack_gpt(synth.gpt_state_dict(CFG, 1234), CFG))  # packed once for both engine objects

    def fresh():
        e = ieng.Engine(CFG, "bf16")
        e.load_packed(packed)
        e.finalize()
        e.set_engine_fp8(True)
        return e

    eng = fresh()
    c = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    ref = run(eng, c, text, 64, no_engine=True)
    got = run(eng, c, text, 64, no_engine=False)
    assert (ref[2], got[2]) == (0, 1)
    assert same_bits(got, ref), float(np.abs(got[1] - ref[1]).max())
    del eng
    monkeypatch.setenv("ITTS_ENGINE_HEAD", "0")
    eng2 = fresh()
    got2 = run(eng2, c, text, 64, no_engine=False)
    assert got2[2] == 1
    assert same_bits(got2, ref), float(np.abs(got2[1] - ref[1]).max())


def test_fp8_engine_is_opt_in(cond, engdq, monkeypatch):
    text = texts(2, 91)

    def mode(eng):
        eng.prefill(cond, text, 4, 10.0, True)
        eng.decode(3)
        eng.fetch()
        eng._exit()
        return eng.decode_mode()

    monkeypatch.delenv("ITTS_ENGINE_FP8", raising=False)
    plain = ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8="fp8")
    assert mode(plain) == 0  # fp8 copies keep the launch path unless asked
    plain.set_engine_fp8(True)
    assert mode(plain) == 1
    monkeypatch.setenv("ITTS_ENGINE_FP8", "0")  # the environment overrides the setter, read per call
    assert mode(plain) == 0
    monkeypatch.setenv("ITTS_ENGINE_FP8", "1")
    plain.set_engine_fp8(False)
    assert mode(plain) == 1
    monkeypatch.delenv("ITTS_ENGINE_FP8")
    assert mode(plain) == 0
    # a model without fp8 copies is on the engine whatever the setting says
    assert mode(engdq) == 1
    engdq.set_engine_fp8(True)
    try:
        assert mode(engdq) == 1
    finally:
        engdq.set_engine_fp8(False)


def test_indextts_gpt_fp8(gold, monkeypatch):
    """`IndexTTS(is_fp16=True, gpt_fp8=True)` at 1.5 dims: quantised GPT on the bfloat16 engine, the product loop (eos enabled,
    greedy, two sentences = 2 rows) on the persistent engine, its codes equal to the launch path's."""
    from indextts.infer import IndexTTS

    assert "gpt_fp8" in inspect.signature(IndexTTS.__init__).parameters
    monkeypatch.delenv("ITTS_HALF", raising=False)
    monkeypatch.delenv("ITTS_ENGINE_FP8", raising=False)
    g3 = gold("smooth_eos_b3")
    sds = {"gpt": synth.gpt_state_dict(CFG, 1234, profile="smooth", stop_bias=float(g3["stop_bias"])),
           "bigvgan": synth.bigvgan_state_dict(CFG, 1234)}
    with pytest.raises(ValueError, match="fp8"):
        IndexTTS(cfg=CFG, model_dir="/nonexistent", is_fp16=False, gpt_fp8=True, state_dicts=sds)
    monkeypatch.setenv("ITTS_HALF", "f16")
    with pytest.raises(ValueError, match="fp8"):
        IndexTTS(cfg=CFG, model_dir="/nonexistent", is_fp16=True, gpt_fp8=True, state_dicts=sds)
    monkeypatch.delenv("ITTS_HALF")
    tts = IndexTTS(cfg=CFG, model_dir="/nonexistent", is_fp16=True, gpt_fp8=True, state_dicts=sds)
    assert tts.half == "bf16" and tts.dtype == torch.bfloat16
    mel = torch.from_numpy(synth.prompt_mel(511, seed=7))
    sents = [g3["text"][r, : int(g3["text_lens"][r])].astype(np.int32) for r in range(2)]
    kw = dict(do_sample=False, num_beams=1, repetition_penalty=10.0, max_generate_length=64)
    text = torch.from_numpy(g3["text"][:2].astype(np.int32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sr, wav = tts.infer(prompt_mel=mel, text=sents, output_path=None, max_mel_tokens=64, do_sample=False, num_beams=1)
        assert tts.engine.decode_mode() == 1, "gpt_fp8=True must run on the persistent decode engine"
        codes = tts.gpt.inference_speech(mel.cuda(), text, **kw).cpu().numpy()
        assert tts.engine.decode_mode() == 1
        tts.engine.debug(no_engine=True)
        try:
            ref = tts.gpt.inference_speech(mel.cuda(), text, **kw).cpu().numpy()
            assert tts.engine.decode_mode() == 0
        finally:
            tts.engine.debug()
    assert sr == 24000 and wav.dtype == np.int16 and wav.shape[0] > 0 and np.abs(wav).max() > 0
    assert np.array_equal(codes, ref)
