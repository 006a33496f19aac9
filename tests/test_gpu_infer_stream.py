"""GPU: the streaming drop-in, IndexTTS.infer_stream, on the micro checkpoint (micro_tts of tests/test_gpu_mixed_batch.py, fp32 engine).

One sentence, greedy and sampled (seed 11), max_mel_tokens = 56 with chunks of 6 frames and a code fetch every 4 decode steps, so that
the greedy run - 56 codes on this text - yields at least three chunks (R = 34 of the 56 frames are held back until the sentence ends): the concatenated chunks equal, as int16
array_equal, the waveform of infer_batch([prompt], [text], num_beams=1, ..) on an object with packed_latent=True, packed_vocoder=True.
Progressive delivery: the first chunk is yielded before the last engine.decode call.  Two sentences: the per-sentence composition
generate -> stream_clean -> latent_packed -> bigvgan_packed.  num_beams=3 raises ValueError at the call.  infer on an object that has
streamed gives the array of an object that never did."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import infer_core, synth  # noqa: E402
from test_gpu_mixed_batch import micro_tts  # noqa: E402

MICRO = icfg.micro()
MAXMEL, CHUNK, EVERY = 56, 6, 4
_TTS = {}


def tts_of(name, **kw):
    if name not in _TTS:
        _TTS[name] = micro_tts(**kw)
    return _TTS[name]


def prompt():
    return torch.from_numpy(synth.prompt_mel(61, seed=7))


def text(n=11, seed=105):
    """seed 105: the micro checkpoint's greedy generation of this text runs to max_mel_tokens (the CPU oracle's greedy_generate gives 56 codes
    without a stop; seed 100 stops after 3), so that whole chunks come out before the sentence ends"""
    return synth.text_ids(n, seed, MICRO.gpt.number_text_tokens).astype(np.int32)


def stream(tts, texts, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached
        return [w for _, w in tts.infer_stream(prompt_mel=prompt(), text=texts, chunk_frames=CHUNK, first_chunk_frames=CHUNK, check_every=EVERY,
                                               max_mel_tokens=MAXMEL, **kw)]


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_one_sentence_equals_infer_batch(mode):
    tts = tts_of("stream")
    ref = tts_of("packed", packed_latent=True, packed_vocoder=True)
    kw = dict(do_sample=False) if mode == "greedy" else dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0)
    chunks = stream(tts, [text()], **kw, **({} if mode == "greedy" else {"seed": 11}))
    assert len(chunks) >= (3 if mode == "greedy" else 1), len(chunks)  # (a sampled row ends where its draws end it)
    assert all(c.dtype == np.int16 and c.ndim == 2 and c.shape[1] == 1 and c.shape[0] % 1024 == 0 and c.shape[0] > 0 for c in chunks)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = ref.infer_batch([prompt()], [[text()]], num_beams=1, max_mel_tokens=MAXMEL, per_utterance=None if mode == "greedy" else [{"seed": 11}],
                               **kw)[0][1]
    got = np.concatenate(chunks, 0)
    assert got.shape == want.shape and np.array_equal(got, want), mode


def test_the_first_chunk_comes_before_the_last_decode_call(monkeypatch):
    tts = tts_of("stream")
    calls = []
    real = tts.engine.decode
    monkeypatch.setattr(tts.engine, "decode", lambda n: (calls.append(n), real(n))[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        it = tts.infer_stream(prompt_mel=prompt(), text=[text()], chunk_frames=CHUNK, first_chunk_frames=CHUNK, check_every=EVERY, do_sample=False,
                              max_mel_tokens=MAXMEL)
        assert not calls  # nothing runs before the first next()
        first = next(it)
        at_first = len(calls)
        rest = list(it)
    assert first[0] == 24000 and first[1].shape[0] > 0
    assert 0 < at_first < len(calls), (at_first, len(calls))
    assert len(rest) >= 2


def test_two_sentences_equal_the_per_sentence_composition():
    tts = tts_of("stream")
    sents = [text(11, 100), text(7, 101)]
    chunks = stream(tts, sents, do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=5)
    eng = tts.engine
    mel = prompt().to(tts.device)
    spk = eng.ecapa(mel.transpose(1, 2), overlap=True)  # as infer_stream runs it (the side arena runs its GEMMs without a K split)
    eng.join_side()
    cond = tts.gpt.get_conditioning(mel)
    parts = []
    for k, s in enumerate(sents):
        codes = eng.generate(cond, s[None], MAXMEL, do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=5 + k)
        clean, _ = infer_core.stream_clean(codes[0], tts.stop_mel_token)
        lat = eng.latent_packed(cond, [s], [clean])
        parts.append(tts._to_int16_range(eng.bigvgan_packed(lat, spk)[0]).type(torch.int16).numpy().T)
    want = np.concatenate(parts, 0)
    got = np.concatenate(chunks, 0)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_beams_are_refused():
    tts = tts_of("stream")
    with pytest.raises(ValueError, match="num_beams"):
        tts.infer_stream(prompt_mel=prompt(), text=[text()], num_beams=3)
    with pytest.raises(ValueError, match="num_beams"):
        tts.engine.generate_stream(torch.zeros(1), text()[None], 8, num_beams=3)
    with pytest.raises(ValueError, match="input_tokens"):
        tts.engine.generate_stream(torch.zeros(1), text()[None], 8, input_tokens=np.zeros((1, 2), np.int32))
    with pytest.raises(ValueError, match="host-side"):
        tts.engine.generate_stream(torch.zeros(1), text()[None], 8, do_sample=True, top_k=0, wide_sampler="host")


def test_infer_is_unchanged_on_an_object_that_streamed():
    tts = tts_of("stream")
    stream(tts, [text()], do_sample=False)
    fresh = tts_of("fresh")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        a = tts.infer(prompt_mel=prompt(), text=[text()], num_beams=1, do_sample=False, max_mel_tokens=24)[1]
        b = fresh.infer(prompt_mel=prompt(), text=[text()], num_beams=1, do_sample=False, max_mel_tokens=24)[1]
    assert a.dtype == np.int16 and np.array_equal(a, b)
