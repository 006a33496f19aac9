"""GPU: the packed latent pass (opt-in) - Engine.latent_packed / itts_gpt_latent_packed on the micro checkpoint (fp32 engine and both
16-bit libraries; D 128, 2 heads of 64, so the 16-bit engines run the matrix-core attention kernel) and IndexTTS(packed_latent=True).

Against the reference: the micro_latent fixture's sentence, alone and as one of five, under the bars of tests/test_gpu_engine.py::
test_latent (relerr < 1e-4 fp32, rms_rel < 3e-2 16-bit).
Invariance, bit for bit: each of five sequences has the same latent in the five-sequence call, alone, in the reversed order, under a
forced chunking of 2 + 3 and in the call where every sequence carries its voice.  The inputs are those of tests/test_gpu_mixed_batch.py
::test_latent_pass_with_a_voice_per_sequence (texts 41, 17, 30, 23, 36, codes 25, 31, 9, 18, 28, voices [2, 0, 1, 0, 2]); the micro
checkpoint has max_text_tokens = 40, one short of the first text, so on it that text has 40 tokens - and the unshortened inputs run
on the checkpoint they come from (1.5 dims, 3 layers, bf16), where every projection takes the packed pass's pinned gemm_p8 family.
Anchor, bit for bit: under ITTS_GEMM_KSPLIT=0 latent_packed of one sequence = Engine.latent of it (micro: the selector's family at that
row count is the packed pass's pinned one).
Refusal: a cond_index outside [0, n_cond), made on the host.
Drop-in: 4 utterances / 3 voices / 3 settings, mixed_batch=True: with packed_latent=True every utterance's int16 waveform is that of
the call in which every utterance is that utterance, engine.latent_packed runs once per decode group and latent_batch never; with
the switch off (ITTS_PACKED_LATENT=0 on the same object) the output is that of an object built without it."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core  # noqa: E402
from itts_hip import synth  # noqa: E402
from test_gpu_engine import relerr, rms_rel  # noqa: E402
from test_gpu_engine_fp8 import CFG3  # noqa: E402
from test_gpu_mixed_batch import micro_tts  # noqa: E402

MICRO = icfg.micro()
VOICE = [2, 0, 1, 0, 2]
TEXT_LENS, CODE_LENS = (41, 17, 30, 23, 36), (25, 31, 9, 18, 28)
KINDS = ("fp32", "bf16", "f16")
_ENGINES = {}


def engine(kind, cfg=MICRO):
    key = (kind, cfg is MICRO)
    if key not in _ENGINES:
        _ENGINES[key] = ieng.build_engine(cfg, kind, parts=("gpt",))
    return _ENGINES[key]


def inputs(cfg):
    g = cfg.gpt
    texts = [synth.text_ids(min(n, g.max_text_tokens), 50 + i, g.number_text_tokens).astype(np.int32) for i, n in enumerate(TEXT_LENS)]
    codes = [np.random.default_rng(60 + i).integers(0, g.stop_mel_token, n).astype(np.int32) for i, n in enumerate(CODE_LENS)]
    return texts, codes


def conds_of(eng, frames):
    return [eng.conditioning(torch.from_numpy(synth.prompt_mel(frames, seed=s))) for s in (7, 8, 9)]


def same_bits(a, b):
    dt = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and torch.equal(a.contiguous().view(dt), b.contiguous().view(dt))


@pytest.mark.parametrize("kind", KINDS)
def test_latent_packed_against_the_reference(kind, gold):
    c, g = gold("micro_conditioning"), gold("micro_latent")
    eng = engine(kind)
    cond = torch.from_numpy(c["cond"])
    texts, codes = inputs(MICRO)
    alone = eng.latent_packed(cond, [g["text"]], [g["codes"]])[0]
    five = eng.latent_packed(cond, texts[:2] + [g["text"]] + texts[2:4], codes[:2] + [g["codes"]] + codes[2:4])[2]
    for what, lat in (("alone", alone), ("one of five", five)):
        err = relerr(lat, g["latent"]) if kind == "fp32" else rms_rel(lat, g["latent"])
        print(f"{kind} latent_packed {what}: {'relerr' if kind == 'fp32' else 'rms_rel'} {err:.3e}")
        assert err < (1e-4 if kind == "fp32" else 3e-2), (kind, what, err)
    assert same_bits(alone, five)


def check_invariance(eng, conds, texts, codes, monkeypatch):
    cond_all = torch.cat(conds, 0)
    n = len(texts)
    got = eng.latent_packed(cond_all, texts, codes, cond_index=VOICE)
    assert len(got) == n
    for i in range(n):
        assert got[i].shape == (1, len(codes[i]), eng.ccfg.model_dim)
        alone = eng.latent_packed(cond_all, [texts[i]], [codes[i]], cond_index=[VOICE[i]])[0]
        assert same_bits(alone, got[i]), f"sequence {i} alone differs"
    rev = eng.latent_packed(cond_all, texts[::-1], codes[::-1], cond_index=VOICE[::-1])
    for i in range(n):
        assert same_bits(rev[n - 1 - i], got[i]), f"sequence {i} differs in the reversed order"
    with monkeypatch.context() as m:
        seen = []
        m.setattr(infer_core, "packed_chunks", lambda rows, *a, **k: (seen.append(list(rows)), [[0, 1], [2, 3, 4]])[1])
        chunked = eng.latent_packed(cond_all, texts, codes, cond_index=VOICE)
        assert len(seen) == 1 and seen[0] == [eng.ccfg.cond_latents + len(t) + len(c) + 4 for t, c in zip(texts, codes)]
    for i in range(n):
        assert same_bits(chunked[i], got[i]), f"sequence {i} differs under the 2 + 3 chunking"
    for v in range(3):  # the call where every sequence carries voice v
        ref = eng.latent_packed(conds[v], texts, codes)
        for i in range(n):
            if VOICE[i] == v:
                assert same_bits(ref[i], got[i]), f"sequence {i} differs from the call in which every sequence has voice {v}"
    assert not same_bits(eng.latent_packed(conds[0], texts[:1], codes[:1])[0], eng.latent_packed(conds[1], texts[:1], codes[:1])[0])  # the voice matters
    return got


@pytest.mark.parametrize("kind", KINDS)
def test_latent_packed_invariance(kind, monkeypatch):
    eng = engine(kind)
    texts, codes = inputs(MICRO)
    assert [len(t) for t in texts] == [40, 17, 30, 23, 36]  # the first text at the micro checkpoint's max_text_tokens
    check_invariance(eng, conds_of(eng, 61), texts, codes, monkeypatch)


def test_latent_packed_invariance_at_full_dims(monkeypatch):
    """The unshortened inputs on the checkpoint of test_latent_pass_with_a_voice_per_sequence: 1.5 dims, where the pinned selector sends
    all four projections to gemm_p8 at every row count (a sequence alone is a single partly filled 256-row tile)."""
    eng = engine("bf16", CFG3)
    texts, codes = inputs(CFG3)
    assert [len(t) for t in texts] == list(TEXT_LENS)
    got = check_invariance(eng, conds_of(eng, 511), texts, codes, monkeypatch)
    padded = eng.latent_batch(torch.cat(conds_of(eng, 511), 0), texts, codes, cond_index=VOICE)  # the left-padded pass: the same function
    for i in range(len(texts)):
        assert rms_rel(got[i], padded[i].float().cpu().numpy()) < 6e-2, i  # each within the 16-bit bar 3e-2 of the exact latent


@pytest.mark.parametrize("kind", KINDS)
def test_latent_packed_of_one_sequence_is_engine_latent(kind, monkeypatch):
    monkeypatch.setenv("ITTS_GEMM_KSPLIT", "0")
    eng = engine(kind)
    texts, codes = inputs(MICRO)
    cond = conds_of(eng, 61)[1]
    for i in (0, 2):
        assert same_bits(eng.latent_packed(cond, [texts[i]], [codes[i]])[0], eng.latent(cond, texts[i], codes[i])), i


def test_latent_packed_refuses_a_bad_cond_index():
    eng = engine("fp32")
    texts, codes = inputs(MICRO)
    conds = conds_of(eng, 61)
    for bad in ([0, 1, 3, 0, 0], [0, -1, 2, 0, 0]):
        with pytest.raises(RuntimeError, match="conditioning index"):
            eng.latent_packed(torch.cat(conds, 0), texts, codes, cond_index=bad)
    with pytest.raises(RuntimeError, match="conditioning index"):
        eng.latent_packed(conds[0], texts, codes, cond_index=[0, 0, 1, 0, 0])
    with pytest.raises(ValueError):
        eng.latent_packed(conds[0], texts, codes, cond_index=[0, 0])


def test_infer_batch_packed_latent_dropin(monkeypatch):
    monkeypatch.delenv("ITTS_MIXED_BATCH", raising=False)
    monkeypatch.delenv("ITTS_PACKED_LATENT", raising=False)
    tts = micro_tts(mixed_batch=True, packed_latent=True)
    mels = [torch.from_numpy(synth.prompt_mel(61, seed=s)) for s in (7, 8, 9)]
    nt = MICRO.gpt.number_text_tokens
    texts = [[synth.text_ids(n, 100 * u + k, nt).astype(np.int32) for k, n in enumerate(ns)] for u, ns in enumerate(((11, 7), (9,), (5, 12), (8,)))]
    prompts = [mels[0], mels[1], mels[2], mels[1]]  # 4 utterances, 3 voices
    per = [dict(do_sample=False), dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=11),
           dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.7, repetition_penalty=2.0, seed=12), dict(do_sample=False)]  # 3 settings
    calls = {"generate": 0, "latent_packed": [], "latent_batch": 0}
    real = {name: getattr(tts.engine, name) for name in calls}
    monkeypatch.setattr(tts.engine, "generate", lambda *a, **k: (calls.__setitem__("generate", calls["generate"] + 1), real["generate"](*a, **k))[1])
    monkeypatch.setattr(tts.engine, "latent_batch", lambda *a, **k: (calls.__setitem__("latent_batch", calls["latent_batch"] + 1), real["latent_batch"](*a, **k))[1])
    monkeypatch.setattr(tts.engine, "latent_packed", lambda *a, **k: (calls["latent_packed"].append(len(a[1])), real["latent_packed"](*a, **k))[1])

    def run(t, prompts, per, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached
            return [w for _, w in t.infer_batch(prompts, texts, num_beams=1, max_mel_tokens=24, per_utterance=per, **kw)]

    got = run(tts, prompts, per)
    # one decode group: one generation of 6 rows, ONE packed latent pass over its 6 sentences, no left-padded pass
    assert calls == {"generate": 1, "latent_packed": [6], "latent_batch": 0}, calls
    for u in range(4):
        ref = run(tts, [prompts[u]] * 4, [per[u]] * 4)
        assert got[u].dtype == np.int16 and got[u].shape == ref[u].shape and np.array_equal(got[u], ref[u]), u
    assert calls["latent_batch"] == 0 and calls["latent_packed"] == [6] * 5
    # plain infer_batch (no mixed batches): latent_packed where it called latent_batch, once per (voice, settings) group
    monkeypatch.setenv("ITTS_MIXED_BATCH", "0")
    calls.update(generate=0, latent_packed=[], latent_batch=0)
    plain = run(tts, prompts, None, do_sample=False)
    assert calls == {"generate": 3, "latent_packed": [2, 2, 2], "latent_batch": 0}, calls
    monkeypatch.delenv("ITTS_MIXED_BATCH")
    # the switch off: today's output - the object built without it - for both paths of infer_batch, and no packed pass
    off = micro_tts(mixed_batch=True)
    monkeypatch.setenv("ITTS_PACKED_LATENT", "0")
    calls.update(generate=0, latent_packed=[], latent_batch=0)
    forced_off = run(tts, prompts, per)
    assert calls == {"generate": 1, "latent_packed": [], "latent_batch": 4}, calls
    monkeypatch.delenv("ITTS_PACKED_LATENT")
    today = run(off, prompts, per)
    for u in range(4):
        assert np.array_equal(forced_off[u], today[u]), u
    monkeypatch.setenv("ITTS_MIXED_BATCH", "0")
    today_plain = run(off, prompts, None, do_sample=False)
    monkeypatch.setenv("ITTS_PACKED_LATENT", "0")
    forced_off_plain = run(tts, prompts, None, do_sample=False)
    for u in range(4):
        assert np.array_equal(forced_off_plain[u], today_plain[u]), u
        assert plain[u].shape == today_plain[u].shape  # (the packed pass computes the same function: same codes, same lengths)
    # ... and the environment turns it on for an object built without it
    monkeypatch.setenv("ITTS_PACKED_LATENT", "1")
    monkeypatch.delenv("ITTS_MIXED_BATCH")
    on = run(off, prompts, per)
    for u in range(4):
        assert np.array_equal(on[u], got[u]), u
