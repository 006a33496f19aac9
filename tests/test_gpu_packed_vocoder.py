"""GPU: the packed vocoder (itts_bigvgan_packed / Engine.bigvgan_packed / IndexTTS(packed_vocoder=True)): the sentences of a call back to
back in ONE BigVGAN item, every sentence the waveform of its latent alone - as bits, whoever shares the pass.

  * micro generator, fp32 engine, sentences of 5, 12, 1 and 9 frames of three voices: each against oracle.vocoder.bigvgan_generator on
    the sentence alone at the fp32 bar of tests/test_gpu_ragged_vocoder.py (relative RMS < 1e-4); everything finite;
  * invariance AS INTEGERS in fp32, bf16 and f16: the four-sentence pass against each sentence alone, the pack reversed, chunks of
    2 + 2, one voice for all (against the sentences that had that voice) and a second run;
  * IndexTTS-1.5 dimensions, bf16, sentences of 64, 40 and 7 frames cut from the `long_bigvgan` latent: the same invariance, the 7-frame
    sentence included - the case the padded ragged form cannot pass (tests/test_gpu_ragged_vocoder.py: 1.7e-2 from its batch-1 run) -
    also inside a pack of 4200 + frames, where gemm_mfma takes its 128 x 128 tiles -
    and each within the bars that file uses (< 4e-2) of its batch-1 Engine.bigvgan run and, the 64-frame one, of the golden waveform.
    The packed pass and Engine.bigvgan are NOT the same bits: the kernel families differ (pinned here, chosen by the tile count there;
    a K split there) and the speaker bias is added behind the convolution's rounding here, inside its epilogue there;
  * the drop-in: 4 utterances, 3 voices, 3 settings with mixed batches + packed latent + packed vocoder: one bigvgan_packed per decode
    group and no bigvgan / bigvgan_grouped call; every utterance's int16 waveform equals the call with that utterance alone (and the
    call in which every utterance carries its prompt and settings); the switch off equals an object built without it on both paths
    of infer_batch.
The measured figures are printed and, where ITTS_TEST_OUT names a directory, written to packed_vocoder_rows.txt there."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import packed_vocoder_ref as PR
from itts_hip import config as icfg
from itts_hip import engine as ieng
from itts_hip import infer_core, prng, synth

MICRO = icfg.micro()
FULL = icfg.indextts_1_5()
RECORD = {}
KINDS = ("fp32", "bf16", "f16")


@pytest.fixture(scope="module", autouse=True)
def record_file():
    yield
    out = os.environ.get("ITTS_TEST_OUT")
    if out and RECORD:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "packed_vocoder_rows.txt"), "w") as f:
            f.write("\n".join(f"{k}: {v}" for k, v in sorted(RECORD.items())) + "\n")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def wavs(eng, lats, spk, **kw):
    out = [w.float().cpu() for w in eng.bigvgan_packed(lats, spk, **kw)]
    torch.cuda.synchronize()
    return out


def check_invariance(eng, lats, spk_rows, voices, tag):
    """spk_rows [n, E] (row i = the embedding of sentence i).  -> the waveforms of the whole pack"""
    n = len(lats)
    got = wavs(eng, lats, spk_rows)
    for i, w in enumerate(got):
        assert w.shape == (1, 1, lats[i].shape[1] * eng.up_total) and bool(torch.isfinite(w).all()), (tag, i)
    again = wavs(eng, lats, spk_rows)
    rev = wavs(eng, lats[::-1], spk_rows.flip(0))[::-1]
    gap = eng.bigvgan_packed_gap()
    two = sum(int(l.shape[1]) + gap for l in lats[:(n + 1) // 2])  # a budget that cuts the pack in two
    chunked = wavs(eng, lats, spk_rows, max_frames=two)
    assert len(infer_core.packed_vocoder_plan([int(l.shape[1]) for l in lats], gap, two)[0]) == 2
    for i in range(n):
        alone = wavs(eng, [lats[i]], spk_rows[i:i + 1])[0]
        assert same_bits(got[i], alone), (tag, i, "differs from the sentence alone")
        assert same_bits(got[i], again[i]), (tag, i, "two runs differ")
        assert same_bits(got[i], rev[i]), (tag, i, "differs in the reversed pack")
        assert same_bits(got[i], chunked[i]), (tag, i, "differs under chunking")
    v0 = voices[0]
    one_voice = wavs(eng, lats, spk_rows[0])  # [E]: one voice for all
    hits = [i for i in range(n) if voices[i] == v0]
    assert hits
    for i in range(n):
        assert same_bits(got[i], one_voice[i]) == (i in hits), (tag, i, "one voice for all")
    return got


def micro_operands(nvoice=3):
    c = PR.micro_case(voices=(0, 1, 2, 1), nvoice=nvoice)
    spk_rows = torch.cat([c["spk"][v, 0:1] for v in c["voices"]], 0)  # [4, E]
    return c, spk_rows


@pytest.mark.gpu
def test_packed_fp32_vs_oracle():
    c, spk_rows = micro_operands()
    eng = ieng.build_engine(MICRO, "fp32", parts=("bigvgan",))
    assert eng.bigvgan_packed_gap() == 7
    got = wavs(eng, c["lats"], spk_rows)
    for i, n in enumerate(c["lens"]):
        e = PR.rel_rms(got[i], c["rows"][i])
        RECORD[f"micro fp32 sentence {i} ({n} frames, voice {c['voices'][i]}) vs the oracle alone rel rms"] = f"{e:.3e}"
        print(f"micro fp32 sentence {i} ({n} frames): packed pass vs the oracle on the sentence alone, rel RMS {e:.3e}")
        assert e < 1e-4, (i, n, e)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_packed_invariance_as_integers(kind):
    c, spk_rows = micro_operands()
    eng = ieng.build_engine(MICRO, kind, parts=("bigvgan",))
    got = check_invariance(eng, c["lats"], spk_rows, c["voices"], f"micro {kind}")
    bound = {"fp32": 1e-4, "bf16": 6e-2, "f16": 4e-3}[kind]  # the bars of tests/test_gpu_ragged_vocoder.py
    for i, n in enumerate(c["lens"]):
        b1 = eng.bigvgan(c["lats"][i], spk_rows[i:i + 1]).float().cpu()
        e = PR.rel_rms(got[i], b1)
        RECORD[f"micro {kind} sentence {i} ({n} frames) vs batch-1 bigvgan rel rms"] = f"{e:.3e}"
        print(f"micro {kind} sentence {i} ({n} frames): packed pass vs its batch-1 Engine.bigvgan run, rel RMS {e:.3e}")
        assert e < bound, (kind, i, n, e)


@pytest.mark.gpu
def test_packed_full_dims_bf16(gold):
    eng = ieng.build_engine(FULL, "bf16", parts=("bigvgan",))
    assert eng.bigvgan_packed_gap() == 7
    mel = torch.from_numpy(synth.prompt_mel(511, seed=7))
    spk1 = eng.ecapa(mel.transpose(1, 2)).float().cpu().reshape(1, -1)
    spk2 = spk1.flip(1).contiguous()  # a second voice: the same numbers in another order
    lens = (64, 40, 7)
    long = torch.from_numpy(prng.tensor("bigvgan.latent.long", 3, (1, 64, FULL.bigvgan.gpt_dim), std=1.0, mean=0.0))
    lats = [long[:, :n].clone() for n in lens]
    voices = (0, 1, 0)
    spk_rows = torch.cat([(spk1, spk2)[v] for v in voices], 0)
    got = check_invariance(eng, lats, spk_rows, voices, "1.5 dims bf16")
    # gemm_mfma (the ups[i] here) picks its tile by the tile count: 64 x 64 for the 7-frame sentence alone, 128 x 64 in the pack above.
    # A pack of more than 4096 frames reaches its 128 x 128 tiles at ups[0] (ring depth 2) and at ups[1] (depth 1, >= 1536 tiles):
    # the 7-frame sentence in front of and behind a 4200-frame one has the bits it has alone.
    filler = torch.from_numpy(prng.tensor("bigvgan.latent.filler", 3, (1, 4200, FULL.bigvgan.gpt_dim), std=1.0, mean=0.0))
    big = wavs(eng, [lats[2], filler, lats[2]], torch.cat([spk1, spk2, spk1], 0))
    assert same_bits(big[0], got[2]) and same_bits(big[2], got[2]), "the 7-frame sentence differs inside a 4200-frame pack"
    for i, n in enumerate(lens):
        b1 = eng.bigvgan(lats[i], spk_rows[i:i + 1]).float().cpu()
        e = PR.rel_rms(got[i], b1)
        RECORD[f"1.5 dims bf16 sentence {i} ({n} frames) vs batch-1 bigvgan rel rms"] = f"{e:.3e}"
        print(f"1.5 dims bf16 sentence {i} ({n} frames): packed pass vs its batch-1 Engine.bigvgan run, rel RMS {e:.3e}")
        assert e < 4e-2, (i, n, e)
    e = PR.rel_rms(got[0].numpy()[0, 0], gold("long_bigvgan")["wav"])
    RECORD["1.5 dims bf16 sentence 0 (64 frames) vs golden rel rms"] = f"{e:.3e}"
    print(f"1.5 dims bf16 sentence 0 vs the golden waveform, rel RMS {e:.3e}")
    assert e < 4e-2, e


@pytest.mark.gpu
def test_packed_refusals_reach_python():
    eng = ieng.build_engine(MICRO, "fp32", parts=("bigvgan",))
    lat = torch.zeros(1, 4, MICRO.bigvgan.gpt_dim)
    spk = torch.zeros(3, MICRO.bigvgan.speaker_embedding_dim)
    with pytest.raises(ValueError, match="speaker embeddings"):
        eng.bigvgan_packed([lat, lat], spk)
    assert eng.bigvgan_packed([], spk) == []  # as bigvgan_grouped, which it stands in for
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    d = torch.zeros(64, MICRO.bigvgan.gpt_dim, device=eng.device)
    out = torch.zeros(64 * eng.up_total, device=eng.device)
    off, ln = np.asarray([0, 10, 20], np.int32), np.asarray([4, 3], np.int32)  # capacities 10: one frame short of 4 + 7
    st = eng.lib.itts_bigvgan_packed(eng.h, d.data_ptr(), d.data_ptr(), P(off), P(ln), 2, out.data_ptr(), eng._s())
    assert st == -1 and b"gap too small" in eng.lib.itts_last_error()


# ---- the drop-in on the micro checkpoint ----------------------------------------------------------------------------------------------
def micro_tts(**kw):
    from indextts.infer import IndexTTS

    sds = {"gpt": synth.gpt_state_dict(MICRO, 1234), "bigvgan": synth.bigvgan_state_dict(MICRO, 1234), "dvae": synth.dvae_state_dict(MICRO, 1234)}
    return IndexTTS(cfg=MICRO, model_dir="/nonexistent", is_fp16=False, state_dicts=sds, **kw)


@pytest.mark.gpu
def test_infer_batch_packed_vocoder_dropin(monkeypatch):
    for env in ("ITTS_MIXED_BATCH", "ITTS_PACKED_LATENT", "ITTS_PACKED_VOCODER", "ITTS_RAGGED_VOCODER"):
        monkeypatch.delenv(env, raising=False)
    tts = micro_tts(mixed_batch=True, packed_latent=True, packed_vocoder=True)
    mels = [torch.from_numpy(synth.prompt_mel(61, seed=s)) for s in (7, 8, 9)]
    nt = MICRO.gpt.number_text_tokens
    texts = [[synth.text_ids(n, 100 * u + k, nt).astype(np.int32) for k, n in enumerate(ns)] for u, ns in enumerate(((11, 7), (9,), (5, 12), (8,)))]
    prompts = [mels[0], mels[1], mels[2], mels[1]]  # 4 utterances, 3 voices
    per = [dict(do_sample=False), dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=11),
           dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.7, repetition_penalty=2.0, seed=12), dict(do_sample=False)]  # 3 settings
    calls = {"bigvgan_packed": [], "bigvgan": 0, "bigvgan_grouped": 0}
    real = {name: getattr(tts.engine, name) for name in calls}
    monkeypatch.setattr(tts.engine, "bigvgan_packed", lambda *a, **k: (calls["bigvgan_packed"].append(len(a[0])), real["bigvgan_packed"](*a, **k))[1])
    monkeypatch.setattr(tts.engine, "bigvgan", lambda *a, **k: (calls.__setitem__("bigvgan", calls["bigvgan"] + 1), real["bigvgan"](*a, **k))[1])
    monkeypatch.setattr(tts.engine, "bigvgan_grouped", lambda *a, **k: (calls.__setitem__("bigvgan_grouped", calls["bigvgan_grouped"] + 1), real["bigvgan_grouped"](*a, **k))[1])

    def run(t, prompts, per, texts=texts, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached
            return [w for _, w in t.infer_batch(prompts, texts, num_beams=1, max_mel_tokens=24, per_utterance=per, **kw)]

    got = run(tts, prompts, per)
    # one decode group: ONE packed vocoder pass over its 6 sentences of 3 voices, no other vocoder call
    assert calls == {"bigvgan_packed": [6], "bigvgan": 0, "bigvgan_grouped": 0}, calls
    for u in range(4):
        alone = run(tts, [prompts[u]], [per[u]], texts=[texts[u]])[0]
        assert got[u].dtype == np.int16 and got[u].shape == alone.shape and np.array_equal(got[u], alone), (u, "differs from the utterance alone")
        ref = run(tts, [prompts[u]] * 4, [per[u]] * 4)
        assert np.array_equal(got[u], ref[u]), (u, "differs from the call in which every utterance carries its prompt and settings")
    assert got[0].shape != got[1].shape or not np.array_equal(got[0], got[1])
    assert calls["bigvgan"] == 0 and calls["bigvgan_grouped"] == 0
    # plain infer_batch (no mixed batches): bigvgan_packed where it called bigvgan_grouped, once per (voice, settings) group
    monkeypatch.setenv("ITTS_MIXED_BATCH", "0")
    calls.update(bigvgan_packed=[], bigvgan=0, bigvgan_grouped=0)
    plain = run(tts, prompts, None, do_sample=False)
    assert calls["bigvgan_packed"] == [2, 2, 2] and calls["bigvgan_grouped"] == 0 and calls["bigvgan"] == 0, calls
    monkeypatch.delenv("ITTS_MIXED_BATCH")
    # the switch off: the output of an object built without it, on both paths of infer_batch, and no packed pass
    off = micro_tts(mixed_batch=True, packed_latent=True)
    monkeypatch.setenv("ITTS_PACKED_VOCODER", "0")
    calls.update(bigvgan_packed=[], bigvgan=0, bigvgan_grouped=0)
    forced_off = run(tts, prompts, per)
    assert calls["bigvgan_packed"] == [] and calls["bigvgan_grouped"] == 4, calls
    monkeypatch.delenv("ITTS_PACKED_VOCODER")
    today = run(off, prompts, per)
    for u in range(4):
        assert np.array_equal(forced_off[u], today[u]), u
    monkeypatch.setenv("ITTS_MIXED_BATCH", "0")
    today_plain = run(off, prompts, None, do_sample=False)
    monkeypatch.setenv("ITTS_PACKED_VOCODER", "0")
    forced_off_plain = run(tts, prompts, None, do_sample=False)
    for u in range(4):
        assert np.array_equal(forced_off_plain[u], today_plain[u]), u
        assert plain[u].shape == today_plain[u].shape  # (the packed pass computes the same function: same codes, same lengths)
    # ... and the environment turns it on for an object built without it
    monkeypatch.setenv("ITTS_PACKED_VOCODER", "1")
    monkeypatch.delenv("ITTS_MIXED_BATCH")
    on = run(off, prompts, per)
    for u in range(4):
        assert np.array_equal(on[u], got[u]), u
