"""GPU: mixed decode batches (opt-in) - every row of a batch with its own sampling settings (itts_gpt_set_sampling_rows), its own
voice in the prefill, the latent pass (itts_gpt_latent_batch_cond) and the vocoder, and IndexTTS(mixed_batch=True).infer_batch.

Every comparison is against the existing path at the same shape, bit for bit: inside one projection-kernel family a row's results
depend neither on its slot nor on the other rows (tests/test_gpu_row_retire.py, header), so row r of a mixed generation has to
equal row r of the generation of the same rows in which every row carries row r's settings (or voice).
Sizes: those of tests/test_gpu_engine_fp8.py (1.5 dims with 3 layers, text length 41, 32 steps), bf16 library; one case on the f16
library; the drop-in on the micro checkpoint."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core  # noqa: E402
from itts_hip import lib as L  # noqa: E402
from itts_hip import synth  # noqa: E402
from test_gpu_engine_fp8 import CFG, CFG3  # noqa: E402
from test_gpu_row_retire import DEAD12, LIVE12, STOP, forced_stops, ragged  # noqa: E402

STEPS = 32
# (mode, top_k, top_p, temperature, penalty): two greedy penalties, a narrow and a wide sampled row
G10, G15, NAR, WID = (0, 0, 1.0, 1.0, 10.0), (0, 0, 1.0, 1.0, 1.5), (1, 30, 0.8, 0.9, 10.0), (1, 0, 0.9, 1.0, 1.5)
NAR2 = (1, 100, 0.95, 1.2, 2.0)


def gen(eng, cond, text, table=None, scalar=None, u=None, retire_after=(), forced=None, chunk=8):
    """prefill + decode to STEPS tokens (suppress_stop: rows end through forced stops only) with a per-row table, or with one
    entry as the scalar setting (today's setters).  -> (codes [B, STEPS], logits [B, V], decode_mode, retire answers)"""
    eng.set_forced(forced)
    penalty = 10.0
    try:
        if table is not None:
            eng.set_sampling_rows(table, u)
        elif scalar is not None:
            mode, top_k, top_p, temp, penalty = scalar
            eng.set_sampling(bool(mode), top_k, top_p, temp, u)
        eng.prefill(cond, text, STEPS, penalty, True)
        done, answered = 1, []
        for stop in sorted(set(retire_after)) + [STEPS]:
            while done < stop:
                n = min(chunk, stop - done)
                eng.decode(n)
                done += n
            if stop in retire_after:
                answered.append(eng.retire_rows())
        assert eng.status()[0] == STEPS
        codes, lg = eng.fetch(logits=True)
        mode = eng.decode_mode()
        eng._exit()
    finally:
        eng.set_forced(None)
        eng.set_sampling_rows(None)
        eng.set_sampling(False)
    return codes, lg, mode, answered


def rows_equal(got, ref, rows, what):
    for r in rows:
        assert np.array_equal(got[0][r], ref[0][r]), f"{what}: codes of row {r} differ"
        assert np.array_equal(got[1][r].view(np.uint32), ref[1][r].view(np.uint32)), f"{what}: logits of row {r} differ"


def check_table(eng, cond, text, table, u, mode, scalar_cache=None):
    """The mixed generation against one scalar generation per distinct entry; scalar_cache: runs shared between tables of one shape."""
    got = gen(eng, cond, text, table=table, u=u)
    assert got[2] == mode
    cache = {} if scalar_cache is None else scalar_cache
    for entry in sorted(set(table)):
        if entry not in cache:
            cache[entry] = gen(eng, cond, text, scalar=entry, u=u)
            assert cache[entry][2] == mode
        rows_equal(got, cache[entry], [r for r, e in enumerate(table) if e == entry], f"{len(table)} rows, entry {entry}")
    return got, cache


@pytest.fixture(scope="module")
def eng():
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def conds(eng):
    return [eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=s))) for s in (7, 8, 9)]


def uniforms(rows, seed=5):
    return np.random.default_rng(seed).random((STEPS, rows), dtype=np.float32)


def table_of(rows):
    return [(G10, NAR, WID, G15, NAR2)[r % 5] for r in range(rows)]


@pytest.mark.parametrize("rows", (4, 8, 20))
def test_settings_per_row(eng, conds, rows):
    """All three classes and several penalties in one batch of ragged texts: the persistent engine's blocks and head at 4 rows
    (decode_mode 1, the token choice as launches), the launch path above."""
    got, cache = check_table(eng, conds[0], ragged(rows, 11), table_of(rows), uniforms(rows), 1 if rows <= 6 else 0)
    assert len(cache) == (4 if rows == 4 else 5)
    codes = [c[0] for c in cache.values()]
    assert any(not np.array_equal(codes[0], c) for c in codes[1:])  # the settings matter at all


def test_settings_per_row_f16_library():
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.fail("libitts_hip_f16.so was not built")
    e = ieng.build_engine(CFG3, "f16", parts=("gpt",))
    check_table(e, e.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7))), ragged(8, 11), table_of(8), uniforms(8), 0)


def test_uniform_table_is_the_scalar_path(eng, conds):
    """All rows equal: itts_gpt_set_sampling_rows is the scalar setter - the persistent engine with its in-launch greedy sampler."""
    text = ragged(2, 21)
    for entry in (G15, NAR):
        got = gen(eng, conds[0], text, table=[entry] * 2, u=uniforms(2))
        ref = gen(eng, conds[0], text, scalar=entry, u=uniforms(2))
        assert got[2] == ref[2] == 1
        rows_equal(got, ref, (0, 1), f"uniform table {entry}")
    # the table's penalty replaces the prefill's argument (10 in gen): 0.5 rewards a repetition, so the codes part
    rep = (0, 0, 1.0, 1.0, 0.5)
    got, ref = gen(eng, conds[0], text, table=[rep] * 2), gen(eng, conds[0], text, scalar=rep)
    rows_equal(got, ref, (0, 1), "uniform table, penalty 0.5")
    assert not np.array_equal(gen(eng, conds[0], text)[0], got[0])


def test_prefill_refuses_what_has_no_per_row_form(eng, conds):
    text = ragged(4, 31)
    eng.set_sampling_rows(table_of(5), uniforms(5))
    try:
        with pytest.raises(RuntimeError, match="another batch size"):
            eng.prefill(conds[0], text, STEPS, 10.0, True)
        eng.set_sampling_rows(table_of(4), uniforms(4))
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.9), "gpt_set_typical")
        with pytest.raises(RuntimeError, match="typical"):
            eng.prefill(conds[0], text, STEPS, 10.0, True)
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.0), "gpt_set_typical")
        eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 1), "gpt_set_host_sampling")
        with pytest.raises(RuntimeError, match="host sampling"):
            eng.prefill(conds[0], text, STEPS, 10.0, True)
        eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 0), "gpt_set_host_sampling")
        eng.set_beam_sample(3, do_sample=False)
        with pytest.raises(RuntimeError, match="beams"):
            eng.prefill(conds[0], text, STEPS, 10.0, True)
    finally:
        eng.set_beam_sample(1)
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.0), "gpt_set_typical")
        eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 0), "gpt_set_host_sampling")
        eng.set_sampling_rows(None)
        eng._exit()
    with pytest.raises(RuntimeError, match="uniforms"):
        eng.set_sampling_rows(table_of(4), None)


def test_voices_per_row(eng, conds):
    """Three voices over 8 rows (per-row cond of the prefill): row r is the run in which every row has row r's voice."""
    voice = [0, 1, 2, 1, 0, 2, 2, 1]
    text = ragged(8, 41)
    got = gen(eng, torch.cat([conds[v] for v in voice], 0), text)
    refs = [gen(eng, conds[v], text) for v in range(3)]
    for v in range(3):
        rows_equal(got, refs[v], [r for r in range(8) if voice[r] == v], f"voice {v}")
    assert not np.array_equal(refs[0][0], refs[1][0])


def test_latent_pass_with_a_voice_per_sequence(eng, conds):
    voice = [2, 0, 1, 0, 2]
    texts = [synth.text_ids(n, 50 + i, CFG.gpt.number_text_tokens).astype(np.int32) for i, n in enumerate((41, 17, 30, 23, 36))]
    codes = [np.random.default_rng(60 + i).integers(0, STOP, n).astype(np.int32) for i, n in enumerate((25, 31, 9, 18, 28))]
    got = eng.latent_batch(torch.cat(conds, 0), texts, codes, cond_index=voice)
    refs = [eng.latent_batch(conds[v], texts, codes) for v in range(3)]
    for i, v in enumerate(voice):
        assert got[i].shape == refs[v][i].shape == (1, len(codes[i]), CFG.gpt.model_dim)
        assert torch.equal(got[i].view(torch.int16), refs[v][i].view(torch.int16)), i
    assert not torch.equal(refs[0][0], refs[1][0])
    with pytest.raises(RuntimeError, match="conditioning index"):
        eng.latent_batch(torch.cat(conds, 0), texts, codes, cond_index=[0, 1, 3, 0, 0])


def test_retirement_carries_the_table(eng, conds):
    """12 -> 7 rows under a table whose wide rows are among the retiring ones: the entries follow their rows into the new slots
    (rows 7, 9 and 11 move), and the step behind the retirement launches the classes that are left."""
    table = [G10, WID, NAR, NAR, G15, G15, G10, NAR2, WID, NAR, G10, G15]
    assert {table[r] for r in DEAD12} >= {WID} and WID not in {table[r] for r in LIVE12}
    text, f, u = ragged(12, 11), forced_stops(12, DEAD12), uniforms(12, 17)
    ref = gen(eng, conds[0], text, table=table, u=u, forced=f)
    got = gen(eng, conds[0], text, table=table, u=u, forced=f, retire_after=(8,))
    assert ref[3] == [] and got[3] == [7] and got[2] == ref[2] == 0
    for r, s in DEAD12.items():
        assert ref[0][r, s] == STOP and np.all(ref[0][r, s:] == STOP)
    assert np.array_equal(got[0], ref[0])
    rows_equal(got, ref, LIVE12, "12 -> 7 with a table")
    greedy = gen(eng, conds[0], text, forced=f)
    assert not np.array_equal(greedy[0][LIVE12], ref[0][LIVE12])  # the table matters for the live rows


def test_graph_key_follows_the_classes(eng, conds):
    """Two generations of one shape whose tables differ only in the classes present: the step captured for the first must not be
    replayed for the second (it would launch the wrong kernels and leave rows uncommitted)."""
    text, u = ragged(8, 71), uniforms(8, 23)
    a = [G10, NAR, G15, NAR, G10, NAR, G15, G10]
    b = [WID if e == NAR else e for e in a]
    _, cache = check_table(eng, conds[0], text, a, u, 0)
    check_table(eng, conds[0], text, b, u, 0, cache)
    check_table(eng, conds[0], text, a, u, 0, cache)


def test_generate_with_sequences(eng, conds):
    """Engine.generate with one entry per row against generate with every entry as the scalar request; per-row seeds."""
    text = ragged(8, 81)
    ds, tk, tp, tt, pen = [True, False, True, True, False, True, False, True], [30, 30, 0, 100, 5, 30, 1, 0], 0.9, [0.9, 1, 1, 1.2, 1, 0.9, 1, 1], \
        [10.0, 1.5, 1.5, 2.0, 10.0, 10.0, 1.5, 1.5]
    seeds = [3, 4, 5, 3, 9, 3, 1, 5]
    kw = dict(suppress_stop=True, wide_sampler="device")
    got = eng.generate(conds[0], text, STEPS, do_sample=ds, top_k=tk, top_p=tp, temperature=tt, repetition_penalty=pen, seed=seeds, **kw)
    assert eng.decode_mode() == 0 and got.shape == (8, STEPS)
    u = infer_core.row_uniforms(seeds, STEPS)
    for r in range(8):
        ref = eng.generate(conds[0], text, STEPS, do_sample=ds[r], top_k=tk[r], top_p=tp, temperature=tt[r], repetition_penalty=pen[r],
                           uniforms=u, **kw)
        assert np.array_equal(got[r], ref[r]), r
    # all entries equal and one seed: the scalar request itself
    same = eng.generate(conds[0], text, STEPS, do_sample=[True] * 8, top_k=[30] * 8, seed=7, **kw)
    assert np.array_equal(same, eng.generate(conds[0], text, STEPS, do_sample=True, top_k=30, seed=7, **kw))


# ---- the drop-in on the micro checkpoint --------------------------------------------------------------------------------------
MICRO = icfg.micro()


def micro_tts(**kw):
    from indextts.infer import IndexTTS

    sds = {"gpt": synth.gpt_state_dict(MICRO, 1234), "bigvgan": synth.bigvgan_state_dict(MICRO, 1234), "dvae": synth.dvae_state_dict(MICRO, 1234)}
    return IndexTTS(cfg=MICRO, model_dir="/nonexistent", is_fp16=False, state_dicts=sds, **kw)


def test_infer_batch_mixed_dropin(monkeypatch):
    monkeypatch.delenv("ITTS_MIXED_BATCH", raising=False)
    tts = micro_tts(mixed_batch=True)
    mels = [torch.from_numpy(synth.prompt_mel(61, seed=s)) for s in (7, 8, 9)]
    nt = MICRO.gpt.number_text_tokens
    texts = [[synth.text_ids(n, 100 * u + k, nt).astype(np.int32) for k, n in enumerate(ns)] for u, ns in enumerate(((11, 7), (9,), (5, 12), (8,)))]
    prompts = [mels[0], mels[1], mels[2], mels[1]]  # 4 utterances, 3 voices
    per = [dict(do_sample=False), dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=11),
           dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.7, repetition_penalty=2.0, seed=12), dict(do_sample=False)]  # 3 settings
    calls = []
    real = tts.engine.generate
    monkeypatch.setattr(tts.engine, "generate", lambda *a, **k: (calls.append(k), real(*a, **k))[1])

    def run(t, prompts, per, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached
            return [w for _, w in t.infer_batch(prompts, texts, num_beams=1, max_mel_tokens=24, per_utterance=per, **kw)]

    got = run(tts, prompts, per)
    assert len(calls) == 1 and isinstance(calls[0]["temperature"], list) and len(calls[0]["temperature"]) == 6  # one generation, 6 rows
    for u in range(4):
        ref = run(tts, [prompts[u]] * 4, [per[u]] * 4)
        assert got[u].dtype == np.int16 and got[u].shape == ref[u].shape and np.array_equal(got[u], ref[u]), u
    assert got[0].shape != got[1].shape or not np.array_equal(got[0], got[1])
    # the switch off: today's output for uniform kwargs, with or without the environment's override of the setter
    off = micro_tts()
    want = run(off, prompts, None, do_sample=False)
    monkeypatch.setenv("ITTS_MIXED_BATCH", "0")
    calls.clear()
    forced_off = run(tts, prompts, None, do_sample=False)
    assert len(calls) == 3  # one generation per voice, as today
    monkeypatch.setenv("ITTS_MIXED_BATCH", "1")
    on = run(off, prompts, None, do_sample=False)
    for u in range(4):
        assert np.array_equal(forced_off[u], want[u]) and np.array_equal(on[u], want[u]), u
