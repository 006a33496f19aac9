"""GPU: retirement of finished beam groups (Engine.set_retire_beams + Engine.retire_rows / itts_gpt_set_retire_beams, opt-in): a
running beam generation is compacted to the rows of its unfinished batch items - a group of num_beams rows moves as a unit -, the
following steps run and are captured at the smaller row count, and the caller still sees every original item.

Every comparison is against the same engine object running the same request WITHOUT retirement, on the launch path.  Inside one
projection-kernel family (5 - 16 rows, 17+ rows) a row's bits depend neither on its slot nor on its companions, so everything is
compared bit for bit: the codes of all original items (all num_return_sequences hypotheses), the last logits of the rows that were
not retired, rows() after the call.  Free-running beams cannot be teacher-forced, so retirements that cross families are not held
to this: there a near-tie may flip, as docs and tests of the single-beam retirement say.

Groups finish on their own: the checkpoint is synth.gpt_state_dict(.., profile="smooth", stop_bias=..) (forced tokens cannot finish
a beam group).  The retirement point is taken from the reference run's own per-step status - the first step at which at least one
group and not all groups are done while the surviving row count stays in the family and above 6 - and every test asserts that such
a step exists before the last one.  Sizes are those of tests/test_gpu_row_retire.py: 1.5 dims, 3 layers, 32 steps, ragged texts.

The settings were chosen on the CPU oracle (oracle/gpt.py beam_sample_generate + oracle/hf_beam.py, fp32, same config, uniforms
default_rng(seed + 6).random((32, items, 2 * num_beams))) so that the groups' done steps are spread over at least 8 steps and at
least two groups are still open 4 steps after the first is done.  The oracle's done steps (tokens generated when the item became
done; - = open after 32):
    beam_sample  5 x 3  stop_bias 3.0  seed 11   14 28 13 23 14   (two retirements: 15 -> 12 -> 9 rows)
    beam_sample  8 x 3  stop_bias 3.0  seed 21   13 17 18 20 11 17 19  6
    beam_search  5 x 3  stop_bias 2.5  seed 11    - 14 12 24 12
    beam_sample  8 x 2  stop_bias 3.0  seed 11   22 30  6 14 11 23 11 23
    3 returns, length_penalty 1, 5 x 3, 3.0, 11  14 31 13 23 15
    typical 0.9  5 x 3  stop_bias 6.0  seed 11   24 15 14 12 31
(the bf16 engine's own done steps are printed by every test; they need not be the oracle's).
top_k = 0 is the exception: hf_beam.warp_row keeps at most 128 candidates (the narrow kernels' cap), so the oracle does not restate
the whole-vocabulary sampler, and without TopK the stop token is drawn far less often.  That case was chosen by the same rule on
the device's own reference trace (5 x 3, seed 11): stop_bias 5.0 -> 21 - 31 - -, 5.5 -> - 15 23 27 -, 6.0 -> 13 9 18 15 9 (taken),
7.0 -> 6 6 3 5 2."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import lib as L  # noqa: E402
from itts_hip import synth  # noqa: E402
from test_gpu_engine_fp8 import CFG3  # noqa: E402
from test_gpu_row_retire import ragged  # noqa: E402

STEPS = 32
STOP = CFG3.gpt.stop_mel_token


@functools.lru_cache(maxsize=None)
def state_dict(stop_bias):
    return synth.gpt_state_dict(CFG3, 1234, profile="smooth", stop_bias=stop_bias)


def build(stop_bias=3.0, dtype="bf16", **kw):
    return ieng.build_engine(CFG3, dtype, parts=("gpt",), state_dicts={"gpt": state_dict(stop_bias)}, **kw)


@pytest.fixture(scope="module")
def eng():
    return build()


@pytest.fixture(scope="module")
def untouched():  # an engine object that never sees the switch
    return build()


@pytest.fixture(scope="module")
def cond(eng):
    return eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))


def uniforms(items, nb, seed):
    return np.random.default_rng(seed + 6).random((STEPS, items, 2 * nb), dtype=np.float32)


def beam_gen(eng, cond, text, nb, u, retire_at=(), trace=False, engine=False, steps=STEPS, typical=0.0, **beam_kw):
    """prefill + decode to `steps` tokens, one step per call, with retire_rows() at the token counts in retire_at.
    -> dict(codes [items * returns, steps], logits [items * nb, V], rows, answered, done {tokens: per-item flags} (trace only))"""
    items = text.shape[0]
    eng.debug(no_engine=not engine, engine=engine)
    if typical:
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, float(typical)), "gpt_set_typical")
    eng.set_beam_sample(nb, uniforms=u, **beam_kw)
    try:
        eng.prefill(cond, text, steps, 10.0, False)
        assert eng.rows() == items * nb
        tokens, answered, done = 1, [], {}
        while True:
            if trace:
                orig, ln, unf = eng.row_status()
                assert np.all(ln == tokens) and orig.tolist() == list(range(items * nb))
                done[tokens] = [not unf[i * nb] for i in range(items)]
            if tokens in retire_at:
                answered.append(eng.retire_rows())
                assert eng.rows() == answered[-1]
            if tokens == steps:
                break
            eng.decode(1)
            tokens += 1
        assert eng.status()[0] == steps
        codes, lg = eng.fetch(logits=True)
        out = dict(codes=codes, logits=lg, rows=eng.rows(), answered=answered, done=done, mode=eng.decode_mode())
        eng._exit()
    finally:
        eng.set_beam_sample(1)
        if typical:
            eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.0), "gpt_set_typical")
        eng.debug()
    return out


def family(rows):
    return 0 if rows <= 4 else 1 if rows <= 16 else 2


def points(done, items, nb, n=1, parity=None):
    """The retirement points of a reference trace: the first token count (of the wanted parity) at which at least one more group is
    done than at the last point, not all are, and the surviving rows stay in the family of the rows before and above 6."""
    out, rows, n_done = [], items * nb, 0
    for t in range(1, STEPS):  # before the last step
        d = sum(done[t])
        after = (items - d) * nb
        if d > n_done and d < items and after > 6 and family(after) == family(rows) and (parity is None or t % 2 == parity):
            out.append(t)
            rows, n_done = after, d
            if len(out) == n:
                break
    return out


def first_done(done, items):
    return [next((t for t in sorted(done) if done[t][i]), None) for i in range(items)]


def retire_case(eng, cond, items, nb, seed, n=1, parity=None, what="", **kw):
    text, u = ragged(items, seed), uniforms(items, nb, seed)
    ref = beam_gen(eng, cond, text, nb, u, trace=True, **kw)
    pts = points(ref["done"], items, nb, n, parity)
    print(f"{what or 'beam retire'} {items} x {nb}: done steps {first_done(ref['done'], items)}, retirement at {pts}")
    # precondition of the yardstick, not a property of the code under test: the groups finish at different steps
    assert len(pts) == n, f"no retirement point: done steps {first_done(ref['done'], items)}"
    got = beam_gen(eng, cond, text, nb, u, retire_at=pts, **kw)
    want_rows = [(items - sum(ref["done"][t])) * nb for t in pts]
    assert got["answered"] == want_rows and got["rows"] == want_rows[-1] and ref["rows"] == items * nb
    assert ref["mode"] == got["mode"] == 0
    keep = kw.get("num_return_sequences", 1)
    assert got["codes"].shape == ref["codes"].shape == (items * keep, STEPS)
    bad = sorted(set((np.nonzero(got["codes"] != ref["codes"])[0] // keep).tolist()))
    assert not bad, f"{what}: codes differ in items {bad} (retired at the last point: {np.nonzero(ref['done'][pts[-1]])[0].tolist()})"
    live = [i * nb + q for i in range(items) if not ref["done"][pts[-1]][i] for q in range(nb)]
    a, b = got["logits"][live].view(np.uint32), ref["logits"][live].view(np.uint32)
    assert np.array_equal(a, b), f"{what}: logits of the live rows differ, max {float(np.abs(got['logits'][live] - ref['logits'][live]).max())}"
    for i in np.nonzero(ref["done"][pts[-1]])[0]:  # the yardstick: a retired item's best hypothesis ends in stop
        assert ref["codes"][i * keep, -1] == STOP
    return ref, got, pts


@pytest.fixture()
def on(eng):
    eng.set_retire_beams(True)
    yield eng
    eng.set_retire_beams(False)


def test_beam_sample_5x3(on, cond):
    """15 rows, the 5 - 16 family on both sides."""
    retire_case(on, cond, 5, 3, 11, what="beam_sample")


def test_beam_sample_8x3(on, cond):
    """24 rows, the 17+ family: at most 2 groups can retire."""
    ref, got, pts = retire_case(on, cond, 8, 3, 21, what="beam_sample 17+")
    assert got["rows"] >= 18


@pytest.mark.parametrize("parity", [0, 1])
def test_both_parities(on, cond, parity):
    """Retirement at an even and at an odd token count: the live half of beam_ids / anc is half 0 (rows_move in place) or half 1
    (two rows_gather launches through the dead half 0, its base moves with the row count)."""
    ref, got, pts = retire_case(on, cond, 5, 3, 11, parity=parity, what=f"parity {parity}")
    assert pts[0] % 2 == parity


def test_two_retirements(on, cond):
    """15 -> 12 -> 9 rows in the oracle (items 2, then 0 and 4): the second retirement works on slots that are no longer the
    original rows, and its store already holds an item."""
    ref, got, pts = retire_case(on, cond, 5, 3, 11, n=2, what="two retirements")
    assert len(got["answered"]) == 2 and 6 < got["answered"][1] < got["answered"][0] < 15


def test_beam_search(cond):
    e = build(2.5, retire_beams=True)
    retire_case(e, cond, 5, 3, 11, do_sample=False, what="beam_search")


def test_two_beams(on, cond):
    retire_case(on, cond, 8, 2, 11, what="nb = 2")


def test_three_returns_with_length_penalty(on, cond):
    retire_case(on, cond, 5, 3, 11, num_return_sequences=3, length_penalty=1.0, what="3 returns, length_penalty 1")


def test_typical_filtering(cond):
    e = build(6.0, retire_beams=True)
    retire_case(e, cond, 5, 3, 11, typical=0.9, what="typical 0.9")


def test_kv_fp8_cache(on, cond):
    on.set_kv_fp8(True)
    try:
        retire_case(on, cond, 5, 3, 11, what="fp8 K/V cache")
    finally:
        on.set_kv_fp8(False)


def test_fp8_weights(cond):
    retire_case(build(gpt_fp8="fp8", retire_beams=True), cond, 5, 3, 11, what="fp8 weights")


def test_f16_library(cond):
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    retire_case(build(dtype="f16", retire_beams=True), cond, 5, 3, 11, what="f16 library")


def test_fp32_engine(cond):
    retire_case(build(dtype="fp32", retire_beams=True), cond, 5, 3, 11, what="fp32 engine")


def test_device_wide_beam_sampler(cond):
    """top_k = 0 on the device: beam_wide_cand_kernel + beam_wide_pick_kernel in front of beam_select_kernel; their block is
    carved at the prefill's row count and indexed by row / item.  (stop_bias 6: see the module docstring.)"""
    retire_case(build(6.0, retire_beams=True), cond, 5, 3, 11, top_k=0, what="top_k 0, device")


def test_generate_loop(eng, cond):
    """generate(num_beams=3, retire_rows=0.5, retire_beams=True) against the same call without the switches: the same codes, it
    did retire (the step was captured again at a smaller row count), and nothing of the switch stays behind."""
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    kw = dict(num_beams=nb, do_sample=True, uniforms=u, check_every=4)
    ref = eng.generate(cond, text, STEPS, **kw)
    assert eng.rows() == items * nb
    c0 = eng.lib.itts_gpt_graph_captures(eng.h)
    plain = eng.generate(cond, text, STEPS, retire_rows=0.5, **kw)  # retire_rows alone: beams ignore it, as before
    assert eng.rows() == items * nb and eng.lib.itts_gpt_graph_captures(eng.h) == c0
    got = eng.generate(cond, text, STEPS, retire_rows=0.5, retire_beams=True, **kw)
    rows = eng.rows()
    print(f"generate(retire_rows=0.5, retire_beams=True): {items * nb} -> {rows} rows")
    assert 6 <= rows < items * nb and rows % nb == 0 and eng.lib.itts_gpt_graph_captures(eng.h) > c0
    again = eng.generate(cond, text, STEPS, **kw)
    assert eng.rows() == items * nb
    assert got.shape == ref.shape and np.array_equal(got, ref) and np.array_equal(plain, ref) and np.array_equal(again, ref)


def done_point(ref, items, nb):
    pts = points(ref["done"], items, nb)
    assert pts, first_done(ref["done"], items)
    return pts


def test_switch_off_is_a_noop_and_the_environment_overrides(eng, untouched, cond, monkeypatch):
    """Without the switch retire_rows() under beams with a done group answers the unchanged count and changes no bit; an engine
    object that never saw the switch produces the same; ITTS_RETIRE_BEAMS overrides the setter in both directions."""
    monkeypatch.delenv("ITTS_RETIRE_BEAMS", raising=False)
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    eng.set_retire_beams(True)
    eng.set_retire_beams(False)
    ref = beam_gen(eng, cond, text, nb, u, trace=True)
    pts = done_point(ref, items, nb)
    off = beam_gen(eng, cond, text, nb, u, retire_at=pts)
    assert off["answered"] == [items * nb] and off["rows"] == items * nb
    never = beam_gen(untouched, cond, text, nb, u)
    for other in (off, never):
        assert np.array_equal(other["codes"], ref["codes"]) and np.array_equal(other["logits"].view(np.uint32), ref["logits"].view(np.uint32))
    want = (items - sum(ref["done"][pts[0]])) * nb
    monkeypatch.setenv("ITTS_RETIRE_BEAMS", "1")
    assert beam_gen(eng, cond, text, nb, u, retire_at=pts)["answered"] == [want]
    eng.set_retire_beams(True)
    try:
        monkeypatch.setenv("ITTS_RETIRE_BEAMS", "0")
        assert beam_gen(eng, cond, text, nb, u, retire_at=pts)["answered"] == [items * nb]
        monkeypatch.delenv("ITTS_RETIRE_BEAMS")
        assert beam_gen(eng, cond, text, nb, u, retire_at=pts)["answered"] == [want]
    finally:
        eng.set_retire_beams(False)


def test_noop_input_tokens(on, cond):
    """`input_tokens`: the given steps read the forced table by the absolute step; the branch leaves such a generation alone."""
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    on.set_input_tokens(np.asarray([[5, 9]], np.int32))
    try:
        ref = beam_gen(on, cond, text, nb, u, trace=True)
        done = [t for t in range(1, STEPS) if 0 < sum(ref["done"][t]) < items]
        assert done, first_done(ref["done"], items)
        got = beam_gen(on, cond, text, nb, u, retire_at=done[:1])
    finally:
        on.set_input_tokens(None)
    assert got["answered"] == [items * nb]
    assert np.array_equal(got["codes"], ref["codes"]) and np.array_equal(got["logits"].view(np.uint32), ref["logits"].view(np.uint32))


def test_noop_host_beam_warpers(on, cond):
    items, nb = 3, 3
    text = ragged(items, 11)
    on._ck(on.lib.itts_gpt_set_host_sampling(on.h, 1), "gpt_set_host_sampling")
    on.set_beam_sample(nb, top_k=0, host=True)
    try:
        on.prefill(cond, text, STEPS, 10.0, False)
        before, after = (np.empty((items * nb, CFG3.gpt.number_mel_codes), np.float32) for _ in range(2))
        on._ck(on.lib.itts_gpt_fetch(on.h, None, before.ctypes.data, on._s()), "gpt_fetch")
        assert on.retire_rows() == items * nb and on.rows() == items * nb
        on._ck(on.lib.itts_gpt_fetch(on.h, None, after.ctypes.data, on._s()), "gpt_fetch")
        on._exit()
    finally:
        on.set_beam_sample(1)
        on._ck(on.lib.itts_gpt_set_host_sampling(on.h, 0), "gpt_set_host_sampling")
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_noop_on_the_persistent_engine(on, cond):
    """2 x 3 = 6 rows on the persistent engine: whatever is done, the rows stay."""
    items, nb = 2, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    ref = beam_gen(on, cond, text, nb, u, engine=True, trace=True)
    got = beam_gen(on, cond, text, nb, u, engine=True, retire_at=(8, 20, 30))
    print(f"persistent engine 2 x 3: done steps {first_done(ref['done'], items)}")
    assert ref["mode"] == got["mode"] == 1 and got["answered"] == [6, 6, 6]
    assert np.array_equal(got["codes"], ref["codes"]) and np.array_equal(got["logits"].view(np.uint32), ref["logits"].view(np.uint32))


def test_infer_batch_default_kwargs(monkeypatch):
    """IndexTTS.infer_batch on the micro checkpoint with the default kwargs (num_beams=3, do_sample=True): the same waveforms with
    and without the switch, and with it the generation did retire."""
    from indextts.infer import IndexTTS

    monkeypatch.delenv("ITTS_RETIRE_BEAMS", raising=False)
    monkeypatch.delenv("ITTS_RETIRE_ROWS", raising=False)
    micro = icfg.micro()
    sds = {"gpt": synth.gpt_state_dict(micro, 1234, stop_bias=MICRO_STOP_BIAS), "bigvgan": synth.bigvgan_state_dict(micro, 1234)}
    tts = IndexTTS(cfg=micro, model_dir="/nonexistent", is_fp16=False, state_dicts=sds)
    mel = torch.from_numpy(synth.prompt_mel(61, seed=7)).cuda()
    utts = [[synth.text_ids(5 + 3 * i, 300 + i, micro.gpt.number_text_tokens).astype(np.int32)] for i in range(4)]
    answered = []
    plain = tts.engine.retire_rows

    def spy():
        answered.append(plain())
        return answered[-1]

    monkeypatch.setattr(tts.engine, "retire_rows", spy)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        torch.manual_seed(MICRO_SEED)
        off = tts.infer_batch(mel, utts, max_mel_tokens=STEPS)
        assert not answered
        tts.retire_rows, tts.retire_beams = 0.5, True
        torch.manual_seed(MICRO_SEED)
        on = tts.infer_batch(mel, utts, max_mel_tokens=STEPS)
    print(f"infer_batch 4 x 3 with retire_beams: retire_rows() answered {answered}")
    assert answered and min(answered) < 12, answered
    for (sa, a), (sb, b) in zip(on, off):
        assert sa == sb and a.shape == b.shape and np.array_equal(a, b)


MICRO_STOP_BIAS = 0.0  # the micro checkpoint of the other drop-in tests: its sentences stop on their own, at different steps
MICRO_SEED = 6
