"""GPU: row retirement of a running batched decode (Engine.retire_rows / itts_gpt_retire_rows, opt-in): the decode state of a
single-beam generation is compacted to its unfinished rows, the following steps run - and are captured - at the smaller row count,
the caller still sees the original batch.

Every comparison is against the same engine object running the same request WITHOUT retirement.  Inside one projection-kernel
family (5 - 16 rows, 17+ rows, and the fp32 engine's kernels) a row's results depend neither on its slot nor on the other rows, so
codes and logits are compared bit for bit; across families (12 -> 3 rows) under teacher forcing against the project's
cross-family bound of tests/test_gpu_configs.py.

Rows are made to finish at chosen steps with set_forced (stop at step s_b for the retiring rows, -1 elsewhere) under
suppress_stop=True, so the other rows run free and never stop.  Sizes: those of tests/test_gpu_engine_fp8.py (1.5 dims with 3
layers, text length 41, 32 steps)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import engine as ieng  # noqa: E402
from itts_hip import lib as L  # noqa: E402
from itts_hip import synth  # noqa: E402
from test_gpu_engine_fp8 import CFG, CFG3, TEXT_LEN, run, same_bits, texts  # noqa: E402

STEPS = 32
STOP = CFG.gpt.stop_mel_token
DEAD12 = {1: 3, 3: 4, 4: 5, 8: 6, 10: 7}  # row -> the step at which it is forced to stop (12 -> 7 rows)
LIVE12 = [r for r in range(12) if r not in DEAD12]


def ragged(rows, seed):
    """[rows, TEXT_LEN] text ids of different lengths (stop ids are stripped and left-padded -> kv_start)."""
    t = np.full((rows, TEXT_LEN), CFG.gpt.stop_text_token, np.int32)
    for r in range(rows):
        n = [41, 30, 17, 36, 23, 33, 12, 39, 27, 20, 35, 15][r % 12] - (r // 12)
        t[r, :n] = synth.text_ids(n, seed + r, CFG.gpt.number_text_tokens)
    return t


def forced_stops(rows, dead, n=8):
    f = np.full((rows, n), -1, np.int32)
    for r, s in dead.items():
        f[r, s] = STOP
    return f


def plan_of(rows, dead):
    unf = np.asarray([0 if r in dead else 1 for r in range(rows)], np.int32)
    src, dst = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    n, m = C.c_int(), C.c_int()
    assert L.load().itts_retire_plan(unf.ctypes.data_as(C.c_void_p), rows, C.byref(n), src.ctypes.data_as(C.c_void_p),
                                     dst.ctypes.data_as(C.c_void_p), C.byref(m)) == 0
    return n.value, src[: m.value].tolist(), dst[: m.value].tolist()


def gen(eng, cond, text, steps=STEPS, retire_after=(), forced=None, engine=None, chunk=8):
    """prefill + decode to `steps` tokens with retire_rows() after the token counts in retire_after.
    -> (codes [B, steps], logits [B, V], decode_mode, the row counts the retire calls answered)"""
    if engine is not None:
        eng.debug(no_engine=not engine, engine=engine)
    eng.set_forced(forced)
    try:
        eng.prefill(cond, text, steps, 10.0, True)
        assert eng.rows() == text.shape[0] * getattr(eng, "_nb", 1)
        done, answered = 1, []
        for stop in sorted(set(retire_after)) + [steps]:
            while done < stop:
                n = min(chunk, stop - done)
                eng.decode(n)
                done += n
            if stop in retire_after:
                answered.append(eng.retire_rows())
                assert eng.rows() == answered[-1]
        assert eng.status()[0] == steps
        codes, lg = eng.fetch(logits=True)
        mode = eng.decode_mode()
        eng._exit()
    finally:
        eng.set_forced(None)
        if engine is not None:
            eng.debug()
    return codes, lg, mode, answered


def assert_same(got, ref, live, what=""):
    """codes of ALL original rows, logits of the live rows: bit for bit; the mode"""
    assert np.array_equal(got[0], ref[0]), f"{what}: codes differ in rows {sorted(set(np.nonzero(got[0] != ref[0])[0].tolist()))}"
    a, b = got[1][live].view(np.uint32), ref[1][live].view(np.uint32)
    assert np.array_equal(a, b), f"{what}: logits differ, max {float(np.abs(got[1][live] - ref[1][live]).max())}"
    assert got[2] == ref[2] == 0


@pytest.fixture(scope="module")
def eng():
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def untouched():  # an engine object on which no retire call is ever made
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def cond(eng):
    return eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))


def retire_12_to_7(e, cond, seed=11, **kw):
    text = ragged(12, seed)
    f = forced_stops(12, DEAD12)
    ref = gen(e, cond, text, forced=f, **kw)
    got = gen(e, cond, text, forced=f, retire_after=(8,), **kw)
    assert ref[3] == [] and got[3] == [7]
    for r, s in DEAD12.items():  # the yardstick itself: the rows stopped where they were told to, the others never
        assert ref[0][r, s] == STOP and np.all(ref[0][r, s:] == STOP) and not np.any(ref[0][r, :s] == STOP)
    assert not np.any(ref[0][LIVE12] == STOP)
    assert_same(got, ref, LIVE12, "12 -> 7")
    return got, ref


def test_12_to_7_rows_in_family(eng, cond):
    """5 - 16 rows on both sides (LayerNorm-in-projection MFMA kernels, 1024-thread attention).  Rows 7, 9 and 11 change slot."""
    n, src, dst = plan_of(12, DEAD12)
    assert n == 7 and src == [7, 9, 11] and dst == [1, 3, 4]
    retire_12_to_7(eng, cond)


def test_40_to_33_rows_in_family(eng, cond):
    """The K-split family on both sides; 33 x 20 and 40 x 20 heads are both >= 512: the 256-thread attention on both sides."""
    dead = {2: 3, 5: 4, 11: 5, 17: 6, 20: 7, 30: 3, 38: 5}
    live = [r for r in range(40) if r not in dead]
    n, src, dst = plan_of(40, dead)
    assert n == 33 and len(src) == 6 and src[0] >= 33
    text = ragged(40, 21)
    f = forced_stops(40, dead)
    ref = gen(eng, cond, text, forced=f)
    got = gen(eng, cond, text, forced=f, retire_after=(8,))
    assert got[3] == [33]
    assert_same(got, ref, live, "40 -> 33")


def test_fp32_engine(cond):
    e = ieng.build_engine(CFG3, "fp32", parts=("gpt",))
    retire_12_to_7(e, cond)


def test_kv_fp8_cache(eng, cond):
    eng.set_kv_fp8(True)
    try:
        retire_12_to_7(eng, cond)
    finally:
        eng.set_kv_fp8(False)


def test_f16_library(cond):
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.skip("libitts_hip_f16.so was not built")
    e = ieng.build_engine(CFG3, "f16", parts=("gpt",))
    retire_12_to_7(e, cond)


def test_fp8_weights(cond):
    e = ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8="fp8")
    retire_12_to_7(e, cond)


@pytest.mark.parametrize("top_k", [30, 0])
def test_sampling_uniforms_are_repacked(eng, cond, top_k):
    """do_sample with given uniforms [32][12]: the sampler reads uniforms[k * B + b], so the retirement re-packs them by original
    row.  top_k = 30: the narrow device sampler; top_k = 0: the whole-vocabulary device sampler."""
    u = np.random.default_rng(17).random((STEPS, 12), dtype=np.float32)
    text = ragged(12, 31)
    f = forced_stops(12, DEAD12)
    eng.set_sampling(True, top_k, 0.8, 1.0, u)
    try:
        ref = gen(eng, cond, text, forced=f)
        got = gen(eng, cond, text, forced=f, retire_after=(8,))
    finally:
        eng.set_sampling(False)
    greedy = gen(eng, cond, text, forced=f)
    assert not np.array_equal(greedy[0], ref[0])  # the draws matter
    assert got[3] == [7]
    assert_same(got, ref, LIVE12, f"sampling top_k={top_k}")


def test_two_retirements(eng, cond):
    dead = {1: 2, 3: 3, 4: 4, 8: 6, 10: 7}
    text = ragged(12, 41)
    f = forced_stops(12, dead)
    ref = gen(eng, cond, text, forced=f)
    got = gen(eng, cond, text, forced=f, retire_after=(5, 9))
    assert got[3] == [9, 7]
    assert_same(got, ref, LIVE12, "12 -> 9 -> 7")


def test_generate_loop(eng, cond):
    """generate(retire_rows=0.75) against generate(): the rows stop through forced stops while the loop polls status() every 4
    steps - 3 rows by step 5 (12 -> 9), 3 more by step 9 (9 -> 6: six rows and below are left alone), 2 later ones."""
    dead = {0: 2, 5: 3, 9: 4, 2: 6, 6: 7, 11: 8, 3: 14, 7: 19}
    text = ragged(12, 51)
    eng.set_forced(forced_stops(12, dead, n=20))
    try:
        ref = eng.generate(cond, text, 40, check_every=4)
        assert eng.rows() == 12
        got = eng.generate(cond, text, 40, check_every=4, retire_rows=0.75)
        assert eng.rows() == 6 and eng.decode_mode() == 0
        again = eng.generate(cond, text, 40, check_every=4)  # and the option leaves nothing behind
        assert eng.rows() == 12
    finally:
        eng.set_forced(None)
    for r, s in dead.items():
        assert ref[r, s] == STOP
    assert got.shape == ref.shape and np.array_equal(got, ref) and np.array_equal(again, ref)


def rms_rel(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)) / np.sqrt(np.mean(b.astype(np.float64) ** 2)))


def test_across_families_12_to_3_rows(eng, cond, accuracy):
    """12 -> 3 rows: the MFMA kernels before, the GEMV kernels and the split attention after.  Every step of every row is
    teacher-forced with the unretired run's ids, so both runs feed the same tokens; the relative RMS of the live rows' last logits
    against the unretired run stays below 3e-2, the project's bound for cross-family differences (tests/test_gpu_configs.py).
    Measured on an MI355X (profiles/row_retire.txt): 12 -> 3 rows 4.3e-3 / 2.8e-3 / 3.2e-3 for the three live rows; the control -
    the same three rows as a 3-row batch from the start against the 12-row run - 4.2e-3 / 3.2e-3 / 3.4e-3."""
    live = [2, 6, 9]
    dead = {r: 3 + i % 5 for i, r in enumerate(r for r in range(12) if r not in live)}
    assert plan_of(12, dead)[0] == 3
    text = ragged(12, 61)
    free = gen(eng, cond, text, forced=forced_stops(12, dead))
    ids = free[0].astype(np.int32)  # [12, 32]: every step of every row
    ref = gen(eng, cond, text, forced=ids)
    assert same_bits(ref, free)
    got = gen(eng, cond, text, forced=ids, retire_after=(8,))
    assert got[3] == [3] and got[2] == 0
    assert np.array_equal(got[0], ref[0])
    control = gen(eng, cond, text[live], forced=ids[live], engine=False)  # launch path, as after a retirement
    errs = [rms_rel(got[1][r], ref[1][r]) for r in live]
    ctl = [rms_rel(control[1][i], ref[1][r]) for i, r in enumerate(live)]
    print(f"row retirement 12 -> 3 rows, last logits vs the unretired run, rel RMS per live row: {errs}")
    print(f"control: the same 3 rows as a 3-row batch from the start vs the 12-row run: {ctl}")
    accuracy["row_retire_12_to_3_last_logits_rel_rms"] = errs
    accuracy["row_retire_control_3_rows_from_start_rel_rms"] = ctl
    assert max(errs) < 3e-2, errs


def test_noop_beams(eng, cond):
    text = ragged(2, 71)
    eng.set_beam_sample(3, do_sample=False)
    try:
        ref = gen(eng, cond, text, engine=False)
        got = gen(eng, cond, text, retire_after=(8,), engine=False)
    finally:
        eng.set_beam_sample(1)
    assert got[3] == [6] and same_bits(got, ref)


def test_noop_host_sampling(eng, cond):
    text = ragged(12, 81)
    eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 1), "gpt_set_host_sampling")
    try:
        eng.prefill(cond, text, STEPS, 10.0, True)
        before = eng.fetch(logits=True)
        assert eng.retire_rows() == 12 and eng.rows() == 12
        after = eng.fetch(logits=True)
        eng._exit()
    finally:
        eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 0), "gpt_set_host_sampling")
    assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))


def test_noop_on_the_persistent_engine(eng, cond):
    text = ragged(6, 91)
    f = forced_stops(6, {1: 3, 4: 5})
    ref = gen(eng, cond, text, forced=f, engine=True)
    got = gen(eng, cond, text, forced=f, retire_after=(8,), engine=True)
    assert ref[2] == 1 and got[2] == 1 and got[3] == [6]
    assert same_bits(got, ref)


def test_noop_nothing_or_everything_finished(eng, cond):
    text = ragged(12, 101)
    ref = gen(eng, cond, text)
    got = gen(eng, cond, text, retire_after=(8,))
    assert got[3] == [12] and same_bits(got, ref)
    f = forced_stops(12, {r: 3 for r in range(12)})
    ref = gen(eng, cond, text, forced=f)
    got = gen(eng, cond, text, forced=f, retire_after=(8,))
    assert got[3] == [12] and same_bits(got, ref)
    assert np.all(ref[0][:, 3:] == STOP)


def test_stale_graph_and_default_unchanged(eng, untouched, cond):
    """After a 12 -> 7 generation the object holds a 7-row step captured over a 12-row cache layout: a fresh 7-row generation must
    not replay it (GraphKey::Bcache).  And with the option unset a generation equals the one of an engine object on which no
    retire call was ever made: codes, logits, decode_mode()."""
    retire_12_to_7(eng, cond)
    for rows in (7, 12):
        text = ragged(rows, 111)
        got = gen(eng, cond, text)
        ref = gen(untouched, cond, text)
        assert got[2] == ref[2] == 0
        assert same_bits(got, ref), rows
    text = texts(2, 121)  # ... and the persistent engine is back for the next small generation
    got = run(eng, cond, text, STEPS, no_engine=False)
    ref = run(untouched, cond, text, STEPS, no_engine=False)
    assert got[2] == ref[2] == 1 and same_bits(got, ref)
