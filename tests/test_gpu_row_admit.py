"""GPU: row admission into a running batched decode (Engine.admit_rows / itts_gpt_admit_rows, opt-in): finished slots of a
single-beam generation take new requests, the steps that follow carry them with len = 0, the caller sees every original row.

The invariant is the one row retirement rests on (tests/test_gpu_row_retire.py): within one projection-kernel family (5 - 16
rows, 17+ rows, the fp32 engine's kernels) a row's bits depend neither on its slot nor on its companions.  So
  - the running rows of a generation with an admission equal the same generation without it, bit for bit (this is what fails
    when an admission steps the running rows, resets a neighbour's state or writes a neighbour's cache), and
  - the admitted rows equal a FRESH generation of the admitted requests alone - the same row count and the same text length L, so
    the prefill runs the same kernels - after the same number of tokens, bit for bit.
Across families (seven rows admitted into 40) the first token is still bit-equal (prefill and head run at 7 rows on both sides);
the later steps are teacher-forced and held to the project's cross-family bound (tests/test_gpu_configs.py: 3e-2 relative RMS).

Rows finish through set_forced stops under suppress_stop=True.  Sizes: those of tests/test_gpu_row_retire.py (1.5 dims, 3 layers,
text length 41, 32 steps)."""
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
from test_gpu_engine_fp8 import CFG, CFG3, TEXT_LEN  # noqa: E402
from test_gpu_row_retire import DEAD12, LIVE12, STOP, forced_stops, ragged, rms_rel  # noqa: E402

STEPS = 32
AT = 8                  # tokens the first rows hold when the admission happens
NEW_TOKENS = STEPS - AT + 1  # tokens an admitted row holds at the end: its first one from the admission, then one per step
G10, G15, NAR, WID = (0, 0, 1.0, 1.0, 10.0), (0, 0, 1.0, 1.0, 1.5), (1, 30, 0.8, 0.9, 10.0), (1, 0, 0.9, 1.0, 1.5)
WID2 = (1, 200, 0.95, 1.0, 10.0)


def run(eng, cond, text, forced=None, table=None, scalar=None, u=None, events=(), tokens=STEPS, no_graph=False, keep=False, chunk=8):
    """prefill + decode until the first rows hold `tokens` tokens (max_gen = STEPS), with events (at_tokens, kind, payload):
    ("admit", dict(cond=, text=, rows=, uniforms=, forced=)), ("retire", None), ("call", fn(eng)).
    Always on the launch path: a fresh generation of <= 6 rows would otherwise run on the persistent engine, another family.
    -> dict(codes [B0, STEPS], logits [B0, V], mode, slots per admission, recaptured per admission, retire answers, status)"""
    eng.debug(no_graph=no_graph, no_engine=True)
    eng.set_forced(forced)
    out = dict(slots=[], recaptured=[], answered=[])
    penalty = 10.0
    try:
        if keep:
            eng.keep_row_table(True)
        if table is not None:
            eng.set_sampling_rows(table, u)
        elif scalar is not None:
            penalty = scalar[4]
            eng.set_sampling(bool(scalar[0]), scalar[1], scalar[2], scalar[3], u)
        eng.prefill(cond, text, STEPS, penalty, True)
        done = 1
        pending = None
        for at, kind, payload in sorted(events, key=lambda e: e[0]) + [(tokens, "end", None)]:
            while done < at:
                n = min(chunk, at - done)
                eng.decode(n)
                done += n
                if pending is not None:
                    out["recaptured"].append(eng.lib.itts_gpt_graph_captures(eng.h) - pending)
                    pending = None
            if kind == "admit":
                pending = eng.lib.itts_gpt_graph_captures(eng.h)
                p = dict(payload)
                out["slots"].append(eng.admit_rows(p.pop("cond"), p.pop("text"), **p).tolist())
            elif kind == "retire":
                out["answered"].append(eng.retire_rows())
            elif kind == "call":
                payload(eng)
        out["status"] = eng.row_status()
        out["codes"], out["logits"] = eng.fetch(logits=True)
        out["mode"] = eng.decode_mode()
        eng._exit()
    finally:
        eng.set_forced(None)
        eng.set_sampling_rows(None)
        eng.set_sampling(False)
        eng.keep_row_table(False)
        eng.debug()
    return out


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_running_rows(got, ref, live, what):
    """the first rows: codes of all of them (a replaced row: its codes, then stop), last logits of the ones still running"""
    nrow = ref["codes"].shape[0]
    assert np.array_equal(got["codes"][:nrow], ref["codes"]), \
        f"{what}: codes of the first rows differ in rows {sorted(set(np.nonzero(got['codes'][:nrow] != ref['codes'])[0].tolist()))}"
    assert bits_equal(got["logits"][live], ref["logits"][live]), f"{what}: last logits of the running rows differ"


def assert_admitted_rows(got, first, fresh, what, n_tok=NEW_TOKENS):
    n = fresh["codes"].shape[0]
    a, f = got["codes"][first:first + n], fresh["codes"]
    assert np.array_equal(a[:, :n_tok], f[:, :n_tok]), f"{what}: codes of the admitted rows differ from the fresh generation's in rows " \
                                                       f"{sorted(set(np.nonzero(a[:, :n_tok] != f[:, :n_tok])[0].tolist()))}"
    assert np.all(a[:, n_tok:] == STOP), f"{what}: something behind an admitted row's own tokens"
    assert bits_equal(got["logits"][first:first + n], fresh["logits"]), f"{what}: last logits of the admitted rows differ"


def free_forced(n):
    return np.full((n, 8), -1, np.int32)


@pytest.fixture(scope="module")
def eng():
    return ieng.build_engine(CFG3, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def conds(eng):
    return [eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=s))) for s in (7, 8)]


def new_requests(conds, n=5, seed=211):
    """n ragged requests with two voices (one conditioning block per row)"""
    text = ragged(12, seed)[[2, 7, 0, 9, 4, 11, 6][:n]]
    cond = torch.cat([conds[i % 2] for i in range(n)], 0)
    return cond, text


def admit_5_into_12(e, conds, **kw):
    """The base case: 12 rows, five forced to stop at steps 3 .. 7; at 8 tokens five requests take their slots; 24 more steps."""
    text, f = ragged(12, 11), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds)
    ref = run(e, conds[0], text, forced=f, **kw)
    got = run(e, conds[0], text, forced=f, events=[(AT, "admit", dict(cond=ncond, text=ntext))], **kw)
    fresh = run(e, ncond, ntext, forced=free_forced(5), tokens=NEW_TOKENS, **kw)
    for r, s in DEAD12.items():  # the yardstick itself: the rows stopped where they were told to, the others never
        assert ref["codes"][r, s] == STOP and np.all(ref["codes"][r, s:] == STOP) and not np.any(ref["codes"][r, :s] == STOP)
    assert not np.any(ref["codes"][LIVE12] == STOP) and not np.any(fresh["codes"][:, :NEW_TOKENS] == STOP)
    assert got["slots"] == [sorted(DEAD12)] and got["codes"].shape == (17, STEPS) and got["logits"].shape[0] == 17
    orig, ln, unf = got["status"]
    assert orig.tolist() == [12 + sorted(DEAD12).index(s) if s in DEAD12 else s for s in range(12)]
    assert ln.tolist() == [NEW_TOKENS if s in DEAD12 else STEPS for s in range(12)] and unf.tolist() == [1] * 12
    assert_running_rows(got, ref, LIVE12, "5 into 12")
    assert_admitted_rows(got, 12, fresh, "5 into 12")
    assert got["mode"] == ref["mode"] == fresh["mode"] == 0
    assert not np.array_equal(fresh["codes"][0], fresh["codes"][1])
    return got, ref, fresh


def test_admit_5_into_12_rows(eng, conds):
    got, _, _ = admit_5_into_12(eng, conds)
    assert got["recaptured"] == [0]  # a scalar generation: B, Bcache and every pointer are what they were - the captured step is kept


def test_graph_replay_equals_eager(eng, conds):
    got, _, _ = admit_5_into_12(eng, conds)
    eager, _, _ = admit_5_into_12(eng, conds, no_graph=True)
    assert np.array_equal(got["codes"], eager["codes"]) and bits_equal(got["logits"], eager["logits"])


def test_fp32_engine(conds):
    admit_5_into_12(ieng.build_engine(CFG3, "fp32", parts=("gpt",)), conds)


def test_kv_fp8_cache(eng, conds):
    eng.set_kv_fp8(True)
    try:
        admit_5_into_12(eng, conds)
    finally:
        eng.set_kv_fp8(False)


def test_fp8_weights(conds):
    admit_5_into_12(ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8="fp8"), conds)


def test_f16_library():
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.fail("libitts_hip_f16.so was not built")
    e = ieng.build_engine(CFG3, "f16", parts=("gpt",))
    admit_5_into_12(e, [e.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=s))) for s in (7, 8)])


def row_u(seeds):
    return np.stack([np.random.default_rng(s).random(STEPS, dtype=np.float32) for s in seeds])  # [n, max_gen]


def test_table_generation_new_class_recaptures(eng, conds):
    """Greedy and top_k = 30 rows run; the admitted rows bring whole-vocabulary rows with per-row seeds: a class that was not
    present, so the graph key changes and the step is captured again.  Replayed and eager."""
    table = [G10 if r % 2 == 0 else NAR for r in range(12)]
    u12 = np.random.default_rng(17).random((STEPS, 12), dtype=np.float32)
    text, f = ragged(12, 31), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds, seed=231)
    ntab, nu = [WID, G15, WID2, NAR, WID], row_u([3, 4, 5, 6, 7])
    ref = run(eng, conds[0], text, forced=f, table=table, u=u12)
    ev = [(AT, "admit", dict(cond=ncond, text=ntext, rows=ntab, uniforms=nu))]
    got = run(eng, conds[0], text, forced=f, table=table, u=u12, events=ev)
    eager = run(eng, conds[0], text, forced=f, table=table, u=u12, events=ev, no_graph=True)
    fresh = run(eng, ncond, ntext, forced=free_forced(5), table=ntab, u=np.ascontiguousarray(nu.T), tokens=NEW_TOKENS)
    assert got["recaptured"] == [1]
    assert_running_rows(got, ref, LIVE12, "table")
    assert_admitted_rows(got, 12, fresh, "table")
    assert np.array_equal(got["codes"], eager["codes"]) and bits_equal(got["logits"], eager["logits"])
    greedy = run(eng, ncond, ntext, forced=free_forced(5), tokens=NEW_TOKENS)
    assert not np.array_equal(greedy["codes"][[0, 2, 3, 4]], fresh["codes"][[0, 2, 3, 4]])  # the admitted rows' settings matter


def test_table_generation_known_classes_keep_the_step(eng, conds):
    """The admitted rows bring other settings but no new class: the captured step is replayed.  And a kept uniform table
    (keep_row_table): all rows greedy at the start, sampled rows admitted into the room the prefill left for their draws."""
    table = [G10 if r % 2 == 0 else NAR for r in range(12)]
    u12 = np.random.default_rng(17).random((STEPS, 12), dtype=np.float32)
    text, f = ragged(12, 31), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds, seed=231)
    ntab, nu = [G15, NAR, (1, 100, 0.95, 1.2, 2.0), G15, NAR], row_u([13, 14, 15, 16, 17])
    got = run(eng, conds[0], text, forced=f, table=table, u=u12, events=[(AT, "admit", dict(cond=ncond, text=ntext, rows=ntab, uniforms=nu))])
    fresh = run(eng, ncond, ntext, forced=free_forced(5), table=ntab, u=np.ascontiguousarray(nu.T), tokens=NEW_TOKENS)
    assert got["recaptured"] == [0]
    assert_admitted_rows(got, 12, fresh, "table, known classes")
    kept = run(eng, conds[0], text, forced=f, table=[G10] * 12, keep=True,
               events=[(AT, "admit", dict(cond=ncond, text=ntext, rows=ntab, uniforms=nu))])
    ref = run(eng, conds[0], text, forced=f)
    assert kept["recaptured"] == [1]  # greedy alone ran: the narrow class is new
    assert_running_rows(kept, ref, LIVE12, "kept uniform table")
    assert_admitted_rows(kept, 12, fresh, "kept uniform table")


def test_one_slot_three_times(eng, conds):
    """Slot 1: the first row 1 (stops at step 3), an admitted request that is told to stop at its step 2, then another one.
    fetch returns every original row once: 12 + 5 + 1."""
    text, f = ragged(12, 11), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds)
    nf = free_forced(5)
    nf[0, 2] = STOP
    last_text = ragged(12, 251)[5:6]
    ref = run(eng, conds[0], text, forced=f)
    got = run(eng, conds[0], text, forced=f, events=[(AT, "admit", dict(cond=ncond, text=ntext, forced=nf)),
                                                      (16, "admit", dict(cond=conds[1], text=last_text))])
    fresh = run(eng, ncond, ntext, forced=nf, tokens=NEW_TOKENS)
    assert got["slots"] == [sorted(DEAD12), [1]] and got["codes"].shape == (18, STEPS)
    assert got["status"][0].tolist()[1] == 17 and sorted(got["status"][0].tolist()) == [0, 2, 5, 6, 7, 9, 11, 13, 14, 15, 16, 17]
    assert_running_rows(got, ref, LIVE12, "slot 1 three times")
    assert np.all(fresh["codes"][0, 2:NEW_TOKENS] == STOP)
    assert np.array_equal(got["codes"][12:17, :NEW_TOKENS], fresh["codes"][:, :NEW_TOKENS]) and np.all(got["codes"][12:17, NEW_TOKENS:] == STOP)
    assert bits_equal(got["logits"][13:17], fresh["logits"][1:])
    mine = STEPS - 16 + 1  # the last request's tokens
    assert not np.any(got["codes"][17, :mine] == STOP) and np.all(got["codes"][17, mine:] == STOP)


def test_admission_then_retirement(eng, conds):
    """The admitted rows are told to stop at their steps 2 .. 6; at 16 tokens the generation retires them: 12 -> 7 rows.  Against
    the same calls without the retirement."""
    text, f = ragged(12, 11), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds)
    nf = free_forced(5)
    for i in range(5):
        nf[i, 2 + i] = STOP
    ev = [(AT, "admit", dict(cond=ncond, text=ntext, forced=nf))]
    ref = run(eng, conds[0], text, forced=f, events=ev)
    got = run(eng, conds[0], text, forced=f, events=ev + [(16, "retire", None)])
    assert got["answered"] == [7] and sorted(got["status"][0].tolist()) == LIVE12 and got["codes"].shape == (17, STEPS)
    assert np.array_equal(got["codes"], ref["codes"]) and bits_equal(got["logits"][LIVE12], ref["logits"][LIVE12])
    for i in range(5):
        assert ref["codes"][12 + i, 2 + i] == STOP and np.all(ref["codes"][12 + i, 2 + i:] == STOP)
    assert got["mode"] == 0


def test_sampled_scalar_generation_then_retirement(eng, conds):
    """A scalar top_k = 30 generation admits rows with its own settings and their draws; the later retirement re-packs the draws
    of the first AND the admitted rows by original row."""
    u12 = np.random.default_rng(27).random((STEPS, 12), dtype=np.float32)
    text, f = ragged(12, 41), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds, seed=261)
    nu, nf = row_u([21, 22, 23, 24, 25]), free_forced(5)
    nf[1, 3] = nf[3, 4] = STOP
    ev = [(AT, "admit", dict(cond=ncond, text=ntext, uniforms=nu, forced=nf))]
    ref = run(eng, conds[0], text, forced=f, scalar=NAR, u=u12)
    noret = run(eng, conds[0], text, forced=f, scalar=NAR, u=u12, events=ev)
    got = run(eng, conds[0], text, forced=f, scalar=NAR, u=u12, events=ev + [(16, "retire", None)])
    fresh = run(eng, ncond, ntext, forced=nf, scalar=NAR, u=np.ascontiguousarray(nu.T), tokens=NEW_TOKENS)
    assert got["answered"] == [10]
    assert_running_rows(noret, ref, LIVE12, "sampled")
    assert np.array_equal(noret["codes"][12:, :NEW_TOKENS], fresh["codes"][:, :NEW_TOKENS])
    assert np.array_equal(got["codes"], noret["codes"])
    live = [r for r in range(17) if r not in DEAD12 and r not in (13, 15)]
    assert bits_equal(got["logits"][live], noret["logits"][live])


def test_7_into_40_rows_across_families(eng, conds, accuracy):
    """The K-split family (17+ rows).  The running rows: bit for bit.  The admitted rows' later steps run beside 39 others, a fresh
    7-row generation's in the 5 - 16 row family: the first token - prefill and head at 7 rows on both sides - is equal, the rest is
    teacher-forced with the fresh run's ids and the last logits are held to the cross-family bound of tests/test_gpu_configs.py."""
    dead = {2: 3, 5: 4, 11: 5, 17: 6, 20: 7, 30: 3, 38: 5}
    live = [r for r in range(40) if r not in dead]
    text, f = ragged(40, 21), forced_stops(40, dead)
    ncond, ntext = new_requests(conds, n=7)
    fresh = run(eng, ncond, ntext, forced=free_forced(7), tokens=NEW_TOKENS)
    ids = fresh["codes"][:, :NEW_TOKENS].astype(np.int32)
    ids[:, 0] = -1  # the first token is the admission's own choice
    ref = run(eng, conds[0], text, forced=f)
    got = run(eng, conds[0], text, forced=f, events=[(AT, "admit", dict(cond=ncond, text=ntext, forced=ids))])
    assert got["slots"] == [sorted(dead)] and got["mode"] == 0
    assert_running_rows(got, ref, live, "7 into 40")
    assert np.array_equal(got["codes"][40:, :NEW_TOKENS], fresh["codes"][:, :NEW_TOKENS])
    errs = [rms_rel(got["logits"][40 + i], fresh["logits"][i]) for i in range(7)]
    print(f"7 rows admitted into 40, last logits vs the fresh 7-row generation, rel RMS per row: {errs}")
    accuracy["row_admit_7_into_40_last_logits_rel_rms"] = errs
    assert max(errs) < 3e-2, errs


def refused(eng, match, **kw):
    with pytest.raises(RuntimeError, match=match):
        eng.admit_rows(**kw)


def test_refusals_leave_the_generation_running(eng, conds):
    text, f = ragged(12, 11), forced_stops(12, DEAD12)
    ncond, ntext = new_requests(conds)
    six = ragged(12, 211)[:6]
    bad_id = ntext.copy()
    bad_id[0, 0] = CFG.gpt.number_text_tokens + 5

    def scalar_refusals(e):
        refused(e, "fewer finished slots", cond=conds[0], text_ids=six)
        refused(e, "more than 128", cond=conds[0], text_ids=np.repeat(six, 22, 0)[:129])
        refused(e, "text id out of range", cond=ncond, text_ids=bad_id)
        refused(e, "text length of the running generation", cond=ncond, text_ids=np.concatenate([ntext, ntext[:, :1]], 1))
        refused(e, "its own settings", cond=ncond, text_ids=ntext, rows=[G15] * 5)
        refused(e, "its own settings", cond=ncond, text_ids=ntext, rows=[NAR] * 5, uniforms=row_u(range(5)))
        refused(e, "top_p", cond=ncond, text_ids=ntext, rows=[(0, 0, 0.0, 1.0, 10.0)] * 5)
        with pytest.raises(ValueError):
            e.admit_rows(torch.cat([conds[0]] * 3, 0), ntext)

    ref = run(eng, conds[0], text, forced=f)
    got = run(eng, conds[0], text, forced=f, events=[(AT, "call", scalar_refusals)])
    assert np.array_equal(got["codes"], ref["codes"]) and bits_equal(got["logits"], ref["logits"]) and got["codes"].shape[0] == 12

    table = [G10 if r % 2 == 0 else NAR for r in range(12)]
    u12 = np.random.default_rng(17).random((STEPS, 12), dtype=np.float32)

    def table_refusals(e):
        refused(e, "uniforms missing", cond=ncond, text_ids=ntext, rows=[WID] * 5)
        refused(e, "temperature > 0", cond=ncond, text_ids=ntext, rows=[(1, 30, 0.8, 0.0, 10.0)] * 5, uniforms=row_u(range(5)))
        refused(e, "mode is 0", cond=ncond, text_ids=ntext, rows=[(2, 30, 0.8, 1.0, 10.0)] * 5)

    ref = run(eng, conds[0], text, forced=f, table=table, u=u12)
    got = run(eng, conds[0], text, forced=f, table=table, u=u12, events=[(AT, "call", table_refusals)])
    assert np.array_equal(got["codes"], ref["codes"]) and bits_equal(got["logits"], ref["logits"])

    # a table of greedy rows that was not kept has no room for draws
    got = run(eng, conds[0], text, forced=f, table=[G10, G15] * 6,
              events=[(AT, "call", lambda e: refused(e, "no room for draws", cond=ncond, text_ids=ntext, rows=[NAR] * 5, uniforms=row_u(range(5))))])
    assert got["codes"].shape[0] == 12
    # forced tokens need a generation that was started with some
    run(eng, conds[0], text, events=[(AT, "call", lambda e: refused(e, "started with forced tokens", cond=ncond, text_ids=ntext, forced=free_forced(5)))])
    # after a retirement
    after = [(AT, "retire", None), (AT, "call", lambda e: refused(e, "after a retirement", cond=ncond, text_ids=ntext))]
    ref = run(eng, conds[0], text, forced=f, events=after[:1])
    got = run(eng, conds[0], text, forced=f, events=after)
    assert got["answered"] == [7] and np.array_equal(got["codes"], ref["codes"]) and bits_equal(got["logits"][LIVE12], ref["logits"][LIVE12])


def test_refusals_by_mode(eng, conds):
    """beams, typical filtering, host sampling, the fused launch's switch, the persistent engine: refused, and the generation goes
    on as if nothing had been asked."""
    ncond, ntext = new_requests(conds)
    fresh = ieng.build_engine(CFG3, "bf16", parts=("gpt",))
    refused(fresh, "no active generation", cond=conds[0], text_ids=ntext)

    def both(match, setup, teardown, rows=12, **kw):
        text = ragged(rows, 11)
        out = []
        for ev in ([], [(AT, "call", lambda e: refused(e, match, cond=ncond, text_ids=ntext))]):
            setup()
            try:
                out.append(run(eng, conds[0], text, events=ev, **kw))
            finally:
                teardown()
        assert np.array_equal(out[0]["codes"], out[1]["codes"]) and bits_equal(out[0]["logits"], out[1]["logits"]), match

    both("beams", lambda: eng.set_beam_sample(3, do_sample=False), lambda: eng.set_beam_sample(1), rows=4)
    both("typical", lambda: eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.9), "typical"), lambda: eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.0), "typical"))
    # (run() resets the debug bits itself, so these two switch theirs on inside the generation: the refusal reads them per call)
    text = ragged(12, 11)
    ref = run(eng, conds[0], text)

    def fused(e):
        e.debug(fuse=True)
        try:
            refused(e, "fused qkv", cond=ncond, text_ids=ntext)
        finally:
            e.debug()

    got = run(eng, conds[0], text, events=[(AT, "call", fused)])
    assert np.array_equal(got["codes"], ref["codes"]) and bits_equal(got["logits"], ref["logits"])

    # the persistent engine: 6 rows, two told to stop
    text6, f6 = ragged(6, 91), forced_stops(6, {1: 3, 4: 5})

    def on_engine(ev):
        eng.debug(engine=True)
        eng.set_forced(f6)
        try:
            eng.prefill(conds[0], text6, STEPS, 10.0, True)
            eng.decode(AT - 1)
            if ev:
                refused(eng, "persistent engine", cond=conds[0], text_ids=ragged(12, 211)[:2])
            eng.decode(STEPS - AT)
            res = eng.fetch(logits=True), eng.decode_mode()
            eng._exit()
        finally:
            eng.set_forced(None)
            eng.debug()
        return res

    a, b = on_engine(False), on_engine(True)
    assert a[1] == b[1] == 1 and np.array_equal(a[0][0], b[0][0]) and bits_equal(a[0][1], b[0][1])

    # host sampling: the prefill stops behind the head
    eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 1), "gpt_set_host_sampling")
    try:
        eng.prefill(conds[0], ragged(12, 81), STEPS, 10.0, True)
        before = eng.fetch(logits=True)
        refused(eng, "host sampling", cond=ncond, text_ids=ntext)
        after = eng.fetch(logits=True)
        eng._exit()
    finally:
        eng._ck(eng.lib.itts_gpt_set_host_sampling(eng.h, 0), "gpt_set_host_sampling")
    assert bits_equal(before[1], after[1])


# ---- Engine.generate(slots=..) -------------------------------------------------------------------------------------------------
def upto_stop(row):
    hit = np.nonzero(np.asarray(row) == STOP)[0]
    return np.asarray(row)[: int(hit[0]) + 1] if len(hit) else np.asarray(row)


def test_generate_with_slots(eng, conds):
    """27 requests through 12 slots, admit_min = 5 / 12, status every 4 tokens.  The stops make the log 12 / 5 / 5 / 5: five of the
    first rows end by token 5, five more by token 9, the first admitted group by token 13; everything else ends later.  Every
    group is replayed as a fresh generation of that group alone."""
    N, S, MG = 27, 12, 32
    lens = [41 - (i * 7) % 30 for i in range(N)]
    ids = np.full((N, TEXT_LEN), CFG.gpt.stop_text_token, np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = synth.text_ids(n, 300 + i, CFG.gpt.number_text_tokens)
    sched = infer_core.AdmitScheduler(lens, S, 5 / 12)
    first, waiting = sched.first, sched.waiting
    assert len(first) == 12 and min(lens[i] for i in first) >= max(lens[i] for i in waiting)
    groups = [first, waiting[0:5], waiting[5:10], waiting[10:15]]
    forced = np.full((N, 24), -1, np.int32)
    for j, r in enumerate(first):  # five by token 5, five by token 9, two at token 21
        forced[r, [1, 2, 3, 4, 4, 6, 7, 8, 8, 7, 20, 20][j]] = STOP
    for j, r in enumerate(groups[1]):  # admitted at 5 tokens with one of their own: they hold 5 at token 9 and 9 at token 13
        forced[r, [6, 7, 8, 8, 6][j]] = STOP
    for r in groups[2] + groups[3]:
        forced[r, 10] = STOP
    cond = torch.cat([conds[i % 2] for i in range(N)], 0)
    eng.set_forced(forced)  # one row per request: generate(slots=) hands every request its own
    try:
        codes, log = eng.generate(cond, ids, MG, suppress_stop=True, check_every=4, slots=S, admit_min=5 / 12, return_log=True)
        with pytest.raises(ValueError, match="wide_sampler='device'"):  # the scalar whole-vocabulary request takes the host path
            eng.generate(cond, ids, MG, suppress_stop=True, slots=S, do_sample=True, top_k=0, seed=1)
    finally:
        eng.set_forced(None)
    assert [(t, len(sl), req) for t, sl, req in log] == [(5, 5, groups[1]), (9, 5, groups[2]), (13, 5, groups[3])], log
    assert codes.shape[0] == N and eng.decode_mode() == 0
    for g in groups:  # every group, none left out
        fresh = run(eng, cond.view(N, -1, CFG.gpt.model_dim)[g].reshape(-1, CFG.gpt.model_dim), ids[g], forced=forced[g])
        for j, r in enumerate(g):
            want = upto_stop(fresh["codes"][j])
            assert want[-1] == STOP and np.array_equal(codes[r, :len(want)], want) and np.all(codes[r, len(want):] == STOP), (r, g)
    again = eng.generate(cond[:12], ids[:12], MG, suppress_stop=True, check_every=4, slots=S)  # no more rows than slots: today's path
    assert again.shape == (12, MG)


def test_generate_with_slots_leaves_no_sampling_state(eng, conds):
    """The twelve longest requests share ONE sampled entry and two short ones wait with a greedy entry: the table as a whole is not
    uniform, its first rows are - which is the scalar setting to the library (do_sample and the draws).  Nothing of it may outlive the
    call: a plain greedy generate, and a host-sampled one, on the same engine object equal those of an engine object that never
    admitted a row."""
    N, S, MG = 14, 12, 16
    lens = [41 - i for i in range(12)] + [9, 7]
    ids = np.full((N, TEXT_LEN), CFG.gpt.stop_text_token, np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = synth.text_ids(n, 500 + i, CFG.gpt.number_text_tokens)
    forced = np.full((N, 8), -1, np.int32)
    forced[:, 3] = STOP
    eng.set_forced(forced)
    try:
        codes, log = eng.generate(conds[0], ids, MG, check_every=4, slots=S, return_log=True, do_sample=[True] * 12 + [False] * 2,
                                  top_k=[30] * N, top_p=[0.8] * N, temperature=[0.9] * N, seed=list(range(N)))
    finally:
        eng.set_forced(None)
    assert [req for _, _, req in log] == [[12, 13]] and codes.shape == (N, 4) and np.all(codes[:, 3] == STOP)
    other = ieng.build_engine(CFG3, "bf16", parts=("gpt",))
    text = ragged(12, 11)
    for kw in (dict(), dict(do_sample=True, top_k=0, top_p=0.9, seed=5)):  # greedy; whole vocabulary on the host (the default)
        got = eng.generate(conds[0], text, 6, suppress_stop=True, **kw)
        want = other.generate(conds[0], text, 6, suppress_stop=True, **kw)
        assert got.shape == want.shape == (12, 6) and np.array_equal(got, want), kw


# ---- the drop-in on the micro checkpoint --------------------------------------------------------------------------------------
MICRO = icfg.micro()


def micro_tts(**kw):
    from indextts.infer import IndexTTS

    sds = {"gpt": synth.gpt_state_dict(MICRO, 1234), "bigvgan": synth.bigvgan_state_dict(MICRO, 1234), "dvae": synth.dvae_state_dict(MICRO, 1234)}
    return IndexTTS(cfg=MICRO, model_dir="/nonexistent", is_fp16=False, state_dicts=sds, **kw)


def test_infer_batch_dropin(monkeypatch):
    """max_batch reduced to 8, 13 sentences of 5 utterances and 2 voices.  Switch off (or overridden off): the int16 output of the
    mixed path as it is.  Switch on: one generation of 8 slots; every utterance returns, and the codes equal the replay of the
    log's groups as fresh generations."""
    monkeypatch.delenv("ITTS_MIXED_BATCH", raising=False)
    monkeypatch.delenv("ITTS_ADMIT_ROWS", raising=False)
    nt = MICRO.gpt.number_text_tokens
    mels = [torch.from_numpy(synth.prompt_mel(61, seed=s)) for s in (7, 8)]
    texts = [[synth.text_ids(n, 100 * u + k, nt).astype(np.int32) for k, n in enumerate(ns)]
             for u, ns in enumerate(((11, 7, 9), (9, 5), (5, 12, 8), (8, 10), (6, 11, 7)))]
    prompts = [mels[0], mels[1], mels[0], mels[1], mels[0]]
    per = [dict(do_sample=False), dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, seed=11), dict(do_sample=False),
           dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.7, repetition_penalty=2.0, seed=12), dict(do_sample=False)]

    def run_tts(t):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached
            return [w for _, w in t.infer_batch(prompts, texts, num_beams=1, max_mel_tokens=24, per_utterance=per)]

    off = micro_tts(mixed_batch=True)
    off.engine.ccfg.max_batch = 8
    want = run_tts(off)
    tts = micro_tts(mixed_batch=True, admit_rows=True)
    tts.engine.ccfg.max_batch = 8
    monkeypatch.setenv("ITTS_ADMIT_ROWS", "0")
    forced_off = run_tts(tts)
    monkeypatch.setenv("ITTS_ADMIT_ROWS", "1")
    env_on_calls = []
    real_off = off.engine._generate_admit
    monkeypatch.setattr(off.engine, "_generate_admit", lambda *a, **k: (env_on_calls.append(1), real_off(*a, **k))[1])
    run_tts(off)
    assert len(env_on_calls) == 1  # the environment switches an object on as well
    monkeypatch.delenv("ITTS_ADMIT_ROWS")
    for u in range(5):
        assert forced_off[u].dtype == np.int16 and np.array_equal(forced_off[u], want[u]), u

    seen = []
    real = tts.engine._generate_admit

    def spy(cond, text_ids, max_gen, table, scalar, uniforms, slots, *a, **k):
        res = real(cond, text_ids, max_gen, table, scalar, uniforms, slots, *a, **k)
        seen.append((cond, np.asarray(text_ids), max_gen, table, uniforms, slots, res))
        return res

    monkeypatch.setattr(tts.engine, "_generate_admit", spy)
    got = run_tts(tts)
    assert len(got) == 5 and all(g.dtype == np.int16 and g.size > 0 for g in got)
    assert len(seen) == 1
    cond, ids, mg, table, u, slots, (codes, log) = seen[0]
    assert slots == 8 and ids.shape[0] == 13 and codes.shape[0] == 13 and sum(len(req) for _, _, req in log) == 5
    lens = [int(np.count_nonzero((r != MICRO.gpt.stop_text_token) & (r != MICRO.gpt.start_text_token))) for r in ids]
    sched = infer_core.AdmitScheduler(lens, 8, 0.125)
    e = tts.engine
    cond = cond.view(13, -1, MICRO.gpt.model_dim)
    for g in [sched.first] + [req for _, _, req in log]:  # every group, none left out
        fresh = e.generate(cond[g], ids[g], mg, do_sample=[bool(table[r][0]) for r in g], top_k=[table[r][1] for r in g],
                           top_p=[table[r][2] for r in g], temperature=[table[r][3] for r in g],
                           repetition_penalty=[table[r][4] for r in g], uniforms=None if u is None else np.ascontiguousarray(u[:, g]),
                           wide_sampler="device")
        for j, r in enumerate(g):
            want_row = upto_stop(fresh[j])
            assert np.array_equal(codes[r, :len(want_row)], want_row), (r, g)
    # without mixed_batch the switch does nothing and says so once
    plain = micro_tts(admit_rows=True)
    with pytest.warns(RuntimeWarning, match="does nothing without mixed_batch"):
        plain.infer_batch(prompts[:1], texts[:1], num_beams=1, max_mel_tokens=24, do_sample=False)
