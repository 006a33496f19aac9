"""GPU: row admission under beams (Engine.set_admit_beams + Engine.admit_rows / itts_gpt_set_admit_beams, opt-in): finished batch
items of a running beam generation take new requests, num_beams rows each; the groups then run at different steps, and the caller
sees every original item.

The invariant is the one the retirement of beam groups rests on (tests/test_gpu_beam_retire.py): inside one projection-kernel
family (5 - 16 rows, 17+ rows) a row's bits depend neither on its slot nor on its companions.  So two things are held bit for bit:
  (a) the running items equal the same generation WITHOUT the admission: all num_return_sequences codes of every first item (a
      replaced item was done, so its result was final), and the last logits of the rows that were not replaced;
  (b) the admitted items equal a FRESH generation of the admitted requests alone - the same text length L, the same item count
      (so the prefill runs the same kernels), the same draws - fetched after the same number of their own tokens.
Conventions, sizes, checkpoints and draws are those of tests/test_gpu_beam_retire.py (CFG3, 32 steps, ragged texts, the smooth
synthetic checkpoint with a stop bias, the launch path forced); its docstring lists the CPU oracle's done steps for every
setting.  The admission point is taken from the reference run's own per-step trace, and every test asserts that it exists."""
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
from test_gpu_beam_retire import STEPS, STOP, build, family, first_done, uniforms  # noqa: E402
from test_gpu_engine_fp8 import CFG3  # noqa: E402
from test_gpu_row_retire import ragged  # noqa: E402

V = CFG3.gpt.number_mel_codes


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run(eng, cond, text, nb, u, events=(), tokens=STEPS, trace=False, **beam_kw):
    """prefill + decode, one step per call, until the FIRST items hold `tokens` tokens (max_gen = STEPS), with events
    (at_tokens, kind, payload): ("admit", dict(cond=, text_ids=, uniforms=)), ("retire", None), ("call", fn(eng)).
    Always on the launch path.  -> dict(codes [items_total * returns, STEPS], logits [rows_total, V], slots per admission,
    recaptured per admission, retire answers, status, done {tokens: per-slot done flags} (trace only))"""
    items = text.shape[0]
    eng.debug(no_engine=True)
    eng.set_beam_sample(nb, uniforms=u, **beam_kw)
    out = dict(slots=[], recaptured=[], answered=[], done={})
    try:
        eng.prefill(cond, text, STEPS, 10.0, False)
        assert eng.rows() == items * nb
        done, pending = 1, None
        ev = sorted(events, key=lambda e: e[0])
        while True:
            if trace:
                orig, ln, unf = eng.row_status()
                out["done"][done] = [not unf[i * nb] for i in range(len(unf) // nb)]
            for at, kind, payload in [e for e in ev if e[0] == done]:
                if kind == "admit":
                    pending = eng.lib.itts_gpt_graph_captures(eng.h)
                    out["slots"].append(eng.admit_rows(**payload).tolist())
                elif kind == "retire":
                    out["answered"].append(eng.retire_rows())
                else:
                    payload(eng)
            if done == tokens:
                break
            eng.decode(1)
            done += 1
            if pending is not None:
                out["recaptured"].append(eng.lib.itts_gpt_graph_captures(eng.h) - pending)
                pending = None
        out["status"] = eng.row_status()
        out["codes"], out["logits"] = eng.fetch(logits=True)
        out["mode"], out["rows"] = eng.decode_mode(), eng.rows()
        eng._exit()
    finally:
        eng.set_beam_sample(1)
        eng.debug()
    return out


def admit_point(done, items, n, parity=None, lo=2, hi=STEPS - 6):
    """The first token count in [lo, hi] (of the wanted parity) at which at least n groups of the reference trace are done."""
    for t in range(lo, hi + 1):
        if sum(done[t]) >= n and (parity is None or t % 2 == parity):
            return t
    return None


def new_requests(n, seed, nb, conds=None):
    """n ragged requests of the running generation's text length with their own draws; conds: one conditioning block per item"""
    text = ragged(12, seed)[[2, 7, 0, 9, 4, 11, 6, 3][:n]]
    u = np.random.default_rng(seed + 77).random((n, STEPS, 2 * nb), dtype=np.float32)  # [n][max_gen][2 nb]: the admission's layout
    cond = None if conds is None else torch.cat([conds[(i + 1) % 2] for i in range(n)], 0)
    return text, u, cond


def admit_case(eng, cond, items, nb, seed, n, parity=None, what="", conds=None, **kw):
    """Cases (a) and (b) for one admission of n items into items x nb rows.  conds: two voices, the admitted items alternate."""
    keep = kw.get("num_return_sequences", 1)
    sample = kw.get("do_sample", True)
    text, u = ragged(items, seed), uniforms(items, nb, seed)
    ntext, nu, ncond = new_requests(n, seed + 200, nb, conds)
    ncond = cond if ncond is None else ncond
    ref = run(eng, cond, text, nb, u, trace=True, **kw)
    t = admit_point(ref["done"], items, n, parity)
    print(f"{what or 'beam admit'} {items} x {nb}: done steps {first_done(ref['done'], items)}, {n} items admitted at {t} tokens")
    # precondition of the yardstick, not a property of the code under test: n groups are done early enough
    assert t is not None, f"no admission point: done steps {first_done(ref['done'], items)}"
    free = [i for i in range(items) if ref["done"][t][i]][:n]
    new_tokens = STEPS - t + 1
    got = run(eng, cond, text, nb, u, events=[(t, "admit", dict(cond=ncond, text_ids=ntext, uniforms=nu if sample else None))], **kw)
    fresh = run(eng, ncond, ntext, nb, np.ascontiguousarray(nu.transpose(1, 0, 2)), tokens=new_tokens, **kw)
    assert ref["mode"] == got["mode"] == fresh["mode"] == 0
    assert family(n * nb) == family(items * nb), "the yardstick: the fresh generation runs in the running generation's family"
    assert got["slots"] == [free] and got["recaptured"] == [0]  # item slots; the captured step is replayed, not captured again
    assert got["codes"].shape == ((items + n) * keep, STEPS) and got["logits"].shape == ((items + n) * nb, V)
    orig, ln, unf = got["status"]
    want_orig = list(range(items * nb))
    for i, g in enumerate(free):
        want_orig[g * nb:(g + 1) * nb] = range((items + i) * nb, (items + i + 1) * nb)
    assert orig.tolist() == want_orig
    assert ln.tolist() == [new_tokens if r // nb in free else STEPS for r in range(items * nb)]
    # (a)
    a, b = got["codes"][:items * keep], ref["codes"]
    bad = sorted(set((np.nonzero(a != b)[0] // keep).tolist()))
    assert not bad, f"{what}: codes of the first items differ in items {bad} (replaced: {free})"
    live = [g * nb + q for g in range(items) if g not in free for q in range(nb)]
    assert bits_equal(got["logits"][live], ref["logits"][live]), f"{what}: last logits of the running rows differ"
    # (b)
    a, b = got["codes"][items * keep:], fresh["codes"]
    bad = sorted(set((np.nonzero(a != b)[0] // keep).tolist()))
    assert not bad, f"{what}: codes of the admitted items differ from the fresh generation's in items {bad}"
    assert bits_equal(got["logits"][items * nb:], fresh["logits"]), f"{what}: last logits of the admitted rows differ"
    assert not np.array_equal(fresh["codes"][0], fresh["codes"][keep])  # the yardstick: two different requests
    return ref, got, fresh, t


@pytest.fixture(scope="module")
def eng():
    e = build()
    e.set_admit_beams(True)
    return e


@pytest.fixture(scope="module")
def conds(eng):
    return [eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=s))) for s in (7, 8)]


@pytest.mark.parametrize("parity", [0, 1])
def test_beam_sample_5x3(eng, conds, parity):
    """15 rows, 2 items admitted: 6 fresh rows, the 5 - 16 family on both sides.  Admission at an even and at an odd token count of
    the running groups: their live ancestry / id half is half 0 or half 1 while the admitted groups start in half 0."""
    ref, got, fresh, t = admit_case(eng, conds[0], 5, 3, 11, 2, parity=parity, what=f"beam_sample, parity {parity}")
    assert t % 2 == parity


def test_beam_sample_8x3(eng, conds):
    """24 rows, 6 items admitted: 18 fresh rows, the 17+ family on both sides."""
    admit_case(eng, conds[0], 8, 3, 21, 6, what="beam_sample 17+")


def test_beam_search(conds):
    """beam_search: the admitted groups start from the running scores [0, -1e9, -1e9]; no draws."""
    e = build(2.5)
    e.set_admit_beams(True)
    admit_case(e, conds[0], 5, 3, 11, 2, do_sample=False, what="beam_search")


def test_two_beams(eng, conds):
    admit_case(eng, conds[0], 8, 2, 11, 3, what="nb = 2")


def test_three_returns_with_length_penalty(eng, conds):
    """length_penalty = 1: the finalisation divides an open beam's score by the ITEM's own token count."""
    admit_case(eng, conds[0], 5, 3, 11, 2, num_return_sequences=3, length_penalty=1.0, what="3 returns, length_penalty 1")


def test_kv_fp8_cache(eng, conds):
    eng.set_kv_fp8(True)
    try:
        admit_case(eng, conds[0], 5, 3, 11, 2, what="fp8 K/V cache")
    finally:
        eng.set_kv_fp8(False)


def test_fp8_weights(conds):
    e = build(gpt_fp8="fp8")
    e.set_admit_beams(True)
    admit_case(e, conds[0], 5, 3, 11, 2, what="fp8 weights")


def test_f16_library():
    if not os.path.exists(L.LIB_PATH_F16):
        pytest.fail("libitts_hip_f16.so was not built")
    e = build(dtype="f16")
    e.set_admit_beams(True)
    admit_case(e, e.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7))), 5, 3, 11, 2, what="f16 library")


def test_fp32_engine(conds):
    e = build(dtype="fp32")
    e.set_admit_beams(True)
    admit_case(e, conds[0], 5, 3, 11, 2, what="fp32 engine")


def test_device_wide_beam_sampler(conds):
    """top_k = 0 on the device: the first token of an admitted group comes from beam_wide_cand_kernel + beam_wide_pick_kernel on a
    grid of one item, in front of beam_select_kernel.  (stop_bias 6: see tests/test_gpu_beam_retire.py.)"""
    e = build(6.0)
    e.set_admit_beams(True)
    admit_case(e, conds[0], 5, 3, 11, 2, top_k=0, what="top_k 0, device")


def test_two_voices(eng, conds):
    """Per-item conditioning: the admitted items carry one conditioning block each, of two voices."""
    ref, got, fresh, t = admit_case(eng, conds[0], 5, 3, 11, 2, conds=conds, what="two voices")
    ntext, nu, _ = new_requests(2, 211, 3)
    one = run(eng, conds[0], ntext, 3, np.ascontiguousarray(nu.transpose(1, 0, 2)), tokens=STEPS - t + 1)
    assert not np.array_equal(one["codes"], fresh["codes"])  # the yardstick: the voice matters


def test_one_item_slot_twice(eng, conds):
    """Item slot 0 holds a first item, then an admitted request that is done at least 4 tokens before the end, then another
    admitted request.  fetch returns every original item once: 5 + 2 + 2."""
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    ref = run(eng, conds[0], text, nb, u, trace=True)
    t1 = admit_point(ref["done"], items, 2)
    assert t1 is not None, first_done(ref["done"], items)
    # the first admitted pair: the requests of the two first items that were done first - as admitted items they are done early too
    early = sorted(range(items), key=lambda i: first_done(ref["done"], items)[i] or 99)[:2]
    atext, au = text[early], np.ascontiguousarray(u[:, early].transpose(1, 0, 2))
    btext, bu, _ = new_requests(2, 411, nb)
    ev1 = [(t1, "admit", dict(cond=conds[0], text_ids=atext, uniforms=au))]
    mid = run(eng, conds[0], text, nb, u, events=ev1, trace=True)
    s0 = mid["slots"][0][0]
    t2 = next((t for t in range(t1 + 2, STEPS - 3) if mid["done"][t][s0] and sum(mid["done"][t]) >= 2 and not any(mid["done"][t][:s0])), None)
    print(f"one slot twice: first admission at {t1} into {mid['slots'][0]}, slot {s0} done again and a second slot free at {t2}")
    # precondition of the yardstick: an admitted group is done at least 4 tokens before the end
    assert t2 is not None and t2 <= STEPS - 4, [(t, mid["done"][t]) for t in sorted(mid["done"])]
    got = run(eng, conds[0], text, nb, u, events=ev1 + [(t2, "admit", dict(cond=conds[0], text_ids=btext, uniforms=bu))])
    assert got["slots"][0] == mid["slots"][0] and got["slots"][1][0] == s0 and got["codes"].shape == (9, STEPS)
    assert got["status"][0].tolist()[s0 * nb:(s0 + 1) * nb] == [21, 22, 23]
    assert np.array_equal(got["codes"][:5], ref["codes"])
    never = [g * nb + q for g in range(items) if g not in got["slots"][0] + got["slots"][1] for q in range(nb)]
    assert never and bits_equal(got["logits"][never], ref["logits"][never])  # the rows that were never replaced
    fa = run(eng, conds[0], atext, nb, np.ascontiguousarray(au.transpose(1, 0, 2)), tokens=STEPS - t1 + 1)
    fb = run(eng, conds[0], btext, nb, np.ascontiguousarray(bu.transpose(1, 0, 2)), tokens=STEPS - t2 + 1)
    assert np.array_equal(got["codes"][5:7], fa["codes"]) and np.array_equal(got["codes"][7:9], fb["codes"])
    assert bits_equal(got["logits"][21:27], fb["logits"])
    assert fa["codes"][0, -1] == STOP  # the yardstick: the replaced admitted item had ended


@pytest.mark.parametrize("parity", [0, 1])
def test_admission_then_retirement(eng, conds, parity):
    """2 items admitted, then the done groups retire (set_retire_beams): the groups differ in step and - admitted at an even token
    count - in the parity of their live half, so both halves of beam ids and ancestry move.  The surviving row count stays in the
    family; codes and the live rows' logits equal the same run without the retirement."""
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    ntext, nu, _ = new_requests(2, 211, nb)
    ref = run(eng, conds[0], text, nb, u, trace=True)
    t = admit_point(ref["done"], items, 3, parity)  # three done: two slots are refilled, one group stays done and can retire
    assert t is not None, first_done(ref["done"], items)
    ev = [(t, "admit", dict(cond=conds[0], text_ids=ntext, uniforms=nu))]
    noret = run(eng, conds[0], text, nb, u, events=ev, trace=True)
    tr = next((x for x in range(t + 1, STEPS - 2) if 0 < sum(noret["done"][x]) <= 2), None)
    assert tr is not None, [(x, noret["done"][x]) for x in sorted(noret["done"])]
    want_rows = (items - sum(noret["done"][tr])) * nb
    assert want_rows > 6 and family(want_rows) == family(items * nb)
    eng.set_retire_beams(True)
    try:
        got = run(eng, conds[0], text, nb, u, events=ev + [(tr, "retire", None)])
    finally:
        eng.set_retire_beams(False)
    print(f"admission at {t}, retirement at {tr} (running groups hold {tr} tokens, admitted groups {tr - t + 1}): {items * nb} -> {want_rows} rows")
    assert got["answered"] == [want_rows] and got["rows"] == want_rows and noret["rows"] == items * nb
    assert got["codes"].shape == noret["codes"].shape == (7, STEPS) and np.array_equal(got["codes"], noret["codes"])
    live = [int(r) for r in got["status"][0]]  # the original rows of the surviving slots
    assert len(live) == want_rows and bits_equal(got["logits"][live], noret["logits"][live])
    assert got["mode"] == 0


def upto_stop(row):
    hit = np.nonzero(np.asarray(row) == STOP)[0]
    return np.asarray(row)[: int(hit[0]) + 1] if len(hit) else np.asarray(row)


def test_generate_with_item_slots(eng, conds, monkeypatch):
    """12 requests of two voices through 5 item slots (15 rows), status every 4 tokens, admit_min 0.4 (2 items).  Every group of
    the returned log - and the first one - is replayed as a fresh generation of that group alone (a group of one item together
    with a copy of itself: 3 rows would run in another kernel family)."""
    monkeypatch.delenv("ITTS_ADMIT_BEAMS", raising=False)
    N, S, nb = 12, 5, 3
    text = ragged(N, 31)
    u = np.random.default_rng(5).random((STEPS, N, 2 * nb), dtype=np.float32)
    cond = torch.cat([conds[i % 2] for i in range(N)], 0)
    kw = dict(num_beams=nb, do_sample=True, check_every=4)
    eng.debug(no_engine=True)
    try:
        with pytest.raises(ValueError, match="one beam"):
            eng.generate(cond, text, STEPS, uniforms=u, slots=S, **kw)
        codes, log = eng.generate(cond, text, STEPS, uniforms=u, slots=S, admit_min=0.4, admit_beams=True, return_log=True, **kw)
        assert codes.shape[0] == N and sum(len(req) for _, _, req in log) == N - S and eng.decode_mode() == 0
        assert all(len(sl) == len(req) and all(0 <= s < S for s in sl) for _, sl, req in log)
        lens = [int(np.count_nonzero((r != CFG3.gpt.start_text_token) & (r != CFG3.gpt.stop_text_token))) for r in text]
        sched = infer_core.AdmitScheduler(lens, S, 0.4)
        print(f"generate(slots=5, num_beams=3, admit_beams=True): admissions {[(t, sl, req) for t, sl, req in log]}")
        for g in [sched.first] + [req for _, _, req in log]:  # every group, none left out
            gg = list(g) * 2 if len(g) == 1 else list(g)
            fresh = eng.generate(cond.view(N, -1, CFG3.gpt.model_dim)[gg].reshape(-1, CFG3.gpt.model_dim), text[gg], STEPS,
                                 uniforms=np.ascontiguousarray(u[:, gg]), **kw)
            for j, r in enumerate(g):
                want = upto_stop(fresh[j])
                assert np.array_equal(codes[r, :len(want)], want) and np.all(codes[r, len(want):] == STOP), (r, g)
        three = eng.generate(cond, text, STEPS, uniforms=u, slots=S, admit_min=0.4, admit_beams=True, num_return_sequences=3, **kw)
        w = min(codes.shape[1], three.shape[1])
        assert three.shape[0] == 3 * N and np.array_equal(three[::3, :w], codes[:, :w])  # the best of three is the one
    finally:
        eng.debug()
    assert getattr(eng, "_admit_beams", None) is True  # the caller's setting is back


def test_switch_off_refuses_and_the_environment_overrides(conds, monkeypatch):
    """On an engine object that has seen the switch on and off: admit_rows under beams is refused with the old message and the
    generation goes on bit for bit.  ITTS_ADMIT_BEAMS overrides the setter in both directions."""
    monkeypatch.delenv("ITTS_ADMIT_BEAMS", raising=False)
    e = build()
    e.set_admit_beams(True)
    e.set_admit_beams(False)
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    ntext, nu, _ = new_requests(2, 211, nb)
    ref = run(e, conds[0], text, nb, u, trace=True)
    t = admit_point(ref["done"], items, 2)
    assert t is not None
    pay = dict(cond=conds[0], text_ids=ntext, uniforms=nu)

    def refused(en):
        with pytest.raises(RuntimeError, match="rows cannot be admitted under beams"):
            en.admit_rows(**pay)

    off = run(e, conds[0], text, nb, u, events=[(t, "call", refused)])
    assert np.array_equal(off["codes"], ref["codes"]) and bits_equal(off["logits"], ref["logits"])
    e.set_admit_beams(True)
    on = run(e, conds[0], text, nb, u, events=[(t, "admit", pay)])
    assert on["codes"].shape[0] == items + 2 and on["recaptured"] == [0]
    monkeypatch.setenv("ITTS_ADMIT_BEAMS", "0")
    off = run(e, conds[0], text, nb, u, events=[(t, "call", refused)])
    assert np.array_equal(off["codes"], ref["codes"]) and bits_equal(off["logits"], ref["logits"])
    e.set_admit_beams(False)
    monkeypatch.setenv("ITTS_ADMIT_BEAMS", "1")
    env_on = run(e, conds[0], text, nb, u, events=[(t, "admit", pay)])
    assert np.array_equal(env_on["codes"], on["codes"]) and bits_equal(env_on["logits"], on["logits"])
    monkeypatch.delenv("ITTS_ADMIT_BEAMS")
    run(e, conds[0], text, nb, u, events=[(t, "call", refused)])


def test_refusals_leave_the_generation_running(eng, conds):
    items, nb = 5, 3
    text, u = ragged(items, 11), uniforms(items, nb, 11)
    ntext, nu, _ = new_requests(2, 211, nb)
    ref = run(eng, conds[0], text, nb, u, trace=True)
    t = admit_point(ref["done"], items, 2)
    assert t is not None and sum(ref["done"][t]) < items

    def refusals(e):
        def no(match, **kw):
            with pytest.raises(RuntimeError, match=match):
                e.admit_rows(**dict(dict(cond=conds[0], text_ids=ntext, uniforms=nu), **kw))

        five, fu, _ = new_requests(5, 311, nb)
        no("fewer finished items", text_ids=five, uniforms=fu)
        no("uniforms missing", uniforms=None)
        no("rows_host and forced_host must be null", rows=[(0, 0, 1.0, 1.0, 10.0)] * 2)
        no("rows_host and forced_host must be null", forced=np.full((2, 4), -1, np.int32))
        no("more than 128 rows", text_ids=np.repeat(ntext, 22, 0)[:43], uniforms=np.repeat(nu, 22, 0)[:43])
        no("text length of the running generation", text_ids=np.concatenate([ntext, ntext[:, :1]], 1))
        bad = ntext.copy()
        bad[0, 0] = CFG3.gpt.number_text_tokens + 5
        no("text id out of range", text_ids=bad)

    got = run(eng, conds[0], text, nb, u, events=[(t, "call", refusals)])
    assert np.array_equal(got["codes"], ref["codes"]) and bits_equal(got["logits"], ref["logits"]) and got["codes"].shape[0] == items

    # after a retirement
    eng.set_retire_beams(True)
    try:
        def after(e):
            with pytest.raises(RuntimeError, match="after a retirement"):
                e.admit_rows(cond=conds[0], text_ids=ntext[:1], uniforms=nu[:1])

        got = run(eng, conds[0], text, nb, u, events=[(t, "retire", None), (t, "call", after)])
        assert got["answered"] and got["answered"][0] < items * nb and got["codes"].shape[0] == items
    finally:
        eng.set_retire_beams(False)

    # typical filtering
    eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.9), "gpt_set_typical")
    try:
        def typical(e):
            with pytest.raises(RuntimeError, match="typical filtering"):
                e.admit_rows(cond=conds[0], text_ids=ntext, uniforms=nu)

        run(eng, conds[0], text, nb, u, events=[(8, "call", typical)])
    finally:
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.0), "gpt_set_typical")

    # `input_tokens`
    eng.set_input_tokens(np.asarray([[5, 9]], np.int32))
    try:
        def given(e):
            with pytest.raises(RuntimeError, match="input_tokens"):
                e.admit_rows(cond=conds[0], text_ids=ntext, uniforms=nu)

        run(eng, conds[0], text, nb, u, events=[(8, "call", given)])
    finally:
        eng.set_input_tokens(None)


# ---- the drop-in on the micro checkpoint --------------------------------------------------------------------------------------
MICRO = icfg.micro()


def micro_tts(**kw):
    from indextts.infer import IndexTTS

    sds = {"gpt": synth.gpt_state_dict(MICRO, 1234), "bigvgan": synth.bigvgan_state_dict(MICRO, 1234), "dvae": synth.dvae_state_dict(MICRO, 1234)}
    return IndexTTS(cfg=MICRO, model_dir="/nonexistent", is_fp16=False, state_dicts=sds, **kw)


def test_infer_batch_dropin(monkeypatch):
    """IndexTTS.infer_batch with the default kwargs (num_beams=3, do_sample=True) on the micro checkpoint, max_batch reduced to 9
    (3 item slots), 11 sentences of 5 utterances.  admit_beams off: the waveforms and the generate calls of an object built without
    it.  On: ONE generate call for the group; the codes of every sentence equal the replay of its log group as a fresh generation
    (an utterance's latent pass and vocoder read nothing but its own sentences' codes), and every utterance returns."""
    for name in ("ITTS_MIXED_BATCH", "ITTS_ADMIT_ROWS", "ITTS_ADMIT_BEAMS", "ITTS_RETIRE_ROWS", "ITTS_RETIRE_BEAMS"):
        monkeypatch.delenv(name, raising=False)
    nt = MICRO.gpt.number_text_tokens
    mel = torch.from_numpy(synth.prompt_mel(61, seed=7))
    texts = [[synth.text_ids(n, 100 * u + k, nt).astype(np.int32) for k, n in enumerate(ns)]
             for u, ns in enumerate(((11, 7, 9), (9, 5), (5, 12), (8, 10), (6, 11)))]
    prompts = [mel] * 5

    def run_tts(t, calls):
        real = t.engine.generate
        monkeypatch.setattr(t.engine, "generate", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached
            torch.manual_seed(6)
            return [w for _, w in t.infer_batch(prompts, texts, max_mel_tokens=24)]

    plain = micro_tts(mixed_batch=True, admit_rows=True)
    plain.engine.ccfg.max_batch = 9
    calls_plain, calls_off, calls_on = [], [], []
    want = run_tts(plain, calls_plain)
    tts = micro_tts(mixed_batch=True, admit_rows=True, admit_beams=True)
    tts.engine.ccfg.max_batch = 9
    monkeypatch.setenv("ITTS_ADMIT_BEAMS", "0")
    off = run_tts(tts, calls_off)
    monkeypatch.delenv("ITTS_ADMIT_BEAMS")
    assert len(calls_off) == len(calls_plain) == 4 and not any("slots" in k for k in calls_off)  # 11 sentences, 3 at a time
    for a, b in zip(off, want):
        assert a.dtype == np.int16 and np.array_equal(a, b)

    seen = []
    real = tts.engine._generate_admit_beams

    def spy(cond, text_ids, max_gen, slots, *a, **k):
        res = real(cond, text_ids, max_gen, slots, *a, **k)
        seen.append((cond, np.asarray(text_ids), max_gen, slots, a, res))
        return res

    monkeypatch.setattr(tts.engine, "_generate_admit_beams", spy)
    got = run_tts(tts, calls_on)
    assert len(calls_on) == 1 and calls_on[0].get("slots") == 3 and calls_on[0].get("admit_beams") is True and len(seen) == 1
    assert len(got) == 5 and all(g.dtype == np.int16 and g.size > 0 for g in got)
    cond, ids, mg, slots, rest, (codes, log) = seen[0]
    # rest: admit_min, suppress_stop, check_every, retire_rows, retire_beams, do_sample, top_k, top_p, temperature, uniforms,
    # num_beams, length_penalty, num_return_sequences, repetition_penalty
    u = rest[9]  # the draws by request
    assert slots == 3 and ids.shape[0] == 11 and codes.shape[0] == 11 and sum(len(req) for _, _, req in log) == 8
    lens = [int(np.count_nonzero((r != MICRO.gpt.stop_text_token) & (r != MICRO.gpt.start_text_token))) for r in ids]
    sched = infer_core.AdmitScheduler(lens, 3, 0.125)
    e = tts.engine
    stop = MICRO.gpt.stop_mel_token
    e.debug(no_engine=True)  # a replayed group has at most 9 rows; the admitting generation ran 9 rows on the launch path
    try:
        for g in [sched.first] + [req for _, _, req in log]:
            gg = (list(g) * 3)[:3] if len(g) < 3 else list(g)  # the family of the 9-row generation: at least 7 rows
            fresh = e.generate(cond, ids[gg], mg, num_beams=3, do_sample=True, top_k=rest[6], top_p=rest[7], temperature=rest[8],
                               uniforms=np.ascontiguousarray(u[:, gg]), length_penalty=rest[11], repetition_penalty=rest[13])
            for j, r in enumerate(g):
                hit = np.nonzero(fresh[j] == stop)[0]
                w = fresh[j][: int(hit[0]) + 1] if len(hit) else fresh[j]
                assert np.array_equal(codes[r, :len(w)], w), (r, g)
    finally:
        e.debug()
