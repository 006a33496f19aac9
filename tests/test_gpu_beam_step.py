"""GPU: beam_cand_kernel + beam_select_kernel (csrc/beam.hip) one call at a time through itts_beam_step, on caller-owned state, against
token_choice_ref.py: the BeamSearchScorer of oracle/hf_beam.py for the bookkeeping, wide_beam_ref.Row (with the narrow kernels' cap of
128 candidates) for the warped rows, fp64 throughout.  Every array lies between guard blocks and starts out full of sentinels; after
every call the WHOLE state is compared with the reference's, so a write anywhere it does not belong - the source ping-pong plane, ids
behind k + 1, another item's rows, an old hypothesis - fails the comparison."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_choice_ref as T  # noqa: E402
import wide_beam_ref as W  # noqa: E402

from itts_hip import lib, prng  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
STATE = ("len", "cur_tok", "unfinished", "ids", "anc", "beam_scores", "hyp_tok", "hyp_score", "hyp_len", "hyp_order", "hyp_n", "hyp_worst",
         "hyp_counter", "done", "h_next")
WORST = {}  # largest deviation / bound seen, by group: printed for profiles/token_choice_ops.txt


def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16).float().numpy()


def tables(cfg, seed):
    """emb [V, D], pos [pos_rows, D]: fp32 values, bf16-representable when the tables are bf16."""
    if not cfg.get("D"):
        return
    emb = prng.uniform(f"beam_step.emb.{seed}", cfg["V"], cfg["V"] * cfg["D"]).reshape(cfg["V"], cfg["D"])
    pos = prng.uniform(f"beam_step.pos.{seed}", cfg["V"], cfg["pos_rows"] * cfg["D"]).reshape(cfg["pos_rows"], cfg["D"])
    if cfg.get("emb_bf16"):
        emb, pos = bf16_round(emb), bf16_round(pos)
    cfg["emb"], cfg["pos"] = emb, pos


def run_step(st, cfg, mode, picks=None, logits=None, uniforms=None, expect=0):
    """One itts_beam_step call on a copy of the state -> (state after, candidate scratch or None)."""
    l = lib.load()
    items, nb = cfg["items"], cfg["nb"]
    rows = items * nb
    d = T.DevArrays(DEV)
    a = lib.BeamStepArgs()
    for name in STATE:
        setattr(a, name, d.put(name, st[name]))
    if not cfg.get("D"):
        a.h_next = None
    a.prefix = d.put("prefix", np.array([cfg.get("prefix0", 0)], np.int32))
    for k in ("items", "nb", "V", "max_gen", "Smax", "stop"):
        setattr(a, k, cfg[k])
    a.mode, a.start_tok, a.fake_id = mode, cfg.get("start", 0), cfg.get("fake", 1)
    a.suppress_stop, a.preprocessed, a.do_sample = cfg.get("suppress", 0), cfg.get("pre", 0), cfg.get("do_sample", 1)
    a.top_k, a.top_p, a.temperature = cfg.get("top_k", 30), cfg.get("top_p", 0.8), cfg.get("temperature", 1.0)
    a.penalty, a.length_penalty, a.input_n = cfg.get("penalty", 10.0), cfg.get("length_penalty", 0.0), cfg.get("input_n", 0)
    if cfg.get("forced") is not None:
        a.forced = d.put("forced", cfg["forced"].astype(np.int32))
    if cfg.get("D"):
        a.D, a.pos_rows, a.emb_bf16 = cfg["D"], cfg["pos_rows"], int(bool(cfg.get("emb_bf16")))
        for name in ("emb", "pos"):
            t = torch.from_numpy(cfg[name])
            raw = t.to(torch.bfloat16).view(torch.int16).numpy() if cfg.get("emb_bf16") else cfg[name]
            setattr(a, name, d.put(name, raw))
    if mode == 0:
        a.logits = d.put("logits", logits)
        a.cand_sc = d.put("cand_sc", np.full((rows, T.CAND), T.SENT_F, F32))
        a.cand_tok = d.put("cand_tok", np.full((rows, T.CAND), T.SENT_I, np.int32))
        a.cand_n = d.put("cand_n", np.full(rows, T.SENT_I, np.int32))
        if uniforms is not None:
            a.uniforms = d.put("uniforms", np.ascontiguousarray(uniforms, F32))
    else:
        psc, ptok, pbeam = picks
        a.pick_score, a.pick_tok, a.pick_beam = (d.put("psc", np.ascontiguousarray(psc, F32)), d.put("ptok", np.ascontiguousarray(ptok, np.int32)),
                                                d.put("pbeam", np.ascontiguousarray(pbeam, np.int32)))
    torch.cuda.synchronize()
    status = l.itts_beam_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == expect, (status, l.itts_last_error())
    got = {name: d.get(name) for name in STATE}
    for name in d.t:  # every input the kernels only read is what it was
        if name not in STATE and not name.startswith("cand_"):
            d.get(name)
    if mode == 0:
        assert T.same_bits(d.get("logits"), logits)
        return got, (d.get("cand_sc"), d.get("cand_tok"), d.get("cand_n"))
    return got, None


def compare(got, want, before, scorer, cfg, k, score_tol=None, hyp_ulps=0, group="scripted"):
    """The whole state against the reference's.  score_tol None: scores compare exactly."""
    items, nb = cfg["items"], cfg["nb"]
    for name in ("len", "cur_tok", "unfinished", "ids", "anc", "done", "hyp_n", "hyp_counter"):
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:6])
    if cfg.get("D"):
        assert T.same_bits(got["h_next"], want["h_next"]), np.argwhere(got["h_next"] != want["h_next"])[:6]
    else:
        assert T.same_bits(got["h_next"], before["h_next"])
    if score_tol is None:
        assert T.same_bits(got["beam_scores"], want["beam_scores"]), (got["beam_scores"], want["beam_scores"])
    else:
        dev = np.abs(got["beam_scores"].astype(np.float64) - want["beam_scores"].astype(np.float64))
        fin = np.isfinite(want["beam_scores"])
        assert np.array_equal(np.isfinite(got["beam_scores"]), fin) and (dev[fin] <= score_tol).all(), (dev, score_tol)
        WORST[group] = max(WORST.get(group, 0.0), float((dev[fin] / score_tol).max()) if fin.any() else 0.0)
    for b in range(items):
        tol_w = hyp_ulps * T.ulp32(want["hyp_worst"][b]) + (score_tol or 0.0)
        assert abs(float(got["hyp_worst"][b]) - float(want["hyp_worst"][b])) <= tol_w, (b, got["hyp_worst"][b], want["hyp_worst"][b])
        dev_h, ref_h = T.hyps_of(got, b), scorer.hyps[b].beams
        assert len(dev_h) == len(ref_h), (b, len(dev_h), len(ref_h))
        for (ds, dt, dl), (rs, rt) in zip(dev_h, ref_h):  # insertion order on both sides
            assert dl == len(rt) and np.array_equal(dt, rt), (b, dt, rt)
            tol_s = hyp_ulps * T.ulp32(rs) + (score_tol or 0.0)
            assert abs(float(ds) - float(rs)) <= tol_s, (b, float(ds), float(rs), tol_s)
            if hyp_ulps and rs != 0:
                WORST["hyp_score_ulps"] = max(WORST.get("hyp_score_ulps", 0.0), abs(float(ds) - float(rs)) / T.ulp32(rs))
        # memory of the hypotheses: nothing behind k in any slot, nothing at all in a slot that was live before and still is
        assert np.array_equal(got["hyp_tok"][b][:, k:], before["hyp_tok"][b][:, k:])
        for q in range(nb + 1):
            if before["hyp_order"][b, q] >= 0 and got["hyp_order"][b, q] == before["hyp_order"][b, q]:
                assert np.array_equal(got["hyp_tok"][b, q], before["hyp_tok"][b, q])
                assert T.same_bits(got["hyp_score"][b, q], before["hyp_score"][b, q]) and got["hyp_len"][b, q] == before["hyp_len"][b, q]
        free = got["hyp_order"][b] < 0
        assert ((got["hyp_order"][b][free] == -1)).all()


class Generation:
    """State + reference scorer walking through calls in mode 1 (the test's picks)."""

    def __init__(self, cfg, k=0, hist=None, anc=None, beam_scores=None):
        self.cfg = cfg
        self.st = T.new_state(cfg["items"], cfg["nb"], cfg["max_gen"], cfg["Smax"], k, cfg.get("D", 0), beam_scores, hist, anc)
        self.scorer = T.new_scorer(cfg["items"], cfg["nb"], cfg.get("length_penalty", 0.0))

    def step(self, picks, hyp_ulps=0):
        k = int(self.st["len"][0])
        want = T.ref_step(self.st, self.cfg, picks, self.scorer)
        got, _ = run_step(self.st, self.cfg, 1, picks)
        compare(got, want, self.st, self.scorer, self.cfg, k, None, hyp_ulps)
        self.st = got
        return got


def as_picks(per_item):
    """[[(score, tok, beam)] * 2 nb] per item -> the three arrays."""
    sc = np.array([[p[0] for p in it] for it in per_item], F32)
    tok = np.array([[p[1] for p in it] for it in per_item], np.int32)
    beam = np.array([[p[2] for p in it] for it in per_item], np.int32)
    return sc, tok, beam


def running(step, base):
    """Picks of an item that just goes on: six distinct tokens, no stop, draw order not sorted, parents 1, 0, 0 in score order."""
    return [(-2.0 - step, base + 1, 2), (-0.5 - step, base + 2, 1), (-1.5 - step, base + 3, 0), (-1.0 - step, base + 4, 0),
            (-2.5 - step, base + 5, 1), (-3.0 - step, base + 6, 2)]


S = 64  # the stop token of the scripted scenarios


def test_scripted_scorer_scenarios():
    """Item 0 walks through every branch of BeamSearchScorer.process; items 1 and 2 run on next to it.  length_penalty 0: exact."""
    cfg = dict(items=3, nb=3, V=66, max_gen=9, Smax=40, stop=S, prefix0=11, D=96, pos_rows=64, emb_bf16=0)
    tables(cfg, 1)
    g = Generation(cfg, anc=np.tile(np.arange(3, dtype=np.uint8)[:, None], (3, 40)))
    others = lambda s: [running(s, 10), running(s, 30)]  # noqa: E731
    # k = 0: re-order with a duplicated parent (sorted: beam 0, beam 1, beam 0)
    st = g.step(as_picks([[(-1.5, 5, 0), (-0.5, 7, 0), (-1.0, 9, 1), (-2.0, 11, 2), (-2.5, 13, 1), (-3.0, 15, 2)]] + others(0)))
    assert list(st["cur_tok"][:3]) == [7, 9, 5] and list(st["anc"][1, :3, 12]) == [0, 1, 2] and list(st["anc"][1, 2, :12]) == [0] * 12
    # k = 1: a stop below rank nb becomes a hypothesis (history without the stop); the stop at rank 3 >= nb is ignored
    st = g.step(as_picks([[(-1.6, 22, 0), (-1.2, S, 1), (-1.0, 20, 2), (-1.5, S, 0), (-1.8, 23, 1), (-1.4, 21, 2)]] + others(1)))
    assert st["hyp_n"][0] == 1 and list(st["cur_tok"][:3]) == [20, 21, 22]
    assert [(float(s), list(t)) for s, t, _ in T.hyps_of(st, 0)] == [(float(F32(-1.2)), [9])]
    # k = 2: two stops of EQUAL score (ranks 1, 2) fill the list to nb; a third stop at rank 3 is ignored; not done (worst < best)
    st = g.step(as_picks([[(-1.3, S, 2), (-1.3, S, 0), (-1.25, 30, 1), (-1.65, S, 1), (-1.8, 32, 0), (-1.9, 33, 2)]] + others(2)))
    assert st["hyp_n"][0] == 3 and st["done"][0] == 0 and st["hyp_worst"][0] == F32(-1.3)
    # k = 3: a better one replaces the lowest - the OLDER of the two equal scores goes; a hypothesis that is not better is not added
    st = g.step(as_picks([[(-1.4, S, 1), (-1.25, S, 0), (-1.5, 41, 2), (-1.6, 42, 0), (-1.7, 43, 1), (-1.8, 44, 2)]] + others(3)))
    hy = T.hyps_of(st, 0)
    assert [float(s) for s, _, _ in hy] == [float(F32(x)) for x in (-1.2, -1.3, -1.25)] and st["hyp_counter"][0] == 4
    assert list(hy[1][1]) == list(g.scorer.hyps[0].beams[1][1]) and st["done"][0] == 0
    # k = 4: every candidate is below the worst hypothesis: done turns on (items 1 and 2 stay running)
    st = g.step(as_picks([[(-1.31, 51, 0), (-1.5, 52, 1), (-1.4, 53, 2), (-1.6, 54, 0), (-1.7, 55, 1), (-1.8, 56, 2)]] + others(4)))
    assert list(st["done"]) == [1, 0, 0] and list(st["unfinished"]) == [0] * 3 + [1] * 6
    # k = 5, 6: the done item emits stops at score 0 and its hypotheses stay; whatever its picks say
    for s in (5, 6):
        st = g.step(as_picks([[(-0.1, S, 0), (-0.2, 1, 1), (-0.3, 2, 2), (-0.4, 3, 0), (-0.5, 4, 1), (-0.6, 5, 2)]] + others(s)))
        assert list(st["cur_tok"][:3]) == [S] * 3 and (st["beam_scores"][:3] == 0).all() and st["hyp_counter"][0] == 4
    assert list(st["done"]) == [1, 0, 0] and (st["len"] == 7).all()


@pytest.mark.parametrize("lp", (1.0, 2.0))
def test_length_penalty_with_given_tokens(lp):
    """input_n = 2 given steps (scores, ancestry and hypotheses untouched, position k + 1), then generated_len = k + 1 - input_n in the
    hypothesis scores: sum / generated_len ** lp within 2 fp32 ulp of fp64; every decision is separated by far more."""
    cfg = dict(items=2, nb=3, V=66, max_gen=8, Smax=24, stop=S, prefix0=5, D=96, pos_rows=64, emb_bf16=1, length_penalty=lp, input_n=2)
    tables(cfg, 2)
    forced = np.full((6, 8), -1, np.int32)
    forced[:, 0], forced[:, 1] = [3, 3, 3, 4, 4, 4], [8, 8, 8, 9, 9, 9]
    cfg["forced"] = forced
    bs0 = np.array([0, -0.25, -0.5, 0, -0.125, -0.75], F32)
    g = Generation(cfg, anc=np.tile(np.arange(3, dtype=np.uint8)[:, None], (2, 24)), beam_scores=bs0)
    for k in (0, 1):
        st = g.step(as_picks([running(k, 10), running(k, 30)]))
        assert T.same_bits(st["beam_scores"], bs0) and list(st["cur_tok"]) == list(forced[:, k]) and (st["hyp_n"] == 0).all()
        want_h = cfg["emb"][forced[:, k]] + cfg["pos"][k + 1][None]  # a given token k is fed at position k + 1
        assert T.same_bits(st["h_next"], want_h.astype(F32))
    other = lambda s: [running(s, 30)]  # noqa: E731
    g.step(as_picks([[(-1.0, S, 1), (-0.9, S, 0), (-1.2, 11, 2), (-1.3, 12, 0), (-1.4, 13, 1), (-1.5, 14, 2)]] + other(2)), 2)  # generated_len 1
    g.step(as_picks([[(-1.7, S, 0), (-1.9, 21, 1), (-2.0, 22, 2), (-2.1, 23, 0), (-2.2, 24, 1), (-2.3, 25, 2)]] + other(3)), 2)  # 2
    st = g.step(as_picks([[(-3.3, S, 2), (-2.4, S, 1), (-3.4, 31, 0), (-3.5, 32, 1), (-3.6, 33, 2), (-3.7, 34, 0)]] + other(4)), 2)  # 3
    assert st["hyp_n"][0] == 3 and st["hyp_counter"][0] == (4 if lp == 1.0 else 5) and st["done"][0] == 0
    st = g.step(as_picks([[(-9.0, 41, 0), (-9.1, 42, 1), (-9.2, 43, 2), (-9.3, 44, 0), (-9.4, 45, 1), (-9.5, 46, 2)]] + other(5)), 2)
    assert list(st["done"]) == [1, 0]
    print(f"length_penalty {lp}: hypothesis score deviation {WORST.get('hyp_score_ulps', 0.0):.2f} ulp (bound 2)")


# (nb, k, D, bf16 tables): every copy loop of beam_select_kernel takes more than one round somewhere - nb * k > 2048, nb * Smax > 4096,
# nb * D > 4096 - the hypothesis copy runs past 1024 ids, both parities of k, max_gen = k + 1 (the new token is the row's last cell)
SIZES = [(2, 0, 0, 0), (2, 1, 96, 0), (10, 1, 0, 0), (3, 700, 96, 1), (3, 701, 96, 0), (3, 1100, 1280, 0), (3, 1100, 1280, 1),
         (10, 700, 96, 0), (10, 1100, 1280, 1), (2, 1101, 96, 1)]


@pytest.mark.parametrize("nb,k,D,bf16", SIZES)
def test_sizes_that_reach_every_loop_round(nb, k, D, bf16):
    items, V = 2, 300
    Smax = {2: 2200, 3: 1500, 10: 450}[nb]
    cfg = dict(items=items, nb=nb, V=V, max_gen=k + 1, Smax=Smax, stop=V - 2, prefix0=37, D=D, pos_rows=k + 2, emb_bf16=bf16)
    tables(cfg, 3)
    rows, nd = items * nb, 2 * nb
    hist = prng.randint(f"beam_step.hist.{nb}.{k}", 1, rows * max(k, 1), 0, V - 2).astype(np.int32).reshape(rows, max(k, 1))
    anc = prng.randint(f"beam_step.anc.{nb}.{k}", 2, rows * Smax, 0, nb).astype(np.uint8).reshape(rows, Smax)
    g = Generation(cfg, k=k, hist=hist, anc=anc, beam_scores=-np.arange(rows, dtype=F32))
    sc = (prng.uniform(f"beam_step.sc.{nb}.{k}", 3, items * nd) * 4 - 6).astype(F32).reshape(items, nd)
    tok = prng.randint(f"beam_step.tok.{nb}.{k}", 4, items * nd, 0, V - 2).astype(np.int32).reshape(items, nd)
    beam = prng.randint(f"beam_step.beam.{nb}.{k}", 5, items * nd, 0, nb).astype(np.int32).reshape(items, nd)
    tok[:, 1] = V - 2  # the best pick of every item is a stop: its history (k ids) becomes a hypothesis
    sc[:, 1] = 0.5
    assert len(set(sc.reshape(-1)[sc.reshape(-1) != 0.5])) == items * nd - items  # no accidental ties
    st = g.step((sc, tok, beam))
    assert (st["hyp_n"] == 1).all() and (st["hyp_len"][:, 0] == k).all() and (st["len"] == k + 1).all()
    if D:  # pos_rows = k + 2: position k + 2 is clamped to the last row, k + 1
        assert T.same_bits(st["h_next"], (cfg["emb"][st["cur_tok"]] + cfg["pos"][k + 1][None]).astype(F32))
    # the step counter has reached max_gen: a further call (a graph replay past the end) writes nothing at all
    got, _ = run_step(st, cfg, 1, (sc, tok, beam))
    for name in STATE:
        assert T.same_bits(got[name], st[name]), name


# ---------------------------------------------------------------------------------------------------------------- mode 0
NARROW_VOCABS = [66, 130, 1025, 8194, 15000]
NARROW_COMBOS = [(1, 0.8, 1.0), (2, 1.0, 0.7), (30, 0.8, 1.0), (127, 0.3, 1.3), (128, 0.8, 1.0)]  # (top_k, top_p, temperature)


def narrow_cfg(c, items, nb, V, k, **kw):
    cfg = dict(items=items, nb=nb, V=V, max_gen=k + 3, Smax=k + 8, stop=int(c["stop"]), start=int(c["start"]), fake=W.FAKE_ID, prefix0=2,
               penalty=float(c["penalty"]), suppress=int(c["suppress"]), pre=int(c["pre"]), D=0)
    cfg.update(kw)
    return cfg


def narrow_rows(c, items, nb, top_k, top_p, temp, k):
    """Per item: (NarrowRow list, score tolerance) - the fp64 side of beam_cand_kernel."""
    V = c["logits"].shape[1]
    out = []
    for bi in range(items):
        rows = [T.NarrowRow(c["logits"][r], W.case_seen(dict(c, k=k), r), c["penalty"], c["stop"], c["suppress"], c["pre"], top_k, top_p,
                            temp, T.delta_n()) for r in range(bi * nb, (bi + 1) * nb)]
        tol = W.score_tol(V, c["penalty"], temp, W.magnitude(rows, c["beam_scores"][bi * nb:(bi + 1) * nb]))
        out.append((rows, tol))
    return out


def check_cands(cands, refs, c, nb, group):
    """The candidate scratch of every row: the kept set exactly where the reference alone decides it, else between its bounds."""
    cand_sc, cand_tok, cand_n = cands
    for bi, (rows, tol) in enumerate(refs):
        for r, row in enumerate(rows):
            g = bi * nb + r
            n = int(cand_n[g])
            assert row.R_lo <= n <= row.R_hi, (g, n, row.R_lo, row.R_hi)
            want = np.sort(row.order[:n])
            assert np.array_equal(cand_tok[g, :n], want), (g, cand_tok[g, :n][:8], want[:8])
            dev = np.abs(cand_sc[g, :n].astype(np.float64) - (row.s[want] + float(c["beam_scores"][g])))
            assert (dev <= tol).all(), (g, float(dev.max()), tol)
            WORST[group] = max(WORST.get(group, 0.0), float(dev.max() / tol))


@pytest.mark.parametrize("variant", W.VARIANTS)
@pytest.mark.parametrize("shape", W.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("V", NARROW_VOCABS)
def test_narrow_pair_sampling(V, shape, variant):
    """beam_sample, 1 <= top_k <= 128: kept sets, draws and the scorer step behind them equal the fp64 reference where it alone
    decides them (uniforms from wide_beam_ref.safe_uniforms, a function of the reference); the whole-vocabulary kernels
    (itts_beam_sample_rows) agree on tokens, beams and kept counts wherever no row overflows the 128 candidates."""
    import test_gpu_wide_beam as WB

    items, nb = shape
    c = W.make_case(variant, V, items, nb)
    k = int(c["k"]) + (1 if (variant == "seen" and nb == 3) else 0)  # both parities of the active history plane
    if k > int(c["k"]):
        c["hist"][:, k - 1] = (np.arange(items * nb) * 7 + 5) % (V - 4)
    rows_n, nd = items * nb, 2 * nb
    exact = 0
    for top_k, top_p, temp in NARROW_COMBOS:
        refs = narrow_rows(c, items, nb, top_k, top_p, temp, k)
        cfg = narrow_cfg(c, items, nb, V, k, top_k=top_k, top_p=top_p, temperature=temp, do_sample=1)
        st = T.new_state(items, nb, cfg["max_gen"], cfg["Smax"], k, 0, c["beam_scores"], c["hist"],
                         np.tile(np.arange(nb, dtype=np.uint8)[:, None], (items, cfg["Smax"])))
        decided = all(row.R_lo == row.R_hi for rows, _ in refs for row in rows)
        margin = T.delta_n(nb * T.CAND)
        u = np.zeros((items, nd), F32)
        picks = None
        if decided:
            try:
                pk = []
                for bi, (rows, tol) in enumerate(refs):
                    sl = slice(bi * nb, (bi + 1) * nb)
                    for r, row in enumerate(rows):
                        W.assert_separated(dict(c, k=k), bi * nb + r, row, tol)
                    u[bi] = W.safe_uniforms(rows, c["beam_scores"][sl], V, nd, margin, f"beam_step.u.{variant}.{top_k}.{bi}", V)
                    drawn, _ = W.draw_margin(rows, c["beam_scores"][sl], V, u[bi])
                    pk.append([(row_score(rows, c, sl, b, t), t, b) for b, t in drawn] +
                              [(-np.inf, int(c["stop"]), 0)] * (nd - len(drawn)))  # no candidate left: the kernel repeats a stop at -inf
                picks = as_picks(pk)
            except AssertionError:
                picks = None  # two scores the reference cannot tell apart, or a distribution too flat for the margin
        if picks is None:
            u = W.uniform_sets(variant, V, items, nb)[1]
        uni = np.zeros((cfg["max_gen"], items, nd), F32)
        uni[k] = u
        got, cands = run_step(st, cfg, 0, logits=c["logits"], uniforms=uni)
        check_cands(cands, refs, c, nb, "narrow_cand_score")
        tol = max(t for _, t in refs)
        if picks is not None:
            scorer = T.new_scorer(items, nb, 0.0)
            want = T.ref_step(st, cfg, picks, scorer)
            compare(got, want, st, scorer, cfg, k, score_tol=tol, group="narrow_pick_score")
            exact += 1
            if all(row.n_ties <= T.CAND for rows, _ in refs for row in rows):  # the whole-vocabulary kernels on the same inputs
                wsc, wtok, wbeam, wkept = WB.beam_rows(dict(c, k=k), items, nb, top_k, top_p, temp, u)
                assert list(wkept) == [int(x) for x in cands[2]]
                scorer2 = T.new_scorer(items, nb, 0.0)
                compare(got, T.ref_step(st, cfg, (wsc, wtok, wbeam), scorer2), st, scorer2, cfg, k, score_tol=tol, group="narrow_vs_wide")
        else:  # not decided by the reference alone: the state is still a well-formed step over the kept candidates
            assert (got["len"] == k + 1).all() and T.same_bits(got["ids"][k & 1], st["ids"][k & 1])
            for g_ in range(rows_n):
                src_ok = [q for q in range((g_ // nb) * nb, (g_ // nb + 1) * nb) if np.array_equal(got["ids"][(k & 1) ^ 1, g_, :k], st["ids"][k & 1, q, :k])]
                assert src_ok, g_
        print(f"V {V} {items}x{nb} {variant} {(top_k, top_p, temp)}: kept {[int(x) for x in cands[2]]} exact {picks is not None}")
    assert exact >= 3, exact  # of the 5 combos: the exact comparison is the rule, not the exception


def row_score(rows, c, sl, b, t):
    return F32(rows[b].s[t] + float(F32(c["beam_scores"][sl][b])))


@pytest.mark.parametrize("V,items,nb", [(5, 1, 3), (66, 2, 3), (8194, 1, 10), (1025, 1, 2)])
def test_narrow_pair_beam_search(V, items, nb):
    """do_sample = 0: the 2 nb best of log_softmax + penalty + beam score over the item's beams, the lower flat index among equals.
    The "ties" inputs (multiples of 1/4, one logits row and one beam score per item) have equal scores across all beams."""
    c = W.make_case("ties", V, items, nb)
    c["start"], c["stop"] = min(c["start"], V - 1), V - 2
    if V == 5:
        c["start"], c["stop"] = 2, 3
    k, nd = 0, 2 * nb
    cfg = narrow_cfg(c, items, nb, V, k, do_sample=0, top_k=0)
    st = T.new_state(items, nb, cfg["max_gen"], cfg["Smax"], k, 0, c["beam_scores"], None, np.tile(np.arange(nb, dtype=np.uint8)[:, None], (items, cfg["Smax"])))
    pk, tol = [], 0.0
    for bi in range(items):
        sl = slice(bi * nb, (bi + 1) * nb)
        rows = [W.Row(c["logits"][r], W.case_seen(c, r), c["penalty"], c["stop"], 0, 0, 0, 1.0, 1.0, 0.0) for r in range(bi * nb, (bi + 1) * nb)]
        tol = max(tol, W.score_tol(V, c["penalty"], 1.0, W.magnitude(rows, c["beam_scores"][sl])))
        flat = np.concatenate([row.s + float(c["beam_scores"][bi * nb + r]) for r, row in enumerate(rows)])
        order = np.lexsort((np.arange(flat.size), -flat))[:nd]
        vals = np.unique(flat[np.isfinite(flat)])
        assert vals.size < 2 or np.diff(vals).min() > 100 * tol  # different scores are far apart, equal ones equal in fp32 too
        pk.append([(F32(flat[f]), int(f % V), int(f // V)) for f in order])
    got, cands = run_step(st, cfg, 0, logits=c["logits"])
    scorer = T.new_scorer(items, nb, 0.0)
    want = T.ref_step(st, cfg, as_picks(pk), scorer)
    compare(got, want, st, scorer, cfg, k, score_tol=tol, group="beam_search_score")
    assert len({(int(t), int(b)) for _, t, b in pk[0]}) == nd


def test_overflow_of_the_candidates_is_deterministic():
    """More than 128 scores tie with the k-th: the survivors are the strictly larger scores, then the ties by ascending id
    (oracle/hf_beam.py warp_row).  All-equal logits plus one larger token at a high id, top_k 30; 127 larger scores plus 50 ties at
    top_k 128; the same bits on every call."""
    V, items, nb = 8194, 1, 2
    for name, top_k in (("one", 30), ("many", 128)):
        lg = np.zeros((nb, V), F32)
        if name == "one":
            lg[:, 8000] = 2.0
            want = [np.sort(np.r_[8000, np.arange(127)])] * nb
        else:
            big = 8193 - 61 * np.arange(127)
            lg[:] = -30.0
            lg[:, big] = 1.0 + (np.arange(127) % 7).astype(F32)
            tie = np.setdiff1d(17 + 160 * np.arange(51), big)[:50]
            assert tie.size == 50 and tie[0] == 17
            lg[:, tie] = 0.5
            want = [np.sort(np.r_[big, tie[:1]])] * nb
        c = dict(logits=lg, hist=np.zeros((nb, 4), np.int32), k=0, beam_scores=np.array([0, -0.5], F32), penalty=1.0, stop=V - 2,
                 start=V - 3, suppress=0, pre=0)
        cfg = narrow_cfg(c, items, nb, V, 0, top_k=top_k, top_p=1.0, temperature=1.0, do_sample=1)
        st = T.new_state(items, nb, cfg["max_gen"], cfg["Smax"], 0, 0, c["beam_scores"], None, np.zeros((nb, cfg["Smax"]), np.uint8))
        uni = np.full((cfg["max_gen"], items, 2 * nb), 0.5, F32)
        runs = [run_step(st, cfg, 0, logits=lg, uniforms=uni) for _ in range(3)]
        for got, cands in runs:
            for r in range(nb):
                assert int(cands[2][r]) == 128 and np.array_equal(cands[1][r], want[r]), (name, r, cands[1][r][:8], want[r][:8])
        for got, cands in runs[1:]:
            assert all(T.same_bits(x, y) for x, y in zip(cands, runs[0][1])) and all(T.same_bits(got[n], runs[0][0][n]) for n in STATE)
        refs = narrow_rows(c, items, nb, top_k, 1.0, 1.0, 0)
        assert all(np.array_equal(np.sort(row.order), want[r]) for r, row in enumerate(refs[0][0]))  # and the reference says the same


def test_typical_rows_then_beam_step():
    """The chain of a typical-sampling beam step: itts_typical_rows over the beam histories, then itts_beam_step with preprocessed = 1
    on its output."""
    import test_gpu_typical_filter as TF

    V, nb, mass, k = 8194, 3, 0.7, T.TYP_K
    tc = T.typical_rows(V, "beams", mass, 2)
    rows = [0, 1, 2]  # flat, mid, wide as the three beams of one item
    out = TF.run_typical(tc, mass, 2, "beams")[rows]
    for r in rows:
        kept = out[r] > -np.inf
        assert not (tc["refs"][r]["must"] & ~kept).any() and not (kept & ~tc["refs"][r]["may"]).any()
    c = dict(logits=np.ascontiguousarray(out), hist=np.ascontiguousarray(tc["hist"][rows]), k=k, beam_scores=np.array([-1.0, -1.5, -2.25], F32),
             penalty=10.0, stop=tc["stop"], start=tc["start"], suppress=0, pre=1)
    top_k, top_p, temp = 30, 0.8, 1.0
    refs = narrow_rows(c, 1, nb, top_k, top_p, temp, k)
    cfg = narrow_cfg(c, 1, nb, V, k, top_k=top_k, top_p=top_p, temperature=temp, do_sample=1)
    st = T.new_state(1, nb, cfg["max_gen"], cfg["Smax"], k, 0, c["beam_scores"], c["hist"], np.tile(np.arange(nb, dtype=np.uint8)[:, None], (1, cfg["Smax"])))
    (rws, tol), = refs
    assert all(row.R_lo == row.R_hi for row in rws)
    u = W.safe_uniforms(rws, c["beam_scores"], V, 2 * nb, T.delta_n(nb * T.CAND), "beam_step.chain.u", V)
    drawn, _ = W.draw_margin(rws, c["beam_scores"], V, u)
    picks = as_picks([[(row_score(rws, c, slice(0, nb), b, t), t, b) for b, t in drawn]])
    uni = np.zeros((cfg["max_gen"], 1, 2 * nb), F32)
    uni[k] = u
    got, cands = run_step(st, cfg, 0, logits=c["logits"], uniforms=uni)
    check_cands(cands, refs, c, nb, "chain_cand_score")
    scorer = T.new_scorer(1, nb, 0.0)
    compare(got, T.ref_step(st, cfg, picks, scorer), st, scorer, cfg, k, score_tol=tol, group="chain_pick_score")


def test_zz_report():
    for k_, v in sorted(WORST.items()):
        print(f"beam step {k_}: worst deviation / bound {v:.3f}")
