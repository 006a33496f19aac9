"""No GPU: the whole-vocabulary beam sampler's acceptance predicate (wide_beam_ref.py) accepts an fp32 emulation of the two
kernels' documented summation structure and the host path's picks, and rejects broken samplers; Engine.generate routes
`wide_beam_sampler`; the public surface (header, libraries, ctypes table, command line) agrees."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_beam_ref as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tolerances_follow_the_chain():
    assert B.chain(16384, 10) == 160 + 6 + 15 + 1 + 160 and B.delta_b(16384, 10) == 512 * 2.0 ** -24
    assert B.chain(130, 2) == 1 + 6 + 15 + 1 + 1 and B.delta_b(130, 2) == 32 * 2.0 ** -24
    assert B.delta_b(8194, 3) == 128 * 2.0 ** -24  # the model's vocabulary at the reference's 3 beams: L = 25
    for V in (130, 1025, 8194, 16384):  # beam_wide_cand_kernel's own chain (53 at most) is never the longer one
        for nb in (2, 3, 10):
            NP = 1024
            while NP < V:
                NP <<= 1
            per = NP // 1024
            assert (per - 1) + 6 + 15 + 1 + per <= B.chain(V, nb)


@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("shape", B.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("V", B.VOCABS)
def test_predicate_accepts_the_emulated_kernels(V, shape, variant):
    items, nb = shape
    c = B.make_case(variant, V, items, nb)
    checked = 0
    for top_k, top_p, temp in B.COMBOS:
        refs = B.case_refs(c, items, nb, top_k, top_p, temp)
        for bi, (rows, delta, tol) in enumerate(refs):
            for r, row in enumerate(rows):
                B.assert_separated(c, bi * nb + r, row, tol)
        for u in B.uniform_sets(variant, V, items, nb):
            for bi, (rows, delta, tol) in enumerate(refs):
                sl = slice(bi * nb, (bi + 1) * nb)
                picks, kept = B.emulate(c["logits"][sl], [B.case_seen(c, r) for r in range(bi * nb, (bi + 1) * nb)], c["beam_scores"][sl],
                                        c["penalty"], c["stop"], c["suppress"], c["pre"], top_k, top_p, temp, u[bi])
                res = B.accepts(rows, c["beam_scores"][sl], V, c["stop"], picks, kept, u[bi], delta, tol)
                assert res, (top_k, top_p, temp, bi, res.reason)
                checked += 1
    assert checked == len(B.COMBOS) * 2 * items


def test_few_finite_case_exhausts_its_candidates():
    """Item 0 of the few_finite case has 2 finite scores in every row: its 2 * nb draws take them all, the last one through the
    'last live entry' fallback (u = 0.99999994 there); with one row emptied the surplus picks are (-inf, stop, 0)."""
    V, items, nb = 130, 2, 3
    c = B.make_case("few_finite", V, items, nb)
    u = B.uniform_sets("few_finite", V, items, nb)[0]
    refs = B.case_refs(c, items, nb, 0, 1.0, 1.0)
    seen = [B.case_seen(c, r) for r in range(nb)]
    (psc, ptok, pbeam), kept = B.emulate(c["logits"][:nb], seen, c["beam_scores"][:nb], 10.0, c["stop"], 0, 1, 0, 1.0, 1.0, u[0])
    assert list(kept) == [2] * nb and np.isfinite(psc).all() and len({(int(b), int(t)) for b, t in zip(pbeam, ptok)}) == 2 * nb
    lg = c["logits"][:nb].copy()
    lg[1] = -np.inf
    rows = B.item_rows(lg, seen, 10.0, c["stop"], 0, 1, 0, 1.0, 1.0, refs[0][1])
    picks, kept = B.emulate(lg, seen, c["beam_scores"][:nb], 10.0, c["stop"], 0, 1, 0, 1.0, 1.0, u[0])
    assert list(kept) == [2, 0, 2] and list(picks[1][4:]) == [c["stop"]] * 2 and (picks[0][4:] == -np.inf).all()
    assert B.accepts(rows, c["beam_scores"][:nb], V, c["stop"], picks, kept, u[0], refs[0][1], refs[0][2])


@pytest.mark.parametrize("V", B.VOCABS)
def test_predicate_accepts_the_host_path(V):
    """infer_core.host_beam_step (torch's warpers, sequential fp32 sums) on the gauss case, 2 items x 3 beams."""
    from itts_hip import infer_core

    items, nb = 2, 3
    c = B.make_case("gauss", V, items, nb)
    u = B.uniform_sets("gauss", V, items, nb)[1]
    for top_k, top_p, temp in B.COMBOS:
        psc, ptok, pbeam = infer_core.host_beam_step(c["logits"], c["hist"], c["k"], c["beam_scores"], np.zeros(items, np.int32), nb,
                                                     c["penalty"], temp, top_k, top_p, 0.0, u, c["stop"], False, c["start"], B.FAKE_ID)
        for bi, (rows, delta, tol) in enumerate(B.case_refs(c, items, nb, top_k, top_p, temp)):
            kept = [len(infer_core.host_distribution(c["logits"][bi * nb + r], B.case_seen(c, bi * nb + r), c["penalty"], temp, top_k,
                                                     top_p, 0.0, c["stop"], False, min_keep=2, log_softmax_first=True)[0])
                    for r in range(nb)]
            res = B.accepts(rows, c["beam_scores"][bi * nb:(bi + 1) * nb], V, c["stop"], (psc[bi], ptok[bi], pbeam[bi]), kept, u[bi],
                            delta, tol)
            assert res, (top_k, top_p, temp, bi, res.reason)


# ---- broken samplers, each on a case built to expose it ----
def _gauss_item(V=1025, nb=3, std=2.5):
    c = B.make_case("gauss", V, 1, nb, std=std)
    return c, [B.case_seen(c, r) for r in range(nb)]


def _mid_u(rows, beam_scores, V, nd, margin=1e-3):
    return B.safe_uniforms(rows, beam_scores, V, nd, margin, "wide_beam.broken", V)


def test_predicate_rejects_draws_with_replacement():
    """Every draw takes the same u: with replacement the same candidate comes back."""
    V, nb = 1025, 3
    c, seen = _gauss_item(V, nb)
    rows, delta, tol = B.case_refs(c, 1, nb, 0, 0.8, 1.0)[0]
    u = np.full(2 * nb, 0.4, dtype=np.float32)
    good, kept = B.plain(rows, c["beam_scores"], V, c["stop"], u)
    assert B.accepts(rows, c["beam_scores"], V, c["stop"], good, kept, u, delta, tol)
    bad, kept = B.plain(rows, c["beam_scores"], V, c["stop"], u, wrong="replacement")
    res = B.accepts(rows, c["beam_scores"], V, c["stop"], bad, kept, u, delta, tol)
    assert not res and "picked twice" in res.reason


def test_predicate_rejects_token_major_order():
    """u = 0.5: in token-major order the middle of the mass lies at another candidate than in beam-major order."""
    V, nb = 1025, 3
    c, seen = _gauss_item(V, nb)
    rows, delta, tol = B.case_refs(c, 1, nb, 0, 0.8, 1.0)[0]
    u = _mid_u(rows, c["beam_scores"], V, 2 * nb)
    good, kept = B.plain(rows, c["beam_scores"], V, c["stop"], u)
    assert B.accepts(rows, c["beam_scores"], V, c["stop"], good, kept, u, delta, tol)
    bad, kept = B.plain(rows, c["beam_scores"], V, c["stop"], u, wrong="token_major")
    assert not np.array_equal(bad[1], good[1]) or not np.array_equal(bad[2], good[2])
    assert not B.accepts(rows, c["beam_scores"], V, c["stop"], bad, kept, u, delta, tol)


def test_predicate_rejects_min_tokens_to_keep_1():
    """std 6 at top_p = 0.3: the best token of a row outweighs the nucleus alone, min_tokens_to_keep = 1 keeps 1 where HF keeps 2."""
    V, nb = 1025, 3
    c, seen = _gauss_item(V, nb, std=6.0)
    rows, delta, tol = B.case_refs(c, 1, nb, 0, 0.3, 1.0)[0]
    rows1 = B.case_refs(c, 1, nb, 0, 0.3, 1.0, min_keep=1)[0][0]
    assert any(r.R == 1 for r in rows1) and all(r.R_lo >= 2 for r in rows)
    u = np.linspace(0.1, 0.9, 2 * nb).astype(np.float32)
    bad, kept = B.plain(rows1, c["beam_scores"], V, c["stop"], u)
    res = B.accepts(rows, c["beam_scores"], V, c["stop"], bad, kept, u, delta, tol)
    assert not res and "kept" in res.reason


def test_predicate_rejects_a_cdf_without_the_beam_scores():
    """Beam scores 0, -0.75 .. apart and more: without them the beams weigh the same and the draws land elsewhere."""
    V, nb = 1025, 3
    c, seen = _gauss_item(V, nb)
    rows, delta, tol = B.case_refs(c, 1, nb, 0, 0.8, 1.0)[0]
    u = _mid_u(rows, c["beam_scores"], V, 2 * nb)
    bad, kept = B.plain(rows, c["beam_scores"], V, c["stop"], u, wrong="no_beam_score")
    good, _ = B.plain(rows, c["beam_scores"], V, c["stop"], u)
    assert not np.array_equal(bad[1], good[1]) or not np.array_equal(bad[2], good[2])
    assert not B.accepts(rows, c["beam_scores"], V, c["stop"], bad, kept, u, delta, tol)


def test_predicate_rejects_ties_broken_by_the_higher_id():
    """Logits quantised to 1/4 at top_p = 0.8: the nucleus ends inside a group of equal scores, of which the lower ids stay.  The
    first draw is aimed at a candidate only the broken sampler keeps."""
    V, nb = 1025, 3
    c = B.make_case("ties", V, 1, nb)
    rows, delta, tol = B.case_refs(c, 1, nb, 0, 0.8, 1.0)[0]
    rowsd = B.case_refs(c, 1, nb, 0, 0.8, 1.0, ties_desc=True)[0][0]
    only_bad = sorted(set(int(t) for t in rowsd[0].order[:rowsd[0].R]) - set(int(t) for t in rows[0].order[:rows[0].R]))
    assert only_bad, "the nucleus boundary of row 0 does not cut a tie group: choose another case"
    # u aimed at the middle of that candidate's interval in the broken sampler's own CDF (beam 0 comes first in flat order)
    ent = [(r, int(t), rowsd[r].s[t] + float(c["beam_scores"][r])) for r in range(nb) for t in np.sort(rowsd[r].order[:rowsd[r].R])]
    S = np.array([x[2] for x in ent])
    cdf = np.cumsum(np.exp(S - S.max()))
    pos = [i for i, x in enumerate(ent) if x[0] == 0 and x[1] == only_bad[0]][0]
    u = np.linspace(0.1, 0.9, 2 * nb).astype(np.float32)
    u[0] = np.float32((cdf[pos] - 0.5 * (cdf[pos] - (cdf[pos - 1] if pos else 0.0))) / cdf[-1])
    bad, kept = B.plain(rowsd, c["beam_scores"], V, c["stop"], u)
    assert (int(bad[2][0]), int(bad[1][0])) == (0, only_bad[0])
    res = B.accepts(rows, c["beam_scores"], V, c["stop"], bad, kept, u, delta, tol)
    assert not res and "not a kept candidate" in res.reason


def test_predicate_rejects_kept_plus_one():
    V, nb = 130, 3
    c, seen = _gauss_item(V, nb)
    rows, delta, tol = B.case_refs(c, 1, nb, 0, 0.8, 1.0)[0]
    assert rows[0].R_lo == rows[0].R_hi  # (boundary margin 2.6e-4 against delta 1.9e-6)
    u = np.linspace(0.1, 0.9, 2 * nb).astype(np.float32)
    bad, kept = B.plain(rows, c["beam_scores"], V, c["stop"], u, wrong="kept+1")
    res = B.accepts(rows, c["beam_scores"], V, c["stop"], bad, kept, u, delta, tol)
    assert not res and "kept[0]" in res.reason


# ---- Engine.generate routing (no library, no GPU) ----
class _Routed(Exception):
    pass


def _stub_engine(calls):
    from itts_hip import engine as ieng

    class Stub(ieng.Engine):
        def __init__(self):  # no library, no device
            class Cfg:
                stop_mel_token = 7
            self.ccfg = Cfg()

        def _generate_host_sampled(self, *a, **k):
            calls.append("host_sampled")
            return np.zeros((1, 1), dtype=np.int64)

        def _generate_host_beams(self, *a, **k):
            calls.append("host_beams")
            return np.zeros((1, 1), dtype=np.int64)

        def set_beam_sample(self, num_beams, top_k=30, *a, **k):
            if num_beams > 1:
                calls.append(("device_beams", top_k, k.get("host", False)))
                raise _Routed()

        def set_sampling(self, do_sample, top_k=30, *a, **k):
            if do_sample:
                calls.append(("device", top_k))
                raise _Routed()

        def __del__(self):
            pass

    return Stub()


def test_generate_routes_wide_beam_sampler(monkeypatch):
    monkeypatch.delenv("ITTS_WIDE_SAMPLER", raising=False)
    monkeypatch.delenv("ITTS_WIDE_BEAM_SAMPLER", raising=False)
    calls = []
    eng = _stub_engine(calls)
    text = np.zeros((1, 4), dtype=np.int32)
    kw = dict(do_sample=True, top_p=0.8, num_beams=3)
    for top_k, want in ((0, 0), (None, 0), (200, 200)):
        calls.clear()
        with pytest.raises(_Routed):
            eng.generate(None, text, 4, top_k=top_k, wide_beam_sampler="device", **kw)
        assert calls == [("device_beams", want, False)]
    calls.clear()
    eng.generate(None, text, 4, top_k=0, **kw)  # None
    eng.generate(None, text, 4, top_k=200, wide_beam_sampler="host", **kw)
    eng.generate(None, text, 4, top_k=0, wide_sampler="device", **kw)  # the one-beam switch alone changes nothing under beams
    assert calls == ["host_beams"] * 3
    for wbs in (None, "host", "device"):  # top_k = 30 goes where it goes today: the narrow device kernels
        calls.clear()
        with pytest.raises(_Routed):
            eng.generate(None, text, 4, top_k=30, wide_beam_sampler=wbs, **kw)
        assert calls == [("device_beams", 30, False)]
    calls.clear()
    eng.generate(None, text, 4, do_sample=True, top_p=0.8, top_k=0, wide_beam_sampler="device")  # one beam: not this switch
    assert calls == ["host_sampled"]
    calls.clear()
    monkeypatch.setenv("ITTS_WIDE_BEAM_SAMPLER", "device")
    with pytest.raises(_Routed):
        eng.generate(None, text, 4, top_k=0, **kw)
    eng.generate(None, text, 4, top_k=0, wide_beam_sampler="host", **kw)  # the keyword wins over the environment
    assert calls == [("device_beams", 0, False), "host_beams"]
    with pytest.raises(ValueError):
        eng.generate(None, text, 4, top_k=0, wide_beam_sampler="gpu", **kw)
    monkeypatch.setenv("ITTS_WIDE_BEAM_SAMPLER", "gpu")
    with pytest.raises(ValueError):
        eng.generate(None, text, 4, top_k=0, **kw)


def test_wide_beam_public_surface():
    from itts_hip import lib

    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        header = f.read()
    for sym in ("itts_beam_sample_rows", "itts_gpt_beam_picks"):
        assert sym in lib.exported_symbols()
        for half in ("bf16", "f16"):
            assert callable(getattr(lib.load(half), sym))
        assert re.search(r"\bint\s+%s\s*\(" % sym, header)
    assert lib.load().itts_abi_version() == 4  # additions: the ABI version stays

    from itts_hip import engine as ieng

    assert inspect.signature(ieng.Engine.generate).parameters["wide_beam_sampler"].default is None

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["wide_beam_sampler"].default is None

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav", "--wide-beam-sampler", "device"]).wide_beam_sampler == "device"
    assert p.parse_args(["hello", "-v", "voice.wav"]).wide_beam_sampler is None
