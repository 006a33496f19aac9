"""GPU: the sort-free whole-vocabulary samplers (csrc/decode_sampler.hip sampler_select_kernel, csrc/beam.hip
beam_wide_cand_sel_kernel) through itts_sample_rows_select / itts_beam_sample_rows_select, and the <ROWS> form through
itts_sampler_step_rows under ITTS_WIDE_SELECT=1.

The predicates and their bounds are those of the sorted kernels, unchanged: wide_sampler_ref.Ref (64 * 2^-24) and wide_beam_ref
(512 * 2^-24).  A row without a finite score has no rank in Ref: there the entry returns sampler_wide_kernel's (token 0, 1 kept)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_sampler_rows as R  # noqa: E402  (case, run_rows, ENTRIES, TABLES)
import test_gpu_sampler_step as S  # noqa: E402  (run_sampler)
import token_choice_ref as T  # noqa: E402
import wide_beam_ref as B  # noqa: E402
import wide_sampler_ref as W  # noqa: E402

from itts_hip import lib, prng  # noqa: E402

DEV, U_TOP = "cuda:0", B.U_TOP


def sample_rows(entry, lg, seen, penalty, stop, suppress, pre, top_k, top_p, temp, u):
    """One of the two operator entries on CPU arrays -> (tok [rows], kept [rows])."""
    l = lib.load()
    n, V = lg.shape
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (lg, np.asarray(u, np.float32))]
    sn = torch.from_numpy(seen).to(DEV) if seen is not None else None
    tok, kept = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    scratch = torch.empty(n * (V + 16), dtype=torch.uint8, device=DEV)
    st = getattr(l, entry)(tok.data_ptr(), kept.data_ptr(), d[0].data_ptr(), sn.data_ptr() if sn is not None else None, n, V,
                           float(penalty), int(stop), int(suppress), int(pre), int(top_k), float(top_p), float(temp), d[1].data_ptr(),
                           scratch.data_ptr(), scratch.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(st, entry, l)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), kept.cpu().numpy()


def make_case(variant, V):
    """-> logits [3, V], seen bytes or None, penalty, stop, suppress_stop, preprocessed"""
    lg = B.gaussian(f"wide_select.{variant}", V, (3, V), 2.5)
    seen, penalty, stop, suppress, pre = None, 1.0, V - 2, 0, 0
    if variant == "ties":  # five distinct values: the TopK boundary, the TopP cut and the draw fall inside groups of hundreds
        lg = np.clip(np.round(lg / 2.5), -2, 2).astype(np.float32)
    elif variant == "few_finite":  # all but 40 entries -inf
        keep = np.zeros((3, V), dtype=bool)
        for b in range(3):
            keep[b, np.argsort(prng.uniform(f"wide_select.keep{b}", V, V), kind="stable")[:40]] = True
        lg, pre = np.where(keep, lg, np.float32(-np.inf)).astype(np.float32), 1
    elif variant == "no_finite":
        lg, pre = np.full((3, V), -np.inf, dtype=np.float32), 1
    elif variant == "seen_stop":  # the best tokens penalised, the arg-max of row 0 is the suppressed stop token
        seen = np.zeros((3, V), dtype=np.uint8)
        for b in range(3):
            seen[b, prng.randint(f"wide_select.seen{b}", V, 60, 0, V)] = 1
            seen[b, np.argsort(lg[b])[-4:-1]] = 1
        penalty, stop, suppress = 10.0, int(np.argmax(lg[0])), 1
    return np.ascontiguousarray(lg), seen, penalty, stop, suppress, pre


@pytest.mark.parametrize("variant", ["gauss", "ties", "few_finite", "no_finite", "seen_stop"])
@pytest.mark.parametrize("V", [129, 1024, 1025, 8194, 16384])
def test_sampler_results_pass_the_predicate(V, variant):
    lg, seen, penalty, stop, suppress, pre = make_case(variant, V)
    u_rand = np.minimum(prng.uniform(f"wide_select.u.{variant}", V, 3) * np.float32(0.5) + np.float32(0.5), np.float32(U_TOP))
    u_sets = [np.asarray([u_rand[0], 0.0, U_TOP], dtype=np.float32), np.asarray([U_TOP, u_rand[1], 0.0], dtype=np.float32)]
    for top_k in (0, 1, 129, V - 1, V, V + 5):
        for top_p in (1.0, 0.8, 1e-6):
            for temp in (1.0, 0.3):
                sc = [W.sampler_scores(lg[b], np.nonzero(seen[b])[0] if seen is not None else (), penalty, stop, suppress, pre, temp)
                      for b in range(3)]
                refs = [W.Ref(s, top_k, top_p) for s in sc]
                for ui, u in enumerate(u_sets):
                    args = (penalty, stop, suppress, pre, top_k, top_p, temp)
                    tok, kept = sample_rows("itts_sample_rows_select", lg, seen, *args, u)
                    for b in range(3 if variant != "no_finite" else 0):
                        what = (top_k, top_p, temp, ui, b, int(tok[b]), int(kept[b]), refs[b].R_lo, refs[b].R_hi)
                        assert 0 <= tok[b] < V and sc[b][tok[b]] > -np.inf, what
                        assert refs[b].accepts(tok[b], u[b], kept[b]), what
                        if top_p == 1e-6:
                            assert kept[b] == 1 and tok[b] == int(refs[b].order[0]), what  # only the best token stays
                    assert variant != "no_finite" or ((tok == 0).all() and (kept == 1).all())
                    if ui == 0:  # the same call twice: the same bits; a row alone equals the row at its place in the batch of 3
                        again = sample_rows("itts_sample_rows_select", lg, seen, *args, u)
                        assert np.array_equal(tok, again[0]) and np.array_equal(kept, again[1])
                        for b in range(3):
                            t1, k1 = sample_rows("itts_sample_rows_select", lg[b:b + 1], seen[b:b + 1] if seen is not None else None,
                                                 *args, u[b:b + 1])
                            assert (t1[0], k1[0]) == (tok[b], kept[b]), (top_k, top_p, temp, b)


@pytest.mark.parametrize("V", [66, 8194])
def test_rows_form_takes_the_wide_rows_only(V, monkeypatch):
    """ITTS_WIDE_SELECT=1: the wide rows of a mixed table have the bits of the scalar form run with their settings, the greedy rows
    those of the greedy kernel - the select kernel's blocks on them returned without a write."""
    monkeypatch.setenv("ITTS_WIDE_SELECT", "1")
    lg, cfg, st, u = R.case(V, 64)
    names = R.TABLES["no_narrow"]
    got = R.run_rows(st, cfg, lg, u, [R.ENTRIES[n] for n in names])
    for r, n in enumerate(names):
        mode, top_k, top_p, temp, pen = R.ENTRIES[n]
        want = S.run_sampler(st, dict(cfg, do_sample=mode, top_k=top_k, top_p=top_p, temperature=temp, penalty=pen), lg, u)
        for arr in S.STATE:
            assert T.same_bits(got[arr][r], want[arr][r]), (r, n, arr)
        if mode:  # and the wide rows' picks are right
            seen_ids = np.nonzero(st["seen"][r])[0]
            ref = W.Ref(W.sampler_scores(lg[r], seen_ids, pen, cfg["stop"], False, False, temp), top_k, top_p)
            if st["unfinished"][r] and cfg["forced"][r, st["step"][r]] < 0:
                assert ref.accepts(got["cur_tok"][r], u[min(int(st["step"][r]), R.MAX_GEN - 1), r]), (r, n)


def beam_rows(entry, c, items, nb, top_k, top_p, temp, u):
    """One of the two beam operator entries -> (picks, kept [rows], the [rows][V] array the first launch left in the scratch)."""
    l = lib.load()
    rows, V = c["logits"].shape
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (c["logits"], c["hist"], c["beam_scores"].astype(np.float32),
                                                                     np.asarray(u, np.float32))]
    psc = torch.zeros((items, 2 * nb), dtype=torch.float32, device=DEV)
    ptok, pbeam = (torch.zeros((items, 2 * nb), dtype=torch.int32, device=DEV) for _ in range(2))
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    scratch = torch.empty(items * nb * (V + 1) + items, dtype=torch.float32, device=DEV)
    st = getattr(l, entry)(psc.data_ptr(), ptok.data_ptr(), pbeam.data_ptr(), kept.data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                           c["hist"].shape[1], int(c["k"]), d[2].data_ptr(), items, nb, V, float(c["penalty"]), int(c["stop"]),
                           int(c["suppress"]), int(c["start"]), B.FAKE_ID, int(c["pre"]), int(top_k), float(top_p), float(temp),
                           d[3].data_ptr(), scratch.data_ptr(), scratch.numel() * 4, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(st, entry, l)
    torch.cuda.synchronize()
    picks, sc = (psc.cpu().numpy(), ptok.cpu().numpy(), pbeam.cpu().numpy()), scratch[:rows * V].cpu().numpy().reshape(items, nb, V)
    for bi in range(items):  # the second launch put -inf where it drew: the array as the first launch wrote it has the picks back
        live = picks[0][bi] > -np.inf
        sc[bi, picks[2][bi][live], picks[1][bi][live]] = picks[0][bi][live]
    return picks, kept.cpu().numpy(), sc.reshape(rows, V)


@pytest.mark.parametrize("variant", ["gauss", "ties", "few_finite", "seen", "stop"])
@pytest.mark.parametrize("V", [1025, 8194])
def test_beam_rows_keep_the_reference_set(V, variant):
    items, nb = 1, 3
    c = B.make_case(variant, V, items, nb)
    for top_k, top_p, temp in B.COMBOS:
        (rows, delta, tol), = B.case_refs(c, items, nb, top_k, top_p, temp)
        for u in B.uniform_sets(variant, V, items, nb):
            picks, kept, sc = beam_rows("itts_beam_sample_rows_select", c, items, nb, top_k, top_p, temp, u)
            res = B.accepts(rows, c["beam_scores"], V, c["stop"], [p[0] for p in picks], kept, u[0], delta, tol)
            assert res, (top_k, top_p, temp, res.reason)
            for r, row in enumerate(rows):
                fin = np.nonzero(sc[r] > -np.inf)[0]
                assert fin.size == kept[r] and np.array_equal(fin, np.sort(row.order[:kept[r]])), (top_k, top_p, temp, r)
                if row.boundary_margin() > delta:
                    assert kept[r] == row.R, (top_k, top_p, temp, r, kept[r], row.R)
                assert np.abs(sc[r][fin] - (row.s[fin] + float(c["beam_scores"][r]))).max() <= tol, (top_k, top_p, temp, r)
        again = beam_rows("itts_beam_sample_rows_select", c, items, nb, top_k, top_p, temp, u)
        assert all(T.same_bits(x, y) for x, y in zip(picks + (kept, sc), again[0] + again[1:]))
