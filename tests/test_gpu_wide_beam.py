"""GPU: the whole-vocabulary beam sampler (csrc/beam.hip beam_wide_cand_kernel + beam_wide_pick_kernel: beam_sample with
top_k = 0 / None or > 128) - at the operator level through itts_beam_sample_rows, and inside the engine's decode step with
beam_select_kernel behind it.

What a result has to satisfy is wide_beam_ref.accepts: the fp64 restatement of HF 4.36.2's warpers and the draws without
replacement over the flat candidates, with DELTA_B and SCORE_TOL derived in that module from the kernels' summation chains - no
case is skipped.  The operator tests draw their inputs on the CPU (itts_hip/prng.py), so the fp64 side needs no GPU.  Without
the feature every test here fails: the two symbols are missing and itts_gpt_set_beams rejects top_k = 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_beam_ref as B  # noqa: E402

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core, lib, synth  # noqa: E402

CFG = icfg.indextts_1_5()
DEV = "cuda:0"
MAX_DEV = {}  # largest |device score - fp64 score| seen, by test: printed for profiles/wide_beam_sampler.txt


# ---------------------------------------------------------------- operator level
def scratch_bytes(items, nb, V):
    return (items * nb * (V + 1) + items) * 4


def beam_rows(c, items, nb, top_k, top_p, temp, u, short_scratch=False, expect=0):
    """itts_beam_sample_rows on the CPU arrays of a case -> (score, tok, beam [items, 2 nb], kept [items * nb]); checks that no
    input array was modified."""
    l = lib.load()
    rows, V = c["logits"].shape
    assert rows == items * nb
    lg = torch.from_numpy(c["logits"]).to(DEV)
    hist = torch.from_numpy(np.ascontiguousarray(c["hist"])).to(DEV)
    bs = torch.from_numpy(np.ascontiguousarray(c["beam_scores"], dtype=np.float32)).to(DEV)
    uu = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(DEV)
    psc = torch.full((items, 2 * nb), 7.0, dtype=torch.float32, device=DEV)
    ptok = torch.full((items, 2 * nb), -7, dtype=torch.int32, device=DEV)
    pbeam = torch.full((items, 2 * nb), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    nbytes = scratch_bytes(items, nb, V) - (4 if short_scratch else 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    st = l.itts_beam_sample_rows(psc.data_ptr(), ptok.data_ptr(), pbeam.data_ptr(), kept.data_ptr(), lg.data_ptr(), hist.data_ptr(),
                                 c["hist"].shape[1], int(c["k"]), bs.data_ptr(), items, nb, V, float(c["penalty"]), int(c["stop"]),
                                 int(c["suppress"]), int(c["start"]), B.FAKE_ID, int(c["pre"]), int(top_k), float(top_p), float(temp),
                                 uu.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if expect:
        assert st == expect, st
        assert (ptok.cpu().numpy() == -7).all() and (kept.cpu().numpy() == -7).all()  # refused before any launch
        return None
    lib.check(st, "beam_sample_rows", l)
    assert np.array_equal(lg.cpu().numpy().view(np.uint32), c["logits"].view(np.uint32))
    assert np.array_equal(hist.cpu().numpy(), c["hist"]) and np.array_equal(bs.cpu().numpy(), c["beam_scores"])
    return psc.cpu().numpy(), ptok.cpu().numpy(), pbeam.cpu().numpy(), kept.cpu().numpy()


def separated(c, items, nb, refs):
    for bi, (rows, delta, tol) in enumerate(refs):
        for r, row in enumerate(rows):
            B.assert_separated(c, bi * nb + r, row, tol)


@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("shape", B.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("V", B.VOCABS)
def test_operator_results_pass_the_predicate(V, shape, variant):
    items, nb = shape
    c = B.make_case(variant, V, items, nb)
    all_refs = {combo: B.case_refs(c, items, nb, *combo) for combo in B.COMBOS}
    for refs in all_refs.values():  # fp64 only, before the GPU is touched
        separated(c, items, nb, refs)
    checked, dev = 0, 0.0
    for (top_k, top_p, temp), refs in all_refs.items():
        for u in B.uniform_sets(variant, V, items, nb):
            psc, ptok, pbeam, kept = beam_rows(c, items, nb, top_k, top_p, temp, u)
            for bi, (rows, delta, tol) in enumerate(refs):
                sl = slice(bi * nb, (bi + 1) * nb)
                res = B.accepts(rows, c["beam_scores"][sl], V, c["stop"], (psc[bi], ptok[bi], pbeam[bi]), kept[sl], u[bi], delta, tol)
                print(f"V {V} {items}x{nb} {variant} {(top_k, top_p, temp)} item {bi}: kept {list(kept[sl])} max score dev {res.max_dev:.3e} "
                      f"tol {tol:.3e} {res.reason}")
                assert res, (top_k, top_p, temp, bi, res.reason)
                dev = max(dev, res.max_dev / tol)
                checked += 1
    if variant == "stop":
        assert c["stop"] == int(np.argmax(c["logits"][0])) and not (ptok[0][pbeam[0] == 0] == c["stop"]).any()
    assert checked == len(B.COMBOS) * 2 * items
    print(f"largest score deviation / SCORE_TOL: {dev:.3f}")


EQ_STD = {130: 2.5, 1025: 6.0, 8194: 10.0}  # logit spreads at which the fp64 reference alone has the margins asserted below


@pytest.mark.parametrize("shape", B.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("V", B.VOCABS)
def test_operator_equals_the_host_path_where_it_must(V, shape):
    """Gaussian logits; every top-p boundary and every draw at least 100 * DELTA_B from a decision boundary in fp64 (asserted on the
    CPU first; the uniforms come from wide_beam_ref.safe_uniforms, a function of the reference alone): tokens and beams then
    equal infer_core.host_beam_step's exactly, in draw order, scores within SCORE_TOL."""
    items, nb = shape
    c = B.make_case("gauss", V, items, nb, std=EQ_STD[V])
    margin = 100 * B.delta_b(V, nb)
    for top_k, top_p, temp in B.COMBOS:
        refs = B.case_refs(c, items, nb, top_k, top_p, temp)
        separated(c, items, nb, refs)
        u = np.empty((items, 2 * nb), dtype=np.float32)
        for bi, (rows, delta, tol) in enumerate(refs):
            sl = slice(bi * nb, (bi + 1) * nb)
            assert min(r.boundary_margin() for r in rows) >= margin, (top_k, top_p, temp, bi)
            u[bi] = B.safe_uniforms(rows, c["beam_scores"][sl], V, 2 * nb, margin, f"wide_beam.eq.{top_k}.{bi}", V)
            assert B.draw_margin(rows, c["beam_scores"][sl], V, u[bi])[1] >= margin
        hsc, htok, hbeam = infer_core.host_beam_step(c["logits"], c["hist"], c["k"], c["beam_scores"], np.zeros(items, np.int32), nb,
                                                     c["penalty"], temp, top_k, top_p, 0.0, u, c["stop"], False, c["start"], B.FAKE_ID)
        psc, ptok, pbeam, kept = beam_rows(c, items, nb, top_k, top_p, temp, u)
        assert np.array_equal(ptok, htok) and np.array_equal(pbeam, hbeam), (top_k, top_p, temp, ptok, htok, pbeam, hbeam)
        for bi, (rows, delta, tol) in enumerate(refs):
            assert list(kept[bi * nb:(bi + 1) * nb]) == [r.R for r in rows]
            d = float(np.abs(psc[bi].astype(np.float64) - hsc[bi].astype(np.float64)).max())
            print(f"V {V} {items}x{nb} {(top_k, top_p, temp)} item {bi}: |score - host score| {d:.3e} tol {tol:.3e}")
            assert d <= tol


def test_operator_is_deterministic_and_independent_of_the_batch():
    V, items, nb = 8194, 2, 3
    c = B.make_case("gauss", V, items, nb)
    u = B.uniform_sets("gauss", V, items, nb)[1]
    for top_k, top_p, temp in ((0, 0.8, 1.0), (200, 0.8, 1.0), (0, 1.0, 0.7)):
        a = beam_rows(c, items, nb, top_k, top_p, temp, u)
        b = beam_rows(c, items, nb, top_k, top_p, temp, u)
        for x, y in zip(a, b):  # the same call twice: the same bits
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        # the two items at other positions of a batch of three: item 1, item 0, item 1
        perm = [1, 0, 1]
        rows = np.concatenate([np.arange(p * nb, (p + 1) * nb) for p in perm])
        c3 = dict(c, logits=np.ascontiguousarray(c["logits"][rows]), hist=np.ascontiguousarray(c["hist"][rows]),
                  beam_scores=np.ascontiguousarray(c["beam_scores"][rows]))
        d = beam_rows(c3, 3, nb, top_k, top_p, temp, u[perm])
        for pos, p in enumerate(perm):
            for x, y in zip(a[:3], d[:3]):
                assert np.array_equal(x[p].view(np.uint32), y[pos].view(np.uint32)), (top_k, pos)
            assert np.array_equal(a[3][p * nb:(p + 1) * nb], d[3][pos * nb:(pos + 1) * nb])


def test_operator_refuses_what_it_cannot_run():
    """Error status -1 and untouched outputs: no launch happened."""
    c = B.make_case("gauss", 130, 1, 2)
    u = B.uniform_sets("gauss", 130, 1, 2)[0]
    beam_rows(c, 1, 2, 0, 0.0, 1.0, u, expect=-1)  # top_p = 0
    beam_rows(c, 1, 2, 0, 0.8, 0.0, u, expect=-1)  # temperature = 0
    beam_rows(c, 1, 2, 0, 0.8, 1.0, u, short_scratch=True, expect=-1)
    big = dict(c, logits=np.zeros((2, 16385), dtype=np.float32), stop=5, start=6)
    beam_rows(big, 1, 2, 0, 0.8, 1.0, u, expect=-1)  # V = 16385
    c11 = B.make_case("gauss", 130, 1, 11)
    beam_rows(c11, 1, 11, 0, 0.8, 1.0, np.zeros((1, 22), np.float32), expect=-1)  # nb = 11
    c1 = dict(c, logits=c["logits"][:1], hist=c["hist"][:1], beam_scores=c["beam_scores"][:1])
    beam_rows(c1, 1, 1, 0, 0.8, 1.0, np.zeros((1, 2), np.float32), expect=-1)  # nb = 1
    assert beam_rows(c, 1, 2, 0, 0.8, 1.0, u) is not None  # and the library still runs what it can


# ---------------------------------------------------------------- engine level
def beam_state(eng, rows, mg, items):
    hist = np.empty((rows, mg), dtype=np.int32)
    scores = np.empty(rows, dtype=np.float32)
    done = np.empty(items, dtype=np.int32)
    step = C.c_int()
    lib.check(eng.lib.itts_gpt_beam_state(eng.h, hist.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p),
                                          done.ctypes.data_as(C.c_void_p), C.byref(step), eng._s()), "gpt_beam_state", eng.lib)
    return step.value, hist, scores, done


def beam_picks(eng, items, nb):
    psc = np.empty((items, 2 * nb), dtype=np.float32)
    ptok = np.empty((items, 2 * nb), dtype=np.int32)
    pbeam = np.empty((items, 2 * nb), dtype=np.int32)
    kept = np.empty(items * nb, dtype=np.int32)
    lib.check(eng.lib.itts_gpt_beam_picks(eng.h, psc.ctypes.data_as(C.c_void_p), ptok.ctypes.data_as(C.c_void_p),
                                          pbeam.ctypes.data_as(C.c_void_p), kept.ctypes.data_as(C.c_void_p), eng._s()), "gpt_beam_picks",
              eng.lib)
    return psc, ptok, pbeam, kept


def check_beam_steps(eng, cfg, cond, text, n, nb, top_k, top_p, temp, u, penalty=10.0, input_tokens=None, tag="steps"):
    """decode(1) at a time.  Around every step: itts_gpt_beam_state before; behind it the step's logits and itts_gpt_beam_picks.
    The predicate accepts the picks for that state, those logits and u[k]; the next state's beam tokens, scores, histories and
    done flags are what oracle.hf_beam's BeamSearchScorer.process makes of the sorted picks.  -> the final codes."""
    from oracle import hf_beam

    g = cfg.gpt
    V, stop, start = g.number_mel_codes, g.stop_mel_token, g.start_mel_token
    items = text.shape[0]
    rows = items * nb
    input_n = 0 if input_tokens is None else int(np.atleast_2d(input_tokens).shape[1])
    scorer = hf_beam.BeamSearchScorer(items, nb, length_penalty=0.0)
    delta = B.delta_b(V, nb)
    checked, dev = 0, 0.0
    if input_tokens is not None:
        eng.set_input_tokens(input_tokens)
    eng.set_beam_sample(nb, top_k, top_p, temp, u, do_sample=True)
    try:
        pre = (0, np.zeros((rows, n), np.int32), np.zeros(rows, np.float32), np.zeros(items, np.int32))
        for k in range(n):
            if k == 0:
                eng.prefill(cond, text, n, penalty, False)
            else:
                eng.decode(1)
            lg = np.empty((rows, V), dtype=np.float32)
            lib.check(eng.lib.itts_gpt_fetch(eng.h, None, lg.ctypes.data_as(C.c_void_p), eng._s()), "gpt_fetch", eng.lib)
            post = beam_state(eng, rows, n, items)
            k0, hist0, sc0, done0 = pre
            assert (k0, post[0]) == (k, k + 1)
            if k < input_n:  # a given token: every beam takes it, scores and hypotheses untouched
                want = np.atleast_2d(input_tokens)
                for row in range(rows):
                    assert post[1][row, k] == want[(row // nb) % want.shape[0], k]
                assert np.array_equal(post[2], sc0) and not post[3].any()
                pre = post
                continue
            psc, ptok, pbeam, kept = beam_picks(eng, items, nb)
            srt_sc = np.zeros((items, 2 * nb), np.float32)
            srt_tok = np.full((items, 2 * nb), stop, np.int64)
            srt_beam = np.zeros((items, 2 * nb), np.int64)
            for bi in range(items):
                if done0[bi]:
                    continue
                sl = slice(bi * nb, (bi + 1) * nb)
                seen = [{B.FAKE_ID, start} | {int(t) for t in hist0[row, :k]} for row in range(bi * nb, (bi + 1) * nb)]
                rws = B.item_rows(lg[sl], seen, penalty, stop, False, False, top_k, top_p, temp, delta)
                tol = B.score_tol(V, penalty, temp, B.magnitude(rws, sc0[sl]))
                res = B.accepts(rws, sc0[sl], V, stop, (psc[bi], ptok[bi], pbeam[bi]), kept[sl], u[k, bi], delta, tol)
                assert res, (k, bi, res.reason)
                dev = max(dev, res.max_dev / tol)
                checked += 1
                o = np.argsort(-psc[bi].astype(np.float64), kind="stable")  # torch.sort(descending), stable
                srt_sc[bi], srt_tok[bi], srt_beam[bi] = psc[bi][o], ptok[bi][o], pbeam[bi][o]
            ns, nt, ni = scorer.process(hist0[:, :k], srt_sc, srt_tok, srt_beam, stop, stop, input_n)
            for bi in range(items):
                if done0[bi]:
                    assert post[3][bi]
                    continue
                for q in range(nb):
                    row = bi * nb + q
                    assert post[1][row, k] == nt[row] and post[2][row] == ns[row], (k, row)
                    assert np.array_equal(post[1][row, :k], hist0[ni[row], :k]), (k, row)
                assert bool(post[3][bi]) == bool(scorer.done[bi]), (k, bi)
            pre = post
        nstep, _ = eng.status()
        codes = eng.fetch()[:, :nstep].astype(np.int64)
        eng._exit()
    finally:
        eng.set_beam_sample(1)
        if input_tokens is not None:
            eng.set_input_tokens(None)
    MAX_DEV[tag] = dev
    print(f"{tag}: {checked} item steps accepted, largest score deviation / SCORE_TOL {dev:.3f}")
    return codes, checked


@pytest.fixture(scope="module")
def micro(gold):
    cfg = icfg.micro()
    eng = ieng.build_engine(cfg, "fp32", parts=("gpt",))
    cond = eng.conditioning(torch.from_numpy(gold("micro_conditioning")["mel"]))
    text = np.concatenate([gold("micro_decode_b1")["text"], gold("micro_decode_b1_alt")["text"]], 0).astype(np.int32)
    return cfg, eng, cond, text


def well_formed(codes, V, stop, rows, n):
    assert codes.dtype == np.int64 and codes.shape[0] == rows and 1 <= codes.shape[1] <= n
    assert ((codes >= 0) & (codes < V)).all()
    for r in range(rows):  # behind a row's first stop token everything is stop
        hit = np.nonzero(codes[r] == stop)[0]
        assert not len(hit) or (codes[r, hit[0]:] == stop).all()
    if codes.shape[1] < n:  # trimmed: every row has stopped, and one of them in the last column
        assert (codes[:, -1] == stop).any() and all((codes[r] == stop).any() for r in range(rows))


def test_set_beams_accepts_topk_off_and_wide(micro):
    """The C ABI: itts_gpt_set_beams(do_sample, top_k = 0) was E_INVALID before the whole-vocabulary beam sampler existed."""
    cfg, eng, cond, text = micro
    u = np.zeros(64, dtype=np.float32)
    for top_k in (0, -1, 129, 100000):
        assert eng.lib.itts_gpt_set_beams(eng.h, 3, 1, top_k, 0.8, 1.0, 0.0, u.ctypes.data_as(C.c_void_p), u.size) == 0
    assert eng.lib.itts_gpt_set_beams(eng.h, 3, 1, 0, 0.0, 1.0, 0.0, u.ctypes.data_as(C.c_void_p), u.size) == -1  # top_p stays checked
    assert eng.lib.itts_gpt_set_beams(eng.h, 3, 1, 0, 0.8, 1.0, 0.0, None, 0) == -1  # and the uniforms
    eng.set_beam_sample(1)
    assert eng.lib.itts_gpt_beam_picks(eng.h, None, None, None, None, None) == -4  # no wide beam generation is active


def test_micro_steps_pass_the_predicate_and_generate_returns_them(micro):
    """fp32 micro model, 3 beams x 2 items, 12 steps, top_k = 0, top_p = 0.8, temperature = 0.9."""
    cfg, eng, cond, text = micro
    V, stop = cfg.gpt.number_mel_codes, cfg.gpt.stop_mel_token
    n, nb = 12, 3
    u = np.random.default_rng(43).random((n, 2, 2 * nb), dtype=np.float32)
    u[3, 0, 1], u[4, 1, 0] = 0.0, B.U_TOP
    stepped, checked = check_beam_steps(eng, cfg, cond, text, n, nb, 0, 0.8, 0.9, u, tag="micro fp32 steps")
    assert checked >= 12
    kw = dict(do_sample=True, num_beams=nb, top_k=0, top_p=0.8, temperature=0.9, uniforms=u, wide_beam_sampler="device")
    one = eng.generate(cond, text, n, **kw)
    well_formed(one, V, stop, 2, n)
    m = min(one.shape[1], stepped.shape[1])
    assert np.array_equal(one[:, :m], stepped[:, :m]) and (stepped[:, m:] == stop).all()
    three = eng.generate(cond, text, n, num_return_sequences=3, **kw)
    well_formed(three, V, stop, 6, n)
    m = min(one.shape[1], three.shape[1])
    assert np.array_equal(three[0::3, :m], one[:, :m])  # best first
    # top_k = None is top_k = 0; the default and "host" are the host path, unchanged
    assert np.array_equal(one, eng.generate(cond, text, n, **dict(kw, top_k=None)))
    host = eng.generate(cond, text, n, **dict(kw, wide_beam_sampler=None))
    assert np.array_equal(host, eng.generate(cond, text, n, **dict(kw, wide_beam_sampler="host")))


def test_item_that_finishes_early_keeps_its_hypotheses(gold):
    """Eos enabled on a micro checkpoint whose mel_head.bias[stop] is raised: the first draw set (of a fixed list) with which one
    item is done while the other still runs; the finished item's finalized hypotheses then stay what they were through the later
    steps, and generate() returns them."""
    cfg = icfg.micro()
    stop, V = cfg.gpt.stop_mel_token, cfg.gpt.number_mel_codes
    n, nb, items = 20, 3, 2
    found = None
    for stop_bias in (3.0, 5.0, 7.0):
        eng = ieng.build_engine(cfg, "fp32", parts=("gpt",), state_dicts={"gpt": synth.gpt_state_dict(cfg, 1234, stop_bias=stop_bias)})
        cond = eng.conditioning(torch.from_numpy(gold("micro_conditioning")["mel"]))
        text = np.concatenate([gold("micro_decode_b1")["text"], gold("micro_decode_b1_alt")["text"]], 0).astype(np.int32)
        for seed in range(6):
            u = np.random.default_rng(100 + seed).random((n, items, 2 * nb), dtype=np.float32)
            eng.set_beam_sample(nb, 0, 0.8, 1.0, u, do_sample=True, num_return_sequences=nb)
            try:
                eng.prefill(cond, text, n, 10.0, False)
                snap = None
                for k in range(1, n):
                    _, _, _, done = beam_state(eng, items * nb, n, items)
                    if snap is None and done.any() and not done.all():
                        snap = (k, done.copy(), eng.fetch().copy())
                    if done.all():
                        break
                    eng.decode(1)
                final = eng.fetch().copy()
                eng._exit()
            finally:
                eng.set_beam_sample(1)
            if snap is not None and k > snap[0]:
                found = (stop_bias, seed, snap, final, k)
                break
        if found:
            break
    assert found, "no draw set of the list lets one item finish while the other runs"
    stop_bias, seed, (k1, done1, codes1), final, k2 = found
    print(f"stop_bias {stop_bias} seed {seed}: item(s) {np.nonzero(done1)[0]} done at step {k1}, generation ended at step {k2}")
    for bi in np.nonzero(done1)[0]:
        assert np.array_equal(codes1[bi * nb:(bi + 1) * nb], final[bi * nb:(bi + 1) * nb])
    got = eng.generate(cond, text, n, do_sample=True, num_beams=nb, top_k=0, top_p=0.8, temperature=1.0, uniforms=u,
                       num_return_sequences=nb, wide_beam_sampler="device")
    well_formed(got, V, stop, items * nb, n)
    assert np.array_equal(got, final[:, :got.shape[1]].astype(np.int64)) and (final[:, got.shape[1]:] == stop).all()


# ---- bf16 engine at IndexTTS-1.5 sizes: 3 beams x 2 items = 6 rows on the persistent engine ----
@pytest.fixture(scope="module")
def mel():
    return torch.from_numpy(synth.prompt_mel(511, seed=7))


@pytest.fixture(scope="module")
def eng16():
    return ieng.build_engine(CFG, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def text2():
    return np.stack([synth.text_ids(40, 21 + i, CFG.gpt.number_text_tokens) for i in range(2)]).astype(np.int32)


def run_beams(eng, cond, text, n, top_k, u, no_graph=False, typical=0.0):
    eng.debug(no_graph=no_graph)
    try:
        ids = eng.generate(cond, text, n, suppress_stop=True, do_sample=True, num_beams=3, top_k=top_k, top_p=0.8, temperature=0.9,
                           uniforms=u, typical_mass=typical, wide_beam_sampler="device")
        mode = eng.decode_mode()
    finally:
        eng.debug()
    return ids, mode


@pytest.mark.parametrize("top_k", [0, 200])
def test_bf16_graph_replay_equals_eager_on_the_persistent_engine(eng16, mel, text2, top_k):
    cond = eng16.conditioning(mel)
    u = np.random.default_rng(23).random((24, 2, 6), dtype=np.float32)
    V = CFG.gpt.number_mel_codes
    for _ in range(2):  # twice in a row on one engine object
        a, mode_a = run_beams(eng16, cond, text2, 24, top_k, u)
        b, mode_b = run_beams(eng16, cond, text2, 24, top_k, u, no_graph=True)
        assert (mode_a, mode_b) == (1, 1)  # the three sampler launches run behind the persistent engine
        assert a.shape[0] == 2 and np.array_equal(a, b) and ((a >= 0) & (a < V)).all()


def test_bf16_graph_key_tells_the_beam_samplers_apart(eng16, mel, text2):
    cond = eng16.conditioning(mel)
    u = np.random.default_rng(29).random((16, 2, 6), dtype=np.float32)
    first, _ = run_beams(eng16, cond, text2, 16, 30, u)
    wide, _ = run_beams(eng16, cond, text2, 16, 0, u)
    third, _ = run_beams(eng16, cond, text2, 16, 30, u)
    assert np.array_equal(first, third)
    assert not np.array_equal(first, wide)  # (a nucleus of 30 against the whole vocabulary's)


def test_bf16_typical_filter_composes(eng16, mel, text2):
    cond = eng16.conditioning(mel)
    u = np.random.default_rng(31).random((16, 2, 6), dtype=np.float32)
    V = CFG.gpt.number_mel_codes
    a, _ = run_beams(eng16, cond, text2, 16, 0, u, typical=0.5)
    b, _ = run_beams(eng16, cond, text2, 16, 0, u, typical=0.5)
    plain, _ = run_beams(eng16, cond, text2, 16, 0, u)
    assert np.array_equal(a, b) and ((a >= 0) & (a < V)).all()
    assert not np.array_equal(a, plain)  # the filter changes the distribution


def test_bf16_input_tokens_are_forced_into_every_beam(eng16, mel, text2):
    """An `input_tokens` prefix of 3 tokens: the wide kernels leave those steps alone (beam_select_kernel takes the given token for
    every beam), the steps after it pass the predicate on the engine's own logits."""
    cond = eng16.conditioning(mel)
    n, nb = 8, 3
    u = np.random.default_rng(37).random((n, 2, 2 * nb), dtype=np.float32)
    given = np.asarray([[11, 222, 3333]], dtype=np.int32)
    codes, checked = check_beam_steps(eng16, CFG, cond, text2, n, nb, 0, 0.8, 0.9, u, input_tokens=given, tag="bf16 1.5 steps behind input_tokens")
    assert checked == (n - 3) * 2
