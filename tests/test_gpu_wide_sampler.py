"""GPU: the whole-vocabulary device sampler (csrc/decode_sampler.hip sampler_wide_kernel: do_sample with top_k = 0 / None or
> 128) - at the operator level through itts_sample_rows, and inside the engine's decode step.

What a result has to satisfy is wide_sampler_ref.Ref: the fp64 restatement of HF 4.36.2's warpers and the inverse-CDF draw,
with the tolerance delta = 64 * 2^-24 derived from the kernel's longest chain of dependent fp32 additions (53) - no case is
skipped.  The operator tests draw their logits on the CPU (itts_hip/prng.py), so the fp64 side needs no GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_sampler_ref as W  # noqa: E402

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core, lib, prng, synth  # noqa: E402

CFG = icfg.indextts_1_5()
U_TOP = float(np.nextafter(np.float32(1), np.float32(0)))  # the largest float below 1


# ---------------------------------------------------------------- operator level
def sample_rows(logits, seen, penalty, stop, suppress_stop, preprocessed, top_k, top_p, temperature, u):
    """itts_sample_rows on CPU arrays -> (tok [B], kept [B]); checks that no input array was modified."""
    l = lib.load()
    B, V = logits.shape
    dev = "cuda:0"
    lg = torch.from_numpy(logits).to(dev)
    sn = torch.from_numpy(seen).to(dev) if seen is not None else None
    uu = torch.from_numpy(np.asarray(u, dtype=np.float32)).to(dev)
    tok = torch.full((B,), -7, dtype=torch.int32, device=dev)
    kept = torch.full((B,), -7, dtype=torch.int32, device=dev)
    scratch = torch.empty(B * (V + 16), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = l.itts_sample_rows(tok.data_ptr(), kept.data_ptr(), lg.data_ptr(), sn.data_ptr() if sn is not None else None, B, V,
                            float(penalty), int(stop), int(suppress_stop), int(preprocessed), int(top_k), float(top_p),
                            float(temperature), uu.data_ptr(), scratch.data_ptr(), scratch.numel(),
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(st, "sample_rows", l)
    torch.cuda.synchronize()
    assert np.array_equal(lg.cpu().numpy().view(np.uint32), logits.view(np.uint32))
    if sn is not None:
        assert np.array_equal(sn.cpu().numpy(), seen)
    return tok.cpu().numpy(), kept.cpu().numpy()


def gaussian(name, seed, shape, std):
    """prng.py has uniforms only: the sum of 12 of them in (-1, 1) has variance 4 and is gaussian enough (Irwin-Hall)."""
    n = int(np.prod(shape))
    return (prng.uniform(name, seed, 12 * n).reshape(n, 12).sum(1) * np.float32(std / 2)).reshape(shape).astype(np.float32)


def make_case(variant, V, B):
    """-> logits [B, V], seen bytes or None, penalty, stop, suppress_stop, preprocessed"""
    lg = gaussian(f"wide_sampler.{variant}", V, (B, V), 2.5)
    seen, penalty, stop, suppress, pre = None, 1.0, V - 2, 0, 0
    if variant == "ties":  # multiples of 0.25: many exact ties (tie order, HF's tie-keeping TopK)
        lg = (np.round(lg * 4) / 4).astype(np.float32)
    elif variant == "few_finite":  # preprocessed rows, all but 40 entries -inf: fewer finite scores than top_k
        keep = np.zeros((B, V), dtype=bool)
        for b in range(B):
            keep[b, np.argsort(prng.uniform(f"wide_sampler.keep{b}", V, V), kind="stable")[:40]] = True
        lg = np.where(keep, lg, np.float32(-np.inf)).astype(np.float32)
        pre = 1
    elif variant == "seen":
        seen = np.zeros((B, V), dtype=np.uint8)
        for b in range(B):
            seen[b, prng.randint(f"wide_sampler.seen{b}", V, 60, 0, V)] = 1
            seen[b, np.argsort(lg[b])[-3:]] = 1  # the best tokens among them
        penalty = 10.0
    elif variant == "stop":  # the stop token is the arg-max of row 0 and suppressed
        stop = int(np.argmax(lg[0]))
        suppress = 1
    return np.ascontiguousarray(lg), seen, penalty, stop, suppress, pre


@pytest.mark.parametrize("variant", ["gauss", "ties", "few_finite", "seen", "stop"])
@pytest.mark.parametrize("V", [129, 1024, 1025, 8194])
def test_operator_results_pass_the_predicate(V, variant):
    from oracle import gpt as ogpt

    lg, seen, penalty, stop, suppress, pre = make_case(variant, V, 3)
    u_rand = np.minimum(prng.uniform(f"wide_sampler.u.{variant}", V, 6) * np.float32(0.5) + np.float32(0.5), np.float32(U_TOP))
    u_sets = [np.asarray([u_rand[0], 0.0, U_TOP], dtype=np.float32), u_rand[3:6].copy()]
    refs = {}
    checked = 0
    for top_k in (0, 129, V - 1, V, V + 5):
        for top_p in (1.0, 0.8, 1e-6):
            for temp in (1.0, 0.3):
                sc = [W.sampler_scores(lg[b], np.nonzero(seen[b])[0] if seen is not None else (), penalty, stop, suppress, pre, temp)
                      for b in range(3)]
                for ui, u in enumerate(u_sets):
                    tok, kept = sample_rows(lg, seen, penalty, stop, suppress, pre, top_k, top_p, temp, u)
                    if 1 <= top_k <= 128:  # (V - 1 at V = 129) the narrow kernel's: its own oracle, exactly; kept is not reported
                        raw = [W.sampler_scores(lg[b], np.nonzero(seen[b])[0] if seen is not None else (), penalty, stop, suppress, pre)
                               for b in range(3)]
                        assert (kept == -1).all()
                        assert [int(t) for t in tok] == [ogpt.sample_pick(raw[b], top_k, top_p, temp, float(u[b])) for b in range(3)]
                        checked += 3
                        continue
                    for b in range(3):
                        key = (b, top_k if 1 <= top_k < V else 0, top_p, temp)  # top_k >= V keeps what TopK off keeps
                        if key not in refs:
                            refs[key] = W.Ref(sc[b], top_k, top_p)
                        ref = refs[key]
                        assert 0 <= tok[b] < V and sc[b][tok[b]] > -np.inf, (top_k, top_p, temp, b, tok[b])
                        assert ref.accepts(tok[b], u[b], kept[b]), (top_k, top_p, temp, b, tok[b], kept[b], ref.R_lo, ref.R_hi)
                        if top_p == 1e-6:
                            assert kept[b] == 1 and tok[b] == int(ref.order[0])  # only the best token stays
                        checked += 1
                    if ui == 0:
                        tok2, kept2 = sample_rows(lg, seen, penalty, stop, suppress, pre, top_k, top_p, temp, u)
                        assert np.array_equal(tok, tok2) and np.array_equal(kept, kept2)  # the same call twice: the same bits
                        for b in range(3):  # a row alone (B = 1) equals the row inside the 3-row call
                            t1, k1 = sample_rows(lg[b:b + 1].copy(), seen[b:b + 1].copy() if seen is not None else None, penalty, stop,
                                                 suppress, pre, top_k, top_p, temp, u[b:b + 1])
                            assert (t1[0], k1[0]) == (tok[b], kept[b]), (top_k, top_p, temp, b)
    if variant == "stop":
        assert stop == int(np.argmax(lg[0]))
    assert checked == 5 * 3 * 2 * 2 * 3


def test_operator_narrow_path_equals_the_oracle():
    """top_k = 30 through the same entry point is sampler_sample_kernel as before: ogpt.sample_pick exactly; kept = -1."""
    from oracle import gpt as ogpt

    lg = gaussian("wide_sampler.narrow", 3, (3, 8194), 2.5)
    u = np.asarray([0.37, 0.0, U_TOP], dtype=np.float32)
    tok, kept = sample_rows(lg, None, 1.0, 8193, 0, 0, 30, 0.8, 0.9, u)
    assert (kept == -1).all()
    for b in range(3):
        assert tok[b] == ogpt.sample_pick(lg[b].copy(), 30, 0.8, 0.9, float(u[b])), b


def test_operator_refuses_what_it_cannot_run():
    l = lib.load()
    t = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    big = torch.zeros(16385 + 64, dtype=torch.float32, device="cuda:0")
    sc = torch.empty(16385 + 64, dtype=torch.uint8, device="cuda:0")
    args = (1.0, 5, 0, 0, 0, 0.8, 1.0, big.data_ptr(), sc.data_ptr())
    assert l.itts_sample_rows(t.data_ptr(), t.data_ptr(), big.data_ptr(), None, 1, 16385, *args, sc.numel(), None) == -1  # V > 16384
    assert l.itts_sample_rows(t.data_ptr(), t.data_ptr(), big.data_ptr(), None, 1, 1024, *args, 1024, None) == -1  # scratch too small
    torch.cuda.synchronize()


# ---------------------------------------------------------------- engine level
@pytest.fixture(scope="module")
def mel():
    return torch.from_numpy(synth.prompt_mel(511, seed=7))


@pytest.fixture(scope="module")
def eng32():
    return ieng.build_engine(CFG, "fp32", parts=("gpt",))


@pytest.fixture(scope="module")
def eng16():
    return ieng.build_engine(CFG, "bf16", parts=("gpt",))


def check_steps(eng, cfg, cond, text, n, top_k, top_p, temp, u, penalty=10.0):
    """decode(1) at a time: the token of every step passes the predicate on the engine's own logits of that step, the penalty
    set rebuilt from the engine's own ids (kept is not visible here: any R' in [R_lo, R_hi]).  -> ids, picks equal to
    infer_core.host_sample_step on the same logits, picks compared."""
    stop, start = cfg.gpt.stop_mel_token, cfg.gpt.start_mel_token
    B = text.shape[0]
    agree = total = 0
    eng.set_sampling(True, top_k, top_p, temp, u)
    try:
        eng.prefill(cond, text, n, penalty, False)
        for k in range(n):
            codes, lg = eng.fetch(logits=True)
            for b in range(B):
                if k > 0 and (codes[b, :k] == stop).any():
                    continue
                seen = {1, start} | {int(t) for t in codes[b, :k]}  # fake ids are 1 (model.py:645)
                s = W.sampler_scores(lg[b], seen, penalty, stop, False, False, temp)
                ref = W.Ref(s, top_k, top_p)
                assert ref.accepts(codes[b, k], u[k, b]), (k, b, int(codes[b, k]), ref.R_lo, ref.R_hi)
                host = infer_core.host_sample_step(lg[b:b + 1], [seen], penalty, temp, top_k, top_p, 0.0, u[k, b:b + 1], stop, False)
                agree += int(host[0]) == int(codes[b, k])
                total += 1
            if k + 1 < n:
                eng.decode(1)
        eng._exit()
    finally:
        eng.set_sampling(False)
    return codes[:, :n].copy(), agree, total


def test_set_sampling_accepts_topk_off_and_wide():
    """The C ABI: itts_gpt_set_sampling(top_k = 0) was E_INVALID before the whole-vocabulary sampler existed."""
    eng = ieng.build_engine(icfg.micro(), "fp32", parts=("gpt",))
    u = np.zeros(8, dtype=np.float32)
    for top_k in (0, -1, 129, 100000):
        assert eng.lib.itts_gpt_set_sampling(eng.h, 1, top_k, 0.8, 1.0, u.ctypes.data_as(C.c_void_p), u.size) == 0
    assert eng.lib.itts_gpt_set_sampling(eng.h, 1, 0, 0.0, 1.0, u.ctypes.data_as(C.c_void_p), u.size) == -1  # top_p stays checked
    eng.set_sampling(False)
    assert callable(eng.lib.itts_sample_rows)


def test_full_wide_sampling_steps_pass_the_predicate_fp32(eng32, mel, gold):
    """IndexTTS-1.5 sizes (V = 8194), fp32, 2 rows, 12 steps, top_k = 0, top_p = 0.8, temperature = 0.9."""
    g = gold("full_decode_b1")
    cond = eng32.conditioning(mel)
    text = np.concatenate([g["text"], g["text"]], 0)
    n = 12
    u = np.random.default_rng(5).random((n, 2), dtype=np.float32)
    u[3, 0], u[4, 1] = 0.0, U_TOP
    codes, agree, total = check_steps(eng32, CFG, cond, text, n, 0, 0.8, 0.9, u)
    print(f"wide sampler, fp32 1.5 sizes: {agree} of {total} picks equal infer_core.host_sample_step on the same logits")
    assert total == 24
    assert (codes[0] != codes[1]).any()  # two rows, same text, different draws


def test_micro_generate_on_the_device(gold):
    """fp32 micro config, the two texts of test_sampling_with_topk_off_runs_on_the_host_exactly, 20 steps: the step-by-step
    check, and generate(wide_sampler="device") returns the same ids as that stepped run, well formed (stop fill, trimming)."""
    cfg = icfg.micro()
    eng = ieng.build_engine(cfg, "fp32", parts=("gpt",))
    g = gold("micro_decode_b1")
    cond = eng.conditioning(torch.from_numpy(gold("micro_conditioning")["mel"]))
    text = np.concatenate([g["text"], gold("micro_decode_b1_alt")["text"]], 0).astype(np.int32)
    V, stop = cfg.gpt.number_mel_codes, cfg.gpt.stop_mel_token
    u = np.random.default_rng(17).random((20, 2), dtype=np.float32)
    stepped, agree, total = check_steps(eng, cfg, cond, text, 20, 0, 0.8, 0.9, u)
    print(f"wide sampler, fp32 micro: {agree} of {total} picks equal infer_core.host_sample_step on the same logits")
    got = eng.generate(cond, text, 20, do_sample=True, top_k=0, top_p=0.8, temperature=0.9, uniforms=u, wide_sampler="device")
    assert got.dtype == np.int64 and got.shape[0] == 2 and 1 <= got.shape[1] <= 20
    assert ((got >= 0) & (got < V)).all()
    assert np.array_equal(got, stepped[:, : got.shape[1]])
    for r in range(2):  # behind a row's first stop token everything is stop
        hit = np.nonzero(got[r] == stop)[0]
        assert not len(hit) or (got[r, hit[0]:] == stop).all()
    if got.shape[1] < 20:  # trimmed: the last column is where the last running row stopped
        assert (got[:, -1] == stop).any() and all((got[r] == stop).any() for r in range(2))
    # the default and "host" are the host path, unchanged
    host = eng.generate(cond, text, 20, do_sample=True, top_k=0, top_p=0.8, temperature=0.9, uniforms=u)
    assert np.array_equal(host, eng.generate(cond, text, 20, do_sample=True, top_k=0, top_p=0.8, temperature=0.9, uniforms=u,
                                             wide_sampler="host"))


def run_sampled(eng, cond, text, n, top_k, u, no_graph=False, typical=0.0):
    eng.debug(no_graph=no_graph)
    try:
        ids = eng.generate(cond, text, n, suppress_stop=True, do_sample=True, top_k=top_k, top_p=0.8, temperature=0.9, uniforms=u,
                           typical_mass=typical, wide_sampler="device")
        mode = eng.decode_mode()
    finally:
        eng.debug()
    return ids, mode


@pytest.fixture(scope="module")
def text2():
    return np.stack([synth.text_ids(40, 21 + i, CFG.gpt.number_text_tokens) for i in range(2)]).astype(np.int32)


@pytest.mark.parametrize("top_k", [0, 200])
def test_bf16_graph_replay_equals_eager_on_the_persistent_engine(eng16, mel, text2, top_k):
    cond = eng16.conditioning(mel)
    u = np.random.default_rng(23).random((24, 2), dtype=np.float32)
    V = CFG.gpt.number_mel_codes
    for _ in range(2):  # twice in a row on one engine object
        a, mode_a = run_sampled(eng16, cond, text2, 24, top_k, u)
        b, mode_b = run_sampled(eng16, cond, text2, 24, top_k, u, no_graph=True)
        assert (mode_a, mode_b) == (1, 1)  # the sampler is a launch of its own behind the persistent engine
        assert a.shape == (2, 24) and np.array_equal(a, b) and ((a >= 0) & (a < V)).all()


def test_bf16_graph_key_tells_the_samplers_apart(eng16, mel, text2):
    cond = eng16.conditioning(mel)
    u = np.random.default_rng(29).random((16, 2), dtype=np.float32)
    first, _ = run_sampled(eng16, cond, text2, 16, 30, u)
    wide, _ = run_sampled(eng16, cond, text2, 16, 0, u)
    third, _ = run_sampled(eng16, cond, text2, 16, 30, u)
    assert np.array_equal(first, third)
    assert not np.array_equal(first, wide)  # (a nucleus of 30 against the whole vocabulary's)


def test_bf16_typical_filter_composes(eng16, mel, text2):
    cond = eng16.conditioning(mel)
    u = np.random.default_rng(31).random((16, 2), dtype=np.float32)
    V = CFG.gpt.number_mel_codes
    a, _ = run_sampled(eng16, cond, text2, 16, 0, u, typical=0.7)
    b, _ = run_sampled(eng16, cond, text2, 16, 0, u, typical=0.7)
    plain, _ = run_sampled(eng16, cond, text2, 16, 0, u)
    assert np.array_equal(a, b) and ((a >= 0) & (a < V)).all()
    assert not np.array_equal(a, plain)  # the filter changes the distribution


def test_eos_row_that_stops_early_is_filled_and_reported(mel, gold):
    """Eos enabled on the checkpoint whose mel_head.bias[stop] is raised (tests/test_gpu_shipped_path.py): row 0 draws with u = 0
    throughout - rank 0, the greedy choice - so it stops where the reference's greedy row stops; row 1 draws at random."""
    g3 = gold("smooth_eos_b3")
    sd = synth.gpt_state_dict(CFG, 1234, profile="smooth", stop_bias=float(g3["stop_bias"]))
    eng = ieng.build_engine(CFG, "fp32", parts=("gpt",), state_dicts={"gpt": sd})
    stop = CFG.gpt.stop_mel_token
    cond = eng.conditioning(mel)
    text = g3["text"][:2].astype(np.int32)
    k0 = int(g3["stop_steps"][0])
    n = min(64, k0 + 9)
    u = np.random.default_rng(37).random((n, 2), dtype=np.float32)
    u[:, 0] = 0.0
    eng.set_sampling(True, 0, 0.8, 1.0, u)
    try:
        eng.prefill(cond, text, n, 10.0, False)
        eng.decode(n - 1)
        step, unf = eng.status()
        codes = eng.fetch()
        eng._exit()
    finally:
        eng.set_sampling(False)
    assert step == n
    assert np.array_equal(codes[0, : k0 + 1], g3["codes"][0, : k0 + 1]) and codes[0, k0] == stop
    assert (codes[0, k0:] == stop).all()  # filled with stop behind it
    running = sum(1 for r in range(2) if not (codes[r] == stop).any())
    assert unf == running and unf <= 1  # status() reports row 0 finished
    full = eng.generate(cond, text, n, do_sample=True, top_k=0, top_p=0.8, temperature=1.0, uniforms=u, wide_sampler="device")
    assert np.array_equal(full, codes[:, : full.shape[1]]) and (full[0, k0:] == stop).all()
