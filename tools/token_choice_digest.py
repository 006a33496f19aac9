"""One SHA-256 per output buffer of the token-choice operator entries (itts_sampler_step, itts_sample_rows, itts_beam_step,
itts_beam_sample_rows, itts_typical_rows) on the inputs of the test generators, in a fixed order: two builds of the library
compute the same bits exactly when their outputs are the same text.

  ITTS_HIP_LIB=index-tts-ipex_amd/csrc/<library>.so python tools/token_choice_digest.py > <library>.digest

Inputs and launch helpers are the tests' own (tests/token_choice_ref.py, wide_beam_ref.py, and run_sampler, run_step, beam_rows,
sample_rows, run_typical, make_case of tests/test_gpu_*.py): the tool is coupled to those helpers' signatures and moves with
them.  Nothing is compared with a reference here."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "index-tts-ipex_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_beam_step as BS  # noqa: E402
import test_gpu_sampler_step as SS  # noqa: E402
import test_gpu_typical_filter as TF  # noqa: E402
import test_gpu_wide_beam as WB  # noqa: E402
import test_gpu_wide_sampler as WS  # noqa: E402
import token_choice_ref as T  # noqa: E402
import wide_beam_ref as W  # noqa: E402

F32 = np.float32
SHAPES = [(1, 2), (2, 3), (1, 10)]  # (items, beams)


def emit(case, **bufs):
    for name in sorted(bufs):
        print(f"{case} {name} {hashlib.sha256(np.ascontiguousarray(bufs[name]).tobytes()).hexdigest()}")


def narrow_sampler():
    """sampler_sample_kernel (and sampler2_kernel at do_sample 0) through itts_sampler_step: the whole state after one launch."""
    for V in (66, 1025, 8194, 15360):
        B, max_gen = 3, 2
        lg = W.gaussian("digest.narrow", V, (B, V), 2.5)
        seen = np.zeros((B, V), bool)
        for b in range(B):
            seen[b, np.argsort(lg[b])[-3:]] = True
        u = np.array([[0.0, 0.37, W.U_TOP], [0.5, 0.5, 0.5]], F32)
        emit(f"sampler_step greedy V{V}", **SS.run_sampler(SS.new_state(B, V, max_gen, seen=seen), dict(max_gen=max_gen, stop=V - 2), lg))
        for top_k in (1, 30, 128):
            for top_p in (0.8, 1.0):
                for pre in (0, 1):
                    cfg = dict(max_gen=max_gen, stop=V - 2, penalty=10.0, pre=pre, do_sample=1, top_k=top_k, top_p=top_p, temperature=0.9)
                    got = SS.run_sampler(SS.new_state(B, V, max_gen, seen=seen), cfg, lg, u)
                    emit(f"sampler_step V{V} k{top_k} p{top_p} pre{pre}", **got)
                    tok, kept = WS.sample_rows(lg, seen.astype(np.uint8), 10.0, V - 2, 0, pre, top_k, top_p, 0.9, u[0])
                    emit(f"sample_rows V{V} k{top_k} p{top_p} pre{pre}", tok=tok, kept=kept)
    # more than 128 scores tie with the top_k-th: test_gpu_sampler_step.test_overflow_of_the_candidates_is_deterministic
    V = 8194
    lg = np.zeros((2, V), F32)
    lg[0, 8000] = 2.0
    big = 8193 - 61 * np.arange(127)
    lg[1] = -30.0
    lg[1, big], lg[1, np.setdiff1d(17 + 160 * np.arange(51), big)[:50]] = 9.0, 0.5
    for top_k, u_row in ((30, [0.0, 0.0]), (128, [0.0, W.U_TOP])):
        cfg = dict(V=V, max_gen=1, stop=V - 2, penalty=1.0, do_sample=1, top_k=top_k, top_p=1.0, temperature=1.0)
        emit(f"sampler_step overflow k{top_k}", **SS.run_sampler(SS.new_state(2, V, 1), cfg, lg, np.array([u_row], F32)))


def beam_state(c, cfg, items, nb, k):
    return T.new_state(items, nb, cfg["max_gen"], cfg["Smax"], k, 0, c["beam_scores"], c["hist"],
                       np.tile(np.arange(nb, dtype=np.uint8)[:, None], (items, cfg["Smax"])))


def narrow_beams():
    """beam_cand_kernel + beam_select_kernel through itts_beam_step (mode 0): the state and the candidate scratch."""
    for V in (66, 1025, 8194, 15000):  # (15000: the largest vocabulary beam_sample_step takes on this path)
        for items, nb in SHAPES:
            for variant in ("gauss", "seen"):  # "seen": a history of 60 ids, 61 at three beams - both parities of the step count
                c = W.make_case(variant, V, items, nb)
                k = int(c["k"]) + (1 if (variant == "seen" and nb == 3) else 0)
                if k > int(c["k"]):
                    c["hist"][:, k - 1] = (np.arange(items * nb) * 7 + 5) % (V - 4)
                u = W.uniform_sets(variant, V, items, nb)[1]
                for do_sample, top_k, top_p, pre in [(1, tk, tp, pr) for tk in (1, 30, 128) for tp in (0.8, 1.0) for pr in (0, 1)] + [(0, 0, 1.0, 0)]:
                    cfg = BS.narrow_cfg(dict(c, pre=pre), items, nb, V, k, top_k=top_k, top_p=top_p, temperature=0.9, do_sample=do_sample)
                    uni = np.zeros((cfg["max_gen"], items, 2 * nb), F32)
                    uni[k] = u
                    got, cands = BS.run_step(beam_state(c, cfg, items, nb, k), cfg, 0, logits=c["logits"], uniforms=uni)
                    emit(f"beam_step V{V} {items}x{nb} {variant} s{do_sample} k{top_k} p{top_p} pre{pre}", cand_sc=cands[0], cand_tok=cands[1],
                         cand_n=cands[2], **got)
    # the overflow cases of test_gpu_beam_step.test_overflow_of_the_candidates_is_deterministic
    V, items, nb = 8194, 1, 2
    for name, top_k in (("one", 30), ("many", 128)):
        lg = np.zeros((nb, V), F32)
        if name == "one":
            lg[:, 8000] = 2.0
        else:
            big = 8193 - 61 * np.arange(127)
            lg[:] = -30.0
            lg[:, big] = 1.0 + (np.arange(127) % 7).astype(F32)
            lg[:, np.setdiff1d(17 + 160 * np.arange(51), big)[:50]] = 0.5
        c = dict(logits=lg, hist=np.zeros((nb, 4), np.int32), k=0, beam_scores=np.array([0, -0.5], F32), penalty=1.0, stop=V - 2,
                 start=V - 3, suppress=0, pre=0)
        cfg = BS.narrow_cfg(c, items, nb, V, 0, top_k=top_k, top_p=1.0, temperature=1.0, do_sample=1)
        st = T.new_state(items, nb, cfg["max_gen"], cfg["Smax"], 0, 0, c["beam_scores"], None, np.zeros((nb, cfg["Smax"]), np.uint8))
        got, cands = BS.run_step(st, cfg, 0, logits=lg, uniforms=np.full((cfg["max_gen"], items, 2 * nb), 0.5, F32))
        emit(f"beam_step overflow {name}", cand_sc=cands[0], cand_tok=cands[1], cand_n=cands[2], **got)


def wide():
    """sampler_wide_kernel through itts_sample_rows, beam_wide_cand_kernel + beam_wide_pick_kernel through itts_beam_sample_rows."""
    for V in (129, 1024, 1025, 8194, 16384):
        for variant in ("gauss", "ties", "few_finite", "seen"):
            lg, seen, penalty, stop, suppress, pre = WS.make_case(variant, V, 3)
            u = np.asarray([0.37, 0.0, W.U_TOP], F32)
            for top_k in (0, 200):
                for top_p, temp in ((0.8, 1.0), (1.0, 0.7)):
                    tok, kept = WS.sample_rows(lg, seen, penalty, stop, suppress, pre, top_k, top_p, temp, u)
                    emit(f"sample_rows wide V{V} {variant} k{top_k} p{top_p} t{temp}", tok=tok, kept=kept)
            for items, nb in SHAPES:
                c = W.make_case(variant, V, items, nb)
                if variant == "seen" and nb == 3:
                    c["k"] = 61
                    c["hist"][:, 60] = (np.arange(items * nb) * 7 + 5) % (V - 4)
                ub = W.uniform_sets(variant, V, items, nb)[0]  # the set that holds 0.0 and 0.99999994
                for top_k in (0, 200):
                    for top_p, temp in ((0.8, 1.0), (1.0, 0.7)):
                        psc, ptok, pbeam, kept = WB.beam_rows(c, items, nb, top_k, top_p, temp, ub)
                        emit(f"beam_sample_rows V{V} {items}x{nb} {variant} k{top_k} p{top_p} t{temp}", score=psc, tok=ptok, beam=pbeam, kept=kept)


def typical():
    """typical_filter_kernel through itts_typical_rows: the filtered scores of the five rows of a case."""
    for V in (66, 1025, 8194, 16384):
        for source in ("map", "beams"):
            c = T.typical_rows(V, source, 0.7, 2)
            for lsf in (0, 1):
                emit(f"typical_rows V{V} {source} lsf{lsf}", out=TF.run_typical(dict(c, lsf=lsf), 0.7, 2, source))


if __name__ == "__main__":
    from itts_hip import lib

    print("# library", os.path.basename(lib.LIB_PATH), file=sys.stderr)
    narrow_sampler()
    narrow_beams()
    wide()
    typical()
