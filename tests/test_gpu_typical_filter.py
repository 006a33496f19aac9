"""GPU: typical_filter_kernel (csrc/beam.hip) through itts_typical_rows against the fp64 reference of token_choice_ref.py, at inputs
flat enough that hundreds to thousands of ranks stay - there the block scan of the run sums, the 16 ranks per thread at the real
vocabulary and the padding decide what is kept.  At those inputs the decision margins are 1e-6 .. 1e-5, so the acceptance is
two-sided (token_choice_ref.typical_ref): everything the reference keeps with the mass moved down by d and the key by e must stay,
nothing the reference drops with them moved up may stay; d and e come from the kernel's summation structure (typical_bounds), and the
band between the two sets is capped at 4 tokens by the choice of the input stream (test_token_choice_api.py asserts it)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_choice_ref as T  # noqa: E402

from itts_hip import lib  # noqa: E402

DEV = "cuda:0"


def run_typical(c, mass, min_keep, source, max_gen=64):
    """One launch on the rows of a case -> out fp32 [rows, V]; checks the guard blocks and that no input changed."""
    l = lib.load()
    rows, V = c["logits"].shape
    d = T.DevArrays(DEV)
    a = lib.TypicalArgs()
    a.logits, a.out = d.put("logits", c["logits"]), d.put("out", np.full((rows, V), T.SENT_F, np.float32))
    a.rows, a.V, a.stop, a.min_keep, a.log_softmax_first, a.penalty, a.mass = rows, V, c["stop"], min_keep, c["lsf"], c["penalty"], mass
    a.suppress_stop = 0
    k = T.TYP_K
    ids = np.full((2, rows, max_gen), T.SENT_I, np.int32)
    if source == "beams":
        ids[k & 1, :, :k] = c["hist"]
        a.beam_ids, a.len = d.put("ids", ids), d.put("len", np.full(rows, k, np.int32))
        a.max_gen, a.start_tok, a.fake_id = max_gen, c["start"], c["fake"]
    else:
        a.seen = d.put("seen", c["seen"].astype(np.uint8))
    outs = []
    for suppress in (0, 1):  # the "holes" row is the one computed with the stop suppressed
        a.suppress_stop = suppress
        torch.cuda.synchronize()
        lib.check(l.itts_typical_rows(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "typical_rows", l)
        torch.cuda.synchronize()
        outs.append(d.get("out"))
    assert T.same_bits(d.get("logits"), c["logits"])
    if source == "beams":
        assert T.same_bits(d.get("ids"), ids) and (d.get("len") == k).all()
    else:
        assert T.same_bits(d.get("seen"), c["seen"].astype(np.uint8))
    out = outs[0].copy()
    hole = T.TYP_ROWS.index("holes")
    out[hole] = outs[1][hole]
    return out


@pytest.mark.parametrize("source", ("map", "beams"))
@pytest.mark.parametrize("V", T.TYP_VOCABS)
def test_kept_set_between_the_two_reference_sets(V, source):
    worst_val, bound_val, band = 0.0, 0.0, 0
    for mass in T.TYP_MASSES:
        for min_keep in (1, 2):
            c = T.typical_rows(V, source, mass, min_keep)
            out = run_typical(c, mass, min_keep, source)
            for r, (kind, ref) in enumerate(zip(T.TYP_ROWS, c["refs"])):
                kept = out[r] > -np.inf
                miss, extra = ref["must"] & ~kept, kept & ~ref["may"]
                print(f"V {V} {source} mass {mass} min_keep {min_keep} {kind}: kept {int(kept.sum())} fp64 {int(ref['kept64'].sum())} must "
                      f"{int(ref['must'].sum())} may {int(ref['may'].sum())} d {ref['d']:.2e} e {ref['e']:.2e} same as fp64: "
                      f"{bool((kept == ref['kept64']).all())}")
                assert not miss.any(), (mass, min_keep, kind, "dropped tokens the reference must keep", np.nonzero(miss)[0][:8])
                assert not extra.any(), (mass, min_keep, kind, "kept tokens the reference cannot keep", np.nonzero(extra)[0][:8])
                assert (out[r][~kept] == -np.inf).all()  # nothing but scores and -inf (no NaN, no sentinel left)
                band = max(band, int(ref["may"].sum() - ref["must"].sum()))
                if c["lsf"]:  # log_softmax first: the kept values within the first stage's bound (scaled by the penalty where seen)
                    tol = ref["d_in"] * np.where(c["seen"][r], c["penalty"], 1.0)[kept]
                    dev = np.abs(out[r][kept].astype(np.float64) - ref["s"][kept])
                    assert (dev <= tol).all(), (mass, min_keep, kind, float((dev / tol).max()))
                    worst_val, bound_val = max(worst_val, float((dev / tol).max())), ref["d_in"]
                else:  # one fp32 operation per element: the kept values are the processed scores, bit for bit
                    want = T.processed32(c["logits"][r], c["seen"][r], c["penalty"], c["stop"], kind == "holes")
                    assert T.same_bits(out[r][kept], want[kept]), (mass, min_keep, kind)
                if kind == "peaked":
                    assert int(kept.sum()) == min_keep and kept[V // 3]
                if kind == "holes":
                    assert not kept[c["stop"]] and not kept[~np.isfinite(c["logits"][r])].any()
    print(f"typical V {V} {source}: widest band {band} tokens (cap {T.BAND_TOKENS}); kept-value deviation / bound {worst_val:.3f} (bound {bound_val:.2e})")


def test_rows_do_not_depend_on_the_batch_and_repeat_bit_for_bit():
    V, mass = 8194, 0.7
    c = T.typical_rows(V, "map", mass, 1)
    a, b = run_typical(c, mass, 1, "map"), run_typical(c, mass, 1, "map")
    assert T.same_bits(a, b)
    perm = [3, 0, 4, 1, 2]
    c2 = dict(c, logits=np.ascontiguousarray(c["logits"][perm]), seen=np.ascontiguousarray(c["seen"][perm]))
    l = lib.load()
    d = T.DevArrays(DEV)
    args = lib.TypicalArgs()
    args.logits, args.out, args.seen = d.put("lg", c2["logits"]), d.put("out", np.zeros((5, V), np.float32)), d.put("seen", c2["seen"].astype(np.uint8))
    args.rows, args.V, args.stop, args.min_keep, args.penalty, args.mass = 5, V, c["stop"], 1, c["penalty"], mass
    lib.check(l.itts_typical_rows(C.byref(args), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "typical_rows", l)
    torch.cuda.synchronize()
    out = d.get("out")
    for pos, p in enumerate(perm):
        if T.TYP_ROWS[p] != "holes":  # (that row of `a` was computed with the stop suppressed)
            assert T.same_bits(out[pos], a[p]), (pos, p)
