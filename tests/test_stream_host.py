"""Host-side pieces of the streaming synthesis (itts_hip/infer_core.py), on the CPU.

vocoder_reach: the CPU vocoder of oracle/ is run on a latent and on the same latent with ONE frame t perturbed; the output may change
nowhere outside frames [t - R, t + R] (sufficient: exact zeros, compared as bits), and some sample at distance >= R / 2 frames must
change (not grossly loose).  Two generators: the micro one, and one with up_rates [4, 2], AMP kernels [3, 7] and dilations [1, 3].
stream_clean: split invariance, agreement with remove_long_silence where the docstring promises it, and the counter-example.
StreamWindow: the emit and hold-back arithmetic for chunk sizes 1, R and R + 1 and for a sentence shorter than the first chunk."""
import itertools

import numpy as np
import pytest
import torch

from itts_hip import config, infer_core, synth
from oracle import gpt as ogpt
from oracle import vocoder as ovoc


def reach_of(h):
    return infer_core.vocoder_reach(h["upsample_rates"], h["upsample_kernel_sizes"], h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])


def small_cfg():
    cfg = config.micro()
    cfg["bigvgan"].update({"upsample_rates": [4, 2], "upsample_kernel_sizes": [8, 4], "resblock_kernel_sizes": [3, 7],
                           "resblock_dilation_sizes": [[1, 3], [1, 3]], "upsample_initial_channel": 32})
    return cfg


def test_reach_values():
    """The 1.5 / micro generator: 3 + 2/4 + 90/4 + 2/16 + 90/16 + 90/64 + 90/256 + 1/512 + 90/512 + 1/1024 + 90/1024 + 8/1024 = 33.8 -> 34;
    the small one: 3 + (2 + 38)/4 + (1 + 38)/8 + 8/8 = 18.9 -> 19"""
    assert reach_of(config.micro()["bigvgan"]) == 34
    assert reach_of(config.indextts_1_5()["bigvgan"]) == 34
    # AMP kernel 7, dilations 1 and 3: (5 + 3 + 5 + 3) + (5 + 9 + 5 + 3) = 38 samples a stage; kernel 3 is shallower
    assert infer_core.vocoder_reach([4, 2], [8, 4], [3, 7], [[1, 3], [1, 3]]) == int(np.ceil(3 + (2 + 38) / 4 + (1 + 38) / 8 + 8 / 8))
    # the packed vocoder's gap is the largest single reach, not the sum
    assert infer_core.packed_vocoder_gap([4, 4, 4, 4, 2, 2], [8, 8, 4, 4, 4, 4], [3, 7, 11], [[1, 3, 5]] * 3) < 34


@pytest.mark.parametrize("which", ["micro", "small"])
def test_reach_is_sufficient_and_not_grossly_loose(which):
    cfg = config.micro() if which == "micro" else small_cfg()
    h = cfg["bigvgan"]
    R = reach_of(h)
    up = int(np.prod(h["upsample_rates"]))
    w = ogpt.to_torch(synth.bigvgan_state_dict(cfg, 1234))
    T = 2 * R + 9
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, T, h["gpt_dim"], generator=g)
    spk = torch.randn(1, 1, h["speaker_embedding_dim"], generator=g)
    base = ovoc.bigvgan_generator(lat, spk, w, h)[0, 0]
    assert base.shape[0] == T * up
    for t in (0, R + 4, T - 1):  # a true edge on either side, and the middle
        pert = lat.clone()
        pert[0, t] += 1.0
        out = ovoc.bigvgan_generator(pert, spk, w, h)[0, 0]
        changed = (out.view(torch.int32) != base.view(torch.int32)).view(T, up).any(1).nonzero().flatten()
        assert len(changed), t
        lo, hi = int(changed.min()), int(changed.max())
        assert lo >= t - R and hi <= t + R, (which, t, R, lo, hi)
        far = max(t - lo, hi - t)
        assert far >= min(R / 2, max(t, T - 1 - t)), (which, t, R, far)


# ---- the causal silence rule ---------------------------------------------------------------------------------------------------------
STOP, SIL = 65, 52


def clean_whole(row):
    return infer_core.stream_clean(row, STOP, SIL)[0]


def batch_rule(row):
    c, n = infer_core.remove_long_silence(np.asarray(row)[None], STOP, SIL)
    return c[0, :int(n[0])]


def rows():
    rng = np.random.default_rng(3)
    few = np.concatenate([rng.integers(0, 50, 20), [SIL] * 14, rng.integers(0, 50, 5), [SIL] * 12, [7, STOP, 9, 9]])  # 26 silent: nothing dropped
    late = np.concatenate([[SIL] * 9, [1], [SIL] * 9, [2], [SIL] * 9, [3], [SIL] * 4, [4], [SIL] * 25, [5], [SIL] * 13, [STOP]])  # long runs begin after the 30th
    early = np.concatenate([[SIL] * 20, [1, 2], [SIL] * 25, [3, STOP]])  # a long run among the first 30: the counter-example
    nostop = np.concatenate([[SIL] * 40, [1], [SIL] * 12])
    return dict(few=few, late=late, early=early, nostop=nostop)


@pytest.mark.parametrize("name", list(rows()))
def test_stream_clean_does_not_depend_on_the_split(name):
    row = rows()[name]
    whole = clean_whole(row)
    for cuts in ([1] * len(row), [3, 1, 7] * len(row), [len(row)], [16] * len(row), [0, 5, 0] * len(row)):
        st, got, i = None, [], 0
        for n in itertools.takewhile(lambda _: i < len(row), cuts):
            piece, st = infer_core.stream_clean(row[i:i + n], STOP, SIL, state=st)
            got.append(piece)
            i += n
        assert np.array_equal(np.concatenate(got), whole), (name, cuts[:3])


def test_stream_clean_against_the_batch_rule():
    r = rows()
    assert int((r["few"] == SIL).sum()) <= 30 and np.array_equal(clean_whole(r["few"]), batch_rule(r["few"]))
    assert np.array_equal(clean_whole(r["few"]), r["few"][:list(r["few"]).index(STOP)])
    assert int((r["late"] == SIL).sum()) > 30 and np.array_equal(clean_whole(r["late"]), batch_rule(r["late"]))
    assert len(clean_whole(r["late"])) < len(r["late"]) - 1  # ... and something was dropped
    # the counter-example: 20 silent codes open the row.  The batch rule, knowing that 45 will come, keeps 10 of them; the causal rule
    # has passed all 20 on (silent codes 11 .. 20 have r >= 10 but are among the first 30).  From the 31st silent code on they agree.
    causal, batch = clean_whole(r["early"]), batch_rule(r["early"])
    assert np.array_equal(batch, [SIL] * 10 + [1, 2] + [SIL] * 10 + [3])
    assert np.array_equal(causal, [SIL] * 20 + [1, 2] + [SIL] * 10 + [3])
    assert np.array_equal(clean_whole(r["nostop"]), [SIL] * 30 + [1] + [SIL] * 10)  # silent codes 11 .. 30 pass, 31 .. 40 do not


# ---- the chunk planner ---------------------------------------------------------------------------------------------------------------
def drive(R, chunk, first, pieces):
    """-> the (lo, a, b) of every push; the last piece is pushed with last=True"""
    w = infer_core.StreamWindow(R, chunk, first)
    return [w.push(n, last=(i == len(pieces) - 1)) for i, n in enumerate(pieces)], w


@pytest.mark.parametrize("R", [4, 34])
def test_window_arithmetic(R):
    for chunk in (1, R, R + 1):
        pieces = [1, 5, R, R + 2, 3 * R - 2, 0]
        steps, w = drive(R, chunk, None, pieces)
        total, have, sent = sum(pieces), 0, 0
        for (lo, a, b), n, last in zip(steps, pieces, [False] * (len(pieces) - 1) + [True]):
            have += n
            assert a == sent and b >= a  # consecutive
            assert lo == max(0, a - R)   # exactly R frames of left context, or the true edge
            if last:
                assert b == have
            else:
                assert b <= max(a, have - R)  # nothing within R of the artificial right edge
                final = max(0, have - R - a)
                assert (b - a == final) if final >= chunk else (b == a)  # everything final once a chunk is, nothing before
            sent = b
        assert sent == total and w.sent == total


def test_window_sentence_shorter_than_the_first_chunk():
    R = 34
    steps, _ = drive(R, 48, 24, [10, 3, 0])
    assert steps == [(0, 0, 0), (0, 0, 0), (0, 0, 13)]  # nothing until the end, then everything from the true left edge
    steps, _ = drive(R, 48, 24, [R + 23, 1, 47, 1, 5])
    assert steps == [(0, 0, 0), (0, 0, 24), (0, 24, 24), (0, 24, 72), (72 - R, 72, R + 77)]
    w = infer_core.StreamWindow(R)
    w.push(3, last=True)
    with pytest.raises(ValueError):
        w.push(1)
