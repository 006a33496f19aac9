"""No GPU: the algorithm of the ragged-batch vocoder and the grouping that feeds it.

tests/ragged_vocoder_ref.py states the masked BigVGAN pass on CPU tensors.  On the micro generator (up-rates 4 4 4 4 2 2, three AMP
kernels x three dilations), B = 4 rows of 5, 12, 1 and 9 frames with NaN behind each row's frames, every row of it has to be the
waveform oracle.vocoder.bigvgan_generator gives for that row alone - relative RMS < 1e-5, fp32 reordering only (measured 1.0e-6 to
1.5e-6) - and zero behind its end.  The same rows from the plain zero-padded batch have to MISS by more than 1e-2 (measured 0.22 to
0.53 for the three short rows): a test that a wrong model passes shows nothing.

infer_core.ragged_groups: a partition; every group within max_pad and cap; equal lengths give one group per cap; max_pad = 0 gives
the equal-length groups Engine.bigvgan_grouped forms without the switch."""
import itertools

import numpy as np
import pytest
import torch

import ragged_vocoder_ref as R
from itts_hip import infer_core


def test_masked_batch_equals_every_row_alone():
    c = R.micro_case()
    up = int(np.prod(c["cfg"].bigvgan.upsample_rates))
    wav = R.bigvgan_generator_ragged(c["lat_nan"], c["lens"], c["spk"], c["w"], c["cfg"].bigvgan)
    assert wav.shape == (len(c["lens"]), 1, max(c["lens"]) * up) and bool(torch.isfinite(wav).all())
    for b, n in enumerate(c["lens"]):
        e = R.rel_rms(wav[b:b + 1, :, :n * up], c["rows"][b])
        print(f"row {b} ({n} frames): masked batch vs the row alone, rel RMS {e:.2e}")
        assert e < 1e-5, (b, n, e)
        assert bool((wav[b, :, n * up:] == 0).all()), (b, "waveform tail")


def test_plain_padding_is_told_apart():
    c = R.micro_case()
    up = int(np.prod(c["cfg"].bigvgan.upsample_rates))
    wav = R.plain_padded(c)
    for b, n in enumerate(c["lens"]):
        e = R.rel_rms(wav[b:b + 1, :, :n * up], c["rows"][b])
        print(f"row {b} ({n} frames): plain zero-padded batch vs the row alone, rel RMS {e:.2e}")
        if n < max(c["lens"]):
            assert e > 1e-2, (b, n, e)
        else:
            assert e < 1e-5, (b, n, e)  # the longest row has no padding


# ---- ragged_groups ------------------------------------------------------------------------------------------------------------
def _length_sets():
    rng = np.random.RandomState(5)
    yield [7]
    yield [5, 12, 1, 9]
    yield [3] * 9
    yield [4, 7, 4, 7, 4, 9, 9, 1]
    for n in (2, 13, 64, 130):
        yield [int(v) for v in rng.randint(1, 600, size=n)]
        yield [int(round(4.57 * v)) for v in rng.randint(60, 121, size=n)]


def _pad_share(lengths, group):
    ls = [lengths[i] for i in group]
    return 1.0 - sum(ls) / (len(ls) * max(ls))


@pytest.mark.parametrize("max_pad,cap", list(itertools.product((0.0, 0.1, 0.25, 0.5, 0.9), (1, 3, 64))))
def test_ragged_groups_partition_within_limits(max_pad, cap):
    for lengths in _length_sets():
        groups = infer_core.ragged_groups(lengths, max_pad, cap)
        flat = [i for g in groups for i in g]
        assert sorted(flat) == list(range(len(lengths))), (lengths, groups)  # a partition
        for g in groups:
            assert 1 <= len(g) <= cap
            assert _pad_share(lengths, g) <= max_pad + 1e-12, (lengths, g)
            assert lengths[g[0]] == max(lengths[i] for i in g)  # opened by its longest row
        heads = [lengths[g[0]] for g in groups]
        assert heads == sorted(heads, reverse=True)  # longest first
        # greedy: the row that opened the next group did not fit the one before it
        for g, nxt in zip(groups, groups[1:]):
            assert len(g) == cap or _pad_share(lengths, g + [nxt[0]]) > max_pad, (lengths, g, nxt)


def test_ragged_groups_equal_lengths_fill_the_cap():
    for n, cap in ((9, 4), (8, 4), (1, 4), (5, 1), (64, 64), (65, 64)):
        groups = infer_core.ragged_groups([31] * n, 0.25, cap)
        assert [len(g) for g in groups] == [cap] * (n // cap) + ([n % cap] if n % cap else []), (n, cap, groups)
        assert [i for g in groups for i in g] == list(range(n))  # ties keep the caller's order


def test_ragged_groups_without_padding_are_the_equal_length_groups():
    """max_pad = 0: the sets Engine.bigvgan_grouped forms without the switch (by length, in chunks of cap in index order)"""
    for lengths in _length_sets():
        for cap in (1, 3, 64):
            by_len = {}
            for i, n in enumerate(lengths):
                by_len.setdefault(n, []).append(i)
            today = {tuple(idx[lo:lo + cap]) for idx in by_len.values() for lo in range(0, len(idx), cap)}
            assert {tuple(g) for g in infer_core.ragged_groups(lengths, 0.0, cap)} == today, (lengths, cap)


def test_ragged_groups_refuses_bad_arguments():
    for kw in (dict(max_pad=-0.1, cap=4), dict(max_pad=1.0, cap=4), dict(max_pad=0.25, cap=0)):
        with pytest.raises(ValueError):
            infer_core.ragged_groups([3, 4], **kw)
    with pytest.raises(ValueError):
        infer_core.ragged_groups([3, 0], 0.25, 4)
    assert infer_core.ragged_groups([], 0.25, 4) == []
