"""GPU: the streaming vocoder (Engine.bigvgan_stream) on the micro generator, fp32 and both 16-bit libraries, R = vocoder_reach(micro).

A latent of 3 R + 11 frames is pushed as 1, 5, R, R + 2 frames and the rest, then the end (last=True) on its own: every push returns only final samples,
the lengths add up, and the concatenation equals Engine.bigvgan_packed of the whole latent bit for bit; at least three pushes return
audio before the last one (the precondition that makes the comparison one of windows with artificial edges on both sides).
A latent shorter than R returns nothing until last=True and then everything, bit-equal.  Two voices in two streams, pushed alternately,
each equal their own whole pass - and differ from each other."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core, prng  # noqa: E402

MICRO = icfg.micro()
KINDS = ("fp32", "bf16", "f16")
_ENGINES = {}


def engine(kind):
    if kind not in _ENGINES:
        _ENGINES[kind] = ieng.build_engine(MICRO, kind, parts=("bigvgan",))
    return _ENGINES[kind]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def operands(eng, frames, tag="a"):
    h = MICRO.bigvgan
    lat = torch.from_numpy(prng.tensor(f"vocoder_stream.lat.{tag}", 5, (1, frames, h["gpt_dim"]))).to(eng.device).to(eng.tdt)
    spk = torch.from_numpy(prng.tensor(f"vocoder_stream.spk.{tag}", 5, (1, h["speaker_embedding_dim"]))).to(eng.device)
    return lat, spk


def whole(eng, lat, spk):
    return eng.bigvgan_packed([lat], spk)[0].clone()


@pytest.mark.parametrize("kind", KINDS)
def test_pushes_concatenate_to_the_whole_pass(kind):
    eng = engine(kind)
    R = eng.vocoder_reach()
    h = MICRO.bigvgan
    assert R == infer_core.vocoder_reach(h["upsample_rates"], h["upsample_kernel_sizes"], h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]) == 34
    T = 3 * R + 11
    lat, spk = operands(eng, T)
    want = whole(eng, lat, spk)
    assert want.shape == (1, 1, T * eng.up_total) and bool(torch.isfinite(want).all())
    pieces = [1, 5, R, R + 2]
    pieces += [T - sum(pieces), 0]  # the rest, then the end of the sentence on its own
    vs = eng.bigvgan_stream(spk)
    got, lo, sent, before_last = [], 0, 0, 0
    for i, n in enumerate(pieces):
        last = i == len(pieces) - 1
        w = vs.push(lat[:, lo:lo + n] if n else None, last=last)
        lo += n
        m = w.shape[-1]
        assert w.shape == (1, 1, m) and m % eng.up_total == 0
        # only final samples: nothing within R frames of the frames received so far, until the sentence ends
        assert sent + m // eng.up_total <= (lo if last else max(0, lo - R))
        assert same_bits(w, want[:, :, sent * eng.up_total:sent * eng.up_total + m]), (kind, i, "a returned sample was not final")
        sent += m // eng.up_total
        before_last += int(m > 0 and not last)
        got.append(w)
    assert before_last >= 3, before_last
    assert sent == T and same_bits(torch.cat(got, -1), want)


@pytest.mark.parametrize("kind", KINDS)
def test_a_latent_shorter_than_the_reach(kind):
    eng = engine(kind)
    R = eng.vocoder_reach()
    lat, spk = operands(eng, R - 3, "short")
    vs = eng.bigvgan_stream(spk)
    assert vs.push(lat[:, :10]).shape[-1] == 0
    assert vs.push(lat[:, 10:]).shape[-1] == 0
    assert same_bits(vs.push(None, last=True), whole(eng, lat, spk))
    with pytest.raises(ValueError):
        vs.push(lat[:, :1])


def test_two_voices_in_two_streams_do_not_mix():
    eng = engine("bf16")
    R = eng.vocoder_reach()
    T = 2 * R + 7
    lat_a, spk_a = operands(eng, T, "a")
    lat_b, spk_b = operands(eng, T, "b")
    a, b = eng.bigvgan_stream(spk_a), eng.bigvgan_stream(spk_b)
    got_a, got_b = [], []
    cuts = [0, R + 3, R + 20, T]
    for i in range(3):
        last = i == 2
        got_a.append(a.push(lat_a[:, cuts[i]:cuts[i + 1]], last=last))
        got_b.append(b.push(lat_b[:, cuts[i]:cuts[i + 1]], last=last))
    wa, wb = torch.cat(got_a, -1), torch.cat(got_b, -1)
    assert same_bits(wa, whole(eng, lat_a, spk_a)) and same_bits(wb, whole(eng, lat_b, spk_b))
    assert not same_bits(wa, whole(eng, lat_a, spk_b))  # the voice matters
