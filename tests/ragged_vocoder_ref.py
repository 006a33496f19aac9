"""Test infrastructure (not product): the masked BigVGAN pass over a padded ragged batch, on torch CPU tensors, from the pieces of
oracle.vocoder - the algorithm Engine::bigvgan runs when it is given per-row lengths (csrc/model_vocoder.hip).

A [B, Tmax, D] batch holds latents of lens[b] frames.  With U the up-sampling so far:
  * the latent tail counts as zero, and the tail (t >= lens[b] * U) of x is zeroed after conv_pre + cond and of the stage output
    after each up-sampling stage - what the next (transposed) convolution reads is the zero "same" padding the row would see alone;
  * every Activation1d takes lens[b] * U as its signal length: replicate padding at the row's own last sample, zeros behind it;
  * residual and accumulate tensors keep whatever their tails hold;
  * the waveform tail is zeroed.
`plain_padded` is the same batch pushed through the unmasked generator: the wrong model the tests must tell apart."""
import functools

import torch
import torch.nn.functional as F

from itts_hip import config as icfg
from itts_hip import prng, synth
from oracle import gpt as ogpt
from oracle import vocoder as ovoc

LENS = (5, 12, 1, 9)  # frames per row: the longest not first, a single frame, two in between


def rel_rms(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def zero_tail(x, lens, mul):
    """x [B, C, T]: columns t >= lens[b] * mul of row b become zero (a copy)"""
    x = x.clone()
    for b, n in enumerate(lens):
        x[b, :, n * mul:] = 0
    return x


def activation1d_len(x, lens, mul, log_alpha, log_beta, filt):
    """Activation1d of every row's own signal x[b, :, :lens[b] * mul]; zeros behind it"""
    out = torch.zeros_like(x)
    for b, n in enumerate(lens):
        out[b:b + 1, :, :n * mul] = ovoc.activation1d(x[b:b + 1, :, :n * mul], log_alpha, log_beta, filt)
    return out


def amp_block1_len(x, lens, mul, w, p, ksize, dilations, filt):
    """oracle.vocoder.amp_block1 with the length-aware activation"""
    for l, d in enumerate(dilations):
        xt = activation1d_len(x, lens, mul, w[f"{p}activations.{2 * l}.act.alpha"], w[f"{p}activations.{2 * l}.act.beta"], filt)
        xt = F.conv1d(xt, w[f"{p}convs1.{l}.weight"], w[f"{p}convs1.{l}.bias"], dilation=d, padding=(ksize * d - d) // 2)
        xt = activation1d_len(xt, lens, mul, w[f"{p}activations.{2 * l + 1}.act.alpha"], w[f"{p}activations.{2 * l + 1}.act.beta"], filt)
        xt = F.conv1d(xt, w[f"{p}convs2.{l}.weight"], w[f"{p}convs2.{l}.bias"], padding=(ksize - 1) // 2)
        x = xt + x
    return x


def bigvgan_generator_ragged(latent_btd, lens, spk_b1e, w, h):
    """oracle.vocoder.bigvgan_generator over a padded ragged batch: latent [B, Tmax, D] (tails ignored), lens [B] frames
    -> wav [B, 1, Tmax * prod(up)], row b the waveform of its own lens[b] frames and zero behind lens[b] * prod(up)."""
    filt = ovoc.kaiser_sinc_filter12()
    spk = spk_b1e.transpose(1, 2)
    x = zero_tail(latent_btd.transpose(1, 2), lens, 1)
    x = F.conv1d(x, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    x = zero_tail(x + F.conv1d(spk, w["cond_layer.weight"], w["cond_layer.bias"]), lens, 1)
    nk = len(h["resblock_kernel_sizes"])
    mul = 1
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(x, w[f"ups.{i}.0.weight"], w[f"ups.{i}.0.bias"], stride=u, padding=(k - u) // 2)
        x = x + F.conv1d(spk, w[f"conds.{i}.weight"], w[f"conds.{i}.bias"])  # (its tail is not zero: only length-aware readers follow)
        mul *= u
        xs = None
        for j in range(nk):
            r = amp_block1_len(x, lens, mul, w, f"resblocks.{i * nk + j}.", h["resblock_kernel_sizes"][j],
                               h["resblock_dilation_sizes"][j], filt)
            xs = r if xs is None else xs + r
        x = zero_tail(xs / nk, lens, mul)
    x = activation1d_len(x, lens, mul, w["activation_post.act.alpha"], w["activation_post.act.beta"], filt)
    x = F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3)
    return zero_tail(torch.tanh(x), lens, mul)


@functools.lru_cache(maxsize=None)
def micro_case(lens=LENS):
    """The micro generator, random latents (NaN behind each row's frames) and speaker rows, and per row the waveform of
    oracle.vocoder.bigvgan_generator on the row cut to its length.  Computed once, never modified."""
    cfg = icfg.micro()
    w = ogpt.to_torch(synth.bigvgan_state_dict(cfg, 1234))
    B, T = len(lens), max(lens)
    lat = torch.from_numpy(prng.tensor("ragged.latent", 11, (B, T, cfg.bigvgan.gpt_dim), std=1.0))
    spk = torch.from_numpy(prng.tensor("ragged.spk", 11, (B, 1, cfg.bigvgan.speaker_embedding_dim), std=1.0))
    rows = [ovoc.bigvgan_generator(lat[b:b + 1, :n], spk[b:b + 1], w, cfg.bigvgan) for b, n in enumerate(lens)]
    nan_tail = lat.clone()
    for b, n in enumerate(lens):
        nan_tail[b, n:] = float("nan")
    return dict(cfg=cfg, w=w, lens=lens, lat=lat, lat_nan=nan_tail, spk=spk, rows=rows)


def plain_padded(case):
    """the zero-padded batch through the unmasked generator (what padding alone computes)"""
    lat = zero_tail(case["lat"].transpose(1, 2), case["lens"], 1).transpose(1, 2)
    return ovoc.bigvgan_generator(lat, case["spk"], case["w"], case["cfg"].bigvgan)
