"""Test infrastructure (not product): the BigVGAN pass over PACKED sentences, on torch CPU tensors, from the pieces of oracle.vocoder -
the algorithm Engine::bigvgan_packed runs (csrc/model_vocoder.hip).

The latents of n sentences lie back to back in time as ONE item [1, Ttot, D]: sentence b owns frames [off[b], off[b + 1]) of which the
first lens[b] are signal and the rest - at least `gap` - zeros.  With U the up-sampling so far:
  * every convolution runs over the whole item; a tap that leaves a sentence reads the zeros of a gap, the zero "same" padding the
    sentence would see alone;
  * the gaps of the latent, of x behind conv_pre, of the output of every ups[i] and of every stage output are zeroed, and the same
    pass adds the sentence's speaker row (cond_layer / conds[i] of ITS embedding) to its signal columns;
  * every Activation1d runs per sentence on its own lens[b] * U columns (replicate padding at its own ends), zeros in its gap;
  * residual and accumulate tensors keep whatever their gaps hold; the waveform's gaps are zeroed.
gap = 0 is the plain concatenation: the same code, and the wrong model the tests must tell apart."""
import functools

import torch
import torch.nn.functional as F

import ragged_vocoder_ref as R
from itts_hip import config as icfg
from itts_hip import prng, synth
from oracle import gpt as ogpt
from oracle import vocoder as ovoc

LENS = R.LENS            # 5 / 12 / 1 / 9 frames
VOICES = (0, 1, 0, 1)    # two voices, alternating
rel_rms = R.rel_rms


def offsets(lens, gap):
    off = [0]
    for n in lens:
        off.append(off[-1] + n + gap)
    return off


def seg_mask(x, off, lens, mul, bias=None):
    """x [1, C, T]: the signal columns of sentence b get bias[b] ([C, 1]) added, the rest of its capacity becomes zero (a copy)"""
    out = torch.zeros_like(x)
    for b, n in enumerate(lens):
        lo = off[b] * mul
        sig = x[:, :, lo:lo + n * mul]
        out[:, :, lo:lo + n * mul] = sig if bias is None else sig + bias[b]
    return out


def activation1d_seg(x, off, lens, mul, log_alpha, log_beta, filt):
    out = torch.zeros_like(x)
    for b, n in enumerate(lens):
        lo = off[b] * mul
        out[:, :, lo:lo + n * mul] = ovoc.activation1d(x[:, :, lo:lo + n * mul], log_alpha, log_beta, filt)
    return out


def amp_block1_seg(x, off, lens, mul, w, p, ksize, dilations, filt):
    for l, d in enumerate(dilations):
        xt = activation1d_seg(x, off, lens, mul, w[f"{p}activations.{2 * l}.act.alpha"], w[f"{p}activations.{2 * l}.act.beta"], filt)
        xt = F.conv1d(xt, w[f"{p}convs1.{l}.weight"], w[f"{p}convs1.{l}.bias"], dilation=d, padding=(ksize * d - d) // 2)
        xt = activation1d_seg(xt, off, lens, mul, w[f"{p}activations.{2 * l + 1}.act.alpha"], w[f"{p}activations.{2 * l + 1}.act.beta"], filt)
        xt = F.conv1d(xt, w[f"{p}convs2.{l}.weight"], w[f"{p}convs2.{l}.bias"], padding=(ksize - 1) // 2)
        x = xt + x
    return x


def bigvgan_generator_packed(latent_1td, off, lens, spk_n1e, w, h):
    """latent [1, off[-1], D] (gaps ignored), spk [n, 1, E] one row per sentence -> wav [1, 1, off[-1] * prod(up)]"""
    filt = ovoc.kaiser_sinc_filter12()
    spk = spk_n1e.transpose(1, 2)  # [n, E, 1]
    x = seg_mask(latent_1td.transpose(1, 2), off, lens, 1)
    x = F.conv1d(x, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    x = seg_mask(x, off, lens, 1, F.conv1d(spk, w["cond_layer.weight"], w["cond_layer.bias"]))
    nk = len(h["resblock_kernel_sizes"])
    mul = 1
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(x, w[f"ups.{i}.0.weight"], w[f"ups.{i}.0.bias"], stride=u, padding=(k - u) // 2)
        mul *= u
        x = seg_mask(x, off, lens, mul, F.conv1d(spk, w[f"conds.{i}.weight"], w[f"conds.{i}.bias"]))
        xs = None
        for j in range(nk):
            r = amp_block1_seg(x, off, lens, mul, w, f"resblocks.{i * nk + j}.", h["resblock_kernel_sizes"][j],
                               h["resblock_dilation_sizes"][j], filt)
            xs = r if xs is None else xs + r
        x = seg_mask(xs / nk, off, lens, mul)
    x = activation1d_seg(x, off, lens, mul, w["activation_post.act.alpha"], w["activation_post.act.beta"], filt)
    x = F.conv1d(x, w["conv_post.weight"], w["conv_post.bias"], padding=3)
    return seg_mask(torch.tanh(x), off, lens, mul)


def pack(lats, off, fill=0.0):
    """latents [1, T_i, D] -> [1, off[-1], D], `fill` in the gaps"""
    out = torch.full((1, off[-1], lats[0].shape[2]), fill, dtype=lats[0].dtype)
    for b, l in enumerate(lats):
        out[0, off[b]:off[b] + l.shape[1]] = l[0]
    return out


@functools.lru_cache(maxsize=None)
def micro_case(lens=LENS, voices=VOICES, nvoice=2):
    """The micro generator, one random latent per sentence, `nvoice` speaker rows, and per sentence the waveform of
    oracle.vocoder.bigvgan_generator on the sentence alone with its voice.  Computed once, never modified."""
    cfg = icfg.micro()
    w = ogpt.to_torch(synth.bigvgan_state_dict(cfg, 1234))
    lat = torch.from_numpy(prng.tensor("packed.latent", 13, (len(lens), max(lens), cfg.bigvgan.gpt_dim), std=1.0))
    spk = torch.from_numpy(prng.tensor("packed.spk", 13, (nvoice, 1, cfg.bigvgan.speaker_embedding_dim), std=1.0))
    lats = [lat[b:b + 1, :n].clone() for b, n in enumerate(lens)]
    rows = [ovoc.bigvgan_generator(lats[b], spk[v:v + 1], w, cfg.bigvgan) for b, v in enumerate(voices)]
    return dict(cfg=cfg, w=w, lens=lens, voices=voices, lats=lats, spk=spk, rows=rows)
