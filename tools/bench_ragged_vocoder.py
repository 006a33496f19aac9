#!/usr/bin/env python3
"""The ragged-batch vocoder (Engine.bigvgan_grouped(ragged=True), opt-in) against the vocoder without it.

    python tools/bench_ragged_vocoder.py [--rows 64] [--max-pad 0.1,0.25,0.5] [--repeat 3] [--seed 5] [--max-batch 64]

Full IndexTTS-1.5 dims, bf16, PRNG weights, the vocoder only.  `--rows` latents of DISTINCT lengths T = round(4.57 L) frames, L spread
over 60 .. 120 text tokens from the seed (4.57 mel codes per text token: the ratio of the benchmark's utterances).  The yardstick is
bigvgan_grouped(ragged=False): every latent has its own length, so it is `--rows` batch-1 vocoder runs.  Against it, ragged=True at
each `--max-pad`.  Every setting runs once as a warm-up (every shape allocates its scratch there); then the settings alternate
`--repeat` times in one process on one engine object, each run timed with device events around a synchronise.  Printed per setting:
the best and the median time, the vocoder passes and their sizes, the frames computed over the frames needed, and the largest and the
mean per-row relative RMS of the waveforms against the yardstick's.
Run it under a time limit (timeout -k 10 600 python tools/bench_ragged_vocoder.py ...); profiles/ragged_vocoder.txt holds a record."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core, prng, synth  # noqa: E402


def lengths(rows, seed):
    """distinct frame counts round(4.57 L), L spread over 60 .. 120"""
    rng = np.random.RandomState(seed)
    out = set()
    while len(out) < rows:
        out.add(int(round(4.57 * rng.uniform(60.0, 120.0))))
    out = sorted(out)
    rng.shuffle(out)
    return [int(v) for v in out]


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def timed(eng, lats, spk, setting):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    wavs = eng.bigvgan_grouped(lats, spk, ragged=setting is not None, max_pad=setting or 0.0)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), wavs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--max-pad", type=str, default="0.1,0.25,0.5")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=64)
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("bigvgan",), max_batch=a.max_batch)
    lens = lengths(a.rows, a.seed)
    D = cfg.bigvgan.gpt_dim
    lats = [torch.from_numpy(prng.tensor(f"bench.ragged.lat{i}", a.seed, (1, n, D), std=1.0)).to(device=eng.device, dtype=eng.tdt)
            for i, n in enumerate(lens)]
    spk = eng.ecapa(torch.from_numpy(synth.prompt_mel(511, seed=7)).transpose(1, 2)).float()
    settings = [None] + [float(v) for v in a.max_pad.split(",") if v]
    name = lambda s: "ragged=False (yardstick)" if s is None else f"ragged=True max_pad={s:g}"  # noqa: E731
    need = sum(lens)
    print(f"{a.rows} latents, {min(lens)} .. {max(lens)} frames ({need} in all), max_batch {a.max_batch}, bf16, IndexTTS-1.5 dims")
    times = {s: [] for s in settings}
    base = None
    for rep in range(a.repeat + 1):  # run 0: warm-up of every shape, accuracy against the yardstick
        for s in settings:
            ms, wavs = timed(eng, lats, spk, s)
            if rep == 0:
                groups = [[i] for i in range(len(lens))] if s is None else infer_core.ragged_groups(lens, s, a.max_batch)
                frames = sum(len(g) * max(lens[i] for i in g) for g in groups)
                if s is None:
                    base = [w.float().cpu() for w in wavs]
                    acc = ""
                else:
                    errs = [rel_rms(w.float().cpu(), b) for w, b in zip(wavs, base)]
                    acc = f"; rel RMS vs the yardstick per row: max {max(errs):.3e}, mean {float(np.mean(errs)):.3e}"
                sizes = sorted((len(g) for g in groups), reverse=True)
                print(f"  {name(s)}: {len(groups)} passes (rows per pass {sizes[:8]}{' ...' if len(sizes) > 8 else ''}), frames computed / "
                      f"needed {frames} / {need} = {frames / need:.3f}{acc}")
            else:
                times[s].append(ms)
    ref = min(times[None]) if times[None] else float("nan")
    for s in settings:
        t = times[s]
        if t:
            print(f"{name(s)}: best {min(t):.1f} ms, median {float(np.median(t)):.1f} ms over {len(t)} runs; yardstick best / this best = "
                  f"{ref / min(t):.2f}")


if __name__ == "__main__":
    main()
