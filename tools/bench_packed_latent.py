#!/usr/bin/env python3
"""The packed latent pass (Engine.latent_packed, IndexTTS(packed_latent=True); opt-in) against the left-padded pass.

    python tools/bench_packed_latent.py [--rounds 2] [--out profiles/packed_latent.txt] [--skip-infer]

One process, full IndexTTS-1.5 dims, IEEE-half engine, PRNG weights; every pair of settings is alternated `--rounds` times after a
warm-up of each (scratch of every shape).  Three legs:
  1. the latent stage alone on 64 ragged sequences (text L in 60 .. 120, T = round(4.57 L) codes): one Engine.latent_batch against
     one Engine.latent_packed - device events;
  2. the same stage on 32 one-sentence sequences of 8 voices: 32 per-utterance latent_batch(cond_index=..) calls (what
     _infer_batch_mixed runs without the switch) against ONE latent_packed - device events;
  3. IndexTTS.infer_batch on the workload of tools/bench_mixed_batch.py with ITTS_MIXED_BATCH=1, ITTS_PACKED_LATENT 0 and 1 - wall time.
Each leg also prints how far the packed latents are from the padded ones (relative RMS: two 16-bit results of one function).
The lines go to stdout and, with --out, are appended to that file.  Run under a time limit (timeout -k 10 900 ...)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from itts_hip import config as icfg  # noqa: E402
from itts_hip import synth  # noqa: E402
from bench_mixed_batch import SETTINGS  # noqa: E402

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def rms_rel(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).mean().sqrt() / (b ** 2).mean().sqrt())


def ab(name, forms, rounds):
    """forms: {label: callable -> list of latents}; alternated, round 0 = warm-up"""
    ms = {k: [] for k in forms}
    outs = {}
    for rnd in range(rounds + 1):
        for k, fn in forms.items():
            t, outs[k] = timed(fn)
            if rnd:
                ms[k].append(t)
    labels = list(forms)
    for k in labels:
        say(f"  {name} | {k:<44s} ms {' '.join(f'{x:8.2f}' for x in ms[k])}   best {min(ms[k]):8.2f}")
    a, b = labels
    worst = max(rms_rel(y.float(), x.float()) for x, y in zip(outs[a], outs[b]))
    say(f"  {name} | {a.split()[0]} / {b.split()[0]} (best): {min(ms[a]) / min(ms[b]):.2f} x; packed against padded latents: worst relative RMS {worst:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-infer", action="store_true")
    a = ap.parse_args()
    from indextts.infer import IndexTTS

    cfg = icfg.indextts_1_5()
    g = cfg.gpt
    sds = {"gpt": synth.gpt_state_dict(cfg, 1234), "bigvgan": synth.bigvgan_state_dict(cfg, 1234)}
    tts = IndexTTS(cfg=cfg, model_dir="/nonexistent", is_fp16=True, state_dicts=sds, mixed_batch=True)
    eng = tts.engine
    say(f"tools/bench_packed_latent.py: IndexTTS-1.5 dims, {tts.half}, one device, {a.rounds} rounds after a warm-up of each form")
    mels = [torch.from_numpy(synth.prompt_mel(511, seed=7 + v)) for v in range(8)]
    conds = torch.cat([eng.conditioning(m).reshape(1, eng.ccfg.cond_latents, g.model_dim).float() for m in mels], 0)
    rng = np.random.default_rng(3)

    def seqs(n, lo, hi):
        Ls = rng.integers(lo, hi + 1, n)
        texts = [synth.text_ids(int(L), 200 + i, g.number_text_tokens).astype(np.int32) for i, L in enumerate(Ls)]
        codes = [rng.integers(0, g.stop_mel_token, int(round(4.57 * L))).astype(np.int32) for L in Ls]
        rows = [eng.ccfg.cond_latents + len(t) + len(c) + 4 for t, c in zip(texts, codes)]
        return texts, codes, rows

    # leg 1: 64 ragged sequences, one voice
    texts, codes, rows = seqs(64, 60, 120)
    say(f"leg 1: 64 ragged sequences, L 60 .. 120, T = round(4.57 L): {sum(rows)} token rows packed, {64 * max(rows)} left-padded "
        f"({1 - sum(rows) / (64 * max(rows)):.1%} padding)")
    ab("leg 1", {"padded  latent_batch (64 rows)": lambda: eng.latent_batch(conds[0], texts, codes),
                 "packed  latent_packed": lambda: eng.latent_packed(conds[0], texts, codes)}, a.rounds)
    # leg 2: 32 one-sentence utterances of 8 voices
    texts, codes, rows = seqs(32, 38, 60)
    voice = [u % 8 for u in range(32)]
    say(f"leg 2: 32 one-sentence sequences of 8 voices, L 38 .. 60: {sum(rows)} token rows")
    ab("leg 2", {"padded  32 x latent_batch(cond_index) of 1 row": lambda: [eng.latent_batch(conds, [texts[u]], [codes[u]], cond_index=[voice[u]])[0] for u in range(32)],
                 "packed  one latent_packed": lambda: eng.latent_packed(conds, texts, codes, cond_index=voice)}, a.rounds)
    if not a.skip_infer:
        # leg 3: infer_batch, the workload of tools/bench_mixed_batch.py, mixed batches on
        n, nv, tt, mm = 32, 8, 60, 150
        prompts = [mels[u % nv] for u in range(n)]
        per = [dict(SETTINGS[(u // nv) % len(SETTINGS)], seed=100 + u) for u in range(n)]
        utexts = [[synth.text_ids(tt - (u * 7) % 23, 11 + u, g.number_text_tokens).astype(np.int32)] for u in range(n)]
        os.environ["ITTS_MIXED_BATCH"] = "1"

        def run(on):
            os.environ["ITTS_PACKED_LATENT"] = "1" if on else "0"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached: PRNG weights never stop
                out = tts.infer_batch(prompts, utexts, num_beams=1, max_mel_tokens=mm, per_utterance=per)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        wall = {False: [], True: []}
        outs = {}
        for rnd in range(a.rounds + 1):
            for on in (False, True):
                dt, outs[on] = run(on)
                if rnd:
                    wall[on].append(dt)
        audio = sum(w.shape[0] for _, w in outs[True]) / 24000.0
        say(f"leg 3: infer_batch, {n} one-sentence utterances, {nv} voices, 4 settings, {mm} mel tokens per row, ITTS_MIXED_BATCH=1; {audio:.1f} s of audio")
        for on in (False, True):
            say(f"  leg 3 | packed_latent {'on ' if on else 'off'} wall s {' '.join(f'{x:.3f}' for x in wall[on])}   best {min(wall[on]):.3f} "
                f"({audio / min(wall[on]):.1f} audio-s/s)")
        diff = max(int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max()) for (_, x), (_, y) in zip(outs[False], outs[True]))
        say(f"  leg 3 | off / on (best): {min(wall[False]) / min(wall[True]):.2f} x; largest int16 sample difference between the two forms {diff}")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
