#!/usr/bin/env python3
"""The packed vocoder (Engine.bigvgan_packed, opt-in) against the two forms the parent has.

    python tools/bench_packed_vocoder.py [--rows 64] [--repeat 3] [--seed 5] [--max-batch 64] [--out profiles/packed_vocoder.txt]
    python tools/bench_packed_vocoder.py --e2e [--utterances 32] [--voices 8] [--text-tokens 60] [--max-mel-tokens 150] [--rounds 2]

Default mode: the workload of tools/bench_ragged_vocoder.py - full IndexTTS-1.5 dims, bf16, PRNG weights, the vocoder only, `--rows`
latents of distinct lengths round(4.57 L) frames, L over 60 .. 120 (275 .. 544 frames at the default seed).  Three forms, each run once
as a warm-up (every shape allocates its scratch there), then alternated `--repeat` times in one process on one engine object, each run
timed with device events around a synchronise:
    batch-1     bigvgan_grouped(ragged=False): every latent has its own length, so `--rows` batch-1 passes
    ragged 0.1  bigvgan_grouped(ragged=True, max_pad=0.1)
    packed      ONE bigvgan_packed call (its passes follow infer_core.packed_vocoder_plan)
first with one voice for all rows, then with one voice per row.  Printed per form: passes, frames computed over frames needed, best and
median milliseconds, and the per-row relative RMS of the waveforms against the batch-1 form's.

--e2e: the infer_batch call of tools/bench_mixed_batch.py (mixed batches on, full dims, IEEE half) with ITTS_PACKED_VOCODER flipped
between the calls, alternated `--rounds` times after one warm-up call of each; vocoder calls and wall time per form.
Every line also goes to `--out` when given.  Run under a time limit (timeout -k 10 900 python tools/bench_packed_vocoder.py ...)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_mixed_batch as bmb  # noqa: E402
import bench_ragged_vocoder as brv  # noqa: E402
from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core, prng, synth  # noqa: E402

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def vocoder_only(a):
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("bigvgan",), max_batch=a.max_batch)
    lens = brv.lengths(a.rows, a.seed)
    D, need, gap = cfg.bigvgan.gpt_dim, sum(lens), eng.bigvgan_packed_gap()
    lats = [torch.from_numpy(prng.tensor(f"bench.ragged.lat{i}", a.seed, (1, n, D), std=1.0)).to(device=eng.device, dtype=eng.tdt)
            for i, n in enumerate(lens)]
    spk1 = eng.ecapa(torch.from_numpy(synth.prompt_mel(511, seed=7)).transpose(1, 2)).float().reshape(1, -1)
    noise = torch.from_numpy(prng.tensor("bench.packed.spk", a.seed, (a.rows, spk1.shape[1]), std=0.05)).to(spk1.device)
    forms = {"batch-1": lambda s: eng.bigvgan_grouped(lats, s), "ragged 0.1": lambda s: eng.bigvgan_grouped(lats, s, ragged=True, max_pad=0.1),
             "packed": lambda s: eng.bigvgan_packed(lats, s)}
    groups = infer_core.ragged_groups(lens, 0.1, a.max_batch)
    chunks, _, frames = infer_core.packed_vocoder_plan(lens, gap)
    computed = {"batch-1": (len(lens), need), "ragged 0.1": (len(groups), sum(len(g) * max(lens[i] for i in g) for g in groups)),
                "packed": (len(chunks), sum(frames))}
    say(f"{a.rows} latents, {min(lens)} .. {max(lens)} frames ({need} in all), gap {gap}, max_batch {a.max_batch}, bf16, IndexTTS-1.5 dims, seed {a.seed}")
    for voices, spk in (("one voice", spk1), ("one voice per row", (spk1 + noise).contiguous())):
        times = {f: [] for f in forms}
        base = None
        for rep in range(a.repeat + 1):  # run 0: warm-up of every shape, accuracy against the batch-1 form
            for f, fn in forms.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                wavs = fn(spk)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[f].append(e0.elapsed_time(e1))
                    continue
                if f == "batch-1":
                    base = [w.float().cpu() for w in wavs]
                    acc = ""
                else:
                    errs = [brv.rel_rms(w.float().cpu(), b) for w, b in zip(wavs, base)]
                    acc = f"; rel RMS vs batch-1 per row: max {max(errs):.3e}, mean {float(np.mean(errs)):.3e}"
                n, fr = computed[f]
                say(f"  [{voices}] {f}: {n} passes, frames computed / needed {fr} / {need} = {fr / need:.3f}{acc}")
        ref = min(times["batch-1"])
        for f, t in times.items():
            say(f"[{voices}] {f}: best {min(t):.1f} ms, median {float(np.median(t)):.1f} ms over {len(t)} runs; batch-1 best / this best = {ref / min(t):.2f}")
        say(f"[{voices}] ragged 0.1 best / packed best = {min(times['ragged 0.1']) / min(times['packed']):.2f}")


def end_to_end(a):
    from indextts.infer import IndexTTS

    cfg = icfg.indextts_1_5()
    sds = {"gpt": synth.gpt_state_dict(cfg, 1234), "bigvgan": synth.bigvgan_state_dict(cfg, 1234)}
    tts = IndexTTS(cfg=cfg, model_dir="/nonexistent", is_fp16=True, state_dicts=sds, mixed_batch=True)
    os.environ["ITTS_MIXED_BATCH"] = "1"
    mels = [torch.from_numpy(synth.prompt_mel(511, seed=7 + v)) for v in range(a.voices)]
    n = a.utterances
    prompts = [mels[u % a.voices] for u in range(n)]
    per = [dict(bmb.SETTINGS[(u // a.voices) % len(bmb.SETTINGS)], seed=100 + u) for u in range(n)]
    texts = [[synth.text_ids(a.text_tokens - (u * 7) % 23, 11 + u, cfg.gpt.number_text_tokens).astype(np.int32)] for u in range(n)]
    calls = []
    for name in ("bigvgan", "bigvgan_packed"):
        real = getattr(tts.engine, name)
        setattr(tts.engine, name, lambda *r, _real=real, _name=name, **k: (calls.append(_name), _real(*r, **k))[1])

    def run(on):
        os.environ["ITTS_PACKED_VOCODER"] = "1" if on else "0"
        calls.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached: PRNG weights never stop
            out = tts.infer_batch(prompts, texts, num_beams=1, max_mel_tokens=a.max_mel_tokens, per_utterance=per)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, sum(w.shape[0] for _, w in out) / 24000.0, list(calls)

    say(f"end to end: {n} utterances, {a.voices} voices, {len(bmb.SETTINGS)} settings, {a.max_mel_tokens} mel tokens per row, mixed batches on, "
        f"IndexTTS-1.5 dims, {tts.half}")
    times, info = {False: [], True: []}, {}
    for rnd in range(a.rounds + 1):  # round 0: warm-up
        for on in (False, True):
            dt, audio, c = run(on)
            info[on] = (audio, c)
            if rnd:
                times[on].append(dt)
    for on in (False, True):
        audio, c = info[on]
        t = times[on]
        say(f"packed_vocoder {'on ' if on else 'off'}: {c.count('bigvgan')} bigvgan + {c.count('bigvgan_packed')} bigvgan_packed calls; {audio:.1f} s of audio; "
            f"wall s {' '.join(f'{x:.2f}' for x in t)}; best {audio / min(t):.1f} audio-s/s")
    say(f"on / off (best audio-s/s): {min(times[False]) / min(times[True]):.3f} x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--voices", type=int, default=8)
    ap.add_argument("--text-tokens", type=int, default=60)
    ap.add_argument("--max-mel-tokens", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    (end_to_end if a.e2e else vocoder_only)(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
