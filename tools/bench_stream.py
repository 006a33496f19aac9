#!/usr/bin/env python3
"""Streaming synthesis (Engine.generate_stream + latent_stream + bigvgan_stream, opt-in) against the parent's non-streamed composition.

    python tools/bench_stream.py [--chunks 24,48,96] [--first 24] [--rounds 3] [--mel-tokens 480] [--text-tokens 105] [--out profiles/stream.txt]

bench.py's batch-1 workload: full IndexTTS-1.5 dims, bf16, PRNG weights, one sentence of L = 105 text tokens and 480 forced codes (the
stop token suppressed), greedy.  Four forms, each run once as a warm-up, then alternated `--rounds` times in one process on one engine
object; wall time from just before the prefill, device idle at the start:
    parent      generate, then latent_packed, then bigvgan_packed - the first sample exists when everything has run
    stream C    the streaming loop with chunks of C frames (first chunk `--first`): time to the first chunk, time between chunks, total
    recompute C the same loop, but every chunk's latents come from latent_packed over the whole prefix so far instead of one append -
                what the append kernel is worth
Printed per form: time to first audio, mean / max time between chunks, total, vocoder frames computed over frames emitted (the halo
arithmetic predicts (chunk + 2 R) / chunk), latent appends.  Every streamed waveform is compared with the parent's, bit for bit.
Every line also goes to `--out` when given.  Run under a time limit (timeout -k 10 600 python tools/bench_stream.py ...)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import infer_core, synth  # noqa: E402

LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=str, default="24,48,96")
    ap.add_argument("--first", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--text-tokens", type=int, default=105)
    ap.add_argument("--mel-tokens", type=int, default=480)
    ap.add_argument("--prompt-frames", type=int, default=511)
    ap.add_argument("--check-every", type=int, default=16)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt", "bigvgan"))
    g = cfg.gpt
    L, T = a.text_tokens, a.mel_tokens
    mel = torch.from_numpy(synth.prompt_mel(a.prompt_frames, seed=7)).to(eng.device)
    text = synth.text_ids(L, 11, g.number_text_tokens).astype(np.int32)
    spk = eng.ecapa(mel.transpose(1, 2))
    cond = eng.conditioning(mel)
    R = eng.vocoder_reach()
    up = eng.up_total

    def parent():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = eng.generate(cond, text[None], T, suppress_stop=True)[0]
        lat = eng.latent_packed(cond, [text], [codes])
        wav = eng.bigvgan_packed(lat, spk)[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(first=dt, total=dt, gaps=[], wav=wav.clone(), frames=T, appends=1, codes=codes)

    def streamed(chunk, recompute):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        voc = eng.bigvgan_stream(spk, chunk, min(a.first, chunk))
        stamps, parts, frames, appends, seen = [], [], 0, 0, []
        ls = None if recompute else eng.latent_stream(cond, [text], T)
        try:
            for new in eng.generate_stream(cond, text[None], T, check_every=a.check_every, suppress_stop=True):
                seen.append(new)
                if recompute:  # the whole prefix again, the new rows kept
                    done = np.concatenate(seen)
                    lat = eng.latent_packed(cond, [text], [done])[0][:, len(done) - len(new):]
                else:
                    lat = ls.append([new])[0]
                appends += 1
                lo = voc.plan.lo
                wav = voc.push(lat)
                if wav.shape[-1]:
                    frames += voc.plan.have - lo  # the window this push ran: every frame held, from the left context on
                    parts.append(wav)
                    torch.cuda.synchronize()
                    stamps.append(time.perf_counter() - t0)
            lo = voc.plan.lo
            wav = voc.push(None, last=True)
            if wav.shape[-1]:
                frames += voc.plan.have - lo
                parts.append(wav)
                torch.cuda.synchronize()
                stamps.append(time.perf_counter() - t0)
        finally:
            if ls is not None:
                ls.close()
        gaps = [b - x for x, b in zip(stamps, stamps[1:])]
        return dict(first=stamps[0], total=stamps[-1], gaps=gaps, wav=torch.cat(parts, -1), frames=frames, appends=appends)

    chunks = [int(c) for c in a.chunks.split(",") if c]
    forms = [("parent", parent)] + [(f"stream {c}", lambda c=c: streamed(c, False)) for c in chunks] + [(f"recompute {chunks[0]}", lambda: streamed(chunks[0], True))]
    say(f"one sentence, L = {L}, {T} forced codes ({T * up / 24000:.1f} s of audio), bf16, IndexTTS-1.5 dims, R = {R} frames, codes fetched every "
        f"{a.check_every} steps, first chunk {a.first} frames, decode mode {eng.decode_mode()}")
    res = {name: [] for name, _ in forms}
    base = None
    for rnd in range(a.rounds + 1):  # round 0: warm-up (every shape allocates its scratch there) and the bit comparison
        for name, fn in forms:
            r = fn()
            if rnd == 0:
                if name == "parent":
                    base = r["wav"]
                else:
                    same = r["wav"].shape == base.shape and torch.equal(r["wav"].view(torch.int32), base.view(torch.int32))
                    say(f"  {name}: {len(r['gaps']) + 1} chunks, {r['appends']} latent passes, vocoder frames computed / emitted {r['frames']} / {T} = "
                        f"{r['frames'] / T:.2f}; waveform equals the parent's bit for bit: {same}")
                continue
            res[name].append(r)
    for name, _ in forms:
        rs = res[name]
        best = min(rs, key=lambda r: r["total"])
        gaps = [x for r in rs for x in r["gaps"]]
        say(f"{name:<13s} first audio {min(r['first'] for r in rs) * 1e3:7.1f} ms   between chunks mean {np.mean(gaps) * 1e3 if gaps else 0.0:6.1f} ms max "
            f"{max(gaps) * 1e3 if gaps else 0.0:6.1f} ms   total best {best['total'] * 1e3:7.1f} ms median {float(np.median([r['total'] for r in rs])) * 1e3:7.1f} ms "
            f"over {len(rs)} runs")
    p = min(r["total"] for r in res["parent"])
    for name, _ in forms[1:]:
        say(f"{name}: total / parent total = {min(r['total'] for r in res[name]) / p:.3f}, first audio / parent first audio = "
            f"{min(r['first'] for r in res[name]) / min(r['first'] for r in res['parent']):.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
