#!/usr/bin/env python3
"""Mixed decode batches (IndexTTS(mixed_batch=True), opt-in) against infer_batch without the switch.

    python tools/bench_mixed_batch.py [--utterances 32] [--voices 8] [--text-tokens 60] [--max-mel-tokens 150] [--rounds 2]
    python tools/bench_mixed_batch.py --sampler-kernels [--rows 64] [--launches 200] [--rounds 3]

Default mode: full IndexTTS-1.5 dims, IEEE-half engine, PRNG weights.  `--utterances` one-sentence utterances of `--voices` prompt
objects carry 4 single-beam settings (greedy; top_k 30 / top_p 0.8; top_k 5 / temperature 0.7 / penalty 2; top_k 100 / top_p 0.95 /
temperature 1.2), utterance u voice u % voices and setting (u // voices) % 4, through ONE IndexTTS object's infer_batch with the
switch off and on (ITTS_MIXED_BATCH is flipped between the calls), alternated `--rounds` times after one warm-up call of each.  PRNG
weights never emit the stop token, so every row runs to `--max-mel-tokens`: both forms synthesise the same amount of audio.  Printed
per form: generations (Engine.generate calls) and decode rows per call, the best and the median wall time, audio-s/s.

--sampler-kernels: the time per launch of the three single-beam sampler kernels in their scalar form (itts_sampler_step: greedy;
top_k 30; top_k 0) at `--rows` rows and the 1.5 vocabulary, device events around `--launches` back-to-back launches, `--rounds` times.
Run it once per library (ITTS_HIP_LIB) and alternate the runs to compare two builds.
Run under a time limit (timeout -k 10 900 python tools/bench_mixed_batch.py ...); profiles/mixed_batch.txt holds a record."""
import argparse
import ctypes as C
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
from itts_hip import lib as L  # noqa: E402
from itts_hip import synth  # noqa: E402

SETTINGS = (dict(do_sample=False), dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0),
            dict(do_sample=True, top_k=5, top_p=0.9, temperature=0.7, repetition_penalty=2.0),
            dict(do_sample=True, top_k=100, top_p=0.95, temperature=1.2))


def sampler_kernels(a):
    cfg = icfg.indextts_1_5()
    V, B, mg = cfg.gpt.number_mel_codes, a.rows, 4
    # the one entry this mode needs, bound by hand: a library built from an earlier commit lacks entries lib.load() would bind
    lib = C.CDLL(L.LIB_PATH)
    lib.itts_sampler_step.restype, lib.itts_sampler_step.argtypes = L._PROTOS["itts_sampler_step"]
    lib.itts_last_error.restype = C.c_char_p
    dev = "cuda:0"
    g = torch.Generator().manual_seed(3)
    t = dict(logits=torch.randn(B, V, generator=g) * 2.0, seen=(torch.rand(B, V, generator=g) < 0.01).to(torch.uint8),
             ids=torch.zeros(B, mg, dtype=torch.int32), cur_tok=torch.zeros(B, dtype=torch.int32), unfinished=torch.ones(B, dtype=torch.int32),
             step=torch.full((B,), mg, dtype=torch.int32),  # past the end: a launch computes its choice and commits nothing, so launches repeat
             uniforms=torch.rand(mg, B, generator=g))
    t = {k: v.to(dev) for k, v in t.items()}
    args = L.SamplerStepArgs()
    for k, v in t.items():
        setattr(args, k, v.data_ptr())
    args.B, args.V, args.max_gen, args.stop, args.penalty = B, V, mg, cfg.gpt.stop_mel_token, 10.0
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"{os.path.basename(L.LIB_PATH)}: {B} rows, V {V}, {a.launches} launches per figure, us per launch")
    for name, (ds, k) in (("sampler2_kernel (greedy)", (0, 0)), ("sampler_sample_kernel (top_k 30)", (1, 30)), ("sampler_wide_kernel (top_k 0)", (1, 0))):
        args.do_sample, args.top_k, args.top_p, args.temperature = ds, k, 0.8, 1.0
        out = []
        for r in range(a.rounds + 1):  # round 0: warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                L.check(lib.itts_sampler_step(C.byref(args), s), "sampler_step", lib)
            e1.record()
            torch.cuda.synchronize()
            if r:
                out.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        print(f"  {name:34s} {' '.join(f'{x:7.2f}' for x in out)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=32)
    ap.add_argument("--voices", type=int, default=8)
    ap.add_argument("--text-tokens", type=int, default=60)
    ap.add_argument("--max-mel-tokens", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sampler-kernels", action="store_true")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if a.sampler_kernels:
        return sampler_kernels(a)
    from indextts.infer import IndexTTS

    cfg = icfg.indextts_1_5()
    sds = {"gpt": synth.gpt_state_dict(cfg, 1234), "bigvgan": synth.bigvgan_state_dict(cfg, 1234)}
    tts = IndexTTS(cfg=cfg, model_dir="/nonexistent", is_fp16=True, state_dicts=sds)
    mels = [torch.from_numpy(synth.prompt_mel(511, seed=7 + v)) for v in range(a.voices)]
    n = a.utterances
    prompts = [mels[u % a.voices] for u in range(n)]
    per = [dict(SETTINGS[(u // a.voices) % len(SETTINGS)], seed=100 + u) for u in range(n)]
    texts = [[synth.text_ids(a.text_tokens - (u * 7) % 23, 11 + u, cfg.gpt.number_text_tokens).astype(np.int32)] for u in range(n)]
    calls = []
    real = tts.engine.generate
    tts.engine.generate = lambda cond, ids, *r, **k: (calls.append(int(np.asarray(ids).shape[0])), real(cond, ids, *r, **k))[1]

    def run(on):
        os.environ["ITTS_MIXED_BATCH"] = "1" if on else "0"
        calls.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # max_mel_tokens reached: PRNG weights never stop
            out = tts.infer_batch(prompts, texts, num_beams=1, max_mel_tokens=a.max_mel_tokens, per_utterance=per)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, sum(w.shape[0] for _, w in out) / 24000.0, list(calls)

    print(f"{n} utterances, {a.voices} voices, {len(SETTINGS)} settings, text {a.text_tokens - 22} .. {a.text_tokens} tokens, {a.max_mel_tokens} mel "
          f"tokens per row, IndexTTS-1.5 dims, {tts.half}")
    times = {False: [], True: []}
    info = {}
    for rnd in range(a.rounds + 1):  # round 0: warm-up (graph captures, scratch of every shape)
        for on in (False, True):
            dt, audio, c = run(on)
            info[on] = (audio, c)
            if rnd:
                times[on].append(dt)
    for on in (False, True):
        audio, c = info[on]
        t = times[on]
        print(f"mixed_batch {'on ' if on else 'off'}: {len(c)} generations, rows per generation {sorted(c, reverse=True)[:8]}{' ...' if len(c) > 8 else ''} "
              f"({sum(c)} rows); {audio:.1f} s of audio; wall s {' '.join(f'{x:.2f}' for x in t)}; best {audio / min(t):.1f} audio-s/s, "
              f"median {audio / float(np.median(t)):.1f}")
    print(f"on / off (best audio-s/s): {min(times[False]) / min(times[True]):.2f} x")


if __name__ == "__main__":
    main()
