#!/usr/bin/env python3
"""Time per token step of do_sample with top_k = 0 (HF: TopK warper off), top_p = 0.8 at IndexTTS-1.5 sizes, bf16, 1 and 2 rows,
stop token suppressed: Engine.generate(wide_sampler="host") - the token choice on the host, one logits read-back and stream
sync per token - against wide_sampler="device" (sampler_wide_kernel behind the decode step, graph replay), alternated in one
process, with top_k = 30 (the narrow device sampler) as context.
    python tools/bench_wide_sampler.py [--steps 200] [--rounds 3] [--rows 1 2] [--device-only]
--device-only: the device form alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/bench_wide_sampler.py
--device-only --rows 2 --rounds 1)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "index-tts-ipex_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",))
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    modes = [("device top_k=0", dict(top_k=0, wide_sampler="device"))]
    if not a.device_only:
        modes = [("host   top_k=0", dict(top_k=0, wide_sampler="host"))] + modes + [("device top_k=30", dict(top_k=30))]
    for rows in a.rows:
        text = np.stack([synth.text_ids(40, 21 + i, cfg.gpt.number_text_tokens) for i in range(rows)]).astype(np.int32)
        u = np.random.default_rng(3).random((a.steps, rows), dtype=np.float32)

        def run(kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = eng.generate(cond, text, a.steps, suppress_stop=True, do_sample=True, top_p=0.8, temperature=1.0, uniforms=u, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ids

        ids = {}
        for name, kw in modes:  # warm-up: graph capture, allocations
            ids[name] = run(kw)[1]
        times = {name: [] for name, _ in modes}
        for _ in range(a.rounds):
            for name, kw in modes:
                times[name].append(run(kw)[0])
        print(f"rows {rows}, {a.steps} token steps (prefill included), decode_mode {eng.decode_mode()}")
        for name, _ in modes:
            t = times[name]
            print(f"  {name:16s} ms per generation {' '.join(f'{x:8.2f}' for x in t)}   ms per step (median) {sorted(t)[len(t) // 2] / a.steps:.4f}")
        if not a.device_only:
            h, d = ids["host   top_k=0"], ids["device top_k=0"]
            first = int(np.argmax((h != d).any(0))) if (h != d).any() else -1
            print(f"  host and device ids (same uniforms) part at step {first} (-1: never); before it they are equal")


if __name__ == "__main__":
    main()
