#!/usr/bin/env python3
"""Time per token step of beam_sample (3 beams) with top_k = 0 (HF: TopK warper off) and top_k = 200, top_p = 0.8 at IndexTTS-1.5
sizes, bf16, 1 and 2 batch items, stop token suppressed: Engine.generate(wide_beam_sampler="host") - warpers and draws on the
host, a logits + beam-state read-back and two stream syncs per token - against wide_beam_sampler="device" (beam_wide_cand_kernel
+ beam_wide_pick_kernel + beam_select_kernel behind the decode step, graph replay), alternated in one process, with top_k = 30
(the narrow device pair) as context.
    python tools/bench_wide_beam_sampler.py [--steps 100] [--rounds 5] [--items 1 2] [--beams 3] [--device-only]
--device-only: the device form alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python
tools/bench_wide_beam_sampler.py --device-only --items 2 --rounds 1)."""
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--items", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--top-k", type=int, nargs="+", default=[0, 200])
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",))
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    nb = a.beams
    for items in a.items:
        text = np.stack([synth.text_ids(40, 21 + i, cfg.gpt.number_text_tokens) for i in range(items)]).astype(np.int32)
        u = np.random.default_rng(3).random((a.steps, items, 2 * nb), dtype=np.float32)
        modes = []
        for tk in a.top_k:
            if not a.device_only:
                modes.append((f"host   top_k={tk}", dict(top_k=tk, wide_beam_sampler="host")))
            modes.append((f"device top_k={tk}", dict(top_k=tk, wide_beam_sampler="device")))
        if not a.device_only:
            modes.append(("device top_k=30", dict(top_k=30)))

        def run(kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = eng.generate(cond, text, a.steps, suppress_stop=True, do_sample=True, num_beams=nb, top_p=0.8, temperature=1.0,
                               uniforms=u, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ids

        ids = {}
        for name, kw in modes:  # warm-up: graph capture, allocations
            ids[name] = run(kw)[1]
        times = {name: [] for name, _ in modes}
        for _ in range(a.rounds):
            for name, kw in modes:
                times[name].append(run(kw)[0])
        print(f"items {items} x {nb} beams = {items * nb} rows, {a.steps} token steps (prefill included), decode_mode {eng.decode_mode()}")
        for name, _ in modes:
            t = sorted(times[name])
            print(f"  {name:17s} ms per step: min {t[0] / a.steps:.4f}  median {t[len(t) // 2] / a.steps:.4f}  max {t[-1] / a.steps:.4f}"
                  f"   ({len(t)} generations)")
        if not a.device_only:
            for tk in a.top_k:
                h, d = ids[f"host   top_k={tk}"], ids[f"device top_k={tk}"]
                n = min(h.shape[1], d.shape[1])
                same = bool(np.array_equal(h[:, :n], d[:, :n]))
                print(f"  top_k={tk}: host and device best hypotheses (same uniforms) {'equal' if same else 'differ'}")


if __name__ == "__main__":
    main()
