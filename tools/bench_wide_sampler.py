#!/usr/bin/env python3
"""Time per token step of do_sample with top_k = 0 (HF: TopK warper off), top_p = 0.8 at IndexTTS-1.5 sizes, bf16, 1 and 2 rows,
stop token suppressed: Engine.generate(wide_sampler="host") - the token choice on the host, one logits read-back and stream
sync per token - against wide_sampler="device" (sampler_wide_kernel behind the decode step, graph replay), alternated in one
process, with top_k = 30 (the narrow device sampler) as context.
    python tools/bench_wide_sampler.py [--steps 200] [--rounds 3] [--rows 1 2] [--device-only] [--select]
--select: the sorted kernel against the sort-free one (ITTS_WIDE_SELECT) instead, alternated in this process at
V = 8194: itts_sample_rows against itts_sample_rows_select at 1, 2 and 64 rows (device events around --launches launches; both
entries enqueue the same memsets in front of their kernel), then the token step with Engine.set_wide_select off and on.
profiles/wide_select.txt holds a record.
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


def select_leg(a, cfg, eng, cond):
    import ctypes as C

    from itts_hip import lib as L
    lib, V, dev = L.load(), cfg.gpt.number_mel_codes, "cuda:0"
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rows in (1, 2, 64):
        g = torch.Generator(device="cpu").manual_seed(5)
        lg = (torch.randn((rows, V), generator=g) * 2.5).to(dev)
        u = torch.rand((rows,), generator=g).to(dev)
        tok, kept = (torch.zeros(rows, dtype=torch.int32, device=dev) for _ in range(2))
        scratch = torch.empty(rows * (V + 16), dtype=torch.uint8, device=dev)

        def launches(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                st = fn(tok.data_ptr(), kept.data_ptr(), lg.data_ptr(), None, rows, V, 1.0, V - 2, 0, 0, 0, 0.8, 1.0, u.data_ptr(),
                        scratch.data_ptr(), scratch.numel(), stream)
            e1.record()
            torch.cuda.synchronize()
            L.check(st, "bench_wide_sampler", lib)
            return e0.elapsed_time(e1) * 1e3 / n, tok.cpu().numpy().copy(), kept.cpu().numpy().copy()

        forms = (("sampler_wide_kernel  ", lib.itts_sample_rows), ("sampler_select_kernel", lib.itts_sample_rows_select))
        res = {name: launches(fn, 20) for name, fn in forms}  # warm-up
        times = {name: [] for name, _ in forms}
        for _ in range(a.rounds):
            for name, fn in forms:
                times[name].append(launches(fn, a.launches)[0])
        same = all(np.array_equal(x, y) for x, y in zip(res[forms[0][0]][1:], res[forms[1][0]][1:]))
        print(f"operator, rows {rows}, V {V}, top_k 0, top_p 0.8: us per call (4 memsets + the kernel), {a.launches} calls per timing")
        for name, _ in forms:
            t = sorted(times[name])
            print(f"  {name} min {t[0]:8.2f}  median {t[len(t) // 2]:8.2f}  max {t[-1]:8.2f}")
        print(f"  tokens and kept counts of the two forms {'equal' if same else 'differ'}")
    for rows in a.rows:
        text = np.stack([synth.text_ids(40, 21 + i, cfg.gpt.number_text_tokens) for i in range(rows)]).astype(np.int32)
        u = np.random.default_rng(3).random((a.steps, rows), dtype=np.float32)

        def run(on):
            eng.set_wide_select(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = eng.generate(cond, text, a.steps, suppress_stop=True, do_sample=True, top_k=0, top_p=0.8, temperature=1.0, uniforms=u,
                               wide_sampler="device")
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ids
        ids = {on: run(on)[1] for on in (False, True)}
        times = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                times[on].append(run(on)[0])
        eng.set_wide_select(False)
        print(f"token step, rows {rows}, {a.steps} steps (prefill included), decode_mode {eng.decode_mode()}")
        for on in (False, True):
            t = sorted(times[on])
            print(f"  wide_select {'on ' if on else 'off'} ms per step: min {t[0] / a.steps:.4f}  median {t[len(t) // 2] / a.steps:.4f}  max {t[-1] / a.steps:.4f}")
        print(f"  ids of the two forms (same uniforms) {'equal' if np.array_equal(ids[False], ids[True]) else 'differ'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--select", action="store_true")
    ap.add_argument("--launches", type=int, default=2000)
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",))
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    if a.select:
        return select_leg(a, cfg, eng, cond)
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
