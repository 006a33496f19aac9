#!/usr/bin/env python3
"""Time per token step of beam_sample (3 beams) with top_k = 0 (HF: TopK warper off) and top_k = 200, top_p = 0.8 at IndexTTS-1.5
sizes, bf16, 1 and 2 batch items, stop token suppressed: Engine.generate(wide_beam_sampler="host") - warpers and draws on the
host, a logits + beam-state read-back and two stream syncs per token - against wide_beam_sampler="device" (beam_wide_cand_kernel
+ beam_wide_pick_kernel + beam_select_kernel behind the decode step, graph replay), alternated in one process, with top_k = 30
(the narrow device pair) as context.
    python tools/bench_wide_beam_sampler.py [--steps 100] [--rounds 5] [--items 1 2] [--beams 3] [--device-only] [--select]
--select: the sorted first launch against the sort-free one (ITTS_WIDE_SELECT) instead, alternated in this process
at V = 8194: itts_beam_sample_rows against itts_beam_sample_rows_select at 1 and 10 items (device events around --launches calls;
both enqueue the same two memsets and beam_wide_pick_kernel), then the beam token step with Engine.set_wide_select off and on.
profiles/wide_select.txt holds a record.
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


def select_leg(a, cfg, eng, cond):
    import ctypes as C

    from itts_hip import lib as L
    lib, V, nb, dev = L.load(), cfg.gpt.number_mel_codes, a.beams, "cuda:0"
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for items in (1, 10):
        rows = items * nb
        g = torch.Generator(device="cpu").manual_seed(5)
        lg = (torch.randn((rows, V), generator=g) * 2.5).to(dev)
        bs = (-torch.rand((rows,), generator=g)).to(dev)
        u = torch.rand((items, 2 * nb), generator=g).to(dev)
        psc = torch.zeros((items, 2 * nb), dtype=torch.float32, device=dev)
        ptok, pbeam = (torch.zeros((items, 2 * nb), dtype=torch.int32, device=dev) for _ in range(2))
        kept = torch.zeros(rows, dtype=torch.int32, device=dev)
        scratch = torch.empty(rows * (V + 1) + items, dtype=torch.float32, device=dev)

        def launches(fn, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                st = fn(psc.data_ptr(), ptok.data_ptr(), pbeam.data_ptr(), kept.data_ptr(), lg.data_ptr(), None, 0, 0, bs.data_ptr(), items,
                        nb, V, 10.0, V - 2, 1, V - 3, 1, 0, 0, 0.8, 1.0, u.data_ptr(), scratch.data_ptr(), scratch.numel() * 4, stream)
            e1.record()
            torch.cuda.synchronize()
            L.check(st, "bench_wide_beam_sampler", lib)
            return e0.elapsed_time(e1) * 1e3 / n, [x.cpu().numpy().copy() for x in (ptok, pbeam, kept)]

        forms = (("beam_wide_cand_kernel    ", lib.itts_beam_sample_rows), ("beam_wide_cand_sel_kernel", lib.itts_beam_sample_rows_select))
        res = {name: launches(fn, 20) for name, fn in forms}  # warm-up
        times = {name: [] for name, _ in forms}
        for _ in range(a.rounds):
            for name, fn in forms:
                times[name].append(launches(fn, a.launches)[0])
        same = all(np.array_equal(x, y) for x, y in zip(res[forms[0][0]][1], res[forms[1][0]][1]))
        print(f"operator, {items} items x {nb} beams, V {V}, top_k 0, top_p 0.8: us per call (2 memsets, the kernel, beam_wide_pick_kernel), "
              f"{a.launches} calls per timing")
        for name, _ in forms:
            t = sorted(times[name])
            print(f"  {name} min {t[0]:8.2f}  median {t[len(t) // 2]:8.2f}  max {t[-1]:8.2f}")
        print(f"  picks and kept counts of the two forms {'equal' if same else 'differ'}")
    for items in a.items:
        text = np.stack([synth.text_ids(40, 21 + i, cfg.gpt.number_text_tokens) for i in range(items)]).astype(np.int32)
        u = np.random.default_rng(3).random((a.steps, items, 2 * nb), dtype=np.float32)

        def run(on):
            eng.set_wide_select(on)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = eng.generate(cond, text, a.steps, suppress_stop=True, do_sample=True, num_beams=nb, top_k=0, top_p=0.8, temperature=1.0,
                               uniforms=u, wide_beam_sampler="device")
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, ids
        ids = {on: run(on)[1] for on in (False, True)}
        times = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                times[on].append(run(on)[0])
        eng.set_wide_select(False)
        print(f"beam token step, {items} items x {nb} beams, {a.steps} steps (prefill included), decode_mode {eng.decode_mode()}")
        for on in (False, True):
            t = sorted(times[on])
            print(f"  wide_select {'on ' if on else 'off'} ms per step: min {t[0] / a.steps:.4f}  median {t[len(t) // 2] / a.steps:.4f}  max {t[-1] / a.steps:.4f}")
        n = min(ids[False].shape[1], ids[True].shape[1])
        print(f"  best hypotheses of the two forms (same uniforms) {'equal' if np.array_equal(ids[False][:, :n], ids[True][:, :n]) else 'differ'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--items", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--top-k", type=int, nargs="+", default=[0, 200])
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--select", action="store_true")
    ap.add_argument("--launches", type=int, default=1000)
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",))
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    nb = a.beams
    if a.select:
        return select_leg(a, cfg, eng, cond)
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
