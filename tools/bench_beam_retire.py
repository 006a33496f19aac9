#!/usr/bin/env python3
"""Retirement of finished beam groups (Engine.generate(retire_rows=, retire_beams=True), opt-in) against the same generation
without it.

    python tools/bench_beam_retire.py [--items 21] [--beams 3] [--max-gen 480] [--stop-bias 3.0] [--ratio 0.5] [--repeat 2]

Full dims, bf16, a synthetic checkpoint (synth.gpt_state_dict(profile="smooth", stop_bias=..)) whose beam groups finish on their
own at different steps; `items` ragged texts x `beams` beams = the rows one `infer_batch` generation of the default kwargs carries
(max_batch 64 // 3 = 21 sentences).  One generation is Engine.generate's loop: prefill, status() every 16 steps and - with the
switch - retire_rows() whenever unfinished <= ratio * rows() and rows() > 6, until every group is done.  The two settings are
alternated `--repeat` times in one process on one engine object, after a warm-up.  Printed per run: total decode ms (prefill
excluded), token steps, the row-count trace as (rows, steps, ms per step) stretches and every retire_rows() call with its time;
once: the spread of the steps at which the groups became done (from the yardstick's status checks, so in units of 16 steps), and
how many items' codes differ from the yardstick's (retirements that cross a kernel family may flip a near-tie).
Run it under a time limit (timeout -k 10 900 python tools/bench_beam_retire.py ...); profiles/beam_retire.txt holds a record."""
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
from itts_hip import synth  # noqa: E402

CHECK_EVERY = 16


def one_run(eng, cond, text, max_gen, nb, u, ratio):
    """Engine.generate's loop with a clock -> dict(total_ms, steps, stretches, retires, done_at, codes)"""
    items = text.shape[0]
    eng.set_beam_sample(nb, 30, 0.8, 1.0, u)
    if ratio:
        eng.set_retire_beams(True)
    try:
        eng.prefill(cond, text, max_gen, 10.0, False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done, stretches, retires, done_at = 1, [], [], {}
        seg_t, seg_steps = t0, 0
        while done < max_gen:
            step, unf = eng.status()
            if not ratio:  # the yardstick also records when the groups became done (status() is part of both loops; this is not)
                orig, _, live = eng.row_status()
                for i in range(items):
                    if not live[i * nb]:
                        done_at.setdefault(i, step)
            if unf == 0:
                break
            rows = eng.rows()
            if ratio and rows > 6 and unf <= ratio * rows:
                now = time.perf_counter()
                if seg_steps:
                    stretches.append((rows, seg_steps, (now - seg_t) * 1e3))
                got = eng.retire_rows()
                tb = time.perf_counter()
                retires.append((rows, got, step, (tb - now) * 1e3))
                seg_t, seg_steps = tb, 0
            n = min(CHECK_EVERY, max_gen - done)
            eng.decode(n)
            done += n
            seg_steps += n
        step, unf = eng.status()
        t1 = time.perf_counter()
        if seg_steps:
            stretches.append((eng.rows(), seg_steps, (t1 - seg_t) * 1e3))
        codes = eng.fetch()[:, :step].copy()
        eng._exit()
    finally:
        eng.set_beam_sample(1)
        eng.set_retire_beams(False)
    return dict(total_ms=(t1 - t0) * 1e3, steps=step, stretches=stretches, retires=retires, done_at=done_at, codes=codes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=21)
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--max-gen", type=int, default=480)
    ap.add_argument("--stop-bias", type=float, default=3.0)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    sd = synth.gpt_state_dict(cfg, 1234, profile="smooth", stop_bias=a.stop_bias)
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",), state_dicts={"gpt": sd}, max_batch=a.items * a.beams)
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    lens = np.random.default_rng(a.seed).integers(20, 106, a.items)
    text = np.full((a.items, 105), cfg.gpt.stop_text_token, np.int32)
    for i, n in enumerate(lens):
        text[i, :n] = synth.text_ids(int(n), 900 + i, cfg.gpt.number_text_tokens)
    u = np.random.default_rng(a.seed + 1).random((a.max_gen, a.items, 2 * a.beams), dtype=np.float32)
    print(f"# bench_beam_retire: {a.items} items x {a.beams} beams = {a.items * a.beams} rows, bf16, full dims, text lengths "
          f"{int(lens.min())} .. {int(lens.max())}, max_gen {a.max_gen}, stop_bias {a.stop_bias}, beam_sample top_k 30 top_p 0.8, "
          f"status() every {CHECK_EVERY} steps, ratio {a.ratio}")
    one_run(eng, cond, text, a.max_gen, a.beams, u, 0.0)  # warm-up: tiles, graphs, allocations
    results, base = {0.0: [], a.ratio: []}, None
    for rep in range(a.repeat):
        for r in (0.0, a.ratio):
            res = one_run(eng, cond, text, a.max_gen, a.beams, u, r)
            results[r].append(res["total_ms"])
            if base is None and not r:
                base = res["codes"]
                d = sorted(res["done_at"].values())
                print(f"done steps of the groups as the status checks saw them: {d}; {a.items - len(d)} open at the end; spread "
                      f"{d[0] if d else '-'} .. {d[-1] if d else '-'}")
            w = min(base.shape[1], res["codes"].shape[1])  # (the loops end at the same status check unless a code differs)
            diff = int(np.any(res["codes"][:, :w] != base[:, :w], axis=1).sum())
            print(f"run {rep} {'retire_rows=%g retire_beams' % r if r else 'off'}: decode total {res['total_ms']:.1f} ms over {res['steps']} "
                  f"token steps; items whose codes differ from the yardstick: {diff}")
            print("    rows: " + ", ".join(f"{rows} x {steps} steps ({ms / steps:.3f} ms)" for rows, steps, ms in res["stretches"]))
            for rb, ra, step, ms in res["retires"]:
                print(f"    retire_rows() at step {step}: {rb:3d} -> {ra:3d} rows, {ms:.2f} ms")
    off, on = results[0.0], results[a.ratio]
    print("summary off: decode total " + " / ".join(f"{x:.1f}" for x in off) + " ms")
    print(f"summary retire_rows={a.ratio:g} retire_beams: decode total " + " / ".join(f"{x:.1f}" for x in on) +
          f" ms; best vs best of off: {min(off) / min(on):.3f}x")


if __name__ == "__main__":
    main()
