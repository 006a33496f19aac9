#!/usr/bin/env python3
"""Row admission into a running batched decode (Engine.generate(slots=..), opt-in) against decoding the same requests as separate
generations.

    python tools/bench_admit_rows.py [--requests 192] [--slots 64] [--admit-min 0.125,0.25,0.5] [--repeat 2] [--max-gen 480]
                                     [--text-len 105] [--gpt-fp8]

Full IndexTTS-1.5 dims, PRNG weights.  Every request is forced to stop at a step drawn once from a seeded uniform spread over
120 .. max_gen - 1 (forced tokens under suppress_stop=True, so nothing else stops a row).  Settings, alternated `--repeat` times in
one process on one engine object:
  sep          requests / slots generations of `slots` rows each, one after the other, each to its slowest row (status() every 16
               steps; what infer_batch does today)
  sep+retire   the same with retire_rows = 0.5 (tools/bench_row_retire.py's loop)
  admit r      ONE generation of `slots` rows, Engine.generate(slots=, admit_min=r, retire_rows=0.5): finished rows' slots take the
               waiting requests, retirement handles the tail
Printed per run: the wall time of everything (prefills and admissions included), the time inside prefill() and inside admit_rows(),
and "decode" = the rest; the token steps launched; for the admit runs every admission's group size and host-clock time.  Then one
summary line per setting and the admit_rows() cost by group size.  Run it under a time limit
(timeout -k 10 900 python tools/bench_admit_rows.py ...); profiles/admit_rows.txt holds a record."""
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


class Clock:
    """wall time spent inside eng.prefill / eng.admit_rows (both return synchronised) and the decode steps launched"""

    def __init__(self, eng):
        self.eng, self.t = eng, dict(prefill=0.0, admit=0.0)
        self.admits, self.steps = [], 0
        self.real = dict(prefill=eng.prefill, admit_rows=eng.admit_rows, decode=eng.decode)

    def __enter__(self):
        def prefill(*a, **k):
            t0 = time.perf_counter()
            r = self.real["prefill"](*a, **k)
            torch.cuda.synchronize()
            self.t["prefill"] += time.perf_counter() - t0
            return r

        def admit_rows(cond, text_ids, *a, **k):
            t0 = time.perf_counter()
            r = self.real["admit_rows"](cond, text_ids, *a, **k)
            dt = time.perf_counter() - t0
            self.t["admit"] += dt
            self.admits.append((len(text_ids), dt * 1e3))
            return r

        def decode(n):
            self.steps += n
            return self.real["decode"](n)

        self.eng.prefill, self.eng.admit_rows, self.eng.decode = prefill, admit_rows, decode
        return self

    def __exit__(self, *exc):
        self.eng.prefill, self.eng.admit_rows, self.eng.decode = self.real["prefill"], self.real["admit_rows"], self.real["decode"]


def separate(eng, cond, text, forced, max_gen, slots, ratio):
    """the requests as generations of `slots` rows, each to its slowest row -> codes [N, max_gen] (stop-padded)"""
    out = np.full((text.shape[0], max_gen), eng.ccfg.stop_mel_token, np.int64)
    for lo in range(0, text.shape[0], slots):
        eng.set_forced(forced[lo:lo + slots])
        eng.prefill(cond, text[lo:lo + slots], max_gen, 10.0, True)
        done = 1
        while done < max_gen:
            step, unf = eng.status()
            if unf == 0:
                break
            rows = eng.rows()
            if ratio and rows > 6 and unf <= ratio * rows:
                eng.retire_rows()
            n = min(CHECK_EVERY, max_gen - done)
            eng.decode(n)
            done += n
        step, _ = eng.status()
        out[lo:lo + slots, :step] = eng.fetch()[:, :step]
        eng._exit()
    eng.set_forced(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=192)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--admit-min", default="0.125,0.25,0.5")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--max-gen", type=int, default=480)
    ap.add_argument("--text-len", type=int, default=105)
    ap.add_argument("--gpt-fp8", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    mins = [float(x) for x in a.admit_min.split(",")]
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",), gpt_fp8="fp8" if a.gpt_fp8 else "", max_batch=a.slots)
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    N = a.requests
    text = np.stack([synth.text_ids(a.text_len, 900 + i, cfg.gpt.number_text_tokens) for i in range(N)]).astype(np.int32)
    stop_step = np.random.default_rng(a.seed).integers(120, a.max_gen, N)
    forced = np.full((N, a.max_gen), -1, np.int32)
    forced[np.arange(N), stop_step] = cfg.gpt.stop_mel_token
    ideal = int(np.ceil((stop_step + 1).sum() / a.slots))
    print(f"# bench_admit_rows: {N} requests, {a.slots} slots, gpt_fp8 {bool(a.gpt_fp8)}, L {a.text_len}, max_gen {a.max_gen}, forced stop "
          f"steps {int(stop_step.min())} .. {int(stop_step.max())} (seed {a.seed}, mean {float(stop_step.mean()):.0f}); "
          f"row-steps / slots = {ideal} token steps if no slot ever idled; status() every {CHECK_EVERY} steps")
    settings = [("sep", None), ("sep+retire", None)] + [(f"admit {r:g}", r) for r in mins]

    def run(name, r):
        with Clock(eng) as ck:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if r is None:
                codes = separate(eng, cond, text, forced, a.max_gen, a.slots, 0.5 if name == "sep+retire" else 0.0)
            else:
                eng.set_forced(forced)  # one row per request: generate(slots=) hands every request its own
                try:
                    codes = eng.generate(cond, text, a.max_gen, suppress_stop=True, check_every=CHECK_EVERY, slots=a.slots, admit_min=r,
                                         retire_rows=0.5)
                finally:
                    eng.set_forced(None)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
        return dict(total=total * 1e3, prefill=ck.t["prefill"] * 1e3, admit=ck.t["admit"] * 1e3, steps=ck.steps, admits=ck.admits, codes=codes)

    run("sep", None)  # warm-up: tiles, graphs, allocations
    run(settings[-1][0], settings[-1][1])
    results = {name: [] for name, _ in settings}
    by_size = {}
    base = None
    for rep in range(a.repeat):
        for name, r in settings:
            res = run(name, r)
            if base is None:
                base = res["codes"]
            w = min(base.shape[1], res["codes"].shape[1])
            diff = int(np.any(res["codes"][:, :w] != base[:, :w], axis=1).sum())
            decode = res["total"] - res["prefill"] - res["admit"]
            results[name].append((res["total"], decode))
            print(f"run {rep} {name}: total {res['total']:.1f} ms = prefill {res['prefill']:.1f} + admit_rows {res['admit']:.1f} + decode "
                  f"{decode:.1f}; {res['steps']} token steps launched; requests whose codes differ from the first run's: {diff}")
            if res["admits"]:
                print("    admissions (rows: ms): " + ", ".join(f"{n}: {ms:.1f}" for n, ms in res["admits"]))
            for n, ms in res["admits"]:
                by_size.setdefault(n, []).append(ms)
    off = min(t for t, _ in results["sep"])
    for name, _ in settings:
        tot, dec = [t for t, _ in results[name]], [d for _, d in results[name]]
        print(f"summary {name}: total " + " / ".join(f"{x:.1f}" for x in tot) + " ms, decode " + " / ".join(f"{x:.1f}" for x in dec) +
              f" ms; best total vs best of sep: {off / min(tot):.3f}x")
    print("admit_rows() host clock by group size (rows: calls, min / median ms): " +
          ", ".join(f"{n}: {len(v)}, {min(v):.1f} / {float(np.median(v)):.1f}" for n, v in sorted(by_size.items())))


if __name__ == "__main__":
    main()
