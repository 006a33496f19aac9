#!/usr/bin/env python3
"""Row admission under beams (Engine.generate(slots=S, num_beams=nb, admit_beams=True), opt-in) against decoding the same requests
as separate beam generations of S items, with and without the retirement of finished beam groups.

    python tools/bench_admit_beams.py [--requests 63] [--slots 21] [--beams 3] [--max-gen 480] [--stop-bias 3.0] [--repeat 2]

Full dims, bf16, a synthetic checkpoint (synth.gpt_state_dict(profile="smooth", stop_bias=..)) whose beam groups finish on their
own at different steps; `requests` ragged texts x `beams` beams through `slots` item slots: what IndexTTS.infer_batch of the default
kwargs decodes when it holds three times the sentences of one generation (max_batch 64 // 3 = 21).  Settings:
    sep           requests / slots generations of `slots` items each (the longest texts first, as the admitting run starts)
    sep+retire    the same with retire_rows=0.5, retire_beams=True
    admit r       ONE generation of `slots` item slots, admit_min = r (1/8, 1/4, 1/2)
All through Engine.generate with status checks every 16 steps, alternated `--repeat` times in one process on one engine object after
a warm-up of each.  Printed per run: total ms (prefills and admissions included), the time inside admit_rows(), token steps
launched, the admissions as (items: ms); at the end admit_rows()'s host clock by item count and, once, the spread of the token
counts at which the first generation's groups were seen done.
Run it under a time limit (timeout -k 10 900 python tools/bench_admit_beams.py ...); profiles/admit_beams.txt holds a record."""
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
    """Counts the token steps an engine object launches and clocks its admit_rows() calls (which synchronise themselves)."""

    def __init__(self, eng):
        self.eng, self.steps, self.admits = eng, 0, []
        self._decode, self._admit = eng.decode, eng.admit_rows
        eng.decode, eng.admit_rows = self.decode, self.admit_rows

    def decode(self, n):
        self.steps += n
        return self._decode(n)

    def admit_rows(self, cond, text_ids, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self._admit(cond, text_ids, **kw)
        self.admits.append((len(text_ids), (time.perf_counter() - t0) * 1e3))
        return out

    def close(self):
        self.eng.decode, self.eng.admit_rows = self._decode, self._admit


def one_run(eng, cond, text, u, a, setting):
    """-> dict(total_ms, admit_ms, steps, admits [(items, ms)], codes [N, n])"""
    N, S, nb = text.shape[0], a.slots, a.beams
    kw = dict(num_beams=nb, do_sample=True, top_k=30, top_p=0.8, temperature=1.0, check_every=CHECK_EVERY)
    lens = [int(np.count_nonzero(r != eng.ccfg.stop_text_token)) for r in text]
    order = sorted(range(N), key=lambda i: (-lens[i], i))
    ck = Clock(eng)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if setting[0] == "admit":
            codes = eng.generate(cond, text, a.max_gen, uniforms=u, slots=S, admit_min=setting[1], admit_beams=True, **kw)
        else:
            if setting[0] == "sep+retire":
                kw.update(retire_rows=0.5, retire_beams=True)
            rows = [None] * N
            for lo in range(0, N, S):
                sel = sorted(order[lo:lo + S])
                out = eng.generate(cond, text[sel], a.max_gen, uniforms=np.ascontiguousarray(u[:, sel]), **kw)
                for j, r in enumerate(sel):
                    rows[r] = out[j]
            w = max(len(r) for r in rows)
            codes = np.full((N, w), eng.ccfg.stop_mel_token, np.int64)
            for r, row in enumerate(rows):
                codes[r, :len(row)] = row
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
    finally:
        ck.close()
    return dict(total_ms=total, admit_ms=sum(ms for _, ms in ck.admits), steps=ck.steps, admits=ck.admits, codes=codes)


def done_spread(eng, cond, text, u, a):
    """the token counts (in units of the status checks) at which the groups of the FIRST `slots`-item generation were seen done"""
    nb, S = a.beams, a.slots
    lens = [int(np.count_nonzero(r != eng.ccfg.stop_text_token)) for r in text]
    sel = sorted(sorted(range(text.shape[0]), key=lambda i: (-lens[i], i))[:S])
    eng.set_beam_sample(nb, 30, 0.8, 1.0, np.ascontiguousarray(u[:, sel]))
    seen, done = {}, 1
    try:
        eng.prefill(cond, text[sel], a.max_gen, 10.0, False)
        while done < a.max_gen:
            _, ln, unf = eng.row_status()
            for i in range(S):
                if not unf[i * nb]:
                    seen.setdefault(i, int(ln[i * nb]))
            if len(seen) == S:
                break
            n = min(CHECK_EVERY, a.max_gen - done)
            eng.decode(n)
            done += n
        eng._exit()
    finally:
        eng.set_beam_sample(1)
    return sorted(seen.values()), S - len(seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=63)
    ap.add_argument("--slots", type=int, default=21)
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--max-gen", type=int, default=480)
    ap.add_argument("--stop-bias", type=float, default=3.0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    cfg = icfg.indextts_1_5()
    sd = synth.gpt_state_dict(cfg, 1234, profile="smooth", stop_bias=a.stop_bias)
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",), state_dicts={"gpt": sd}, max_batch=a.slots * a.beams)
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    lens = np.random.default_rng(a.seed).integers(20, 106, a.requests)
    text = np.full((a.requests, 105), cfg.gpt.stop_text_token, np.int32)
    for i, n in enumerate(lens):
        text[i, :n] = synth.text_ids(int(n), 900 + i, cfg.gpt.number_text_tokens)
    u = np.random.default_rng(a.seed + 1).random((a.max_gen, a.requests, 2 * a.beams), dtype=np.float32)
    print(f"# bench_admit_beams: {a.requests} requests x {a.beams} beams through {a.slots} item slots ({a.slots * a.beams} rows), bf16, "
          f"full dims, text lengths {int(lens.min())} .. {int(lens.max())}, max_gen {a.max_gen}, stop_bias {a.stop_bias}, beam_sample "
          f"top_k 30 top_p 0.8, status checks every {CHECK_EVERY} steps")
    d, open_ = done_spread(eng, cond, text, u, a)
    print(f"token counts at which the groups of the first {a.slots}-item generation were seen done: {d}; {open_} open at max_gen")
    settings = [("sep",), ("sep+retire",), ("admit", 0.125), ("admit", 0.25), ("admit", 0.5)]
    name = lambda s: s[0] if len(s) == 1 else f"admit {s[1]:g}"  # noqa: E731
    for s in settings:  # warm-up of each: tiles, graphs at every row count, allocations
        one_run(eng, cond, text, u, a, s)
    results, base, by_size = {s: [] for s in settings}, None, {}
    for rep in range(a.repeat):
        for s in settings:
            res = one_run(eng, cond, text, u, a, s)
            results[s].append(res)
            if base is None:
                base = res["codes"]
            w = min(base.shape[1], res["codes"].shape[1])
            diff = int(np.any(res["codes"][:, :w] != base[:, :w], axis=1).sum())
            print(f"run {rep} {name(s)}: total {res['total_ms']:.1f} ms (admit_rows {res['admit_ms']:.1f}); {res['steps']} token steps "
                  f"launched; requests whose codes differ from the first run's: {diff}")
            if res["admits"]:
                print("    admissions (items: ms): " + ", ".join(f"{n}: {ms:.1f}" for n, ms in res["admits"]))
            for n, ms in res["admits"]:
                by_size.setdefault(n, []).append(ms)
    best_sep = min(r["total_ms"] for r in results[settings[0]])
    for s in settings:
        tot = [r["total_ms"] for r in results[s]]
        print(f"summary {name(s)}: total " + " / ".join(f"{x:.1f}" for x in tot) + f" ms; best vs best of sep: {best_sep / min(tot):.3f}x")
    if by_size:
        print("admit_rows() host clock by item count (items: calls, min / median ms): " +
              ", ".join(f"{n}: {len(v)}, {min(v):.1f} / {float(np.median(v)):.1f}" for n, v in sorted(by_size.items())))


if __name__ == "__main__":
    main()
