#!/usr/bin/env python3
"""Row retirement of a batched decode (Engine.retire_rows, opt-in) against the same generation without it.

    python tools/bench_row_retire.py [--rows 64] [--gpt-fp8] [--ratios 0,0.5,0.75] [--repeat 2] [--max-gen 480] [--text-len 105]

Full IndexTTS-1.5 dims, PRNG weights.  Every row is forced to stop at a step drawn once from a seeded uniform spread over
120 .. max_gen - 1 (set_forced under suppress_stop=True, so nothing else stops a row); the loop is Engine.generate's: status() every
16 steps, retire_rows() whenever unfinished <= ratio * rows() and rows() > 6, until no row is unfinished.  Ratio 0 is the yardstick
(no retire call at all).  The settings are alternated `--repeat` times in one process on one engine object.  Printed per run: total
decode time (prefill excluded), the mean time per token step of every stretch between two retirements with its row count, and per
retire_rows() call its time, the rows moved and the bytes the kernel copied; then one summary line per setting.  The codes of every
run are compared with the yardstick's (how many rows differ and from which step on: a retirement that crosses kernel families - to
16 rows and fewer, to 4 and fewer - changes the fp32 summation order, and with PRNG weights near-ties flip; before it the bits are equal).
Run it under a time limit (timeout -k 10 900 python tools/bench_row_retire.py ...); profiles/row_retire.txt holds a record."""
import argparse
import ctypes as C
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
from itts_hip import lib as L  # noqa: E402
from itts_hip import synth  # noqa: E402

CHECK_EVERY = 16


def plan(unf):
    u = np.ascontiguousarray(unf, dtype=np.int32)
    src, dst = np.zeros(len(u), np.int32), np.zeros(len(u), np.int32)
    n, m = C.c_int(), C.c_int()
    assert L.load().itts_retire_plan(u.ctypes.data_as(C.c_void_p), len(u), C.byref(n), src.ctypes.data_as(C.c_void_p),
                                     dst.ctypes.data_as(C.c_void_p), C.byref(m)) == 0
    return n.value, src[: m.value].tolist(), dst[: m.value].tolist()


def one_run(eng, cond, text, max_gen, stop_step, ratio, row_bytes_per_pos, state_bytes, prefix):
    """-> dict(total_ms, stretches [(rows, steps, ms)], retires [(rows_before, rows_after, moved, bytes, ms)], codes)"""
    B = text.shape[0]
    orig = list(range(B))
    eng.prefill(cond, text, max_gen, 10.0, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done, stretches, retires = 1, [], []
    seg_t, seg_steps = t0, 0
    while done < max_gen:
        step, unf = eng.status()
        if unf == 0:
            break
        rows = eng.rows()
        if ratio and rows > 6 and unf <= ratio * rows:
            now = time.perf_counter()
            if seg_steps:
                stretches.append((rows, seg_steps, (now - seg_t) * 1e3))
            n, src, dst = plan([1 if stop_step[r] >= step else 0 for r in orig])  # the host's view of what the call will do
            ta = time.perf_counter()
            got = eng.retire_rows()
            tb = time.perf_counter()
            assert got == n, (got, n)
            for s, d in zip(src, dst):
                orig[d] = orig[s]
            orig = orig[:n]
            nbytes = len(src) * (row_bytes_per_pos * min(prefix + step, 1 << 30) + state_bytes)
            retires.append((rows, n, len(src), nbytes, (tb - ta) * 1e3))
            seg_t, seg_steps = tb, 0
        n_steps = min(CHECK_EVERY, max_gen - done)
        eng.decode(n_steps)
        done += n_steps
        seg_steps += n_steps
    step, unf = eng.status()
    t1 = time.perf_counter()
    if seg_steps:
        stretches.append((eng.rows(), seg_steps, (t1 - seg_t) * 1e3))
    codes = eng.fetch()[:, :step].copy()
    eng._exit()
    return dict(total_ms=(t1 - t0) * 1e3, steps=step, stretches=stretches, retires=retires, codes=codes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--gpt-fp8", action="store_true")
    ap.add_argument("--ratios", default="0,0.5,0.75")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--max-gen", type=int, default=480)
    ap.add_argument("--text-len", type=int, default=105)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    ratios = [float(x) for x in a.ratios.split(",")]
    cfg = icfg.indextts_1_5()
    eng = ieng.build_engine(cfg, "bf16", parts=("gpt",), gpt_fp8="fp8" if a.gpt_fp8 else "", max_batch=max(a.rows, 1))
    cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    text = np.stack([synth.text_ids(a.text_len, 900 + i, cfg.gpt.number_text_tokens) for i in range(a.rows)]).astype(np.int32)
    stop_step = np.random.default_rng(a.seed).integers(120, a.max_gen, a.rows)
    forced = np.full((a.rows, a.max_gen), -1, np.int32)
    forced[np.arange(a.rows), stop_step] = cfg.gpt.stop_mel_token
    g = cfg.gpt
    D, H, V = g.model_dim, g.heads, g.number_mel_codes
    ces = 2  # the 16-bit cache
    row_bytes_per_pos = 2 * g.layers * H * (D // H) * ces  # K and V, every layer and head, one position
    state_bytes = D * 4 + V * 4 + 2 * a.max_gen * 4 + V + 4 * 4  # h, logits, ids, forced, seen, len / kv_start / cur_tok / unfinished
    prefix = int(eng.ccfg.cond_latents) + a.text_len + 2
    print(f"# bench_row_retire: rows {a.rows}, gpt_fp8 {bool(a.gpt_fp8)}, L {a.text_len}, max_gen {a.max_gen}, forced stop steps "
          f"{int(stop_step.min())} .. {int(stop_step.max())} (seed {a.seed}, mean {float(stop_step.mean()):.0f}), status() every {CHECK_EVERY} steps")
    eng.set_forced(forced)
    results = {r: [] for r in ratios}
    base = None
    try:
        one_run(eng, cond, text, a.max_gen, stop_step, 0.0, row_bytes_per_pos, state_bytes, prefix)  # warm-up: tiles, graphs, allocations
        for rep in range(a.repeat):
            for r in ratios:
                res = one_run(eng, cond, text, a.max_gen, stop_step, r, row_bytes_per_pos, state_bytes, prefix)
                if base is None and not r:
                    base = res["codes"]
                diff = -1 if base is None else int(np.any(res["codes"] != base, axis=1).sum())
                first = int(np.argmax(np.any(res["codes"] != base, axis=0))) if diff > 0 else -1  # (in-family retirements: same bits)
                results[r].append(res["total_ms"])
                print(f"run {rep} retire_rows={r:g}: decode total {res['total_ms']:.1f} ms over {res['steps']} steps; rows whose codes differ "
                      f"from the yardstick: {diff}" + (f", the first at step {first}" if diff > 0 else ""))
                for rows, steps, ms in res["stretches"]:
                    print(f"    {rows:3d} rows: {steps:4d} steps, {ms / steps:.3f} ms per step")
                for rb, ra, moved, nbytes, ms in res["retires"]:
                    print(f"    retire_rows() {rb:3d} -> {ra:3d} rows: {ms:.2f} ms, {moved} rows moved, {nbytes / 1e6:.1f} MB copied")
    finally:
        eng.set_forced(None)
    off = results.get(0.0)
    for r in ratios:
        line = f"summary retire_rows={r:g}: decode total " + " / ".join(f"{x:.1f}" for x in results[r]) + " ms"
        if off and r:
            line += f"; best vs best of off: {min(off) / min(results[r]):.3f}x"
        print(line)


if __name__ == "__main__":
    main()
