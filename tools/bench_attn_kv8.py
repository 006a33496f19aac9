#!/usr/bin/env python
"""The cache attention written for the e4m3 K/V cache (itts_decode_attn_kv8, csrc/decode_attn_kv8.hip) against the kernel it replaces
under the switch (itts_decode_attn with tc = ITTS_FP8: decode_attn2_kernel<fp8_t, ..>), operator alone, then the whole benchmark.

    python tools/bench_attn_kv8.py [--heads 20] [--layers 8] [--iters 48] [--rounds 5] [--no-bench]

bf16 library, random e4m3 caches of Smax 1024, tiled 16-bit ctx as the step uses it, B = 8 / 26 / 64 rows (8 x 20 heads < 512: there
itts_decode_attn runs its 1024-thread form, which the switch never replaces - the line is for the later decision on the gate), S =
pos + 1 in 200, 500, 900, kv_start 0; then 21 items x 3 beams with a trunk ancestry (every position up to the last 6 in one physical
row per item).  Consecutive launches walk `layers` different caches, as the layers of a decode step do.  The two kernels are
alternated `rounds` times in one process after a warm-up of both; per kernel `iters` launches between two device events.  Printed:
us per launch (min and median of the rounds), the K + V bytes the operation has to fetch and that rate, the ratio, and the largest
difference between the two results.  Then `bench.py --gpus 1 --steps 3 --warmup 1 --batch 32` under ITTS_KV_FP8=1 with
ITTS_ATTN_KV8=0 and =1, alternated twice, each in a fresh process (its JSON line is printed as it comes).  Run it under a time
limit; profiles/attn_kv8.txt holds a record."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from itts_hip import lib as L  # noqa: E402

SMAX = 1024


def operator(a, B, nb, S_list):
    lib, dev, H = L.load(), "cuda:0", a.heads
    g = torch.Generator(device=dev).manual_seed(5)
    kc = torch.randn(a.layers, B, H, SMAX, 64, device=dev, dtype=torch.bfloat16, generator=g).to(torch.float8_e4m3fn)
    vc = torch.randn(a.layers, B, H, SMAX, 64, device=dev, dtype=torch.bfloat16, generator=g).to(torch.float8_e4m3fn)
    qkv = torch.randn(B, 3 * H * 64, device=dev, generator=g)
    qkv[:, :H * 64] *= 2.0
    ks = torch.zeros(B, dtype=torch.int32, device=dev)
    pre = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = [torch.zeros((B + 15) // 16 * 16, H * 64, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(3)
    for S in S_list:
        pos = S - 1
        ln = torch.full((B,), pos, dtype=torch.int32, device=dev)
        anc = None
        if nb > 1:
            tab = np.repeat(rng.integers(0, nb, (B // nb, SMAX)), nb, axis=0).astype(np.uint8)
            tab[:, pos - 6:] = np.tile((np.arange(B) % nb)[:, None], (1, SMAX))[:, pos - 6:]
            anc = torch.from_numpy(np.stack([tab, tab])).to(dev)
        ap = anc.data_ptr() if anc is not None else None

        def launch(which, i):
            k, v = kc[i % a.layers].data_ptr(), vc[i % a.layers].data_ptr()
            if which:
                st = lib.itts_decode_attn_kv8(ctx[1].data_ptr(), L.BF16, qkv.data_ptr(), k, v, ln.data_ptr(), ks.data_ptr(), pre.data_ptr(), B, H,
                                              64, SMAX, L.FP8, 1, ap, nb, s)
            else:
                st = lib.itts_decode_attn(ctx[0].data_ptr(), L.BF16, qkv.data_ptr(), k, v, ln.data_ptr(), ks.data_ptr(), pre.data_ptr(), B, H, 64,
                                          SMAX, L.FP8, 1, None, None, ap, nb, s)
            L.check(st, "bench_attn_kv8", lib)

        for which in (0, 1):  # warm-up, and both results on the same cache (the appended row is the same bytes)
            for i in range(a.layers):
                launch(which, i + 1)
        torch.cuda.synchronize()
        diff = float((ctx[0].float() - ctx[1].float()).abs().max())
        ms = [[], []]
        for _ in range(a.rounds):
            for which in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.iters):
                    launch(which, i)
                e1.record()
                torch.cuda.synchronize()
                ms[which].append(e0.elapsed_time(e1) / a.iters)
        need = B * pos * H * 128  # K + V bytes of the visible history
        tag = f"B={B:3d}" + (f" ({B // nb} x {nb} beams, trunk)" if nb > 1 else "")
        for which, label in ((0, "decode_attn2<fp8_t>" + (" 1024 thr" if B * H < 512 else " 256 thr")), (1, "decode_attn_kv8")):
            t = ms[which]
            print(f"{tag} S={S:4d} {label:<28s} {min(t) * 1e3:7.1f} us min  {float(np.median(t)) * 1e3:7.1f} us median   "
                  f"fetches {need / 2**20:6.1f} MiB -> {need / min(t) / 1e6:7.1f} GB/s")
        print(f"{tag} S={S:4d} kv8 / decode_attn2 time (min): {min(ms[1]) / min(ms[0]):.3f}   max |ctx difference| {diff:.3e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=20)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-bench", action="store_true", help="the operator lines only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_kv8: needs a GPU")
    print(f"# bench_attn_kv8: H = {a.heads}, e4m3 caches, Smax {SMAX}, {a.layers} caches walked, {a.iters} launches per timing, "
          f"{a.rounds} alternated rounds")
    for B in (8, 26, 64):
        operator(a, B, 1, (200, 500, 900))
    operator(a, 63, 3, (200, 500, 900))
    if a.no_bench:
        return
    for rep in range(2):
        for on in ("0", "1"):
            env = dict(os.environ, ITTS_KV_FP8="1", ITTS_ATTN_KV8=on)
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32"],
                                 env=env, capture_output=True, text=True, timeout=600)
            last = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            print(f"bench.py --batch 32 ITTS_KV_FP8=1 ITTS_ATTN_KV8={on} (pass {rep + 1}): " + (last[-1] if last else f"exit {out.returncode}: {out.stderr[-300:]}"),
                  flush=True)


if __name__ == "__main__":
    main()
