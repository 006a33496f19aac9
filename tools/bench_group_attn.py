#!/usr/bin/env python3
"""The grouped cache attention under beams (itts_decode_attn_group, csrc/decode_attn_group.hip) against the per-row ancestry form it
replaces (itts_decode_attn with `anc`, the 256-thread "many" form), operator alone.

    python tools/bench_group_attn.py [--items 21 ..] [--beams 3] [--heads 20] [--layers 8] [--iters 48] [--rounds 5] [--kv-fp8] [--split N ..]

bf16 library, random caches, `items` x `beams` rows (what one infer_batch generation of the default kwargs carries), S = pos + 1 in
200, 500, 900 of Smax 1024, kv_start 0.  Two ancestries: "trunk" - every position up to the last 6 lies in ONE (random) physical row
of its item for all beams, the last 6 in each beam's own row - and "identity" - every beam in its own row everywhere, the first
step's table and the grouped kernel's worst case (beams passes per tile).  Consecutive launches walk `layers` different caches, as
the layers of a decode step do, so that no launch finds its rows in the caches of the one before (the footprint is printed).  The
two kernels are alternated `rounds` times in one process after a warm-up of both; per kernel `iters` launches between two device
events.  Printed: ms per launch (min and median of the rounds), the bytes each algorithm has to fetch and that rate, and the
largest difference between the two results.  --kv-fp8: the same on e4m3 caches (tc = ITTS_FP8) - the per-row e4m3 kernel against
itts_decode_attn_group_kv8 (csrc/decode_attn_group.hip), half the bytes per row.  --split N (repeatable, 16-bit caches): the
key-split form itts_decode_attn_group_split (csrc/decode_attn_group.hip, its two kernels) at N splits joins the alternation as
a further contender, in the same process and the same rounds; its time is also printed over the unsplit grouped kernel's.  --items
takes several item counts, measured one after another.  Run it under a time limit; profiles/group_attn.txt,
profiles/group_attn_kv8.txt and profiles/group_attn_split.txt hold records."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from itts_hip import lib as L  # noqa: E402

SMAX = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, nargs="+", default=[21])
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--heads", type=int, default=20)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--iters", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kv-fp8", action="store_true", help="e4m3 caches: the per-row e4m3 kernel against itts_decode_attn_group_kv8")
    ap.add_argument("--split", type=int, action="append", default=[], help="also the key-split grouped form at this many splits (2 .. 8; repeatable)")
    a = ap.parse_args()
    if a.split and a.kv_fp8:
        sys.exit("bench_group_attn: the key-split form reads a 16-bit cache only")
    if not torch.cuda.is_available():
        sys.exit("bench_group_attn: needs a GPU")
    for items in a.items:
        run(a, items)


def run(a, items):
    a = argparse.Namespace(**{**vars(a), "items": items})
    lib, dev = L.load(), "cuda:0"
    nb, H, B = a.beams, a.heads, a.items * a.beams
    g = torch.Generator(device=dev).manual_seed(5)
    kc = torch.randn(a.layers, B, H, SMAX, 64, device=dev, dtype=torch.bfloat16, generator=g)
    vc = torch.randn(a.layers, B, H, SMAX, 64, device=dev, dtype=torch.bfloat16, generator=g)
    tc, row_bytes, grouped = L.BF16, 256, lib.itts_decode_attn_group  # (K + V bytes of one cache row)
    if a.kv_fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
        tc, row_bytes, grouped = L.FP8, 128, lib.itts_decode_attn_group_kv8
    qkv = torch.randn(B, 3 * H * 64, device=dev, generator=g)
    qkv[:, :H * 64] *= 2.0
    ks = torch.zeros(B, dtype=torch.int32, device=dev)
    pre = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx = [torch.zeros(B, H * 64, device=dev, dtype=torch.bfloat16) for _ in range(2 + len(a.split))]
    part_o, part_ml = torch.zeros(8, B, H, 64, device=dev), torch.zeros(8, B, H, 2, device=dev)  # the split form's workspaces
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"# bench_group_attn: {a.items} items x {nb} beams = {B} rows, H = {H}, {'e4m3' if a.kv_fp8 else 'bf16'} caches, Smax {SMAX}, {a.layers} caches walked "
          f"({kc[0].numel() * 2 * kc.element_size() / 2**20:.0f} MiB of K + V each), {a.iters} launches per timing, {a.rounds} alternated rounds")
    rng = np.random.default_rng(3)
    for S in (200, 500, 900):
        pos = S - 1
        ln = torch.full((B,), pos, dtype=torch.int32, device=dev)
        ident = np.tile((np.arange(B) % nb)[:, None], (1, SMAX)).astype(np.uint8)
        trunk = np.repeat(rng.integers(0, nb, (a.items, SMAX)), nb, axis=0).astype(np.uint8)
        trunk[:, pos - 6:] = ident[:, pos - 6:]
        for name, tab, rows_read in (("trunk", trunk, a.items * ((pos - 6) + 6 * nb)), ("identity", ident, B * pos)):
            anc = torch.from_numpy(np.stack([tab, tab])).to(dev)

            def launch(which, i):
                k, v = kc[i % a.layers].data_ptr(), vc[i % a.layers].data_ptr()
                if which >= 2:
                    st = lib.itts_decode_attn_group_split(ctx[which].data_ptr(), L.BF16, qkv.data_ptr(), k, v, ln.data_ptr(), ks.data_ptr(),
                                                          pre.data_ptr(), B, H, 64, SMAX, tc, 0, anc.data_ptr(), nb, a.split[which - 2],
                                                          part_o.data_ptr(), part_ml.data_ptr(), s)
                elif which:
                    st = grouped(ctx[1].data_ptr(), L.BF16, qkv.data_ptr(), k, v, ln.data_ptr(), ks.data_ptr(), pre.data_ptr(), B, H, 64,
                                 SMAX, tc, 0, anc.data_ptr(), nb, s)
                else:
                    st = lib.itts_decode_attn(ctx[0].data_ptr(), L.BF16, qkv.data_ptr(), k, v, ln.data_ptr(), ks.data_ptr(), pre.data_ptr(),
                                              B, H, 64, SMAX, tc, 0, None, None, anc.data_ptr(), nb, s)
                L.check(st, "bench_group_attn", lib)

            every = range(2 + len(a.split))
            for which in every:  # warm-up, and the results on the same cache
                for i in range(a.layers):
                    launch(which, i + 1)
            torch.cuda.synchronize()
            diff = float((ctx[0].float() - ctx[1].float()).abs().max())
            sdiff = [float((ctx[w].float() - ctx[1].float()).abs().max()) for w in every[2:]]
            ms = [[] for _ in every]
            for _ in range(a.rounds):
                for which in every:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for i in range(a.iters):
                        launch(which, i)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[which].append(e0.elapsed_time(e1) / a.iters)
            need = (B * pos * H * row_bytes, rows_read * H * row_bytes)  # K + V bytes: per row its whole history / every (position, row) once
            for which, label in ((0, "decode_attn2 ANC many"), (1, "decode_attn_group_kv8" if a.kv_fp8 else "decode_attn_group")):
                t = ms[which]
                print(f"S={S:4d} {name:<8s} {label:<22s} {min(t) * 1e3:7.1f} us min  {float(np.median(t)) * 1e3:7.1f} us median   "
                      f"fetches {need[which] / 2**20:6.1f} MiB -> {need[which] / min(t) / 1e6:7.1f} GB/s")
            print(f"S={S:4d} {name:<8s} grouped / per-row time (min): {min(ms[1]) / min(ms[0]):.3f}   max |ctx difference| {diff:.3e}")
            for w in every[2:]:  # the split form: both its kernels per launch, the bytes of the grouped kernel
                t = ms[w]
                print(f"S={S:4d} {name:<8s} {'decode_attn_group_split NS=' + str(a.split[w - 2]):<28s} {min(t) * 1e3:7.1f} us min  "
                      f"{float(np.median(t)) * 1e3:7.1f} us median   split / unsplit grouped (min): {min(t) / min(ms[1]):.3f}   "
                      f"max |ctx difference| {sdiff[w - 2]:.3e}")


if __name__ == "__main__":
    main()
