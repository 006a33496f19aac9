"""Debugging aid: phase timeline of the persistent decode engine (ITTS_ENGINE_STAMPS=1), one decode step.
Stamps per workgroup and block (100 MHz wall clock): 0 E1 gathered, 1 after B1, 2 q/k/v polled (attention WGs), 3 context
published, 4 E3 gathered, 5 E4 gathered, 6 E5 gathered, 7 after B5; compute side: 8 q/k/v published, 9 c_proj published,
10 c_fc published, 11 mlp.c_proj published.  Around the blocks (slot 15 of blocks 3 .. 10): scalars resolved, first weights
requested, h gathered, ln_f + final_norm done, dots done, candidates published and, on the workgroups that finish a row, candidates
gathered and token committed - printed as the split of the launch's fixed cost into prologue, head and sampler tail.
Slot 15 of blocks 11 / 12: the workgroup's XCC_ID / HW_ID registers.  Last section: the per-workgroup skew of every stage over
blocks 2..NL-2 - how often a workgroup is among the last 8 and its mean lateness against the stage median, by role, by cu % 8,
by place in the head's group and by XCD - and how much of median -> max the per-workgroup means explain (systematic) or not (noise).
Needs the probes library (`make -C index-tts-ipex_amd/csrc probes`): the product library compiles the engine's stamps, block taps and
gather divisor out and ignores their switches.  Select it through the usual override:
ITTS_HIP_LIB=index-tts-ipex_amd/csrc/libitts_hip_probes.so python tools/eng_timeline.py ..."""
import os
import sys

import numpy as np
import torch

os.environ["ITTS_ENGINE_STAMPS"] = "1"
os.environ["ITTS_ENGINE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-ipex_amd")):
    sys.path.insert(0, p)
from itts_hip import config as icfg, engine as ieng, synth  # noqa: E402

CFG = icfg.indextts_1_5()
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 2
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 240
eng = ieng.build_engine(CFG, "bf16", parts=("gpt",))
cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
text = np.stack([synth.text_ids(105, 11 + r, CFG.gpt.number_text_tokens) for r in range(rows)]).astype(np.int32)
eng.prefill(cond, text, 480, 10.0, True)
eng.decode(warm)
eng.debug(taps=True, no_graph=True)
eng.decode(1)
eng.fetch()
eng._exit()
st = eng.fetch_tap("eng_stamps").view(np.uint32).reshape(256, -1, 16).astype(np.int64)
eng.debug()
NL = st.shape[1]
t0 = st[:, 0, 0].min()
us = (st - t0) / 100.0
acu = np.array([(c < 240) and (c % 12 < rows) for c in range(256)])
print(f"rows {rows}, S ~ {139 + warm}; step span {us[:, :, 11].max():.1f} us, per block {(us[:, -1, 11].max() - us[:, 0, 0].min()) / NL:.2f} us")
names = ["E1 gathered", "after B1", "qkv polled (attn WG)", "ctx published (attn WG)", "E3 gathered", "E4 gathered", "E5 gathered",
         "after B5", "qkv published", "h1 published", "act published", "h2 published"]
for l in (1, NL // 2, NL - 2):
    base = us[:, l, 0].min()
    print(f"-- block {l} (t = 0 at the first WG's E1)")
    for i in (0, 1, 8, 2, 3, 4, 9, 5, 10, 6, 7, 11):
        v = us[:, l, i] - base
        if i in (2, 3):
            v = v[acu]
        print(f"   {names[i]:26s} min {v.min():6.2f}  median {np.median(v):6.2f}  max {v.max():6.2f}")
k0, k1 = (st[:, 1, 15] - t0) / 100.0, (st[:, 2, 15] - t0) / 100.0
print(f"-- launch: workgroups start {k0.min():.2f} .. {k0.max():.2f} us, first block's E1 gathered at 0 .. {us[:, 0, 0].max():.2f}; last h2 published "
      f"{us[:, -1, 11].max():.2f}, workgroups end {k1.min():.2f} .. {k1.max():.2f} us (head + sampler: {k1.max() - us[:, -1, 11].max():.2f} us; "
      f"whole launch {k1.max() - k0.min():.2f} us)")
# attention workgroups against the rest: mean over blocks 2..NL-2 of (stage time - block's first E1)
base = us[:, 2:NL - 1, 0].min(axis=0, keepdims=True)
rel = us[:, 2:NL - 1, :] - base[:, :, None]
print("-- attention workgroups vs the others (mean us since the block's first E1): " +
      ", ".join(f"{names[i]} {rel[acu][:, :, i].mean():.2f} / {rel[~acu][:, :, i].mean():.2f}" for i in (4, 9, 5, 10, 6, 11)))
if NL >= 11:  # prologue / head / sampler tail: slot 15 of blocks 3.. (ENG_HSTAMP in decode_engine.hip), median over workgroups
    hs = (st[:, 3:11, 15] - t0) / 100.0  # [256][8]
    h2 = us[:, -1, 11].max()
    wg_end = np.median(k1[rows:]) if rows < 256 else np.median(k1)
    print(f"-- prologue (us since the workgroup's start, median / max over workgroups): scalars resolved {np.median(hs[:, 0] - k0):.2f} / {(hs[:, 0] - k0).max():.2f}, "
          f"first weights requested {np.median(hs[:, 1] - k0):.2f} / {(hs[:, 1] - k0).max():.2f}, block 0 E1 gathered {np.median(us[:, 0, 0] - k0):.2f} / {(us[:, 0, 0] - k0).max():.2f}, "
          f"after B1 {np.median(us[:, 0, 1] - k0):.2f} / {(us[:, 0, 1] - k0).max():.2f}; first start -> last after B1 {us[:, 0, 1].max() - k0.min():.2f}")
    print(f"-- head (us since the last h2 publish, median / max over workgroups): h gathered {np.median(hs[:, 2]) - h2:.2f} / {hs[:, 2].max() - h2:.2f}, "
          f"ln_f + final_norm done {np.median(hs[:, 3]) - h2:.2f} / {hs[:, 3].max() - h2:.2f}, dots + wave sums done {np.median(hs[:, 4]) - h2:.2f} / {hs[:, 4].max() - h2:.2f}, "
          f"candidates published {np.median(hs[:, 5]) - h2:.2f} / {hs[:, 5].max() - h2:.2f}, workgroup end (cu >= rows) {wg_end - h2:.2f}")
    print(f"-- sampler tail (workgroups cu < rows, us since the last h2 publish): candidates gathered {hs[:rows, 6].max() - h2:.2f}, token committed {hs[:rows, 7].max() - h2:.2f}, "
          f"embedding stored / end {k1[:rows].max() - h2:.2f}")
    print(f"-- fixed cost: launch {k1.max() - k0.min():.2f} - {NL} x block {(us[:, -1, 11].max() - us[:, 0, 0].min()) / NL:.2f} = "
          f"{k1.max() - k0.min() - (us[:, -1, 11].max() - us[:, 0, 0].min()):.2f} us: prologue (first start -> first E1) {us[:, 0, 0].min() - k0.min():.2f}, "
          f"head (last h2 -> median end) {wg_end - h2:.2f}, sampler tail (-> last end) {k1.max() - wg_end:.2f}")
clk = st[:, 0, 15]
print(f"shader clock over the launch: {np.median(clk) / 10.0:.0f} MHz (min {clk.min() / 10.0:.0f}, max {clk.max() / 10.0:.0f})")
d = us[:, 2:NL - 1, :]
print("-- c_fc phase of a compute wave (mean over WGs and blocks): E4 gathered (wave 0) -> after B4 %.2f -> LN2 done (2 barriers; mlp.c_proj DMA issued meanwhile) %.2f -> dots + wave sums %.2f -> gelu + publish %.2f us"
      % ((d[:, :, 12] - d[:, :, 5]).mean(), (d[:, :, 13] - d[:, :, 12]).mean(), (d[:, :, 14] - d[:, :, 13]).mean(), (d[:, :, 10] - d[:, :, 14]).mean()))
mx = us.max(axis=0)  # [NL][16] last WG
mx[:, 3] = us[acu][:, :, 3].max(axis=0)
seq = [(0, "E1 all gathered"), (8, "qkv all published"), (3, "ctx all published"), (4, "E3 all gathered"), (9, "h1 all published"),
       (5, "E4 all gathered"), (10, "act all published"), (6, "E5 all gathered"), (11, "h2 all published")]
prev = None
print("-- mean over blocks 2..NL-2 of (last WG at stage) - (last WG at previous stage)")
for i, nm in seq:
    if prev is not None:
        d = (mx[2:NL - 1, i] - mx[2:NL - 1, prev]).mean()
        print(f"   {nm:22s} +{d:5.2f} us")
    prev = i
print(f"   next block E1          +{(mx[3:NL, 0] - mx[2:NL - 1, 11]).mean():5.2f} us")

# ---- per-workgroup skew: which workgroups are late at a stage in EVERY block (systematic) and which only now and then ----
# lateness = a workgroup's stamp minus the stage's median over workgroups in the same block, over blocks 2..NL-2.  Every edge is
# an all-to-all, so the consumers of a stage start behind its LAST workgroup: the part of (max - median) that the per-workgroup
# mean lateness explains is what a change of ownership / order / placement could remove, the rest is arbitration noise.
LAST = 8
cus = np.arange(256)
qcu = cus < 240
role = np.where(acu, 0, np.where(qcu, 1, 2))
role_names = ["attention workgroups", "others, cu < 240", "cu >= 240"]
xcd = None
if NL > 12:  # probes build: hardware ids of the workgroup (slot 15 of blocks 11 / 12): XCC id, HW_ID
    x = st[:, 11, 15] & 15
    if x.max() < 8 and len(np.unique(x)) > 1:
        xcd = x
        agree = int((xcd == cus % 8).sum())
        print(f"-- placement: XCC id recorded; workgroups per XCD {np.bincount(xcd, minlength=8).tolist()}; XCC id == cu % 8 on {agree} of 256 workgroups")
        hw = st[:, 12, 15]
        print(f"   HW_ID cu_id (bits 11:8) x se_id (bits 15:13) distinct pairs per XCD: "
              f"{[len(set(zip(((hw >> 8) & 15)[xcd == k].tolist(), ((hw >> 13) & 7)[xcd == k].tolist()))) for k in range(8)]}")
if xcd is None:
    print("-- placement: no XCC id in the stamps (not the probes build of this tree, or fewer than 13 blocks): no grouping by XCD")
blk = slice(2, NL - 1)
print(f"-- per-stage skew over blocks 2..{NL - 2} ({NL - 3} blocks): lateness = stamp - stage median of the block; 'last {LAST}' = share of the blocks in which")
print(f"   the workgroup is among the {LAST} latest (chance: {100.0 * LAST / 256:.1f} % over all 256, {100.0 * LAST / max(1, int(acu.sum())):.1f} % among the attention workgroups)")
for i in (0, 8, 2, 3, 4, 9, 5, 10, 6, 11):
    sel = acu if i in (2, 3) else np.ones(256, bool)
    v = us[sel][:, blk, i]  # [n][blocks]
    ids = cus[sel]
    late = v - np.median(v, axis=0, keepdims=True)
    mean_late = late.mean(axis=1)  # per workgroup
    resid = late - mean_late[:, None]
    order = np.argsort(-late, axis=0)[:LAST]  # [LAST][blocks]
    cnt = np.zeros(len(ids))
    np.add.at(cnt, order.ravel(), 1)
    share = cnt / late.shape[1]
    tot_var = late.var()
    sys_frac = mean_late.var() / tot_var if tot_var > 0 else 0.0
    gap = late.max(axis=0).mean()
    gap_resid = (resid.max(axis=0) - np.median(resid, axis=0)).mean()
    print(f"   == {names[i]}: median -> max {gap:.2f} us (mean over blocks); with every workgroup's mean lateness taken out {gap_resid:.2f} us; "
          f"per-workgroup means explain {100 * sys_frac:.0f} % of the variance; workgroup means span {mean_late.min():+.2f} .. {mean_late.max():+.2f} us")
    top = np.argsort(-share)[:12]
    print("      most often last: " + ", ".join(f"cu {ids[k]} {100 * share[k]:.0f}% ({mean_late[k]:+.2f})" for k in top))

    def group(label, keys, labels):
        parts = []
        for kk, lb in labels:
            m = keys == kk
            if m.any():
                parts.append(f"{lb} n={int(m.sum())} {mean_late[m].mean():+.2f} us / {100 * share[m].mean():.1f}%")
        print(f"      by {label} (mean lateness / mean 'last {LAST}' share): " + "; ".join(parts))

    group("role", role[sel], list(enumerate(role_names)))
    if not (i in (2, 3)):
        group("row finisher", (ids < rows).astype(int), [(1, "cu < rows"), (0, "others")])
    group("cu % 8", ids % 8, [(k, str(k)) for k in range(8)])
    group("cu % 12 (place in the head's group)", np.where(ids < 240, ids % 12, 12), [(k, str(k)) for k in range(12)] + [(12, "none")])
    if xcd is not None:
        group("XCD", xcd[sel], [(k, str(k)) for k in range(8)])
