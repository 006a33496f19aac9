"""The grouped fp8-cache attention inside the decode step (Engine.set_group_attn_kv_fp8 / ITTS_GROUP_ATTN_KV_FP8) on the fixture of
tests/test_gpu_group_attn_engine.py (its `run`, texts, draws, top_k): 3 layers, 4 sentences x 3 beams, 24 steps, kv_fp8 on.  Yardstick:
the grouped run is another summation order on the same cache bytes, so it must lie no farther from the per-row fp8 run than that run
lies from the fp32 engine, and follow it at least as long (capped at 8).  Values: group_attn_kv8.txt under ITTS_TEST_OUT."""
import os

import numpy as np
import pytest
import torch

from itts_hip import synth
from test_gpu_beam_retire import build, ragged
from test_gpu_group_attn_engine import STEPS, run


@pytest.fixture(scope="module")
def runs():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ITTS_GEMM_KSPLIT", "0")
        for name in ("ITTS_GROUP_ATTN", "ITTS_GROUP_ATTN_KV_FP8", "ITTS_KV_FP8"):
            mp.delenv(name, raising=False)
        eng, plain, f32 = build(kv_fp8=True, group_attn=True), build(kv_fp8=True), build(dtype="f32")
        cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
        text = ragged(4, 11)
        r = dict(parent=run(plain, cond, text), f32=run(f32, cond, text), off=run(eng, cond, text))
        eng.set_group_attn_kv_fp8(True)
        r.update(on=run(eng, cond, text), eager=run(eng, cond, text, graph=False), again=run(eng, cond, text),
                 six=run(eng, cond, text[:2], engine=True), six_parent=run(plain, cond, text[:2], engine=True))
        eng.set_group_attn_kv_fp8(False)
        r["off2"] = run(eng, cond, text)
        eng.set_group_attn_kv_fp8(True)
        r["on2"] = run(eng, cond, text)
        mp.setenv("ITTS_GROUP_ATTN_KV_FP8", "0")  # the environment overrides the setter
        r["env0"] = run(eng, cond, text)
        yield r


@pytest.mark.gpu
def test_switch_and_graph_key(runs):
    r, same = runs, lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert r["parent"][2] == 0 and r["off"][2] == 0 and same(r["off"], r["parent"]), "new switch off != an engine without any grouped switch"
    assert r["on"][2] == 2 and r["on"][3] == 0, "the grouped fp8 kernel did not run at 12 rows"
    assert same(r["eager"], r["on"]) and r["eager"][2] == 2, "graph replay != eager"
    assert same(r["again"], r["on"]), "a repeat differs"
    assert same(r["off2"], r["parent"]) and r["off2"][2] == 0 and same(r["on2"], r["on"]) and r["on2"][2] == 2, "flipping the switch"
    assert r["env0"][2] == 0 and same(r["env0"], r["parent"]), "ITTS_GROUP_ATTN_KV_FP8=0 does not override the setter"
    assert r["six"][2] == 0 and r["six"][3] == r["six_parent"][3] and same(r["six"], r["six_parent"]), "6 rows did not stay where they were"


@pytest.mark.gpu
def test_grouped_fp8_against_the_per_row_fp8_and_fp32(runs):
    def compare(a, b):
        diff = [k for k in range(STEPS - 1) if not np.array_equal(a[0][k], b[0][k])]
        n = diff[0] if diff else STEPS - 1
        x, y = a[1][:n].astype(np.float64), b[1][:n].astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        return n, float(np.sqrt(((x - y)[ok] ** 2).mean() / (y[ok] ** 2).mean()))

    n32, yard = compare(runs["parent"], runs["f32"])
    ng, got = compare(runs["on"], runs["parent"])
    lines = [f"per-row fp8 cache vs fp32 engine:       beam histories agree through step {n32}, logits rel RMS {yard:.3e} (the yardstick)",
             f"grouped fp8 attention vs per-row fp8:   beam histories agree through step {ng}, logits rel RMS {got:.3e}"]
    if os.environ.get("ITTS_TEST_OUT"):
        os.makedirs(os.environ["ITTS_TEST_OUT"], exist_ok=True)
        with open(os.path.join(os.environ["ITTS_TEST_OUT"], "group_attn_kv8.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert n32 > 4 and ng >= min(n32, 8), (ng, n32)  # (n32 <= 4: the per-row fp8 run itself leaves fp32 at once - other draws are needed)
    assert got <= yard, (got, yard)
