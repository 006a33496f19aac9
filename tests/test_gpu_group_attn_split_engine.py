"""The grouped attention's key split inside the decode step (Engine.set_group_attn_split / ITTS_GROUP_ATTN_SPLIT) on the fixture of
tests/test_gpu_group_attn_engine.py (its `run`, draws, top_k): 3 layers, 3 sentences x 3 beams = 9 rows, 24 steps, group_attn on.
Yardstick: the split run is another summation order of the same attention, so it must lie no farther from the parent's 16-bit run
than that run lies from the fp32 engine, over the steps at which the beam histories agree (through step 8 at least).  Forced to 4
splits, so that the assertions do not move with the measured rule.  Values: group_attn_split.txt under ITTS_TEST_OUT."""
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
        for name in ("ITTS_GROUP_ATTN", "ITTS_GROUP_ATTN_SPLIT"):
            mp.delenv(name, raising=False)
        eng, grp, plain, f32 = build(group_attn=True), build(group_attn=True), build(), build(dtype="f32")
        cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
        text = ragged(3, 11)
        r = dict(parent=run(plain, cond, text), f32=run(f32, cond, text), grouped=run(grp, cond, text), off=run(eng, cond, text))
        eng.set_group_attn_split(4)
        r.update(on=run(eng, cond, text), eager=run(eng, cond, text, graph=False), again=run(eng, cond, text),
                 six=run(eng, cond, text[:2], engine=True))
        eng.set_group_attn_split(0)
        r["off2"] = run(eng, cond, text)
        eng.set_group_attn_split(4)
        r["on2"] = run(eng, cond, text)
        mp.setenv("ITTS_GROUP_ATTN_SPLIT", "0")  # the environment overrides the setter
        r["env0"] = run(eng, cond, text)
        yield r


@pytest.mark.gpu
def test_switch_and_graph_key(runs):
    r, same = runs, lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert r["grouped"][2] == 1 and r["off"][2] == 1 and same(r["off"], r["grouped"]), "switch off != group_attn alone"
    assert r["on"][2] == 3 and r["on"][3] == 0, "the split form did not run at 9 rows"
    assert same(r["eager"], r["on"]) and r["eager"][2] == 3, "graph replay != eager"
    assert same(r["again"], r["on"]), "a repeat differs"
    assert same(r["off2"], r["grouped"]) and r["off2"][2] == 1 and same(r["on2"], r["on"]) and r["on2"][2] == 3, "flipping the switch"
    assert r["env0"][2] == 1 and same(r["env0"], r["grouped"]), "ITTS_GROUP_ATTN_SPLIT=0 does not override the setter"
    assert r["six"][3] == 1 and r["six"][2] == 0, "6 rows left the persistent engine"


@pytest.mark.gpu
def test_split_against_the_parent_and_fp32(runs):
    def compare(a, b):
        diff = [k for k in range(STEPS - 1) if not np.array_equal(a[0][k], b[0][k])]
        n = diff[0] if diff else STEPS - 1
        x, y = a[1][:n].astype(np.float64), b[1][:n].astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        return n, float(np.sqrt(((x - y)[ok] ** 2).mean() / (y[ok] ** 2).mean()))

    n32, yard = compare(runs["parent"], runs["f32"])
    ng, got = compare(runs["on"], runs["parent"])
    lines = [f"parent bf16 launch path vs fp32 engine:       beam histories agree through step {n32}, logits rel RMS {yard:.3e} (the yardstick)",
             f"split grouped attention vs parent bf16 path:  beam histories agree through step {ng}, logits rel RMS {got:.3e}"]
    print("\n".join(lines))
    if os.environ.get("ITTS_TEST_OUT"):
        os.makedirs(os.environ["ITTS_TEST_OUT"], exist_ok=True)
        with open(os.path.join(os.environ["ITTS_TEST_OUT"], "group_attn_split.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert n32 >= 8 and ng >= 8, (n32, ng)
    assert got <= yard, (got, yard)
