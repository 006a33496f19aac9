"""decode_attn_kv8 inside the decode step (Engine.set_attn_kv8 / ITTS_ATTN_KV8) at the sizes of tests/test_gpu_engine_fp8.py (3 layers at
1.5 dims, its greedy `run`), 32 rows x 20 heads >= 512, 20 steps, rows 30 / 31 = rows 0 / 1; self-consistency is compared as bits.
Accuracy: the teacher-forced top-8-logits check of tests/test_gpu_kv_fp8_accuracy.py at 32 rows (smooth full-size checkpoint, fp32
reference fixture, bound 8.5e-3 = twice the 4.24e-3 measured for decode_attn2<fp8_t>); the value is printed (profiles/attn_kv8.txt)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402
from test_gpu_bf16_accuracy import CFG, forced_trace, mel, sd_smooth, top8_err  # noqa: E402,F401
from test_gpu_beam_retire import build as build_beams  # noqa: E402
from test_gpu_engine_fp8 import CFG3, run, same_bits  # noqa: E402
from test_gpu_group_attn_engine import run as run_beams  # noqa: E402
from test_gpu_kv_fp8 import ragged  # noqa: E402
from test_gpu_kv_fp8_accuracy import BOUND_KV_FP8  # noqa: E402

STEPS = 20
build = lambda **kw: ieng.build_engine(CFG3, "bf16", parts=("gpt",), kv_fp8=True, **kw)  # noqa: E731


@pytest.fixture(scope="module")
def runs():
    with pytest.MonkeyPatch.context() as mp:
        for name in ("ITTS_ATTN_KV8", "ITTS_KV_FP8", "ITTS_GROUP_ATTN", "ITTS_GROUP_ATTN_KV_FP8"):
            mp.delenv(name, raising=False)
        eng, plain, text = build(attn_kv8=True), build(), ragged(32, 11)
        cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
        text[30:] = text[:2]

        def go(e, rows=32, **kw):
            return run(e, cond, text[:rows], STEPS, no_engine=True, **kw) + (e.attn_kv8_used(),)

        r = dict(parent=go(plain), on=go(eng), eager=go(eng, no_graph=True), again=go(eng), fresh=go(build(attn_kv8=True)), rows8=go(eng, rows=8))
        for key, setter, on in (("off", eng.set_attn_kv8, False), ("on2", eng.set_attn_kv8, True), ("cache16", eng.set_kv_fp8, False)):
            setter(on)
            r[key] = go(eng)
        eng.set_kv_fp8(True)
        mp.setenv("ITTS_ATTN_KV8", "0")  # the environment overrides the setter
        r["env0"] = go(eng)
        mp.delenv("ITTS_ATTN_KV8")
        yield r


def test_what_ran_and_self_consistency(runs):
    r = runs
    assert {k: v[3] for k, v in r.items()} == dict(parent=0, on=1, eager=1, again=1, fresh=1, rows8=0, off=0, on2=1, cache16=0, env0=0)
    assert all(v[2] == 0 for v in r.values())  # the launch path
    assert same_bits(r["eager"], r["on"]), "graph replay != eager launches"
    assert same_bits(r["again"], r["on"]), "a repeat differs"
    assert np.array_equal(r["on"][1][30:].view(np.uint32), r["on"][1][:2].view(np.uint32)), "identical rows, different logits"
    assert same_bits(r["off"], r["parent"]) and same_bits(r["env0"], r["parent"]), "switch off != an engine object that never saw it"
    assert same_bits(r["on2"], r["on"]) and same_bits(r["fresh"], r["on"]), "flipping the switch: not the result of a fresh object"
    assert not np.array_equal(r["on"][1], r["parent"][1]), "another summation order, yet the same bits: the kernel did not run"


def test_beam_steps():
    """33 beam rows x 20 heads: with an ancestry the switch takes the step too, unless the grouped fp8 kernel does"""
    both = build_beams(kv_fp8=True, attn_kv8=True, group_attn=True, group_attn_kv_fp8=True)
    cond, text = both.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7))), ragged(11, 11)
    for grouped in (True, False):
        both.set_group_attn_kv_fp8(grouped)
        got = run_beams(both, cond, text)
        assert (got[2], both.attn_kv8_used()) == ((2, 0) if grouped else (0, 1)) and bool(np.isfinite(got[1]).any())


def test_accuracy_against_the_fp32_reference(sd_smooth, mel, gold):  # noqa: F811
    eng, g = ieng.build_engine(CFG, "bf16", parts=("gpt",), state_dicts={"gpt": sd_smooth}, kv_fp8=True, attn_kv8=True), gold("smooth_decode_b1")
    lgs = forced_trace(eng, eng.conditioning(mel), g, 32)
    assert eng.attn_kv8_used() == 1 and eng.decode_mode() == 0
    for k, lg in lgs.items():
        assert np.array_equal(lg, np.repeat(lg[:1], 32, 0)), (k, "identical rows, different logits")
    res = top8_err(lgs, g)
    agree = [int(lgs[int(k)][0].argmax()) == int(g["top_idx"][i][0]) for i, k in enumerate(g["trace_steps"])]
    print(f"attn_kv8 on, fp8 cache, 32 rows, smooth checkpoint: top-8 logits rel RMS vs fp32 reference, worst {max(res.values()):.3e} by S " +
          " ".join(f"{S}:{v:.3e}" for S, v in sorted(res.items())) + f"; arg-max equal at {sum(agree)} of {len(agree)} traced steps")
    assert max(res.values()) < BOUND_KV_FP8, res
    assert all(agree), agree
