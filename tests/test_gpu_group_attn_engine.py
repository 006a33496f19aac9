"""The grouped cache attention inside the decode step (Engine.set_group_attn / ITTS_GROUP_ATTN).  3 layers at the 1.5 dims, bf16, 4
sentences x 3 beams = 12 rows, beam_sample with fixed draws, 24 steps, suppress_stop, ITTS_GEMM_KSPLIT=0.  Picked: the ragged texts of
tests/test_gpu_row_retire.py seed 11, draws default_rng(9), top_k = 2, the "smooth" weights of tests/test_gpu_beam_retire.py (their
flat distributions put a draw so close to a boundary at top_k = 30 that the parent's bf16 run leaves the fp32 engine's beams within
two steps for 2 texts x 4 draw seeds; at top_k = 2 it follows them through all 23 steps).
On against off: the two 16-bit paths differ in summation order and in terms below 2^-16, so the grouped run must lie no farther from
the parent's 16-bit run than that run lies from the fp32 engine: relative RMS of the logits over the steps at which the runs' beams
hold the same id histories (through step 8 at least, asserted).  Values: group_attn.txt under ITTS_TEST_OUT."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from itts_hip import synth
from test_gpu_beam_retire import build, ragged

STEPS, NB, DRAWS, TOP_K = 24, 3, 9, 2


def run(eng, cond, text, on=None, graph=True, engine=False, draws=DRAWS, top_k=TOP_K):
    # -> (the beams' id histories per step, entries behind the step zeroed; logits per step; group_attn_used; decode_mode)
    u = np.random.default_rng(draws).random((STEPS, text.shape[0], 2 * NB), dtype=np.float32)
    eng.debug(no_graph=not graph, no_engine=not engine, engine=engine)
    if on is not None:
        eng.set_group_attn(on)
    eng.set_beam_sample(NB, top_k=top_k, uniforms=u)
    try:
        eng.prefill(cond, text, STEPS, 10.0, True)
        ids, lgs = [], []
        for _ in range(STEPS - 1):
            eng.decode(1)
            hist, k = np.zeros((text.shape[0] * NB, STEPS), dtype=np.int32), C.c_int()
            eng._ck(eng.lib.itts_gpt_beam_state(eng.h, hist.ctypes.data_as(C.c_void_p), None, None, C.byref(k), eng._s()), "gpt_beam_state")
            hist[:, k.value:] = 0
            ids.append(hist), lgs.append(eng.fetch(logits=True)[1])
        used, mode = eng.group_attn_used(), eng.decode_mode()
        eng._exit()
    finally:
        eng.set_beam_sample(1)
        eng.debug()
    return np.stack(ids), np.stack(lgs), used, mode


@pytest.fixture(scope="module")
def runs():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ITTS_GEMM_KSPLIT", "0")
        mp.delenv("ITTS_GROUP_ATTN", raising=False)
        eng, plain, f32 = build(), build(), build(dtype="f32")
        cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
        text = ragged(4, 11)
        r = dict(parent=run(plain, cond, text), f32=run(f32, cond, text), off=run(eng, cond, text, on=False), on=run(eng, cond, text, on=True),
                 eager=run(eng, cond, text, graph=False), again=run(eng, cond, text), off2=run(eng, cond, text, on=False),
                 on2=run(eng, cond, text, on=True), six=run(eng, cond, text[:2], engine=True))
        mp.setenv("ITTS_GROUP_ATTN", "0")  # the environment overrides the setter
        r["env0"] = run(eng, cond, text)
        yield r


@pytest.mark.gpu
def test_switch_and_graph_key(runs):
    r, same = runs, lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert r["parent"][2] == 0 and r["off"][2] == 0 and same(r["off"], r["parent"]), "switch off != an engine without the switch"
    assert r["on"][2] == 1 and r["on"][3] == 0, "the grouped kernel did not run at 12 rows"
    assert same(r["eager"], r["on"]) and r["eager"][2] == 1, "graph replay != eager"
    assert same(r["again"], r["on"]), "a repeat differs"
    assert same(r["off2"], r["parent"]) and r["off2"][2] == 0 and same(r["on2"], r["on"]) and r["on2"][2] == 1, "flipping the switch"
    assert r["env0"][2] == 0 and same(r["env0"], r["parent"]), "ITTS_GROUP_ATTN=0 does not override the setter"
    assert r["six"][3] == 1 and r["six"][2] == 0, "6 rows left the persistent engine"


@pytest.mark.gpu
def test_grouped_against_the_parent_and_fp32(runs):
    def compare(a, b):
        diff = [k for k in range(STEPS - 1) if not np.array_equal(a[0][k], b[0][k])]
        n = diff[0] if diff else STEPS - 1
        x, y = a[1][:n].astype(np.float64), b[1][:n].astype(np.float64)
        ok = np.isfinite(x) & np.isfinite(y)
        return n, float(np.sqrt(((x - y)[ok] ** 2).mean() / (y[ok] ** 2).mean()))

    n32, yard = compare(runs["parent"], runs["f32"])
    ng, got = compare(runs["on"], runs["parent"])
    lines = [f"parent bf16 launch path vs fp32 engine: beam histories agree through step {n32}, logits rel RMS {yard:.3e} (the yardstick)",
             f"grouped attention vs parent bf16 path:  beam histories agree through step {ng}, logits rel RMS {got:.3e}"]
    print("\n".join(lines))
    if os.environ.get("ITTS_TEST_OUT"):
        os.makedirs(os.environ["ITTS_TEST_OUT"], exist_ok=True)
        with open(os.path.join(os.environ["ITTS_TEST_OUT"], "group_attn.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    assert n32 >= 8 and ng >= 8, (n32, ng)
    assert got <= yard, (got, yard)
