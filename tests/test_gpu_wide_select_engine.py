"""GPU: Engine.set_wide_select / ITTS_WIDE_SELECT inside the decode step, fp32 micro model: every stepped pick passes the predicates of
tests/test_gpu_wide_sampler.py / test_gpu_wide_beam.py, graph replay equals eager, the switch off again gives the earlier bits."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_wide_beam as WB  # noqa: E402  (check_beam_steps)
import test_gpu_wide_sampler as WS  # noqa: E402  (check_steps)

from itts_hip import config as icfg, engine as ieng  # noqa: E402

N = 20


@pytest.mark.parametrize("nb", [1, 3])
def test_switch_on_off_and_environment(gold, nb, monkeypatch):
    cfg = icfg.micro()
    eng = ieng.build_engine(cfg, "fp32", parts=("gpt",))
    cond = eng.conditioning(torch.from_numpy(gold("micro_conditioning")["mel"]))
    text = np.concatenate([gold("micro_decode_b1")["text"], gold("micro_decode_b1_alt")["text"]], 0).astype(np.int32)
    monkeypatch.delenv("ITTS_WIDE_SELECT", raising=False)
    if nb == 1:
        u = np.random.default_rng(17).random((N, 2), dtype=np.float32)
        kw = dict(do_sample=True, top_k=0, top_p=0.8, temperature=0.9, uniforms=u, wide_sampler="device")
    else:
        u = np.random.default_rng(43).random((N, 2, 2 * nb), dtype=np.float32)
        kw = dict(do_sample=True, num_beams=nb, top_k=0, top_p=0.8, temperature=0.9, uniforms=u, wide_beam_sampler="device")

    def gen(no_graph=False):
        eng.debug(no_graph=no_graph)
        try:
            return eng.generate(cond, text, N, **kw), eng.decode_mode()
        finally:
            eng.debug()

    parent, mode = gen()
    eng.set_wide_select(True)
    try:
        if nb == 1:
            stepped, _, total = WS.check_steps(eng, cfg, cond, text, N, 0, 0.8, 0.9, u)
        else:
            stepped, total = WB.check_beam_steps(eng, cfg, cond, text, N, nb, 0, 0.8, 0.9, u, tag=f"wide_select micro {nb} beams")
        assert total >= N
        on, mode_on = gen()
        eager, _ = gen(no_graph=True)
        m = min(on.shape[1], stepped.shape[1])
        assert mode_on == mode and np.array_equal(on, eager) and np.array_equal(on[:, :m], stepped[:, :m])
        monkeypatch.setenv("ITTS_WIDE_SELECT", "0")  # the environment overrides the setter
        assert np.array_equal(gen()[0], parent)
        monkeypatch.delenv("ITTS_WIDE_SELECT")
        assert np.array_equal(gen()[0], on)
    finally:
        eng.set_wide_select(False)
    assert np.array_equal(gen()[0], parent)  # flipped back on the same engine object: the step is captured again
    monkeypatch.setenv("ITTS_WIDE_SELECT", "1")  # and over the setter in the other direction
    assert np.array_equal(gen()[0], on)
