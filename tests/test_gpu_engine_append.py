"""GPU: the cache append of the persistent decode engine (csrc/decode_engine.hip, attention phase).

The engine keeps this step's k / v fragment packed in registers, scores it like any other cache row and writes it to the cache
behind the publish of the context, one 16-byte store per lane.  What these tests pin:

  * the launch path READS what the engine appended: 12 steps on the engine, then 12 on the launch path after the same prefill, equal
    an all-launch-path run bit for bit, codes and logits of every step (1 - 3 rows, and 1 x 3 beam rows through the ancestry gather);
  * ragged rows (kv_start > 0), the fp8 opt-in engine and the IEEE-half library: engine == launch path bit for bit;
  * the product library ignores the probe switch ITTS_ENG_FAKE_DIV (the probe code lives in the probes library only).

Every comparison is exact (view(np.uint32)); there is no tolerance."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402

CFG = icfg.indextts_1_5()
CFG3 = icfg.indextts_1_5()  # 3 blocks: the smallest depth at which the weight-slot rotation is in steady state
CFG3.gpt.layers = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng16():
    return ieng.build_engine(CFG, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def cond(eng16):
    return eng16.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))


def texts(rows, seed, n=105):
    return np.stack([synth.text_ids(n, seed + r, CFG.gpt.number_text_tokens) for r in range(rows)]).astype(np.int32)


def logits_only(eng, nrows):
    lg = np.empty((nrows, eng.ccfg.number_mel_codes), dtype=np.float32)
    eng._ck(eng.lib.itts_gpt_fetch(eng.h, None, lg.ctypes.data_as(C.c_void_p), eng._s()), "gpt_fetch")
    return lg


def stepwise(eng, cond, text, steps, engine_steps, nrows=None):
    """Prefill, then `steps` single decode steps: the first `engine_steps` on the persistent engine, the rest on the launch path
    (the switch is honoured in mid-generation: the path is chosen per step).  Returns the final codes, the logits behind the
    prefill and behind every step, and the path every step ran on."""
    nrows = nrows or text.shape[0]
    lgs, modes = [], []
    try:
        eng.debug(no_engine=engine_steps == 0, engine=engine_steps > 0)
        eng.prefill(cond, text, steps + 1, 10.0, True)
        lgs.append(logits_only(eng, nrows))
        for k in range(steps):
            if k == engine_steps:
                eng.debug(no_engine=True)
            eng.decode(1)
            lgs.append(logits_only(eng, nrows))
            modes.append(eng.decode_mode())
        codes = eng.fetch().copy()
        eng._exit()
    finally:
        eng.debug()
    return codes, np.stack(lgs), modes


def assert_same(got, ref):
    assert np.array_equal(got[0], ref[0])
    bad = np.nonzero((got[1].view(np.uint32) != ref[1].view(np.uint32)).reshape(got[1].shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, f"logits differ first behind step {int(bad[0])}"


@pytest.mark.parametrize("rows", [1, 2, 3])
def test_launch_path_reads_the_rows_the_engine_appended(eng16, cond, rows):
    text = texts(rows, 11)
    ref = stepwise(eng16, cond, text, 24, 0)
    got = stepwise(eng16, cond, text, 24, 12)
    assert ref[2] == [0] * 24 and got[2] == [1] * 12 + [0] * 12, (ref[2], got[2])
    assert_same(got, ref)


def test_launch_path_reads_the_rows_the_engine_appended_beam_rows(eng16, cond):
    """1 sentence x 3 beams (beam_sample): the launch path gathers the rows the engine appended through the ancestry table."""
    text, nb, n = texts(1, 51), 3, 24
    u = np.random.default_rng(9).random((n + 1, 1, 2 * nb), dtype=np.float32)
    res = []
    try:
        for engine_steps in (0, 12):
            eng16.set_beam_sample(nb, 30, 0.8, 1.0, u, do_sample=True)
            res.append(stepwise(eng16, cond, text, n, engine_steps, nrows=nb))
    finally:
        eng16.set_beam_sample(1)
    ref, got = res
    assert ref[2] == [0] * n and got[2] == [1] * 12 + [0] * 12, (ref[2], got[2])
    assert_same(got, ref)


def both_paths(eng, cond, text, steps):
    out = []
    for no_engine in (True, False):
        eng.debug(no_engine=no_engine, engine=not no_engine)
        try:
            eng.prefill(cond, text, steps, 10.0, True)
            eng.decode(steps - 1)
            codes, lg = eng.fetch(logits=True)
            out.append((codes.copy(), lg.copy(), eng.decode_mode()))
            eng._exit()
        finally:
            eng.debug()
    ref, got = out
    assert (ref[2], got[2]) == (0, 1)
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), float(np.abs(got[1] - ref[1]).max())


def test_ragged_rows(eng16, cond):
    """Text lengths 105 and 33: row 1 is left-padded (kv_start > 0), its first valid cache row is not row 0."""
    text = np.full((2, 105), CFG.gpt.stop_text_token, np.int32)
    for r, n in enumerate([105, 33]):
        text[r, :n] = synth.text_ids(n, 21 + r, CFG.gpt.number_text_tokens)
    both_paths(eng16, cond, text, 40)


def test_fp8_engine(cond):
    eng8 = ieng.build_engine(CFG3, "bf16", parts=("gpt",), gpt_fp8="fp8", engine_fp8=True)
    both_paths(eng8, cond, texts(2, 31, 41), 16)


def test_ieee_half_library():
    engh = ieng.build_engine(CFG3, "f16", parts=("gpt",))
    assert engh.lib.itts_half_is_f16() == 1
    condh = engh.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
    both_paths(engh, condh, texts(2, 41, 41), 16)


_CHILD = r"""
import json, sys
import numpy as np
import torch
sys.path[:0] = [%r, %r]
from itts_hip import config as icfg, engine as ieng, synth
cfg = icfg.indextts_1_5()
cfg.gpt.layers = 3
eng = ieng.build_engine(cfg, "bf16", parts=("gpt",))
cond = eng.conditioning(torch.from_numpy(synth.prompt_mel(511, seed=7)))
text = np.stack([synth.text_ids(41, 61 + r, cfg.gpt.number_text_tokens) for r in range(2)]).astype(np.int32)
eng.debug(engine=True)
codes = eng.generate(cond, text, 16, suppress_stop=True)
print("CODES " + json.dumps([eng.decode_mode(), codes.tolist()]))
"""


def test_product_library_ignores_the_gather_divisor_probe():
    """ITTS_ENG_FAKE_DIV=3 makes the probes library gather a third of two edges (wrong results by design).  The product library has
    no such code: a fresh process with the variable set returns the codes of one without it."""
    out = []
    for fake in (None, "3"):
        env = {k: v for k, v in os.environ.items() if k != "ITTS_ENG_FAKE_DIV"}
        if fake:
            env["ITTS_ENG_FAKE_DIV"] = fake
        p = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "index-tts-ipex_amd"))], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        line = [x for x in p.stdout.splitlines() if x.startswith("CODES ")][-1]
        out.append(json.loads(line[6:]))
    assert out[0][0] == 1 and out[1][0] == 1, "the persistent engine did not run"
    assert out[0][1] == out[1][1]
