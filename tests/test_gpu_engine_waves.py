"""GPU: which wave does what in a block of the persistent decode engine (csrc/decode_engine.hip).

The engine's results do not depend on which wave runs a c_attn row, on which waves the `own` counter counts, or on which lanes hold
a dimension of the attention partial behind the slot reduction - only its timing does.  These tests pin that, bit for bit:

  * window edges: 1 - 4 rows against the launch path (ITTS_ENGINE=0: gemv_bf16_kernel + decode_attn2_kernel) while the sequence
    length S crosses an edge of the attention's key windows during the run: a slot-window edge (a multiple of 32: here S = 31 -> 34
    and 63 -> 66) and the split edge (S = 127 -> 130: the first key of the second round of windows).  Behind such an edge a split
    or a slot that was empty holds its first key - a wrong lane map of the slot reduction, or of the store of a wave's partial,
    shows there.  The prefix of the 1.5 model is 32 conditioning latents + text + 2, so S >= 36 behind the shortest text:
    S = 31 -> 34 runs on a model with 24 conditioning latents (same GPT blocks);
  * slot reuse: the loader refills weight slot A (c_attn -> c_fc) as soon as the `own` counter says that every wave is through
    c_attn.  The pacing switches are read once per process, so each setting runs in a fresh child process, one at a time, each under
    a time limit: rows 2 and 4 against the launch path, row 6 (the half-slot map) against the engine at default settings;
  * the head outside the launch (ITTS_ENGINE_HEAD=0): the counter's targets differ (rows 2 and 4 against the launch path; 6 rows:
    ids only, the separate head launch runs on the matrix cores there).

Every comparison is np.array_equal on ids and on the bits of the last step's logits; Engine.status() raises if a hand-off gave up."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = 3  # the smallest depth at which the weight-slot rotation is in steady state
STEPS = 12  # the sequence length moves by STEPS - 1 during a run


def cfg3(latents=32):
    c = icfg.indextts_1_5()
    c.gpt.layers = LAYERS
    c.gpt.condition_num_latent = latents
    return c


def build(latents=32):
    c = cfg3(latents)
    sd = synth.gpt_state_dict(c, 1234)
    sd["perceiver_encoder.latents"] = sd["perceiver_encoder.latents"][:latents]
    eng = ieng.build_engine(c, "bf16", parts=("gpt",), state_dicts={"gpt": sd})
    cond = torch.from_numpy(np.random.default_rng(5).standard_normal((latents, c.gpt.model_dim)).astype(np.float32))
    return eng, cond


@pytest.fixture(scope="module")
def eng32():
    return build(32)


@pytest.fixture(scope="module")
def eng24():
    return build(24)


def texts(cfg, lens, seed):
    """One row per entry of lens; shorter rows are left-padded by the prefix builder (kv_start > 0)."""
    text = np.full((len(lens), max(lens)), cfg.gpt.stop_text_token, np.int32)
    for r, n in enumerate(lens):
        text[r, :n] = synth.text_ids(n, seed + r, cfg.gpt.number_text_tokens)
    return text


def run(eng, cond, text, steps, engine):
    eng.debug(no_engine=not engine, engine=engine)
    try:
        eng.prefill(cond, text, steps, 10.0, True)
        eng.decode(steps - 1)
        eng.status()  # raises lib.HandoffTimeout if a wait of the engine gave up
        codes, lg = eng.fetch(logits=True)
        mode = eng.decode_mode()
        eng._exit()
    finally:
        eng.debug()
    return codes.copy(), lg.copy(), mode


def both_paths_equal(eng, cond, text, steps=STEPS):
    ref = run(eng, cond, text, steps, engine=False)
    got = run(eng, cond, text, steps, engine=True)
    assert (ref[2], got[2]) == (0, 1), (ref[2], got[2])
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), float(np.abs(got[1] - ref[1]).max())


def text_len(latents, s_edge):
    """Text length whose run of STEPS - 1 decode steps has the sequence length cross s_edge: the prefix is latents + text + 2, the
    first decode step sees prefix + 1 or + 2 keys, the run starts five keys below the edge and ends at least four above it."""
    n = s_edge - 5 - latents - 2
    assert n >= 1
    return n


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
@pytest.mark.parametrize("s_edge", [64, 128])
def test_window_edges(eng32, rows, s_edge):
    eng, cond = eng32
    n = text_len(32, s_edge)
    both_paths_equal(eng, cond, texts(cfg3(), [n] * rows, 11 + s_edge))


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_first_window_edge_with_24_latents(eng24, rows):
    """S = 31 -> 34: the second slot window (keys 32 .. 63, split 1) gets its first key."""
    eng, cond = eng24
    n = text_len(24, 32)
    both_paths_equal(eng, cond, texts(cfg3(24), [n] * rows, 71))


@pytest.mark.parametrize("s_edge", [64, 128])
def test_window_edges_ragged_pair(eng32, s_edge):
    """Two rows of different text lengths: row 1 is left-padded, its first valid key is not key 0 (kv_start = 9)."""
    eng, cond = eng32
    n = text_len(32, s_edge)
    both_paths_equal(eng, cond, texts(cfg3(), [n, n - 9], 31 + s_edge))


# ---- the pacing switches and the head switch: one fresh process per setting ----
_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%r, %r]
sys.path.insert(0, %r)
import test_gpu_engine_waves as T
eng, cond = T.build(32)
cfg = T.cfg3()
out = {}
for rows in (2, 4):
    T.both_paths_equal(eng, cond, T.texts(cfg, [41] * rows, 61))
codes, lg, mode = T.run(eng, cond, T.texts(cfg, [41] * 6, 81), T.STEPS, engine=True)
assert mode == 1, "the persistent engine did not run"
np.savez(sys.argv[1], codes=codes, logits=lg)
print("CHILD OK")
"""
SWITCHES = ("ITTS_ENGINE_EARLY_FC", "ITTS_ENGINE_THIN_FC", "ITTS_ENGINE_FIRST_DELAY", "ITTS_ENGINE_PASS_SLEEP", "ITTS_ENGINE_HEAD")


def child(tmp_path, name, setting):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(setting)
    out = str(tmp_path / (name + ".npz"))
    src = _CHILD % (ROOT, os.path.join(ROOT, "index-tts-ipex_amd"), os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", src, out], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and "CHILD OK" in p.stdout, (setting, p.stdout[-1000:], p.stderr[-3000:])
    with np.load(out) as z:
        return z["codes"].copy(), z["logits"].copy()


@pytest.fixture(scope="module")
def six_rows_default(tmp_path_factory):
    return child(tmp_path_factory.mktemp("waves"), "default", {})


@pytest.mark.parametrize("setting", [
    {"ITTS_ENGINE_EARLY_FC": "1"},  # slot A refilled as soon as the counter allows: catches a reader the counter forgot
    {"ITTS_ENGINE_EARLY_FC": "0"},
    {"ITTS_ENGINE_THIN_FC": "1"},
    {"ITTS_ENGINE_FIRST_DELAY": "1", "ITTS_ENGINE_PASS_SLEEP": "0"},
], ids=lambda s: ",".join(f"{k[12:]}={v}" for k, v in s.items()))
def test_slot_reuse_under_the_pacing_switches(tmp_path, six_rows_default, setting):
    codes, lg = child(tmp_path, "set", setting)
    assert np.array_equal(codes, six_rows_default[0])
    assert np.array_equal(lg.view(np.uint32), six_rows_default[1].view(np.uint32))


def test_head_outside_the_launch(tmp_path, six_rows_default):
    """ITTS_ENGINE_HEAD=0: ln_f -> final_norm -> mel_head as launches of their own.  Rows 2 and 4 equal the launch path bit for bit
    (checked in the child).  At 6 rows that separate head runs on the matrix cores, so its logits are not the bits of the head
    inside the launch: the ids are compared, the logits are not."""
    codes, _ = child(tmp_path, "head", {"ITTS_ENGINE_HEAD": "0"})
    assert np.array_equal(codes, six_rows_default[0])
