"""GPU: results of the persistent decode engine (csrc/decode_engine.hip) that must not depend on WHICH workgroup owns a feature, in
which order a gather walks an edge, or where a workgroup runs on the chip.

Which workgroup computes a projection feature, a head's attention or a mel_head row, and in which order its gather waves request
the granules of an edge, is free: a feature's dot product, wave reduction and epilogue are the same wherever it runs, and a gather
puts granule i into LDS word i whenever it arrives.  These cases pin what follows from that - they pass before and after any change
of ownership, sweep order or placement, and do not look for one:

  * 1 - 4 rows (bf16, and fp8 weights at 2 rows): ids and the uint32 bits of EVERY decode step's logits equal the launch path's
    (debug(no_engine=True): gemv_bf16_kernel + decode_attn2_kernel + sampler2_kernel);
  * 6 rows (bf16, fp8 weights, fp8 K/V cache) and 2 rows on the fp8 K/V cache: every row equals the same row decoded alone on the
    engine, ids and bits of every step (ITTS_GEMM_KSPLIT=0, the project's batch-invariance mode for the prefill).  The launch path
    is no bit reference there: at 5 - 6 rows its projections run on the matrix cores, and on an fp8 cache it has the whole-form
    attention only, another summation order than the engine's four key splits (tests/test_gpu_engine_kv_fp8.py holds those two
    to a tolerance);
  * the head's extra-row owners: V = 8194 (the model's own: 32 rows per workgroup + 2 workgroups with a 33rd) is every case above;
    one case runs V = 8448 (33 rows everywhere, no extra owner);
  * two generations on one engine object, graph replay against eager launches against the launch path;
  * one case whose 6 decode steps cross S = 256, the first edge of the attention's register window that is tested at run time (the
    window pairs below it are requested unconditionally), with ragged rows (kv_start > 0).

Engine.status() runs after every generation: it raises if a hand-off of the engine gave up.

Sizes: engine dims (D = 1280, H = 20: the kernel is compiled for them), 2 blocks (the first block has no E1 hop and the last one
publishes to the head: both special forms and nothing else), 8 text tokens (S = 44 ..), prefill + 6 decode steps; the window-edge case
219 text tokens (S = 255 ..).  A case takes about a second."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402

LAYERS = 2
L_TEXT = 8
STEPS = 7  # the prefill's token + 6 decode steps
L_EDGE = 219  # prefix 32 + 219 + 2 = 253: the first decode step appends row 254 (S = 255), the third one reads past 256


@pytest.fixture(autouse=True)
def no_env(monkeypatch):
    for name in ("ITTS_KV_FP8", "ITTS_ENGINE_KV_FP8", "ITTS_ENGINE_FP8", "ITTS_ENGINE_TIMEOUT_TICKS", "ITTS_ENGINE", "ITTS_ENGINE_HEAD"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ITTS_GEMM_KSPLIT", "0")  # a row's prefill does not depend on the batch it is in


def cfg_v(V=None):
    c = icfg.indextts_1_5()
    c.gpt.layers = LAYERS
    if V is not None:
        c.gpt.number_mel_codes = V
    return c


def build(V=None, **kw):
    c = cfg_v(V)
    eng = ieng.build_engine(c, "bf16", parts=("gpt",), state_dicts={"gpt": synth.gpt_state_dict(c, 1234)}, **kw)
    cond = torch.from_numpy(np.random.default_rng(5).standard_normal((32, c.gpt.model_dim)).astype(np.float32))
    return eng, cond, c


@pytest.fixture(scope="module")
def eng_bf16():
    return build()


@pytest.fixture(scope="module")
def eng_w8():
    return build(gpt_fp8="fp8", engine_fp8=True)


@pytest.fixture(scope="module")
def eng_kv8():
    return build(kv_fp8=True, engine_kv_fp8=True)


def texts(cfg, lens, seed, width=None):
    """rows of the given lengths, padded with the stop id (prefill strips it and left-pads: kv_start > 0 on the shorter rows)"""
    text = np.full((len(lens), width or max(lens)), cfg.gpt.stop_text_token, np.int32)
    for r, n in enumerate(lens):
        text[r, :n] = synth.text_ids(n, seed + r, cfg.gpt.number_text_tokens)
    return text


def run(eng, cond, text, engine, steps=STEPS, no_graph=False):
    """-> ids [rows, steps], logits of every decode step [steps - 1][rows, V], decode mode; status() raises on a give-up"""
    eng.debug(no_engine=not engine, engine=engine, no_graph=no_graph)
    per_step = []
    try:
        eng.prefill(cond, text, steps, 10.0, True)
        for _ in range(steps - 1):
            eng.decode(1)
            per_step.append(eng.fetch(logits=True)[1].copy())
        eng.status()
        codes = eng.fetch(logits=True)[0].copy()
        mode = eng.decode_mode()
        eng._exit()
    finally:
        eng.debug()
    return codes, per_step, mode


def assert_same(got, ref, rows_got=slice(None), rows_ref=slice(None), what=""):
    assert np.array_equal(got[0][rows_got], ref[0][rows_ref]), (what, got[0][rows_got], ref[0][rows_ref])
    assert len(got[1]) == len(ref[1]) == STEPS - 1
    for s, (a, b) in enumerate(zip(got[1], ref[1])):
        a, b = a[rows_got], b[rows_ref]
        assert np.isfinite(b).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "step", s, float(np.abs(a - b).max()))


def engine_equals_launch_path(eng, cond, text, **kw):
    ref = run(eng, cond, text, engine=False, **kw)
    got = run(eng, cond, text, engine=True, **kw)
    assert (ref[2], got[2]) == (0, 1), (ref[2], got[2])
    assert_same(got, ref)
    return ref, got


def rows_equal_rows_alone(eng, cond, text):
    got = run(eng, cond, text, engine=True)
    assert got[2] == 1
    for r in range(text.shape[0]):
        one = run(eng, cond, text[r:r + 1], engine=True)
        assert one[2] == 1
        assert_same(got, one, rows_got=slice(r, r + 1), what=f"row {r}")


LENS = [8, 5, 7, 8, 3, 6]


# ---- 1 - 4 rows against the launch path ----
@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_bf16_rows_equal_launch_path(eng_bf16, rows):
    eng, cond, cfg = eng_bf16
    assert cfg.gpt.number_mel_codes == 8194 and cfg.gpt.number_mel_codes % 256 == 2  # two workgroups own a 33rd mel_head row
    lens = [L_TEXT] * rows if rows < 4 else LENS[:rows]
    ref, _ = engine_equals_launch_path(eng, cond, texts(cfg, lens, 11 + rows, width=L_TEXT))
    assert ref[1][0].shape == (rows, cfg.gpt.number_mel_codes)


def test_fp8_weights_two_rows_equal_launch_path(eng_w8):
    eng, cond, cfg = eng_w8
    engine_equals_launch_path(eng, cond, texts(cfg, [L_TEXT, 5], 31, width=L_TEXT))


# ---- 6 rows (and the fp8 K/V cache at 2): every row against its own one-row run on the engine ----
def test_bf16_six_rows_equal_rows_alone(eng_bf16):
    eng, cond, cfg = eng_bf16
    rows_equal_rows_alone(eng, cond, texts(cfg, LENS, 41, width=L_TEXT))


def test_fp8_weights_six_rows_equal_rows_alone(eng_w8):
    eng, cond, cfg = eng_w8
    rows_equal_rows_alone(eng, cond, texts(cfg, LENS, 51, width=L_TEXT))


@pytest.mark.parametrize("rows", [2, 6])
def test_fp8_kv_rows_equal_rows_alone(eng_kv8, rows):
    eng, cond, cfg = eng_kv8
    rows_equal_rows_alone(eng, cond, texts(cfg, LENS[:rows], 61, width=L_TEXT))


# ---- the head's row owners: 33 rows on every workgroup (8194, two extra-row owners, is every other case) ----
def test_vocabulary_multiple_of_256():
    eng, cond, cfg = build(8448)
    assert cfg.gpt.number_mel_codes % 256 == 0
    engine_equals_launch_path(eng, cond, texts(cfg, [L_TEXT, 6], 71, width=L_TEXT))


# ---- two generations on one engine object: graph replay against eager launches ----
def test_two_generations_replay_equals_eager(eng_bf16):
    eng, cond, cfg = eng_bf16
    for lens, seed in (([8, 4], 81), ([6, 8], 91)):
        text = texts(cfg, lens, seed, width=L_TEXT)
        _, got = engine_equals_launch_path(eng, cond, text)
        eager = run(eng, cond, text, engine=True, no_graph=True)
        assert eager[2] == 1
        assert_same(eager, got)


# ---- the decode steps cross the first run-time edge of the attention's register window (S = 256) ----
def test_steps_cross_the_attention_window_edge(eng_bf16):
    eng, cond, cfg = eng_bf16
    assert 32 + L_EDGE + 2 + 1 < 256 < 32 + L_EDGE + 2 + STEPS
    engine_equals_launch_path(eng, cond, texts(cfg, [L_EDGE, 150], 101))
