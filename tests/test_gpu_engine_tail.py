"""GPU: what the persistent decode engine (csrc/decode_engine.hip) does around the blocks of a launch - the prologue, the head
(ln_f -> final_norm -> mel_head) and the in-launch greedy sampler.

Every workgroup scores its 32 - 33 mel_head rows (penalty, stop suppression), one wave per batch row reduces the workgroup's 33
candidates to its best (score, id) with a DPP arg-max (larger score, lower id on ties), and workgroup b gathers the 256 bests of
row b, commits the token and writes the next input embedding.  Every case compares the engine with the launch path
(debug(no_engine=True): gemv_bf16_kernel + decode_attn2_kernel + sampler2_kernel) with np.array_equal on the ids and on the uint32
bits of the last step's logits, and calls Engine.status() (raises if a hand-off gave up) after every run:

  * head row ownership: V = 8194 (32 rows per workgroup + 2 workgroups with an extra row), 8448 (33 rows everywhere, the largest
    vocabulary the head inside the launch takes) and 515 (2 rows per workgroup + 3 extras: most waves of a workgroup own no row, and
    most of the 33 candidates of a workgroup are the empty one), 1 - 4 rows;
  * penalty and stop handling: rep_penalty 1 / 10 x suppress_eos on / off - a `seen` byte read a step early or late flips ids;
  * ties across workgroups: mel_head rows at ids of two other workgroups are copies of the row that wins the first decode step
    (without penalty), so there the best score comes from three workgroups at once: the lowest id has to win, inside a workgroup
    (one wave per row reduces its 33 candidates) and through the candidate hop;
  * two generations on one engine object (step counter tag and prologue scalars across launches), graph replay against eager launches;
  * the fp8-weight form of the head.

Sizes: 3 blocks (the smallest depth with the slot rotation in steady state; the head and the sampler do not depend on the depth),
8 - 12 steps; a case takes about a second."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402

LAYERS = 3
NCU = 256  # workgroups of the engine: id n < NCU * (V // NCU) belongs to workgroup n // (V // NCU), the rest to workgroup n - NCU * (V // NCU)
SMALL_V = 515  # V % 256 != 0 and V // 256 < 3


def cfg_v(V):
    c = icfg.indextts_1_5()
    c.gpt.layers = LAYERS
    if V != c.gpt.number_mel_codes:
        c.gpt.number_mel_codes = V
        if V < 8194:  # start / stop ids inside the vocabulary
            c.gpt.start_mel_token, c.gpt.stop_mel_token = V - 2, V - 1
    return c


def build(V, sd=None, **kw):
    c = cfg_v(V)
    sd = synth.gpt_state_dict(c, 1234) if sd is None else sd
    eng = ieng.build_engine(c, "bf16", parts=("gpt",), state_dicts={"gpt": sd}, **kw)
    cond = torch.from_numpy(np.random.default_rng(5).standard_normal((32, c.gpt.model_dim)).astype(np.float32))
    return eng, cond, c


@pytest.fixture(scope="module")
def eng_model():
    return build(8194)


@pytest.fixture(scope="module")
def eng_8448():
    return build(8448)


@pytest.fixture(scope="module")
def eng_small():
    return build(SMALL_V)


def texts(cfg, lens, seed):
    text = np.full((len(lens), max(lens)), cfg.gpt.stop_text_token, np.int32)
    for r, n in enumerate(lens):
        text[r, :n] = synth.text_ids(n, seed + r, cfg.gpt.number_text_tokens)
    return text


def run(eng, cond, text, steps, engine, penalty=10.0, suppress=True, no_graph=False, every_step=False):
    """-> ids, last step's logits, decode mode (, the logits of every decode step)."""
    eng.debug(no_engine=not engine, engine=engine, no_graph=no_graph)
    per_step = []
    try:
        eng.prefill(cond, text, steps, penalty, suppress)
        if every_step:
            for _ in range(steps - 1):
                eng.decode(1)
                per_step.append(eng.fetch(logits=True)[1].copy())
        else:
            eng.decode(steps - 1)
        eng.status()
        codes, lg = eng.fetch(logits=True)
        mode = eng.decode_mode()
        eng._exit()
    finally:
        eng.debug()
    return (codes.copy(), lg.copy(), mode) + ((per_step,) if every_step else ())


def same_bits(got, ref):
    assert np.array_equal(got[0], ref[0]), (got[0], ref[0])
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), float(np.abs(got[1] - ref[1]).max())


def both_paths_equal(eng, cond, text, steps, **kw):
    ref = run(eng, cond, text, steps, engine=False, **kw)
    got = run(eng, cond, text, steps, engine=True, **kw)
    assert (ref[2], got[2]) == (0, 1), (ref[2], got[2])
    same_bits(got, ref)
    return ref, got


# ---- head row ownership ----
@pytest.mark.parametrize("rows", [1, 2, 3, 4])
@pytest.mark.parametrize("which", ["eng_model", "eng_8448", "eng_small"])
def test_head_row_ownership(request, which, rows):
    eng, cond, cfg = request.getfixturevalue(which)
    V = cfg.gpt.number_mel_codes
    assert (V + NCU - 1) // NCU <= 33
    if which == "eng_small":
        assert V % 256 != 0 and V // 256 < 3 and 0 <= cfg.gpt.start_mel_token < V and 0 <= cfg.gpt.stop_mel_token < V
    ref, _ = both_paths_equal(eng, cond, texts(cfg, [23 + 5 * r for r in range(rows)], 11 + rows), 9)  # prefill + 8 decode steps
    assert ref[1].shape == (rows, V) and np.isfinite(ref[1]).all()


# ---- penalty and stop handling ----
@pytest.mark.parametrize("suppress", [True, False])
@pytest.mark.parametrize("penalty", [1.0, 10.0])
def test_penalty_and_stop(eng_model, penalty, suppress):
    eng, cond, cfg = eng_model
    both_paths_equal(eng, cond, texts(cfg, [31, 27], 41), 13, penalty=penalty, suppress=suppress)  # prefill + 12 decode steps


# ---- ties across workgroups ----
def owner(n, V):
    per = V // NCU
    return n // per if n < NCU * per else n - NCU * per


def test_cross_workgroup_ties(eng_model):
    eng0, cond, cfg = eng_model
    V = cfg.gpt.number_mel_codes
    text = texts(cfg, [29, 29], 61)
    # the id that wins row 0's decode step 0 without penalty (ids[:, 0] is the prefill's token, chosen by the prefill's own sampler
    # launch; ids[:, 1] is the first token step - the first one the engine's in-launch sampler picks)
    w = int(run(eng0, cond, text, 2, engine=False, penalty=1.0, suppress=True)[0][0, 1])
    assert w < 8192
    lo, hi = (w + 32 * 37) % 8192, (w + 32 * 111) % 8192
    near = w // 32 * 32 + (w % 32 + 16) % 32  # the same workgroup, another wave's row (a wave owns three consecutive rows)
    assert len({owner(w, V), owner(lo, V), owner(hi, V)}) == 3 and owner(near, V) == owner(w, V) and abs(near - w) == 16
    sd = synth.gpt_state_dict(cfg, 1234)
    for k in ("mel_head.weight", "mel_head.bias"):
        sd[k] = sd[k].copy() if isinstance(sd[k], np.ndarray) else sd[k].clone()
        for c in (lo, hi, near):
            sd[k][c] = sd[k][w]
    eng, _, _ = build(8194, sd=sd)
    steps = 13
    ref = run(eng, cond, text, steps, engine=False, penalty=1.0, suppress=True)
    got = run(eng, cond, text, steps, engine=True, penalty=1.0, suppress=True, every_step=True)
    assert (ref[2], got[2]) == (0, 1)
    same_bits(got, ref)
    tied = 0
    for lg in got[3]:
        for r in range(lg.shape[0]):
            assert lg[r, w] == lg[r, lo] == lg[r, hi] == lg[r, near]
            tied += int((lg[r] == lg[r].max()).sum() >= 2)
    print("steps x rows whose top logit occurred at two ids or more:", tied, "of", len(got[3]) * 2)
    assert tied >= 1
    assert got[3][0][0].max() == got[3][0][0, w]  # by construction: row 0's first decode step
    first = min(w, lo, hi, near)  # the lowest id wins wherever the copies are on top
    for s, lg in enumerate(got[3]):
        for r in range(lg.shape[0]):
            if lg[r].max() == lg[r, w]:
                assert got[0][r, s + 1] == first, (s, r, got[0][r, s + 1], first)


# ---- two generations on one engine object ----
def test_two_generations_on_one_engine(eng_model):
    eng, cond, cfg = eng_model
    for lens, seed, steps in (([9, 7], 71, 9), ([57, 44], 81, 13)):
        text = texts(cfg, lens, seed)
        ref, got = both_paths_equal(eng, cond, text, steps)
        eager = run(eng, cond, text, steps, engine=True, no_graph=True)
        assert eager[2] == 1
        assert np.array_equal(eager[0], got[0])


# ---- fp8 weights ----
def test_fp8_head(eng_model):
    _, cond, cfg = eng_model
    eng8 = ieng.build_engine(cfg, "bf16", parts=("gpt",), state_dicts={"gpt": synth.gpt_state_dict(cfg, 1234)}, gpt_fp8="fp8", engine_fp8=True)
    both_paths_equal(eng8, cond, texts(cfg, [31, 22], 91), 9)
