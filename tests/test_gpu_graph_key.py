"""GPU: the captured decode step is replayed only while its key (csrc/engine.h GraphKey) is unchanged.

Everything SamplerArgs / BeamArgs / EngArgs carry by value is baked into the nodes of the captured hipGraph, so a request
that changes one of those values on the same engine object has to re-capture.  A value missing from the key replays the
previous request's step and reports nothing - so every case here generates with setting A on the graph path, changes ONE
per-request value, generates again on the same object (and then once more with A: the way back) and compares with eager
launches (debug(no_graph=True)) of the same requests on the same object: ids exact, last-step logits bit for bit.  The two eager
runs must differ, otherwise a stale graph could not be seen.

Micro configuration, bf16, 2 rows (3 where the row count is the value), 12 - 16 steps in chunks of 8 (both executables: the
8-step one and the single step).  Reference hot loop: indextts/gpt/model.py:115-192, 655-708."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import config as icfg  # noqa: E402
from itts_hip import engine as ieng  # noqa: E402
from itts_hip import synth  # noqa: E402

CFG = icfg.micro()
TEXT = np.stack([synth.text_ids(9, 500 + i, CFG.gpt.number_text_tokens) for i in range(3)]).astype(np.int32)
GIVEN = np.array([[7, 21, 40, 3, 58], [33, 12, 60, 47, 9]], np.int32)  # forced tokens / `input_tokens` of the two rows

# one request: what the Python Engine API lets a caller set per generation
BASE = dict(rows=2, max_gen=14, penalty=10.0, suppress_stop=True, sample=False, top_k=30, top_p=0.8, temperature=1.0, typical=0.0,
            forced=0, input_tokens=0, beams=1, beam_sample=True, length_penalty=0.0, seed=5)
SAMPLE = dict(sample=True)
# close to uniform draws over the 66 codes: with eos enabled both rows draw the stop token inside the run (seed 5)
EOS = dict(sample=True, top_k=64, top_p=1.0, temperature=4.0)
BEAMS = dict(beams=3, suppress_stop=False)

# (name, request A, request B): B differs from A in exactly one value
CASES = [
    ("max_gen", dict(max_gen=16), dict(max_gen=12)),
    ("repetition_penalty", dict(), dict(penalty=1.0)),
    ("suppress_stop", dict(EOS), dict(EOS, suppress_stop=False)),
    ("sampling_off_on", dict(), dict(SAMPLE)),
    ("top_k", dict(SAMPLE), dict(SAMPLE, top_k=3)),
    ("top_p", dict(SAMPLE), dict(SAMPLE, top_p=0.3)),
    ("temperature", dict(SAMPLE), dict(SAMPLE, temperature=0.4)),
    ("typical_off_on", dict(), dict(typical=0.5)),
    ("typical_mass", dict(typical=0.2), dict(typical=0.9)),
    ("forced_off_on", dict(), dict(forced=3)),
    ("forced_to_input_tokens", dict(forced=3), dict(input_tokens=3)),
    ("input_tokens_length", dict(input_tokens=3), dict(input_tokens=5)),
    ("host_sampling", dict(SAMPLE, top_k=3), dict(SAMPLE, top_k=0)),  # (3: a nucleus the whole-vocabulary warpers do not share)
    ("beams_1_to_3", dict(suppress_stop=False), dict(BEAMS)),
    ("beams_2_to_3_at_six_rows", dict(BEAMS, beams=2, rows=3), dict(BEAMS, beams=3, rows=2)),  # (B unchanged: only nb tells them apart)
    ("beam_search_vs_beam_sample", dict(BEAMS), dict(BEAMS, beam_sample=False)),
    ("length_penalty", dict(BEAMS, beam_sample=False), dict(BEAMS, beam_sample=False, length_penalty=2.0)),
    ("rows_2_to_3", dict(), dict(rows=3)),
]


@pytest.fixture(scope="module")
def eng():
    return ieng.build_engine(CFG, "bf16", parts=("gpt",))


@pytest.fixture(scope="module")
def cond(gold):
    return torch.from_numpy(gold("micro_conditioning")["cond"])


def generate(eng, cond, req, no_graph):
    """One request through the engine's public calls -> (ids, last-step logits or None where the caller samples)."""
    r = dict(BASE, **req)
    rows, n, nb = r["rows"], r["max_gen"], r["beams"]
    text = TEXT[:rows]
    warp = dict(top_k=r["top_k"], top_p=r["top_p"], temperature=r["temperature"])
    rng = np.random.default_rng(r["seed"])
    eng.debug(no_graph=no_graph)
    try:
        if r["sample"] and r["top_k"] == 0:  # the warpers over the whole vocabulary: token choice on the host, decode(1) per token
            ids = eng.generate(cond, text, n, r["penalty"], r["suppress_stop"], do_sample=True, uniforms=rng.random((n, rows), dtype=np.float32), **warp)
            return ids, None
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, float(r["typical"])), "gpt_set_typical")
        if nb > 1:
            eng.set_beam_sample(nb, uniforms=rng.random((n, rows, 2 * nb), dtype=np.float32), do_sample=r["beam_sample"],
                                length_penalty=r["length_penalty"], **warp)
        elif r["sample"]:
            eng.set_sampling(True, uniforms=rng.random((n, rows), dtype=np.float32), **warp)
        if r["forced"]:
            eng.set_forced(GIVEN[:, :r["forced"]])
        if r["input_tokens"]:
            eng.set_input_tokens(GIVEN[:, :r["input_tokens"]])
        eng.prefill(cond, text, n, r["penalty"], r["suppress_stop"])
        for done in range(1, n, 8):
            eng.decode(min(8, n - done))
        ids, lg = eng.fetch(logits=True)
        eng._exit()
        return ids.copy(), lg.copy()
    finally:
        eng.debug()
        eng._ck(eng.lib.itts_gpt_set_typical(eng.h, 0.0), "gpt_set_typical")
        eng.set_beam_sample(1)
        eng.set_sampling(False)
        eng.set_forced(None)


def same(got, want):
    return np.array_equal(got[0], want[0]) and (want[1] is None or np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))


@pytest.mark.parametrize("name,a,b", CASES, ids=[c[0] for c in CASES])
def test_changed_request_value_recaptures_the_step(eng, cond, name, a, b):
    eager_a = generate(eng, cond, a, no_graph=True)
    eager_b = generate(eng, cond, b, no_graph=True)
    assert not np.array_equal(eager_a[0], eager_b[0]), "A and B give the same ids: a stale graph would not show"
    assert same(generate(eng, cond, a, no_graph=False), eager_a)
    assert same(generate(eng, cond, b, no_graph=False), eager_b), f"{name}: the step captured for A was replayed for B"
    assert same(generate(eng, cond, a, no_graph=False), eager_a), f"{name}: the step captured for B was replayed for A"
