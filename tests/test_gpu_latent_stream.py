"""GPU: the incremental packed latent pass (opt-in) - Engine.latent_stream / itts_gpt_latent_stream_open, _append, _close on the micro
checkpoint (fp32 engine and both 16-bit libraries) and at 1.5 dims.

The identity, bit for bit: after any sequence of appends the rows delivered so far are the first rows of Engine.latent_packed over the
complete inputs.  Inputs of tests/test_gpu_packed_latent.py: texts 40, 17, 30, codes 25, 31, 9, voices [2, 0, 1].  Three sequences are
opened together and fed in the uneven schedule [16, 0, 9], [0, 31, 0], [8, 0, 0], [1, 0, 0]: a first append of two sequences, one that
leaves two sequences alone, an 8-row append - below 16 GEMM rows, so that the 16-bit engines re-run the last 8 rows they already
computed - and a one-row append.  At 1.5 dims (CFG3 of tests/test_gpu_engine_fp8.py, 3 layers, bf16: every projection on gemm_p8 with
partly filled tiles) one sequence, text 41, gets its codes as 17 + 3 + 5.
Against the reference: the micro_latent fixture's sentence in two appends, under the bars of tests/test_gpu_engine.py::test_latent.
Refusals (host, message begins with the entry's name): an append without an open stream, a second open, an append past max_codes, a mel
code out of range.  Decode safety: decode_mode() and the codes of a generation after a closed stream are those before it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from itts_hip import synth  # noqa: E402
from test_gpu_engine import relerr, rms_rel  # noqa: E402
from test_gpu_engine_fp8 import CFG3  # noqa: E402
from test_gpu_packed_latent import KINDS, MICRO, conds_of, engine, inputs, same_bits  # noqa: E402

VOICE = [2, 0, 1]
SCHEDULE = ([16, 0, 9], [0, 31, 0], [8, 0, 0], [1, 0, 0])


@pytest.mark.parametrize("kind", KINDS)
def test_uneven_appends_deliver_the_rows_of_the_packed_pass(kind):
    eng = engine(kind)
    texts, codes = inputs(MICRO)
    texts, codes = texts[:3], codes[:3]
    assert [len(t) for t in texts] == [40, 17, 30] and [len(c) for c in codes] == [25, 31, 9]
    assert [sum(s[b] for s in SCHEDULE) for b in range(3)] == [25, 31, 9]
    cond_all = torch.cat(conds_of(eng, 61), 0)
    want = [w.clone() for w in eng.latent_packed(cond_all, texts, codes, cond_index=VOICE)]
    done = [0, 0, 0]
    with eng.latent_stream(cond_all, texts, max_codes=31, cond_index=VOICE) as ls:
        for step in SCHEDULE:
            got = ls.append([codes[b][done[b]:done[b] + n] for b, n in enumerate(step)])
            for b, n in enumerate(step):
                assert got[b].shape == (1, n, eng.ccfg.model_dim)
                assert same_bits(got[b], want[b][:, done[b]:done[b] + n]), f"{kind}: sequence {b} rows {done[b]} .. {done[b] + n} differ from latent_packed"
                done[b] += n
    assert done == [25, 31, 9]


def test_appends_at_full_dims():
    eng = engine("bf16", CFG3)
    g = CFG3.gpt
    text = synth.text_ids(41, 50, g.number_text_tokens).astype(np.int32)
    codes = np.random.default_rng(60).integers(0, g.stop_mel_token, 25).astype(np.int32)
    cond = conds_of(eng, 511)[0]
    want = eng.latent_packed(cond, [text], [codes])[0].clone()
    lo = 0
    with eng.latent_stream(cond, [text], max_codes=25) as ls:
        for n in (17, 3, 5):
            got = ls.append([codes[lo:lo + n]])[0]
            assert same_bits(got, want[:, lo:lo + n]), f"rows {lo} .. {lo + n} differ from latent_packed"
            lo += n


@pytest.mark.parametrize("kind", KINDS)
def test_streamed_latent_against_the_reference(kind, gold):
    c, g = gold("micro_conditioning"), gold("micro_latent")
    eng = engine(kind)
    cond = torch.from_numpy(c["cond"])
    codes = np.asarray(g["codes"]).reshape(-1)
    half = len(codes) // 2
    with eng.latent_stream(cond, [g["text"]], max_codes=len(codes)) as ls:
        lat = torch.cat([ls.append([codes[:half]])[0], ls.append([codes[half:]])[0]], 1)
    err = relerr(lat, g["latent"]) if kind == "fp32" else rms_rel(lat, g["latent"])
    print(f"{kind} latent_stream in two appends: {'relerr' if kind == 'fp32' else 'rms_rel'} {err:.3e}")
    assert err < (1e-4 if kind == "fp32" else 3e-2), (kind, err)


def test_refusals():
    eng = engine("fp32")
    texts, codes = inputs(MICRO)
    cond = conds_of(eng, 61)[0]
    one = np.zeros(1, dtype=np.int32)
    out = torch.empty(4, eng.ccfg.model_dim, device=eng.device)

    def raw_append(c, n):
        c, n = np.asarray(c, dtype=np.int32), np.asarray(n, dtype=np.int32)
        return eng.lib.itts_gpt_latent_stream_append(eng.h, c.ctypes.data, n.ctypes.data, out.data_ptr(), eng._s())

    assert raw_append(one, [1]) == -1 and eng.lib.itts_last_error().decode().startswith("itts_gpt_latent_stream_append: no open stream")
    with eng.latent_stream(cond, texts[:1], max_codes=4) as ls:
        with pytest.raises(RuntimeError, match="itts_gpt_latent_stream_open: a stream is already open"):
            eng.latent_stream(cond, texts[:1], max_codes=4)
        with pytest.raises(RuntimeError, match="itts_gpt_latent_stream_append: mel code out of range"):
            ls.append([[MICRO.gpt.number_mel_codes]])
        with pytest.raises(RuntimeError, match="itts_gpt_latent_stream_append: mel code out of range"):
            ls.append([[-1]])
        assert ls.append([codes[0][:3]])[0].shape[1] == 3
        with pytest.raises(RuntimeError, match="itts_gpt_latent_stream_append: append past max_codes"):
            ls.append([codes[0][3:5]])
        assert ls.append([codes[0][3:4]])[0].shape[1] == 1  # a refused call took nothing
    assert raw_append(one, [1]) == -1 and eng.lib.itts_last_error().decode().startswith("itts_gpt_latent_stream_append: no open stream")
    with pytest.raises(RuntimeError, match="itts_gpt_latent_stream_open: max_codes"):
        eng.latent_stream(cond, texts[:1], max_codes=0)
    with eng.latent_stream(cond, texts[:1], max_codes=4):  # ... and a stream opens again after a close and after a refused open
        pass


def test_a_generation_after_a_closed_stream_is_what_it_was():
    eng = engine("bf16")
    texts, codes = inputs(MICRO)
    cond = conds_of(eng, 61)[0]
    text = texts[1][None]
    before = eng.generate(cond, text, 24)
    mode = eng.decode_mode()
    with eng.latent_stream(cond, texts[:2], max_codes=31) as ls:
        ls.append([codes[0], codes[1]])
    after = eng.generate(cond, text, 24)
    assert eng.decode_mode() == mode
    assert np.array_equal(before, after)
