"""No GPU: the whole-vocabulary sampler's acceptance predicate (wide_sampler_ref.py) accepts an fp32 emulation of the
kernel's documented summation structure and rejects broken samplers; Engine.generate routes `wide_sampler`; the public surface
(header, library, ctypes table, command line) agrees."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_sampler_ref as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(n, V, seed, quant=False):
    rng = np.random.default_rng(seed)
    for i in range(n):
        lg = (rng.standard_normal(V) * rng.uniform(1.0, 4.0)).astype(np.float32)
        if quant:
            lg = (np.round(lg * 4) / 4).astype(np.float32)
        yield lg, (0.8, 0.95, 1.0)[i % 3], (1.0, 0.3)[(i // 3) % 2], np.float32(rng.random(dtype=np.float32))


def test_predicate_accepts_the_emulated_kernel_at_model_size():
    """V = 8194, logit std 1 .. 4, top_p 0.8 / 0.95 / 1, temperature 1 / 0.3: no violation.  (The issue's own run of 2000 rows
    found none either and the fp64 pick in all 2000; 240 rows keep this test at a few seconds.)"""
    exact = total = 0
    for lg, top_p, temp, u in _rows(240, 8194, 1):
        s = W.sampler_scores(lg, temperature=temp)
        tok, kept = W.emulate(s, 0, top_p, u)
        assert W.Ref(s, 0, top_p).accepts(tok, u, kept), (total, tok, kept)
        exact += (tok, kept) == W.pick_fp64(s, 0, top_p, u)
        total += 1
    print(f"emulated kernel == plain fp64 sampler in {exact} of {total} rows")


@pytest.mark.parametrize("V", [129, 1024, 1025])
@pytest.mark.parametrize("top_k", [0, 129, 2000])
def test_predicate_accepts_the_emulated_kernel_small(V, top_k):
    for quant in (False, True):
        for lg, top_p, temp, u in _rows(30, V, 7 + V, quant):
            for uu in (u, np.float32(0.0), np.nextafter(np.float32(1), np.float32(0))):
                s = W.sampler_scores(lg, temperature=temp)
                tok, kept = W.emulate(s, top_k, top_p, uu)
                assert W.Ref(s, top_k, top_p).accepts(tok, uu, kept)
                assert W.Ref(s, top_k, top_p).accepts(tok, uu)


def test_predicate_on_rows_with_few_finite_scores_and_tiny_top_p():
    rng = np.random.default_rng(3)
    s = np.full(1025, -np.inf, dtype=np.float32)
    s[rng.choice(1025, 40, replace=False)] = rng.standard_normal(40).astype(np.float32)
    for top_k in (0, 129, 1030):
        tok, kept = W.emulate(s, top_k, 1.0, 0.5)
        assert kept == 40 and np.isfinite(s[tok]) and W.Ref(s, top_k, 1.0).accepts(tok, 0.5, kept)
    tok, kept = W.emulate(s, 0, 1e-6, 0.99)
    assert kept == 1 and tok == int(np.argmax(s)) and W.Ref(s, 0, 1e-6).accepts(tok, 0.99, kept)


def test_predicate_rejects_wrong_samplers():
    """Rank off by one, kept count off by one, the inclusive descending cumsum as the nucleus (V = 1025, logit std 2.5: a single
    token at the boundary weighs ~1e-3 of the mass, far above delta, so every row must be rejected), and ties in descending-id
    order (logits quantised to 0.25: rejected wherever the draw lands inside a group of equal scores)."""
    rng = np.random.default_rng(11)
    n = 40
    tie_rejected = cut_rejected = 0
    for i in range(n):
        lg = (rng.standard_normal(1025) * 2.5).astype(np.float32)
        u = np.float32(rng.uniform(0.05, 0.95))
        for top_p in (0.8, 1.0):
            ref = W.Ref(lg, 0, top_p)
            good = W.emulate(lg, 0, top_p, u)
            assert ref.accepts(*good[:1], u, good[1])
            tok, kept = W.emulate(lg, 0, top_p, u, wrong="rank+1")
            assert not ref.accepts(tok, u, kept) and not ref.accepts(tok, u)
            tok, kept = W.emulate(lg, 0, top_p, u, wrong="kept+1")
            assert not ref.accepts(tok, u, kept)
        good = W.emulate(lg, 0, 0.8, u)
        tok, kept = W.emulate(lg, 0, 0.8, u, wrong="desc_cumsum")
        if good[1] >= 2:  # (a best token that outweighs top_p alone is the whole nucleus either way)
            cut_rejected += 1
            assert kept == good[1] - 1 and not W.Ref(lg, 0, 0.8).accepts(tok, u, kept)
        q = (np.round(lg * 4) / 4).astype(np.float32)
        refq = W.Ref(q, 0, 1.0)
        tok, kept = W.emulate(q, 0, 1.0, u)
        assert refq.accepts(tok, u, kept)
        tok, kept = W.emulate(q, 0, 1.0, u, wrong="ties_desc")
        tie_rejected += not refq.accepts(tok, u, kept)
    assert cut_rejected >= n // 2, cut_rejected
    assert tie_rejected >= n // 2, tie_rejected  # ~1025 scores on ~80 levels: most draws land inside a tie group


# ---- Engine.generate routing (no library, no GPU) ----
class _Routed(Exception):
    pass


def _stub_engine(calls):
    from itts_hip import engine as ieng

    class Stub(ieng.Engine):
        def __init__(self):  # no library, no device
            class Cfg:
                stop_mel_token = 7
            self.ccfg = Cfg()

        def _generate_host_sampled(self, *a, **k):
            calls.append("host_sampled")
            return np.zeros((1, 1), dtype=np.int64)

        def _generate_host_beams(self, *a, **k):
            calls.append("host_beams")
            return np.zeros((1, 1), dtype=np.int64)

        def set_sampling(self, do_sample, top_k=30, *a, **k):
            if do_sample:
                calls.append(("device", top_k))
                raise _Routed()

        def __del__(self):
            pass

    return Stub()


def test_generate_routes_wide_sampler(monkeypatch):
    monkeypatch.delenv("ITTS_WIDE_SAMPLER", raising=False)
    calls = []
    eng = _stub_engine(calls)
    text = np.zeros((1, 4), dtype=np.int32)
    kw = dict(do_sample=True, top_p=0.8)
    eng.generate(None, text, 4, top_k=0, **kw)
    eng.generate(None, text, 4, top_k=200, wide_sampler="host", **kw)
    assert calls == ["host_sampled", "host_sampled"]
    for top_k, want in ((0, 0), (None, 0), (200, 200)):
        calls.clear()
        with pytest.raises(_Routed):
            eng.generate(None, text, 4, top_k=top_k, wide_sampler="device", **kw)
        assert calls == [("device", want)]
    calls.clear()
    eng.generate(None, text, 4, top_k=0, num_beams=3, wide_sampler="device", **kw)  # beams ignore it
    assert calls == ["host_beams"]
    calls.clear()
    monkeypatch.setenv("ITTS_WIDE_SAMPLER", "device")
    with pytest.raises(_Routed):
        eng.generate(None, text, 4, top_k=0, **kw)
    eng.generate(None, text, 4, top_k=0, wide_sampler="host", **kw)  # the keyword wins over the environment
    assert calls == [("device", 0), "host_sampled"]
    with pytest.raises(ValueError):
        eng.generate(None, text, 4, top_k=0, wide_sampler="gpu", **kw)


def test_wide_sampler_public_surface():
    from itts_hip import lib

    assert "itts_sample_rows" in lib.exported_symbols()
    for half in ("bf16", "f16"):
        assert callable(getattr(lib.load(half), "itts_sample_rows"))
    assert lib.load().itts_abi_version() == 4  # an addition: the ABI version stays
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        assert re.search(r"\bint\s+itts_sample_rows\s*\(", f.read())

    from itts_hip import engine as ieng

    assert inspect.signature(ieng.Engine.generate).parameters["wide_sampler"].default is None

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["wide_sampler"].default is None

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav", "--wide-sampler", "device"]).wide_sampler == "device"
    assert p.parse_args(["hello", "-v", "voice.wav"]).wide_sampler is None
