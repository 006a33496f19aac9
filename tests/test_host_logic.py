"""CPU: host-side product logic (no GPU): silence clean-up known answers from the reference, bucketing, the
C-ABI library loads and exports every declared symbol, packer round trips."""
import os
import re

import numpy as np
import pytest

from itts_hip import config as icfg
from itts_hip import infer_core, lib, pack, prng, synth


def test_remove_long_silence_known_answers(gold):
    g = gold("silence_cases")
    for i in range(int(g["n"])):
        oc, ol = infer_core.remove_long_silence(g[f"in{i}"], int(g["stop"]))
        assert np.array_equal(oc, g[f"out{i}"]), i
        assert np.array_equal(ol, g[f"len{i}"]), i


def test_remove_long_silence_edges():
    S = 65
    c, n = infer_core.remove_long_silence(np.array([[S, S, S]]), S)
    assert c.shape == (1, 0) and n.tolist() == [0]
    row = [52] * 100
    c, n = infer_core.remove_long_silence(np.array([row]), S)
    assert n.tolist() == [10] and c.shape == (1, 10)
    row = ([52] * 15 + [7]) * 3
    c, n = infer_core.remove_long_silence(np.array([row]), S)
    assert n.tolist() == [33] and (c[0] == 7).sum() == 3


def test_bucket_sentences():
    sents = [[0] * n for n in (5, 3, 9, 1, 7)]
    one = infer_core.bucket_sentences(sents, 8)
    assert len(one) == 1 and [x["idx"] for x in one[0]] == [0, 1, 2, 3, 4]
    b = infer_core.bucket_sentences(sents, 2)
    assert [[x["len"] for x in bk] for bk in b] == [[1, 3], [5, 7], [9]]
    p = infer_core.pad_tokens_cat([np.array([4, 5, 6]), np.array([7])], 1)
    assert p.tolist() == [[4, 5, 6], [7, 1, 1]]


def test_library_loads_and_exports_header_symbols():
    l = lib.load()
    assert l.itts_abi_version() == 4
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "itts_hip.h")).read()
    declared = set(re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(l, name), f"{name} declared in include/itts_hip.h but not exported"
    assert declared == set(lib.exported_symbols())


def test_prng_is_stable():
    x = prng.tensor("unit/test", 7, (5,), std=1.0)
    assert np.allclose(x, prng.tensor("unit/test", 7, (5,), std=1.0))
    # pinned values: the fixtures under tests/golden depend on this exact stream
    ref = np.array([-0.9305234, -0.584689, 0.28166455, -0.520244, 0.06148376], dtype=np.float32)
    assert np.allclose(x, ref, atol=1e-6), x
    r = prng.randint("unit/int", 3, 6, 2, 10)
    assert r.min() >= 2 and r.max() < 10


def test_pack_layouts():
    w = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)  # [Cout, Cin, k]
    p = pack.conv_w(w)
    assert p.shape == (2, 12) and p[1, 2 * 3 + 1] == w[1, 1, 2]
    wt = np.arange(3 * 2 * 8, dtype=np.float32).reshape(3, 2, 8)  # [Cin, Cout, k], u=4, p=2
    q = pack.convT_w(wt, 4, 2)
    assert q.shape == (4, 2, 6)
    # phase 2: (2+2)%4 = 0 -> kernel taps 0 and 4
    assert q[2, 1, 0 * 3 + 2] == wt[2, 1, 0] and q[2, 1, 1 * 3 + 2] == wt[2, 1, 4]
    v = np.random.RandomState(0).randn(4, 3, 5).astype(np.float32)
    g = np.random.RandomState(1).rand(4, 1, 1).astype(np.float32) + 0.5
    f = pack._fold_weight_norm({"c.weight_g": g, "c.weight_v": v})
    assert np.allclose(np.sqrt((f["c.weight"] ** 2).sum(axis=(1, 2))), g[:, 0, 0], rtol=1e-5)


def test_packed_micro_matches_engine_contract():
    cfg = icfg.micro()
    P = pack.pack_gpt(synth.gpt_state_dict(cfg, 1), cfg)
    D = cfg.gpt.model_dim
    assert P["gpt.h.0.attn.c_attn.weight"][1].shape == (3 * D, D)
    assert P["perc.0.ff2.weight"][1].shape[1] % 32 == 0
    B = pack.pack_bigvgan(synth.bigvgan_state_dict(cfg, 1), cfg)
    assert B["bv.ups.0.weight"][1].shape[0] == cfg.bigvgan.upsample_rates[0]
    assert B["bv.filter"][1].shape == (12,) and abs(float(B["bv.filter"][1].sum()) - 1) < 1e-6


def test_sinc_resampler_is_torchaudio_shaped():
    """The prompt resampler (infer.py:88 torchaudio.transforms.Resample defaults: Hann-windowed sinc, width 6, rolloff
    0.99), pinned analytically since torchaudio is absent: output length ceil(new * n / orig), unit DC gain, a tone well
    below both Nyquists comes out as the same tone, a tone above the new Nyquist is removed, same rate = identity."""
    import math

    import torch

    from indextts.utils.feature_extractors import resample, sinc_resample_kernel

    k, width = sinc_resample_kernel(2, 3)
    assert k.shape == (3, 1, 2 * width + 2) and k.dtype == torch.float32 and width == math.ceil(6 * 2 / (2 * 0.99))
    assert torch.allclose(k.sum(dim=(1, 2)), torch.ones(3), atol=2e-3)  # every phase has unit DC gain
    for sr, new in ((16000, 24000), (44100, 24000), (48000, 24000), (22050, 24000)):
        n = sr // 4 + 13
        t = torch.arange(n, dtype=torch.float64) / sr
        x = torch.sin(2 * math.pi * 440.0 * t).float()[None]
        y = resample(x, sr, new)
        assert y.shape == (1, math.ceil(new * n / sr))
        tt = torch.arange(y.shape[1], dtype=torch.float64) / new
        want = torch.sin(2 * math.pi * 440.0 * tt).float()
        m = slice(200, y.shape[1] - 200)
        assert float((y[0, m] - want[m]).abs().max()) < 2e-3, (sr, new)
        dc = resample(torch.ones(1, n), sr, new)
        assert float((dc[0, m] - 1).abs().max()) < 2e-3
    hi = torch.sin(2 * math.pi * 15000.0 * torch.arange(48000, dtype=torch.float64) / 48000).float()[None]
    assert float(resample(hi, 48000, 24000)[0, 300:-300].abs().max()) < 1e-2  # above the 12 kHz Nyquist: gone
    x = torch.randn(2, 1000)
    assert resample(x, 24000, 24000) is x


def test_mel_front_end_shapes_and_bank():
    """MelSpectrogramFeatures (feature_extractors.py:24-50): 511 frames for the 130 560-sample prompt of SURVEY 8 (center
    padding: 1 + n // hop), HTK triangular bank with unit peaks that covers 0..12 kHz, log clip at 1e-7."""
    import math

    import torch

    from indextts.utils.feature_extractors import MelSpectrogramFeatures, mel_filterbank

    fe = MelSpectrogramFeatures()
    mel = fe(torch.zeros(1, 130560))
    assert mel.shape == (1, 100, 511) and torch.allclose(mel, torch.full_like(mel, math.log(1e-7)))
    fb = mel_filterbank(513, 0.0, 12000.0, 100, 24000)
    assert fb.shape == (513, 100) and float(fb.min()) >= 0.0 and float(fb.max()) <= 1.0 + 1e-6
    peaks = fb.argmax(0)
    assert bool((peaks[1:] > peaks[:-1]).all())  # centre frequencies increase
    tone = torch.sin(2 * math.pi * 3000.0 * torch.arange(24000) / 24000)[None]
    m = fe(tone)[0, :, 20]
    f_pts = 700.0 * (10.0 ** (torch.linspace(0, 2595.0 * math.log10(1 + 12000.0 / 700.0), 102) / 2595.0) - 1.0)
    assert abs(float(f_pts[1 + int(m.argmax())]) - 3000.0) < 150.0  # the loudest band sits on the tone


def test_bench_dump_outputs_within_and_beyond_the_budget(tmp_path):
    """bench.py --dump-outputs: every sample while the waveforms fit in 64 MB, a fixed seeded sample (values + positions,
    the same on every call) beyond it."""
    import bench

    small = [np.arange(-5, 5, dtype=np.int16), np.full(3, 7, np.int16)]
    bench.dump_outputs(str(tmp_path / "a"), small)
    assert np.load(tmp_path / "a" / "wav.npy").tolist() == list(range(-5, 5)) + [7, 7, 7]
    assert np.load(tmp_path / "a" / "wav_lengths.npy").tolist() == [10.0, 3.0] and not (tmp_path / "a" / "wav_index.npy").exists()
    rng = np.random.default_rng(1)
    big = [rng.integers(-32767, 32768, 9 * 2 ** 20, dtype=np.int16) for _ in range(2)]
    flat = np.concatenate(big)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    files = [tmp_path / "b" / f for f in ("wav.npy", "wav_index.npy", "wav_lengths.npy")]
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_BUDGET_BYTES == 64 * 10 ** 6
    wav, idx = np.load(files[0]), np.load(files[1])
    assert wav.dtype == np.float32 and idx.dtype == np.float64 and wav.shape == idx.shape == (bench.DUMP_SAMPLE,)
    assert np.all(np.diff(idx) > 0) and np.array_equal(wav, flat[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "c" / "wav_index.npy"))
