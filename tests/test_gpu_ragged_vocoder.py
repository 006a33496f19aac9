"""GPU: the vocoder over a padded ragged batch (itts_bigvgan_ragged / Engine.bigvgan_ragged / bigvgan_grouped(ragged=True) /
IndexTTS(ragged_vocoder=True)): latents of unequal length share one BigVGAN pass and every row is the waveform of its latent alone.

  * micro generator, fp32 engine, rows of 5, 12, 1 and 9 frames with NaN behind each row's frames: every row against
    oracle.vocoder.bigvgan_generator on the row alone (tests/ragged_vocoder_ref.py) and against the engine's own batch-1 run, both at
    the fp32 waveform tolerance of tests/test_gpu_engine.py (relative RMS < 1e-4); the waveform behind a row's end is exactly zero
    and everything is finite;
  * bf16 and f16 engines: every row against its own batch-1 run within the bound the engine has against the reference - 6e-2 for
    bf16 (test_gpu_engine.py test_bigvgan_bf16), 4e-3 for f16 (the f16 engine's waveform bound, test_gpu_f16.py);
  * IndexTTS-1.5 dimensions, bf16, rows of 64, 40 and 7 frames cut from the `long_bigvgan` latent (the narrow stages take the fused
    ragged convolution, the short rows end inside its tiles): row 0 against the golden waveform, rows 1 and 2 against their batch-1
    runs, at the bf16 bound of tests/test_gpu_fullsize.py (< 4e-2).  The same comparison with ITTS_GEMM_KSPLIT=0 is printed and, where
    ITTS_TEST_OUT names a directory, written to ragged_vocoder_rows.txt there; it measured 0.0 for the 64- and 40-frame rows (asserted)
    and 1.7e-2 for the 7-frame row (not asserted beyond the bound);
  * what itts_bigvgan_ragged refuses on the host (an engine exists only on a device, so these are here and not in the CPU file);
  * bigvgan_grouped(ragged=True) returns the shapes and the order of ragged=False;
  * IndexTTS(ragged_vocoder=True).infer_batch over three sentences of different length matches the default."""
import ctypes as C
import inspect
import os
import warnings

import numpy as np
import pytest
import torch

import ragged_vocoder_ref as R
from itts_hip import config as icfg
from itts_hip import engine as ieng
from itts_hip import infer_core, prng, synth

MICRO = icfg.micro()
FULL = icfg.indextts_1_5()
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def record_file():
    yield
    out = os.environ.get("ITTS_TEST_OUT")
    if out and RECORD:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ragged_vocoder_rows.txt"), "w") as f:
            f.write("\n".join(f"{k}: {v}" for k, v in sorted(RECORD.items())) + "\n")


def ragged(eng, lat_padded, lens, spk):
    """itts_bigvgan_ragged on a caller-made padded batch (Engine.bigvgan_ragged packs zeros; the tests want NaN tails)"""
    lat = lat_padded.to(device=eng.device, dtype=eng.tdt).contiguous()
    B, T, _ = lat.shape
    spk = spk.to(device=eng.device, dtype=torch.float32).reshape(B, -1).contiguous()
    ln = np.asarray(lens, dtype=np.int32)
    out = torch.full((B, 1, T * eng.up_total), float("nan"), dtype=torch.float32, device=eng.device)
    eng._enter()
    eng._ck(eng.lib.itts_bigvgan_ragged(eng.h, lat.data_ptr(), spk.data_ptr(), B, T, ln.ctypes.data_as(C.c_void_p), out.data_ptr(),
                                        eng._s()), "bigvgan_ragged")
    eng._exit()
    torch.cuda.synchronize()
    return out.cpu()


def rows_alone(eng, lat, lens, spk):
    return [eng.bigvgan(lat[b:b + 1, :n], spk[b].reshape(1, -1)).float().cpu() for b, n in enumerate(lens)]


def check_rows(eng, lat_nan, lat, lens, spk, bound, tag, refs=None):
    wav = ragged(eng, lat_nan, lens, spk)
    up = eng.up_total
    assert bool(torch.isfinite(wav).all()), tag
    alone = rows_alone(eng, lat, lens, spk)
    for b, n in enumerate(lens):
        assert bool((wav[b, :, n * up:] == 0).all()), (tag, b, "waveform tail not zero")
        e = R.rel_rms(wav[b:b + 1, :, :n * up], alone[b])
        RECORD[f"{tag} row {b} ({n} frames) vs batch-1 rel rms"] = f"{e:.3e}"
        print(f"{tag} row {b} ({n} frames): ragged batch vs its batch-1 run, rel RMS {e:.3e}")
        assert e < bound, (tag, b, n, e)
        if refs is not None:
            e = R.rel_rms(wav[b:b + 1, :, :n * up], refs[b])
            print(f"{tag} row {b} ({n} frames): ragged batch vs the oracle on the row alone, rel RMS {e:.3e}")
            assert e < bound, (tag, b, n, e)
    return wav


@pytest.mark.gpu
def test_ragged_rows_fp32_vs_oracle_and_batch1():
    c = R.micro_case()
    eng = ieng.build_engine(MICRO, "fp32", parts=("bigvgan",))
    check_rows(eng, c["lat_nan"], c["lat"], c["lens"], c["spk"][:, 0], 1e-4, "micro fp32", refs=c["rows"])


@pytest.mark.gpu
@pytest.mark.parametrize("half,bound", (("bf16", 6e-2), ("f16", 4e-3)))
def test_ragged_rows_16bit_vs_batch1(half, bound):
    c = R.micro_case()
    eng = ieng.build_engine(MICRO, half, parts=("bigvgan",))
    check_rows(eng, c["lat_nan"], c["lat"], c["lens"], c["spk"][:, 0], bound, f"micro {half}")


@pytest.mark.gpu
def test_ragged_rows_full_dims_bf16(gold, monkeypatch):
    eng = ieng.build_engine(FULL, "bf16", parts=("bigvgan",))
    mel = torch.from_numpy(synth.prompt_mel(511, seed=7))
    spk1 = eng.ecapa(mel.transpose(1, 2)).float().cpu().reshape(1, -1)
    lens = (64, 40, 7)
    long = torch.from_numpy(prng.tensor("bigvgan.latent.long", 3, (1, 64, FULL.bigvgan.gpt_dim), std=1.0, mean=0.0))
    lat = long.expand(3, -1, -1).clone()
    lat_nan = lat.clone()
    for b, n in enumerate(lens):
        lat_nan[b, n:] = float("nan")
    spk = spk1.expand(3, -1).contiguous()
    for ks in (None, "0"):
        if ks is not None:
            monkeypatch.setenv("ITTS_GEMM_KSPLIT", ks)
        tag = "1.5 dims bf16" + ("" if ks is None else " ITTS_GEMM_KSPLIT=0")
        wav = check_rows(eng, lat_nan, lat, lens, spk, 4e-2, tag)
        if ks == "0":
            # without the K split the 64- and 40-frame rows measure 0.0 against their batch-1 runs (every kernel family sums K in one
            # order whatever T is); the 7-frame row does not (1.7e-2: alone, its few-tile GEMMs take other families than in the batch)
            for b in (0, 1):
                assert torch.equal(wav[b, :, :lens[b] * eng.up_total], rows_alone(eng, lat[b:b + 1], lens[b:b + 1], spk[b:b + 1])[0][0]), b
        e = R.rel_rms(wav[0:1].numpy()[0, 0], gold("long_bigvgan")["wav"])
        RECORD[f"{tag} row 0 (64 frames) vs golden rel rms"] = f"{e:.3e}"
        print(f"{tag} row 0 vs the golden waveform, rel RMS {e:.3e}")
        assert e < 4e-2, (tag, e)


@pytest.mark.gpu
def test_bigvgan_ragged_refusals_before_any_launch():
    eng = ieng.build_engine(MICRO, "fp32", parts=("bigvgan",), max_batch=4)
    lat = torch.zeros(2, 8, MICRO.bigvgan.gpt_dim, device=eng.device)
    spk = torch.zeros(2, MICRO.bigvgan.speaker_embedding_dim, device=eng.device)
    out = torch.zeros(2, 8 * eng.up_total, device=eng.device)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = np.asarray([8, 3], dtype=np.int32)

    def call(latp=lat.data_ptr(), spkp=spk.data_ptr(), B=2, T=8, lens=good, outp=out.data_ptr()):
        st = eng.lib.itts_bigvgan_ragged(eng.h, latp, spkp, B, T, None if lens is None else P(lens), outp, eng._s())
        return st, eng.lib.itts_last_error()

    for kw, word in ((dict(latp=None), b"null pointer"), (dict(spkp=None), b"null pointer"), (dict(lens=None), b"null pointer"),
                     (dict(outp=None), b"null pointer"), (dict(B=0), b"max_batch"), (dict(B=5, lens=np.ones(5, np.int32)), b"max_batch"),
                     (dict(T=0), b"T < 1"), (dict(lens=np.asarray([8, 0], np.int32)), b"length"),
                     (dict(lens=np.asarray([9, 3], np.int32)), b"length"), (dict(lens=np.asarray([-1, 3], np.int32)), b"length")):
        st, msg = call(**kw)
        assert st == -1 and msg.startswith(b"itts_bigvgan_ragged: ") and word in msg, (kw, st, msg)
    eng._enter()
    assert call()[0] == 0
    eng._exit()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_grouped_ragged_returns_the_shapes_and_order_of_the_default():
    eng = ieng.build_engine(MICRO, "bf16", parts=("bigvgan",), max_batch=4)
    lens = (5, 12, 1, 9, 12, 5, 11)
    lats = [torch.from_numpy(prng.tensor(f"ragged.grouped{i}", 3, (1, n, MICRO.bigvgan.gpt_dim), std=1.0)) for i, n in enumerate(lens)]
    spk = torch.from_numpy(prng.tensor("ragged.grouped.spk", 3, (1, MICRO.bigvgan.speaker_embedding_dim), std=1.0))
    calls = []
    plain_ragged = eng.bigvgan_ragged
    eng.bigvgan_ragged = lambda sub, s: calls.append(len(sub)) or plain_ragged(sub, s)
    default = eng.bigvgan_grouped(lats, spk)
    assert not calls
    for max_pad in (0.1, 0.25, 0.9):
        got = eng.bigvgan_grouped(lats, spk, ragged=True, max_pad=max_pad)
        assert len(got) == len(default)
        for i, (a, b) in enumerate(zip(got, default)):
            assert a.shape == b.shape == (1, 1, lens[i] * eng.up_total) and a.dtype == b.dtype
            assert R.rel_rms(a.float().cpu(), b.float().cpu()) < 6e-2, (max_pad, i)
    assert calls and max(calls) <= 4  # rows of unequal length did share passes, within max_batch
    calls.clear()
    same = eng.bigvgan_grouped(lats, spk, ragged=True, max_pad=0.0)  # no padding allowed: the equal-length groups, no ragged pass
    assert not calls and all(torch.equal(a, b) for a, b in zip(same, default))


@pytest.mark.gpu
def test_infer_batch_with_the_ragged_vocoder_matches_the_default(monkeypatch):
    from indextts.infer import IndexTTS

    sds = {"gpt": synth.gpt_state_dict(MICRO, 1234), "bigvgan": synth.bigvgan_state_dict(MICRO, 1234)}
    tts = IndexTTS(cfg=MICRO, model_dir="/nonexistent", is_fp16=False, state_dicts=sds, ragged_vocoder=True)
    monkeypatch.delenv("ITTS_RAGGED_VOCODER", raising=False)
    mel = torch.from_numpy(synth.prompt_mel(61, seed=7)).cuda()
    utts = [[synth.text_ids(5 + 3 * i, 300 + i, MICRO.gpt.number_text_tokens).astype(np.int32)] for i in range(3)]
    # three sentences whose latents differ in length whatever the random model generates: sentence i loses its last i frames
    latents = tts._clean_and_latents
    seen = []

    def cut(*a, **kw):
        lats = [l[:, :l.shape[1] - i] for i, l in enumerate(latents(*a, **kw))]
        seen.append([int(l.shape[1]) for l in lats])
        return lats

    monkeypatch.setattr(tts, "_clean_and_latents", cut)
    passes = []
    plain_ragged = tts.engine.bigvgan_ragged
    monkeypatch.setattr(tts.engine, "bigvgan_ragged", lambda sub, s: passes.append(len(sub)) or plain_ragged(sub, s))
    kw = dict(max_mel_tokens=12, do_sample=False, num_beams=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        on = tts.infer_batch(mel, utts, **kw)
        assert len(set(seen[-1])) == 3, seen
        max_pad = inspect.signature(tts.engine.bigvgan_grouped).parameters["max_pad"].default
        groups = infer_core.ragged_groups(seen[-1], max_pad, tts.engine.ccfg.max_batch)
        shared = [len(g) for g in groups if len(g) > 1]
        assert shared and passes == shared, (passes, groups, seen)  # sentences of unequal length did share a pass
        monkeypatch.setenv("ITTS_RAGGED_VOCODER", "0")  # the environment overrides the setter
        off = tts.infer_batch(mel, utts, **kw)
        assert passes == shared and seen[-1] == seen[0]
    for (sa, a), (sb, b) in zip(on, off):
        assert sa == sb == 24000 and a.shape == b.shape and a.dtype == np.int16
        # the fp32 waveform tolerance, plus the one step by which the cast to int16 may turn any difference of two floats
        d, ref = a.astype(np.float64) - b.astype(np.float64), b.astype(np.float64)
        print(f"infer_batch ragged vs default: rms diff {np.sqrt((d ** 2).mean()):.3f} steps, signal rms {np.sqrt((ref ** 2).mean()):.1f}")
        assert np.abs(d).max() <= 1 + 1e-4 * np.abs(ref).max() and np.sqrt((d ** 2).mean()) <= 1e-4 * np.sqrt((ref ** 2).mean()) + 1.0
