"""No GPU: the packed vocoder's algorithm, gap rule, planner, public surface, host-side refusals, switch and pinned conv selector.

tests/packed_vocoder_ref.py states the BigVGAN pass over sentences back to back in ONE item on CPU tensors.  On the micro generator
(up-rates 4 4 4 4 2 2, three AMP kernels x three dilations), sentences of 5, 12, 1 and 9 frames of two voices, gaps filled with NaN
in the latent, every sentence has to be the waveform oracle.vocoder.bigvgan_generator gives for it alone - relative RMS < 1e-5, the
bar of tests/test_ragged_vocoder_host.py (fp32 reordering only) - and its gap zero.  The same pack with gap = 0, the plain
concatenation, has to be OUTSIDE that bar for at least one sentence: a test that a wrong model passes shows nothing.

The refusals run on host memory with no device: a HIP call would answer ITTS_E_HIP or touch host pointers as device memory."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import packed_vocoder_ref as PR
import test_act_conv_api as A
from itts_hip import config as icfg
from itts_hip import engine as ieng
from itts_hip import infer_core
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = ("bf16", "f16")
P = A.P  # aligned host memory: never read, every call below is refused first
E_INVALID = -1
BAR = 1e-5  # tests/test_ragged_vocoder_host.py


def _gap_of(cfg):
    h = cfg.bigvgan
    return infer_core.packed_vocoder_gap(h.upsample_rates, h.upsample_kernel_sizes, h.resblock_kernel_sizes, h.resblock_dilation_sizes)


# ---- the algorithm ------------------------------------------------------------------------------------------------------------
def _packed_errors(gap):
    c = PR.micro_case()
    h = c["cfg"].bigvgan
    up = int(np.prod(h.upsample_rates))
    off = PR.offsets(c["lens"], gap)
    lat = PR.pack(c["lats"], off, fill=float("nan"))  # the gaps of the caller's latent are not read as signal
    spk = torch.cat([c["spk"][v:v + 1] for v in c["voices"]], 0)
    wav = PR.bigvgan_generator_packed(lat, off, c["lens"], spk, c["w"], h)
    assert wav.shape == (1, 1, off[-1] * up) and bool(torch.isfinite(wav).all())
    errs = []
    for b, n in enumerate(c["lens"]):
        lo = off[b] * up
        errs.append(PR.rel_rms(wav[:, :, lo:lo + n * up], c["rows"][b]))
        assert bool((wav[:, :, lo + n * up:off[b + 1] * up] == 0).all()), (b, "gap of the waveform")
    return errs


def test_packed_sentences_equal_every_sentence_alone():
    gap = _gap_of(icfg.micro())
    for b, e in enumerate(_packed_errors(gap)):
        print(f"sentence {b} ({PR.LENS[b]} frames, voice {PR.VOICES[b]}): packed with gap {gap} vs alone, rel RMS {e:.2e}")
        assert e < BAR, (b, e)


def test_plain_concatenation_is_told_apart():
    errs = _packed_errors(0)
    for b, e in enumerate(errs):
        print(f"sentence {b} ({PR.LENS[b]} frames): plain concatenation (gap 0) vs alone, rel RMS {e:.2e}")
    assert max(errs) > BAR, errs


# ---- the gap rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("micro", "indextts_1_5"))
def test_gap_rule(name):
    """Both configs share the generator's geometry: conv_pre reaches 3 frames; ups[i] one input row (k = 2u: two polyphase taps, shifts 0
    and 1); the widest AMP conv, k = 11 with dilation 5, reaches (55 - 5) / 2 = 25 rows, at stage 0 (4 rows a frame) 7 frames, at
    stage 1 (16 rows) 2; conv_post 3 rows of 1024 a frame.  The C++ rule, which checks every call again, answers the same."""
    cfg = getattr(icfg, name)()
    h = cfg.bigvgan
    assert list(h.upsample_rates) == [4, 4, 4, 4, 2, 2] and list(h.resblock_kernel_sizes) == [3, 7, 11]
    assert _gap_of(cfg) == 7
    for half in HALVES:
        cc = ieng.make_config(cfg, L.BF16)
        assert L.load(half).itts_bigvgan_packed_gap(C.byref(cc)) == 7
    # the pieces: one stage at rate 1 sees the whole reach; a narrower kernel set lowers it; k = u has no overlap at all
    assert infer_core.packed_vocoder_gap([1], [1], [11], [[1, 3, 5]]) == 25
    assert infer_core.packed_vocoder_gap([4], [8], [3], [[1]]) == 3
    assert infer_core.packed_vocoder_gap([8, 8], [16, 16], [3], [[1, 3, 5]]) == 3


# ---- the planner ----------------------------------------------------------------------------------------------------------------
def _length_sets():
    rng = np.random.RandomState(9)
    yield [7]
    yield [5, 12, 1, 9]
    yield [3] * 9
    yield [600, 1, 600]
    for n in (2, 13, 64, 130, 300):
        yield [int(v) for v in rng.randint(1, 600, size=n)]


@pytest.mark.parametrize("gap,max_frames", [(0, 1), (7, 64), (7, 700), (3, 2000), (7, infer_core.PACKED_VOCODER_MAX_FRAMES)])
def test_planner_properties(gap, max_frames):
    for lengths in _length_sets():
        before = list(lengths)
        chunks, offsets, frames = infer_core.packed_vocoder_plan(lengths, gap, max_frames)
        assert lengths == before  # pure
        assert [i for ch in chunks for i in ch] == list(range(len(lengths)))  # order-preserving, every sentence once
        assert len(chunks) == len(offsets) == len(frames)
        for ch, off, tot in zip(chunks, offsets, frames):
            assert 1 <= len(ch) <= infer_core.PACKED_VOCODER_MAX_SEQ and len(off) == len(ch) + 1 and off[0] == 0 and tot == off[-1]
            for j, i in enumerate(ch):
                assert off[j + 1] > off[j] and off[j + 1] - off[j] >= lengths[i] + gap  # increasing, capacity >= len + gap
                assert off[j + 1] - off[j] == lengths[i] + gap                           # ... and no frame more than that
            assert tot <= max_frames or len(ch) == 1  # the budget; an oversize sentence is alone
        # greedy: the sentence that opened the next chunk did not fit the one before it
        for ch, tot, nxt in zip(chunks, frames, chunks[1:]):
            assert len(ch) == infer_core.PACKED_VOCODER_MAX_SEQ or tot + lengths[nxt[0]] + gap > max_frames


def test_planner_edges():
    assert infer_core.packed_vocoder_plan([], 7) == ([], [], [])
    assert infer_core.packed_vocoder_plan([5, 12, 1, 9], 7) == ([[0, 1, 2, 3]], [[0, 12, 31, 39, 55]], [55])
    assert infer_core.packed_vocoder_plan([5, 12, 1, 9], 7, 31) == ([[0, 1], [2, 3]], [[0, 12, 31], [0, 8, 24]], [31, 24])
    assert infer_core.packed_vocoder_plan([5, 100, 5], 7, 50)[0] == [[0], [1], [2]]  # the oversize sentence alone
    assert [len(c) for c in infer_core.packed_vocoder_plan([1] * 300, 7)[0]] == [128, 128, 44]
    for bad in (dict(gap=-1), dict(max_frames=0), dict(max_seqs=0)):
        with pytest.raises(ValueError):
            infer_core.packed_vocoder_plan([3, 4], **dict(dict(gap=7), **bad))
    with pytest.raises(ValueError):
        infer_core.packed_vocoder_plan([3, 0], 7)


# ---- surface ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    tab = r"\s*const\s+int32_t\s*\*\s*off_host\s*,\s*const\s+int32_t\s*\*\s*lens_host\s*,\s*int\s+n\s*,"
    assert re.search(r"\bint\s+itts_bigvgan_packed\s*\(\s*itts_engine\s*\*\s*e\s*,\s*const\s+void\s*\*\s*latent\s*,\s*const\s+float\s*\*\s*spk\s*," + tab +
                     r"\s*float\s*\*\s*wav_out\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_snake_aa_fwd_seg\s*\(\s*void\s*\*\s*dst\s*,\s*const\s+void\s*\*\s*src\s*,\s*const\s+float\s*\*\s*up12\s*,"
                     r"\s*const\s+float\s*\*\s*down12\s*,\s*const\s+float\s*\*\s*log_alpha\s*,\s*const\s+float\s*\*\s*log_beta\s*,\s*int\s+C\s*," + tab +
                     r"\s*int\s+mul\s*,\s*int\s+dtype\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_act_conv_seg\s*\(\s*const\s+itts_gemm_args\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*log_alpha\s*,\s*const\s+float"
                     r"\s*\*\s*log_beta\s*,\s*const\s+float\s*\*\s*filt12\s*," + tab + r"\s*int\s+mul\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_seg_bias_mask\s*\(\s*void\s*\*\s*x\s*,\s*const\s+float\s*\*\s*bias\s*,\s*int\s+C\s*," + tab +
                     r"\s*int\s+mul\s*,\s*int\s+dtype\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    for word in ("offsets not increasing", "a length < 1", "gap too small", "n outside [1, 128]", "null engine / pointers"):
        assert word in h, word  # the list of refusals is part of the header
    for name, nargs in (("itts_bigvgan_packed", 8), ("itts_bigvgan_packed_check", 7), ("itts_bigvgan_packed_gap", 1),
                        ("itts_snake_aa_fwd_seg", 13), ("itts_act_conv_seg", 9), ("itts_seg_bias_mask", 9), ("itts_gemm_which_pinned_conv", 1)):
        assert name in L.exported_symbols()
        for half in HALVES:
            fn = getattr(L.load(half), name)
            assert callable(fn) and len(fn.argtypes) == nargs and fn.restype is L.i32
    for half in HALVES:
        assert L.load(half).itts_abi_version() == 4  # additions: the ABI version stays


def test_python_surface_and_switch_precedence(monkeypatch):
    sig = inspect.signature(ieng.Engine.bigvgan_packed).parameters
    assert list(sig) == ["self", "lats", "spk", "max_frames"] and sig["max_frames"].default is None
    assert list(inspect.signature(infer_core.packed_vocoder_plan).parameters)[:3] == ["lengths", "gap", "max_frames"]
    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["packed_vocoder"].default is False
    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav"]).packed_vocoder is False
    assert p.parse_args(["hello", "-v", "voice.wav", "--packed-vocoder"]).packed_vocoder is True
    # the environment overrides the setter in both directions; unset or anything else leaves it
    monkeypatch.delenv("ITTS_PACKED_VOCODER", raising=False)
    assert infer_core.env_switch("ITTS_PACKED_VOCODER", True) is True and infer_core.env_switch("ITTS_PACKED_VOCODER", False) is False
    monkeypatch.setenv("ITTS_PACKED_VOCODER", "0")
    assert infer_core.env_switch("ITTS_PACKED_VOCODER", True) is False
    monkeypatch.setenv("ITTS_PACKED_VOCODER", "1")
    assert infer_core.env_switch("ITTS_PACKED_VOCODER", False) is True
    monkeypatch.setenv("ITTS_PACKED_VOCODER", "yes")
    assert infer_core.env_switch("ITTS_PACKED_VOCODER", False) is False
    src = inspect.getsource(IndexTTS)
    assert src.count('env_switch("ITTS_PACKED_VOCODER", self.packed_vocoder)') == 2  # both paths of infer_batch, nowhere else


# ---- refusals, all on host memory ---------------------------------------------------------------------------------------------------
def refused(lib, status, entry):
    msg = lib.itts_last_error()
    assert status == E_INVALID and msg.startswith(entry.encode() + b": "), (entry, status, msg)
    return msg


def _ints(v):
    return None if v is None else np.asarray(v, dtype=np.int32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


BAD_TABLES = (  # (off, lens, the word of the refusal) for mul = 1 and a required gap of 0
    (None, [5, 3], b"null pointer"), ([0, 5, 8], None, b"null pointer"),
    ([0, 5, 5], [5, 1], b"offsets not increasing"), ([0, 5, 3], [5, 1], b"offsets not increasing"),
    ([0, 5, 8], [0, 3], b"a length < 1"), ([0, 5, 8], [5, -1], b"a length < 1"),
    ([0, 5, 8], [6, 3], b"gap too small"), ([-1, 5, 8], [5, 3], b"off[0] < 0"))


@pytest.mark.parametrize("half", HALVES)
def test_segment_operators_refuse_on_the_host(half, monkeypatch):
    lib = L.load(half)
    for env in ("ITTS_NO_CONV_LDS", "ITTS_NO_CONV_ACT"):
        monkeypatch.delenv(env, raising=False)
    good_off, good_len = [0, 12, 31], [5, 12]
    ok = dict(dst=P, src=P, up12=P, down12=P, la=P, lb=P, C=24, off=good_off, lens=good_len, n=2, mul=4, dtype=L.BF16)

    def snake(**kw):
        a = dict(ok, **kw)
        o, l = _ints(a["off"]), _ints(a["lens"])
        return lib.itts_snake_aa_fwd_seg(a["dst"], a["src"], a["up12"], a["down12"], a["la"], a["lb"], a["C"], _ptr(o), _ptr(l), a["n"],
                                         a["mul"], a["dtype"], None)

    def mask(**kw):
        a = dict(ok, **kw)
        o, l = _ints(a["off"]), _ints(a["lens"])
        return lib.itts_seg_bias_mask(a["dst"], a["src"], a["C"], _ptr(o), _ptr(l), a["n"], a["mul"], a["dtype"], None)

    def conv(la=P, lb=P, filt=P, off=good_off, lens=good_len, n=2, mul=4, **kw):
        g = A.block(**dict(dict(M=256, T=256, bias_bstride=0), **kw))
        o, l = _ints(off), _ints(lens)
        return lib.itts_act_conv_seg(C.byref(g), la, lb, filt, _ptr(o), _ptr(l), n, mul, None)

    for name, call in (("itts_snake_aa_fwd_seg", snake), ("itts_seg_bias_mask", mask), ("itts_act_conv_seg", conv)):
        for off, lens, word in BAD_TABLES:
            assert word in refused(lib, call(off=off, lens=lens), name), (name, off, lens)
        for n in (0, -1, 129):
            assert b"n outside [1, 128]" in refused(lib, call(n=n), name), (name, n)
        for mul in (0, -2):
            assert b"mul < 1" in refused(lib, call(mul=mul), name), (name, mul)
        assert b"2^31" in refused(lib, call(off=[0, 12, 1 << 30], mul=4), name), name
    for k in ("dst", "src", "up12", "down12", "la", "lb"):
        assert b"null pointer" in refused(lib, snake(**{k: None}), "itts_snake_aa_fwd_seg"), k
    assert b"C must be >= 1" in refused(lib, snake(C=0), "itts_snake_aa_fwd_seg")
    for bad in (L.FP8, 2, -1):
        assert b"dtype" in refused(lib, snake(dtype=bad), "itts_snake_aa_fwd_seg"), bad
    assert b"null pointer" in refused(lib, mask(dst=None), "itts_seg_bias_mask")
    assert b"C must be >= 1" in refused(lib, mask(C=0), "itts_seg_bias_mask")
    for bad in (L.F16, L.FP8, -1):
        assert b"dtype" in refused(lib, mask(dtype=bad), "itts_seg_bias_mask"), bad
    assert b"2^31 - 1 elements" in refused(lib, mask(off=[0, 1 << 20], lens=[5], n=1, mul=1024, C=96), "itts_seg_bias_mask")
    # itts_act_conv_seg: what itts_act_conv refuses, by the rule that does not look at the row count
    assert b"null args" in refused(lib, lib.itts_act_conv_seg(None, P, P, P, P, P, 1, 1, None), "itts_act_conv_seg")
    for k in ("A", "W", "C"):
        assert b"null pointer" in refused(lib, conv(**{k: None}), "itts_act_conv_seg")
    for k in ("la", "lb", "filt"):
        assert b"null pointer" in refused(lib, conv(**{k: None}), "itts_act_conv_seg")
    assert b"force_simple" in refused(lib, conv(force_simple=1), "itts_act_conv_seg")
    for k in ("dtype_a", "dtype_w", "dtype_c"):
        assert b"dtype" in refused(lib, conv(**{k: L.F32}), "itts_act_conv_seg")
    assert b"lda != Cin" in refused(lib, conv(lda=32), "itts_act_conv_seg")
    assert b"bias_bstride != 0" in refused(lib, conv(bias_bstride=24), "itts_act_conv_seg")  # one item: a stride would step by sentence
    for kw in (dict(Cin=104, lda=104), dict(N=20), dict(pad_mode=1), dict(taps=2), dict(taps=3, dil=33), dict(nphase=2), dict(in_up=2),
               dict(ldc=28), dict(A=P + 2)):
        assert b"itts_gemm_which_pinned_conv != 4" in refused(lib, conv(**kw), "itts_act_conv_seg"), kw
    assert b"M == T >= off[n] * mul" in refused(lib, conv(M=512, T=256), "itts_act_conv_seg")
    assert b"M == T >= off[n] * mul" in refused(lib, conv(M=120, T=120), "itts_act_conv_seg")  # 31 * 4 = 124 rows
    monkeypatch.setenv("ITTS_NO_CONV_ACT", "1")
    assert b"ITTS_NO_CONV_ACT" in refused(lib, conv(), "itts_act_conv_seg")


@pytest.mark.parametrize("half", HALVES)
def test_bigvgan_packed_refuses_on_the_host(half):
    """itts_bigvgan_packed is itts_bigvgan_packed_check (engine-free, host memory only), then the launch sequence"""
    lib = L.load(half)
    assert b"null engine" in refused(lib, lib.itts_bigvgan_packed(None, P, P, P, P, 2, P, None), "itts_bigvgan_packed")
    cc = ieng.make_config(icfg.micro(), L.BF16)
    gap = lib.itts_bigvgan_packed_gap(C.byref(cc))
    good_len = [5, 12, 1, 9]
    good_off = PR.offsets(good_len, gap)

    def check(lat=P, spk=P, off=good_off, lens=good_len, n=4, wav=P, cfg=cc):
        o, l = _ints(off), _ints(lens)
        return lib.itts_bigvgan_packed_check(None if cfg is None else C.byref(cfg), lat, spk, _ptr(o), _ptr(l), n, wav)

    assert check() == 0
    assert b"null config" in refused(lib, check(cfg=None), "itts_bigvgan_packed")
    for kw in (dict(lat=None), dict(spk=None), dict(wav=None), dict(off=None), dict(lens=None)):
        assert b"null pointer" in refused(lib, check(**kw), "itts_bigvgan_packed"), kw
    for n in (0, -1, 129):
        assert b"n outside [1, 128]" in refused(lib, check(n=n), "itts_bigvgan_packed"), n
    assert b"off[0] != 0" in refused(lib, check(off=[o + 1 for o in good_off]), "itts_bigvgan_packed")
    assert b"a length < 1" in refused(lib, check(lens=[5, 12, 0, 9]), "itts_bigvgan_packed")
    assert b"offsets not increasing" in refused(lib, check(off=[0, 12, 12, 20, 36]), "itts_bigvgan_packed")
    assert b"offsets not increasing" in refused(lib, check(off=[0, 12, 31, 25, 60]), "itts_bigvgan_packed")
    one_short = PR.offsets(good_len, gap - 1)
    assert b"gap too small" in refused(lib, check(off=one_short), "itts_bigvgan_packed")
    tight_last = list(good_off[:-1]) + [good_off[-1] - 1]  # the LAST sentence needs its gap too
    assert b"gap too small" in refused(lib, check(off=tight_last), "itts_bigvgan_packed")
    assert b"2^31 - 1 output samples" in refused(lib, check(off=[0, 1 << 22], lens=[5], n=1), "itts_bigvgan_packed")
    assert check(off=PR.offsets(good_len, gap + 3)) == 0  # larger capacities are fine


# ---- the pinned conv selector ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", HALVES)
def test_pinned_conv_selector_does_not_look_at_the_row_count(half, monkeypatch):
    lib = L.load(half)
    for env in ("ITTS_NO_CONV_LDS", "ITTS_NO_CONV_ACT", "ITTS_NO_GEMM_GLDS", "ITTS_GEMM_FORCE_OLD", "ITTS_GEMM_P8"):
        monkeypatch.delenv(env, raising=False)
    rows = [16, 23, 255, 256, 257, 1024, 5 * 1024, 12 * 1024, 544 * 1024, 64 * 544 * 256]  # one short sentence .. a pack of 64
    shapes = {  # name -> (block, the family)
        "narrow AMP conv, C = 24 k = 11 d = 5": (dict(N=24, Cin=24, lda=24, ldc=24, ldr=24, ldadd=24, taps=11, dil=5, pad_left=25), 4),
        "narrow AMP conv, C = 96 k = 3": (dict(N=96, Cin=96, lda=96, ldc=96, ldr=96, ldadd=96, taps=3, dil=1, pad_left=1), 4),
        "wide AMP conv, C = 768 k = 7": (dict(N=768, Cin=768, lda=768, ldc=768, ldr=768, ldadd=768, taps=7, dil=3, pad_left=9), 3),
        "conv_pre 1280 -> 1536": (dict(N=1536, Cin=1280, lda=1280, ldc=1536, R=None, ADD=None, taps=7, pad_left=3), 3),
        "ups[0] polyphase 1536 -> 4 x 768": (dict(N=768, Cin=1536, lda=1536, ldc=4 * 768, R=None, ADD=None, taps=2, nphase=4, dil=-1, pad_left=0), 1),
        "C = 128 (too wide for the narrow conv, too narrow for gemm_p8)": (dict(N=128, Cin=128, lda=128, ldc=128, ldr=128, ldadd=128, taps=3), 1),
        "conv_post 24 -> 1 fp32": (dict(N=1, Cin=24, lda=24, ldc=1, R=None, ADD=None, bias=None, taps=7, pad_left=3, dtype_c=L.F32), 1),
        "fp32 engine": (dict(N=24, Cin=24, taps=3, dtype_a=L.F32, dtype_w=L.F32, dtype_c=L.F32), 0),
    }
    for name, (kw, family) in shapes.items():
        got = {m: lib.itts_gemm_which_pinned_conv(C.byref(A.block(**dict(kw, M=m, T=m)))) for m in rows}
        assert set(got.values()) == {family}, (name, got)
    # the selector it stands beside moves with the row count on the same shape - the dependence the packed pass removes
    narrow = shapes["narrow AMP conv, C = 24 k = 11 d = 5"][0]
    assert {lib.itts_gemm_which(C.byref(A.block(**dict(narrow, M=m, T=m)))) for m in (16, 255, 256)} == {1, 4}
    assert all(lib.itts_gemm_which_pinned_conv(C.byref(A.block(**dict(kw, M=m, T=m)))) != 2 for kw, _ in shapes.values() for m in rows)
    assert lib.itts_gemm_which_pinned_conv(None) == E_INVALID
    assert lib.itts_gemm_which_pinned_conv(C.byref(A.block(**dict(narrow, M=256, T=256, force_simple=1)))) == 0
    monkeypatch.setenv("ITTS_NO_CONV_LDS", "1")  # the family's own A/B switch still holds
    assert lib.itts_gemm_which_pinned_conv(C.byref(A.block(**dict(narrow, M=256, T=256)))) == 1
