"""No GPU: the public surface of the opt-in row admission under beams (itts_gpt_set_admit_beams, the operator entry
itts_beam_admit), what the operator entry refuses before it touches the device, the Python scheduler with batch items as slots,
the precedence of ITTS_ADMIT_BEAMS on the Python side (the library's own precedence needs a running generation:
tests/test_gpu_beam_admit.py) and the ValueErrors of Engine.generate(slots=, num_beams=3)."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

from itts_hip import infer_core, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = ("bf16", "f16")
E_INVALID = -1


def test_entry_points():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+itts_gpt_set_admit_beams\s*\(\s*itts_engine\s*\*\s*\w+\s*,\s*int\s+on\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_beam_admit\s*\(\s*const\s+itts_beam_admit_args\s*\*\s*\w+\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    for name, nargs in (("itts_gpt_set_admit_beams", 2), ("itts_beam_admit", 2)):
        assert name in lib.exported_symbols()
        for half in HALVES:
            fn = getattr(lib.load(half), name)
            assert callable(fn) and len(fn.argtypes) == nargs and fn.restype is lib.i32
    for half in HALVES:
        assert lib.load(half).itts_abi_version() == 4  # additions: the ABI version stays
    # the argument block: the header's fields in the binding's order
    block = re.search(r"typedef struct \{([^}]*)\} itts_beam_admit_args;", h).group(1)
    names = re.findall(r"\*?\s*\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", block))
    assert names == [n for n, _ in lib.BeamAdmitArgs._fields_], names
    # the existing refusal stays in the library's text
    with open(os.path.join(ROOT, "index-tts-ipex_amd", "csrc", "model_gpt.hip")) as f:
        assert "gpt_admit_rows: rows cannot be admitted under beams" in f.read()


def test_python_options():
    from itts_hip import engine as ieng

    assert list(inspect.signature(ieng.Engine.set_admit_beams).parameters) == ["self", "on"]
    assert list(inspect.signature(ieng.Engine.admit_rows).parameters) == ["self", "cond", "text_ids", "rows", "uniforms", "forced"]
    g = inspect.signature(ieng.Engine.generate).parameters
    assert g["admit_beams"].default is None and g["admit_min"].default == 0.125

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["admit_beams"].default is False

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav"]).admit_beams is False
    assert p.parse_args(["hello", "-v", "voice.wav", "--admit-beams"]).admit_beams is True


@pytest.mark.parametrize("half", HALVES)
def test_beam_admit_refusals(half):
    """Every one of these is refused with ITTS_E_INVALID before any HIP call: the pointers are not device memory, and no GPU is
    here."""
    l = lib.load(half)
    two, far, neg, same = (np.asarray(v, np.int32) for v in ([3, 1], [1, 5], [-1, 2], [2, 2]))
    ok = dict(beam_scores=0x1000, anc=0x2000, hyp_order=0x3000, hyp_n=0x4000, hyp_worst=0x5000, hyp_counter=0x6000, beam_done=0x7000,
              uniforms=0x8000, uniforms_src=0x9000, items_host=two.ctypes.data, n=2, nb=3, items=5, Smax=256, max_gen=7, do_sample=1)

    def call(**kw):
        a = lib.BeamAdmitArgs(**dict(ok, **kw))
        return l.itts_beam_admit(C.byref(a), None)

    assert l.itts_beam_admit(None, None) == E_INVALID
    many = np.arange(129, dtype=np.int32)
    cases = [(dict(**{name: None}), b"null pointer") for name in ("beam_scores", "anc", "hyp_order", "hyp_n", "hyp_worst", "hyp_counter",
                                                                  "beam_done", "items_host")]
    cases += [(dict(n=0), b"1 <= n <= 128"), (dict(n=129, items_host=many.ctypes.data, items=200, nb=2), b"1 <= n <= 128"),
              (dict(nb=1), b"2 <= num_beams <= 10"), (dict(nb=11), b"2 <= num_beams <= 10"), (dict(nb=0), b"2 <= num_beams <= 10"),
              (dict(n=43, items_host=many.ctypes.data, items=200), b"more than 128 rows"),
              (dict(n=13, nb=10, items_host=many.ctypes.data, items=200), b"more than 128 rows"),
              (dict(items=0), b"need 1 <= items"), (dict(max_gen=0), b"need 1 <= items"), (dict(Smax=0), b"need 1 <= items"),
              (dict(Smax=250), b"multiple of 16"), (dict(Smax=24), b"multiple of 16"), (dict(anc=0x2008), b"multiple of 16"),
              (dict(uniforms=None), b"without a uniforms table"),
              (dict(items_host=far.ctypes.data), b"item outside"), (dict(items_host=neg.ctypes.data), b"item outside"),
              (dict(items_host=same.ctypes.data), b"written twice")]
    for kw, msg in cases:
        assert call(**kw) == E_INVALID, kw
        assert msg in l.itts_last_error(), (kw, l.itts_last_error())


# ---- the scheduler with batch items as slots ------------------------------------------------------------------------------------
def simulate_items(lengths, stops, slots, nb, admit_min, check_every=4, max_gen=48):
    """Drive AdmitScheduler as Engine.generate(slots=, admit_beams=True) does: the engine answers per ROW (nb rows per item, which
    step together), an item is live when unf[i * nb] != 0 and ln[i * nb] < max_gen.  Request r is done after stops[r] tokens."""
    sched = infer_core.AdmitScheduler(lengths, slots, admit_min)
    held = [[r, 1] for r in sched.first]
    log, steps = [], 1
    while True:
        ln = np.repeat([k for _, k in held], nb)
        unf = np.repeat([int(k < stops[r]) for r, k in held], nb)
        live = (unf[::nb] != 0) & (ln[::nb] < max_gen)
        sl, req = sched.take(np.nonzero(~live)[0].tolist())
        for s, r in zip(sl, req):
            held[s] = [r, 1]
            live[s] = True
        if req:
            log.append((steps, sl, req))
        if not sched.waiting and not live.any():
            break
        assert live.any(), "the loop would decode with no live item"
        for s in np.nonzero(live)[0]:
            held[s][1] = min(held[s][1] + check_every, max_gen)
        steps += check_every
    return sched, log


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("slots,nb,admit_min", [(5, 3, 0.125), (21, 3, 0.25), (8, 2, 0.5), (3, 10, 1.0)])
def test_scheduler_with_items_as_slots(seed, slots, nb, admit_min):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(slots + 1, 4 * slots))
    lengths = rng.integers(1, 40, N).tolist()
    stops = rng.integers(2, 70, N).tolist()
    sched, log = simulate_items(lengths, stops, slots, nb, admit_min)
    assert sorted(sched.order()) == list(range(N))  # nothing lost, nothing admitted twice
    admitted = [r for _, _, req in log for r in req]
    assert admitted == sorted(admitted) == [r for r in range(N) if r not in sched.first]
    assert min(lengths[i] for i in sched.first) >= max(lengths[i] for i in admitted)  # longest first: every later text fits L
    left = N - slots
    for t, sl, req in log:
        assert len(sl) == len(req) and sl == sorted(set(sl)) and all(0 <= s < slots for s in sl)  # ITEM slots
        assert len(req) >= min(sched.need, left) or len(req) == left
        left -= len(req)
    assert left == 0


# ---- the switch on the Python side, and generate()'s ValueErrors ---------------------------------------------------------------
def bare_engine(max_batch=64):
    """Engine.generate raises these before it touches the library: an object without one will do."""
    from itts_hip import engine as ieng

    e = object.__new__(ieng.Engine)
    e.ccfg = types.SimpleNamespace(max_batch=max_batch)
    return e


TEXT = np.ones((12, 9), np.int32)
OLD = r"row admission \(slots=\) runs with one beam and without typical filtering only"


def test_generate_value_errors(monkeypatch):
    monkeypatch.delenv("ITTS_ADMIT_BEAMS", raising=False)
    e = bare_engine()
    kw = dict(slots=5, num_beams=3, do_sample=True)
    with pytest.raises(ValueError, match="^" + OLD + "$"):  # without the switch: today's message, word for word
        e.generate(None, TEXT, 32, **kw)
    with pytest.raises(ValueError, match="^" + OLD + "$"):
        e.generate(None, TEXT, 32, admit_beams=False, **kw)
    with pytest.raises(ValueError, match="without typical filtering"):
        e.generate(None, TEXT, 32, admit_beams=True, typical_mass=0.9, **kw)
    with pytest.raises(ValueError, match="wide_beam_sampler='device'"):
        e.generate(None, TEXT, 32, admit_beams=True, top_k=0, **kw)
    with pytest.raises(ValueError, match="wide_beam_sampler='device'"):
        e.generate(None, TEXT, 32, admit_beams=True, top_k=200, wide_beam_sampler="host", **kw)
    with pytest.raises(ValueError, match="above 6"):
        e.generate(None, TEXT, 32, admit_beams=True, slots=2, num_beams=3)
    with pytest.raises(ValueError, match="max_batch"):
        bare_engine(12).generate(None, TEXT, 32, admit_beams=True, **kw)
    with pytest.raises(ValueError, match="^" + OLD + "$"):  # one beam with typical filtering: nothing new
        e.generate(None, TEXT, 32, slots=5, typical_mass=0.9, admit_beams=True)


def test_environment_precedence_on_the_python_side(monkeypatch):
    """generate(admit_beams=None) reads ITTS_ADMIT_BEAMS; an explicit argument wins.  IndexTTS: the variable overrides the
    constructor's setting in both directions (infer_core.env_switch)."""
    e = bare_engine()
    kw = dict(slots=5, num_beams=3, do_sample=True, typical_mass=0.9)  # the typical filter tells the two paths apart without a GPU
    monkeypatch.setenv("ITTS_ADMIT_BEAMS", "1")
    with pytest.raises(ValueError, match="admit_beams=True"):
        e.generate(None, TEXT, 32, **kw)
    with pytest.raises(ValueError, match="^" + OLD + "$"):
        e.generate(None, TEXT, 32, admit_beams=False, **kw)
    monkeypatch.setenv("ITTS_ADMIT_BEAMS", "0")
    with pytest.raises(ValueError, match="^" + OLD + "$"):
        e.generate(None, TEXT, 32, **kw)
    with pytest.raises(ValueError, match="admit_beams=True"):
        e.generate(None, TEXT, 32, admit_beams=True, **kw)
    for env, setting, want in (("1", False, True), ("0", True, False), ("", True, True), ("", False, False)):
        monkeypatch.setenv("ITTS_ADMIT_BEAMS", env)
        assert infer_core.env_switch("ITTS_ADMIT_BEAMS", setting) is want
