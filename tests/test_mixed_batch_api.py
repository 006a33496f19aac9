"""No GPU: the public surface of mixed decode batches - the three new entries in the header, both builds of the library and lib.py,
everything itts_sampler_step_rows refuses before any device call, the pure grouping and table functions of itts_hip/infer_core.py,
the per-row seeds' draws, and Engine.generate's refusal of per-row settings under beams or typical filtering."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from itts_hip import engine as E
from itts_hip import infer_core
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("itts_sampler_step_rows", "itts_gpt_set_sampling_rows", "itts_gpt_latent_batch_cond")
_HOST = np.zeros(64, dtype=np.float32)
P = _HOST.ctypes.data  # host memory that a refused call never touches
OK_ARGS = dict(logits=P, seen=P, ids=P, cur_tok=P, unfinished=P, step=P, uniforms=P, B=3, V=66, max_gen=4, stop=64)
G, N, Wd = (0, 0, 1.0, 1.0, 10.0), (1, 30, 0.8, 1.0, 10.0), (1, 0, 0.9, 1.0, 2.0)  # one row of every class


def test_header_binding_and_both_libraries():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*itts_row_sampling\s*;", h).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int mode, top_k; float top_p, temperature, penalty;"
    assert [(n, t) for n, t in L.RowSampling._fields_] == [("mode", L.i32), ("top_k", L.i32), ("top_p", L.f32), ("temperature", L.f32),
                                                           ("penalty", L.f32)]
    assert C.sizeof(L.RowSampling) == 20
    for fn in NEW:
        decl = re.search(rf"\bint\s+{fn}\s*\(([^)]*)\)\s*;", h)
        assert decl, fn
        assert len(decl.group(1).split(",")) == len(L._PROTOS[fn][1]), fn  # one ctypes argument per declared parameter
        assert fn in L.exported_symbols()
    for half in ("bf16", "f16"):
        lib = L.load(half)
        for fn in NEW:
            assert getattr(lib, fn).restype is L.i32
        assert lib.itts_abi_version() == 4  # additions: the ABI version stays


def call(lib, table, scratch=P, **kw):
    a = L.SamplerStepArgs()
    for k, v in dict(OK_ARGS, **kw).items():
        setattr(a, k, v)
    rows = (L.RowSampling * len(table))(*[L.RowSampling(*r) for r in table]) if table is not None else None
    return lib.itts_sampler_step_rows(C.byref(a), rows, C.c_void_p(scratch) if scratch else None, None)


def refused(lib, table, scratch=P, **kw):
    st = call(lib, table, scratch, **kw)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(b"itts_sampler_step_rows: "), (table, kw, st, msg)  # ITTS_E_INVALID, its own message: no HIP call ran
    return msg


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_sampler_step_rows_refuses_bad_arguments_on_the_host(half):
    lib = L.load(half)
    ok = [G, N, Wd]
    assert lib.itts_sampler_step_rows(None, None, None, None) == -1 and lib.itts_last_error().startswith(b"itts_sampler_step_rows: null args")
    assert b"row table" in refused(lib, None) and b"scratch" in refused(lib, ok, scratch=None)
    assert b"aligned" in refused(lib, ok, scratch=P + 2)
    # the entries
    for bad in (-1, 2, 7):
        assert b"mode" in refused(lib, [G, (bad, 30, 0.8, 1.0, 10.0), Wd])
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        assert b"top_p" in refused(lib, [G, N, (1, 0, bad, 1.0, 2.0)])
    for bad in (0.0, -1.0, float("nan")):
        assert b"temperature" in refused(lib, [(1, 30, 0.8, bad, 10.0), G, G])
        assert b"penalty" in refused(lib, [G, (0, 0, 1.0, 1.0, bad), N])
    # a sampled row needs the draws; greedy rows alone do not (that call would run: it is not made here)
    assert b"uniforms" in refused(lib, [G, G, N], uniforms=None) and b"uniforms" in refused(lib, [Wd, G, G], uniforms=None)
    # the vocabulary limit of every class that is present - and only of those
    assert b"V <= 15360" in refused(lib, ok, V=15361, stop=5)
    assert b"V <= 16384" in refused(lib, [G, Wd, Wd], V=16385, stop=5) and b"V <= 16384" in refused(lib, [G, (1, 129, 0.8, 1.0, 1.0), G], V=16385, stop=5)
    assert b"V <= 15360" in refused(lib, [G, (1, 128, 0.8, 1.0, 1.0), Wd], V=16000, stop=5)
    # everything itts_sampler_step refuses
    for k in ("logits", "seen", "ids", "cur_tok", "unfinished", "step"):
        assert b"null state pointer" in refused(lib, ok, **{k: None}), k
    for k in ("B", "V", "max_gen"):
        for bad in (0, -1):
            refused(lib, ok, **{k: bad})
    for bad in (-1, 66):
        assert b"stop outside" in refused(lib, ok, stop=bad)
    full = dict(h_next=P, emb=P, pos=P, D=8, pos_rows=4)
    for k, bad in (("emb", None), ("pos", None), ("D", 0), ("pos_rows", 0)):
        assert b"h_next needs" in refused(lib, ok, **dict(full, **{k: bad})), k
    assert b"emb_bf16" in refused(lib, ok, **dict(full, emb_bf16=3))
    assert b"input_n" in refused(lib, ok, input_n=1)
    # the scalar sampling fields are not looked at: values itts_sampler_step refuses do not change the verdict on the table
    assert b"mode" in refused(lib, [G, (5, 0, 1.0, 1.0, 1.0), G], do_sample=7, penalty=-1.0, top_p=0.0, temperature=0.0)


def S(**kw):
    return dict(dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, num_beams=1, typical_sampling=False,
                     typical_mass=0.9, length_penalty=0.0, max_mel_tokens=600), **kw)


def test_mixed_groups():
    # one group across temperatures, top_k, penalties and greedy / sampled rows (the voice is no part of the settings at all)
    one = [S(), S(temperature=0.7), S(do_sample=False), S(top_k=0, top_p=0.9), S(repetition_penalty=2.0), S(typical_mass=0.5)]
    assert infer_core.mixed_groups(one) == [[0, 1, 2, 3, 4, 5]]
    # beams: split by every setting; equal settings still share
    beams = [S(num_beams=3), S(num_beams=3, temperature=0.7), S(num_beams=3), S(num_beams=2), S(num_beams=3, repetition_penalty=2.0), S()]
    assert infer_core.mixed_groups(beams) == [[0, 2], [1], [3], [4], [5]]
    assert infer_core.mixed_groups([S(num_beams=3, length_penalty=1.0), S(num_beams=3)]) == [[0], [1]]
    # typical filtering: the same, and the mass counts
    typ = [S(typical_sampling=True), S(), S(typical_sampling=True, top_p=0.5), S(typical_sampling=True), S(typical_sampling=True, typical_mass=0.5)]
    assert infer_core.mixed_groups(typ) == [[0, 3], [1], [2], [4]]
    # max_mel_tokens is a property of the generation
    assert infer_core.mixed_groups([S(), S(max_mel_tokens=300), S(temperature=1.3), S(max_mel_tokens=300, do_sample=False)]) == [[0, 2], [1, 3]]
    assert infer_core.mixed_groups([]) == []


def test_row_sampling_table():
    t = infer_core.row_sampling_table(4, [True, False, True, True], [30, 30, None, 200], 0.8, [1.0, 0.5, 0.7, None], [10.0, 2.0, 10.0, 1.5])
    assert t == [(1, 30, 0.8, 1.0, 10.0), (0, 0, 1.0, 1.0, 2.0), (1, 0, 0.8, 0.7, 10.0), (1, 200, 0.8, 1.0, 1.5)]
    assert infer_core.row_sampling_table(2, False, 5, 0.1, 3.0, 10.0) == [(0, 0, 1.0, 1.0, 10.0)] * 2  # greedy rows compare equal
    assert infer_core.row_sampling_table(1, True, -3, None, 1.0, 1.0) == [(1, 0, 1.0, 1.0, 1.0)]
    assert infer_core.row_sampling_table(1, True, 5, 7.0, 1.0, 1.0)[0][2] == 1.0 and infer_core.row_sampling_table(1, True, 5, 0.0, 1.0, 1.0)[0][2] == 1e-6
    for bad in (dict(top_k=[1, 2]), dict(temperature=-1.0), dict(repetition_penalty=[1.0, 0.0, 1.0])):
        with pytest.raises(ValueError):
            infer_core.row_sampling_table(3, **dict(dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0), **bad))
    t = infer_core.row_sampling_table(3, np.array([1, 0, 1]), (1, 2, 3), 1.0, 1.0, 10.0)  # arrays and tuples are sequences too
    assert [r[:2] for r in t] == [(1, 1), (0, 0), (1, 3)]


def test_per_row_seeds_give_every_row_its_own_column():
    seeds, max_gen = [7, 7, 123456789, 0], 9
    u = infer_core.row_uniforms(seeds, max_gen)
    assert u.shape == (max_gen, 4) and u.dtype == np.float32
    for b, s in enumerate(seeds):
        assert np.array_equal(u[:, b], np.random.default_rng(s).random(max_gen, dtype=np.float32))
    # a request's draws do not depend on who shares its batch, nor on its row
    assert np.array_equal(infer_core.row_uniforms([123456789], max_gen)[:, 0], u[:, 2])
    assert np.array_equal(infer_core.row_uniforms([0, 5, 7], max_gen)[:, 2], u[:, 0])


def test_generate_refuses_per_row_settings_under_beams_and_typical():
    eng = object.__new__(E.Engine)  # no device: the refusal comes before anything touches the engine
    ids = np.zeros((2, 5), np.int32)
    for kw in (dict(temperature=[1.0, 0.7], num_beams=3), dict(seed=[1, 2], num_beams=2), dict(do_sample=[True, False], typical_mass=0.9),
               dict(top_k=(30, 0), num_beams=2, do_sample=True)):
        with pytest.raises(ValueError, match="per-row"):
            E.Engine.generate(eng, None, ids, 8, **kw)
    with pytest.raises(ValueError, match="3 rows|for 2 rows"):
        E.Engine.generate(eng, None, ids, 8, temperature=[1.0, 0.7, 0.5])
