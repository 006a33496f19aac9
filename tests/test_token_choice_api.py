"""No GPU: the public surface of itts_beam_step / itts_typical_rows / itts_sampler_step (header, both builds of the library, lib.py),
everything the three entries refuse before any device call, the fp64 references of tests/token_choice_ref.py against oracle/hf_beam.py
on inputs where fp32 and fp64 must agree, and the cap on the ambiguous band of every typical-filter case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import token_choice_ref as T
import wide_beam_ref as W
from itts_hip import lib as L
from oracle import hf_beam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_HOST = np.zeros(64, dtype=np.float32)
P = _HOST.ctypes.data  # host memory that a refused call never touches

ENTRIES = {"itts_beam_step": ("itts_beam_step_args", L.BeamStepArgs), "itts_typical_rows": ("itts_typical_args", L.TypicalArgs),
           "itts_sampler_step": ("itts_sampler_step_args", L.SamplerStepArgs)}


def test_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    kinds = {L.vp: "ptr", L.f32: "float", L.i32: "int"}
    for fn, (struct_name, cls) in ENTRIES.items():
        assert re.search(rf"\bint\s+{fn}\s*\(\s*const\s+{struct_name}\s*\*\s*\w+\s*,\s*itts_stream\s+\w+\s*\)\s*;", h), fn
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct_name + r"\s*;", h).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ctype = "ptr" if "*" in decl else "float" if decl.startswith("float") else "int"
                fields += [(n.strip(), ctype) for n in re.sub(r"^(const\s+)?(void|float|int)\s*\*?", "", decl).split(",")]
        assert fields == [(n, kinds[t]) for n, t in cls._fields_], fn  # the header's fields in the header's order
        assert fn in L.exported_symbols()
        for half in ("bf16", "f16"):
            lib = L.load(half)
            assert getattr(lib, fn).restype is L.i32 and len(getattr(lib, fn).argtypes) == 2
            assert lib.itts_abi_version() == 4  # additions: the ABI version stays


BEAM_OK = dict(len=P, cur_tok=P, unfinished=P, ids=P, anc=P, prefix=P, beam_scores=P, hyp_tok=P, hyp_score=P, hyp_len=P, hyp_order=P, hyp_n=P,
               hyp_worst=P, hyp_counter=P, done=P, logits=P, uniforms=P, cand_sc=P, cand_tok=P, cand_n=P, mode=0, items=1, nb=3, V=66,
               max_gen=4, Smax=8, stop=64, start_tok=63, fake_id=1, do_sample=1, top_k=30, top_p=0.8, temperature=1.0, penalty=10.0)
BEAM_OK1 = dict({k: v for k, v in BEAM_OK.items() if k not in ("logits", "uniforms", "cand_sc", "cand_tok", "cand_n")}, mode=1, pick_score=P,
                pick_tok=P, pick_beam=P)
TYP_OK = dict(logits=P, out=P, rows=1, V=66, stop=64, min_keep=1, penalty=10.0, mass=0.9)
TYP_OK_BEAMS = dict(TYP_OK, beam_ids=P, len=P, max_gen=4, start_tok=63, fake_id=1, log_softmax_first=1, min_keep=2)
SAMP_OK = dict(logits=P, seen=P, ids=P, cur_tok=P, unfinished=P, step=P, B=1, V=66, max_gen=4, stop=64, penalty=10.0)
SAMP_OK_S = dict(SAMP_OK, do_sample=1, top_k=30, top_p=0.8, temperature=1.0, uniforms=P)


def refused(lib, fn, cls, **kw):
    a = cls()
    for k, v in kw.items():
        setattr(a, k, v)
    st = getattr(lib, fn)(C.byref(a), None)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(fn.encode() + b": "), (fn, kw, st, msg)  # ITTS_E_INVALID, the entry's own message: no HIP call ran
    return msg


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_beam_step_refuses_bad_arguments_on_the_host(half):
    lib = L.load(half)
    assert lib.itts_beam_step(None, None) == -1 and b"null args" in lib.itts_last_error()
    no = lambda ok, **kw: refused(lib, "itts_beam_step", L.BeamStepArgs, **dict(ok, **kw))  # noqa: E731
    for ok in (BEAM_OK, BEAM_OK1):
        for nb in (-1, 0, 1, 11, 100):
            assert b"num_beams" in no(ok, nb=nb)
        no(ok, items=0)
        for V in (-5, 0, 1, 15001, 16384):
            assert b"V <= 15000" in no(ok, V=V, stop=0, start_tok=0, fake_id=0)
        for k in ("stop", "start_tok", "fake_id"):
            for bad in (-1, 66, 1000):
                assert b"outside the vocabulary" in no(ok, **{k: bad})
        for k in ("max_gen", "Smax"):
            for bad in (0, -2):
                assert b"max_gen, Smax" in no(ok, **{k: bad})
        for k in ("len", "cur_tok", "unfinished", "ids", "anc", "prefix", "beam_scores", "done", "hyp_tok", "hyp_score", "hyp_len",
                  "hyp_order", "hyp_n", "hyp_worst", "hyp_counter"):
            assert b"null state pointer" in no(ok, **{k: None}), k
        # h_next without its tables, rows or width
        full = dict(h_next=P, emb=P, pos=P, D=8, pos_rows=4)
        for k, bad in (("emb", None), ("pos", None), ("D", 0), ("pos_rows", 0), ("pos_rows", -1)):
            assert b"h_next needs" in no(ok, **dict(full, **{k: bad})), k
        for bad in (2, -1):
            assert b"emb_bf16" in no(ok, **dict(full, emb_bf16=bad))
        assert b"input_n" in no(ok, input_n=2) and b"input_n" in no(ok, input_n=-1, forced=P)
        assert b"mode" in no(ok, mode=2) and b"mode" in no(ok, mode=-1)
    for k in ("cand_sc", "cand_tok", "cand_n"):
        assert b"candidate scratch" in no(BEAM_OK, **{k: None})
    assert b"logits" in no(BEAM_OK, logits=None)
    for top_k in (0, -1, 129, 1000):
        assert b"top_k" in no(BEAM_OK, top_k=top_k)
    for k in ("top_p", "temperature"):
        for bad in (0.0, -0.5):
            assert b"top_p > 0, temperature > 0" in no(BEAM_OK, **{k: bad})
    assert b"uniforms" in no(BEAM_OK, uniforms=None)
    assert b"do_sample" in no(BEAM_OK, do_sample=2)
    assert b"penalty" in no(BEAM_OK, penalty=0.0)
    for k in ("pick_score", "pick_tok", "pick_beam"):
        assert b"picks" in no(BEAM_OK1, **{k: None})


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_typical_rows_refuses_bad_arguments_on_the_host(half):
    lib = L.load(half)
    assert lib.itts_typical_rows(None, None) == -1 and b"null args" in lib.itts_last_error()
    no = lambda ok, **kw: refused(lib, "itts_typical_rows", L.TypicalArgs, **dict(ok, **kw))  # noqa: E731
    for ok in (TYP_OK, TYP_OK_BEAMS):
        for k in ("logits", "out"):
            assert b"null logits / out" in no(ok, **{k: None})
        for V in (-1, 0, 1, 16385, 100000):
            assert b"V <= 16384" in no(ok, V=V, stop=0, start_tok=0, fake_id=0)
        for mass in (0.0, 1.0, -0.1, 1.5, float("nan")):
            assert b"mass" in no(ok, mass=mass)
        for bad in (0, -1):
            assert b"rows" in no(ok, rows=bad)
            assert b"min_keep" in no(ok, min_keep=bad)
        assert b"penalty" in no(ok, penalty=0.0)
        for bad in (-1, 66):
            assert b"stop outside" in no(ok, stop=bad)
    assert b"one seen source" in no(TYP_OK_BEAMS, seen=P)
    assert b"beam_ids needs len" in no(TYP_OK_BEAMS, len=None) and b"beam_ids needs len" in no(TYP_OK_BEAMS, max_gen=0)
    for k in ("start_tok", "fake_id"):
        for bad in (-1, 66):
            assert b"outside the vocabulary" in no(TYP_OK_BEAMS, **{k: bad})


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_sampler_step_refuses_bad_arguments_on_the_host(half):
    lib = L.load(half)
    assert lib.itts_sampler_step(None, None) == -1 and b"null args" in lib.itts_last_error()
    no = lambda ok, **kw: refused(lib, "itts_sampler_step", L.SamplerStepArgs, **dict(ok, **kw))  # noqa: E731
    for ok in (SAMP_OK, SAMP_OK_S):
        for k in ("logits", "seen", "ids", "cur_tok", "unfinished", "step"):
            assert b"null state pointer" in no(ok, **{k: None}), k
        for k in ("B", "V", "max_gen"):
            for bad in (0, -1):
                no(ok, **{k: bad})
        for bad in (-1, 66):
            assert b"stop outside" in no(ok, stop=bad)
        assert b"penalty" in no(ok, penalty=-1.0)
        full = dict(h_next=P, emb=P, pos=P, D=8, pos_rows=4)
        for k, bad in (("emb", None), ("pos", None), ("D", 0), ("pos_rows", 0)):
            assert b"h_next needs" in no(ok, **dict(full, **{k: bad})), k
        assert b"emb_bf16" in no(ok, **dict(full, emb_bf16=3))
        assert b"input_n" in no(ok, input_n=1)
        assert b"do_sample" in no(ok, do_sample=-1)
    assert b"uniforms" in no(SAMP_OK_S, uniforms=None)
    for k in ("top_p", "temperature"):
        assert b"top_p > 0, temperature > 0" in no(SAMP_OK_S, **{k: 0.0})
    assert b"V <= 15360" in no(SAMP_OK_S, V=15361) and b"V <= 15360" in no(SAMP_OK_S, V=16000, top_k=128)
    assert b"V <= 16384" in no(SAMP_OK_S, V=16385, top_k=0) and b"V <= 16384" in no(SAMP_OK_S, V=16385, top_k=129)


# ---- the references against oracle/hf_beam.py ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (66, 1025, 8194))
def test_narrow_row_against_warp_row(V):
    """Where no top-p boundary is within DELTA_N of a tail mass, NarrowRow keeps exactly the tokens the fp32 restatement keeps."""
    c = W.make_case("gauss", V, 1, 3)
    compared = 0
    for top_k, top_p, temp in ((1, 0.8, 1.0), (2, 1.0, 0.7), (30, 0.8, 1.0), (127, 0.3, 1.3), (128, 0.8, 1.0)):
        for r in range(3):
            row = T.NarrowRow(c["logits"][r], W.case_seen(c, r), c["penalty"], c["stop"], 0, 0, top_k, top_p, temp, T.delta_n())
            if row.R_lo != row.R_hi:
                continue
            lp = W.emulate_scores(c["logits"][r], W.case_seen(c, r), c["penalty"], c["stop"], 0, 0, 1.0)  # processed log-probs, fp32
            keep, _ = hf_beam.warp_row(lp, top_k, top_p, temp)
            assert np.array_equal(keep, np.sort(row.order[:row.R])), (top_k, r)
            compared += 1
    assert compared >= 12


def test_narrow_row_caps_ties_in_warp_row_order():
    lg = np.zeros(8194, F32)
    lg[8000] = 2.0
    row = T.NarrowRow(lg, set(), 1.0, 8192, 0, 0, 30, 1.0, 1.0, T.delta_n())
    assert row.n_ties == 8194 and row.n == 128 and list(row.order[:3]) == [8000, 0, 1] and row.R == 128
    keep, _ = hf_beam.warp_row(W.emulate_scores(lg, set(), 1.0, 8192, 0, 0, 1.0), 30, 1.0, 1.0)
    assert np.array_equal(keep, np.sort(row.order))


def test_scorer_model_walks_like_the_oracle_scorer():
    """ref_step over three calls: re-ordering, a hypothesis, the insertion counter, the untouched source plane."""
    cfg = dict(items=1, nb=2, max_gen=4, Smax=6, stop=9, prefix0=1)
    st = T.new_state(1, 2, 4, 6, 0, anc=np.array([[0] * 6, [1] * 6], np.uint8))
    sc = T.new_scorer(1, 2, 0.0)
    picks = (np.array([[-1.0, -0.5, -2.0, -3.0]], F32), np.array([[4, 5, 6, 7]]), np.array([[1, 1, 0, 0]]))
    s1 = T.ref_step(st, cfg, picks, sc)
    assert list(s1["cur_tok"]) == [5, 4] and list(s1["ids"][1, :, 0]) == [5, 4] and (s1["ids"][0] == T.SENT_I).all()
    assert list(s1["anc"][1, 0]) == [1, 1, 0, 1, 1, 1] and list(s1["anc"][1, 1]) == [1, 1, 1, 1, 1, 1] and list(s1["len"]) == [1, 1]
    picks = (np.array([[-0.6, -0.7, -0.8, -0.9]], F32), np.array([[9, 3, 9, 2]]), np.array([[1, 0, 0, 1]]))
    s2 = T.ref_step(s1, cfg, picks, sc)
    assert [(float(F32(s)), list(t)) for s, t in sc.hyps[0].beams] == [(float(F32(-0.6)), [4])]  # rank 0; the stop at rank 2 >= nb is ignored
    assert s2["hyp_counter"][0] == 1 and list(s2["cur_tok"]) == [3, 2] and list(s2["ids"][0, 0, :2]) == [5, 3] and s2["done"][0] == 0
    assert np.array_equal(s2["ids"][1], s1["ids"][1])  # the source plane of the call
    s3 = T.ref_step(dict(s2, len=np.array([4, 4], np.int32)), cfg, picks, sc)  # past the end: nothing moves
    assert all(np.array_equal(s3[k], s2[k]) for k in s2 if k != "len")


# ---- typical filter: the band caps, and the reference against the fp32 restatement ---------------------------------------------
@pytest.mark.parametrize("source", ("map", "beams"))
@pytest.mark.parametrize("V", T.TYP_VOCABS)
def test_typical_cases_meet_the_band_cap(V, source):
    agree = total = 0
    for mass in T.TYP_MASSES:
        for min_keep in (1, 2):
            c = T.typical_rows(V, source, mass, min_keep)
            for kind, ref in zip(T.TYP_ROWS, c["refs"]):
                assert ref["last_hi"] - ref["last_lo"] <= T.BAND_RANKS and ref["clear"], (mass, min_keep, kind)
                assert 0 <= int(ref["may"].sum()) - int(ref["must"].sum()) <= T.BAND_TOKENS, (mass, min_keep, kind)
                assert not (ref["must"] & ~ref["may"]).any() and not (ref["must"] & ~ref["kept64"]).any() and not (ref["kept64"] & ~ref["may"]).any()
                assert ref["d"] < 2e-5 and ref["e"] < 2e-4  # the bounds stay what they are derived to be: a few hundred / thousand units of 2^-24
                if kind == "peaked":
                    assert int(ref["kept64"].sum()) == min_keep
                elif V >= 8194:
                    assert int(ref["kept64"].sum()) >= 217, (mass, kind)  # flat enough: hundreds to thousands of ranks stay
                if not c["lsf"]:  # the fp32 restatement of the reference's warper lies between the two sets as well
                    want = T.processed32(c["logits"][T.TYP_ROWS.index(kind)], c["seen"][T.TYP_ROWS.index(kind)], 10.0, c["stop"], kind == "holes")
                    k32 = hf_beam.typical_filter(want, mass, min_keep) > -np.inf
                    assert not (ref["must"] & ~k32).any() and not (k32 & ~ref["may"]).any(), (mass, min_keep, kind)
                    agree += int(np.array_equal(k32, ref["kept64"]))
                    total += 1
    if total:
        print(f"typical V {V}: fp32 restatement equals the fp64 kept set in {agree} of {total} rows")
