"""No GPU: the public surface of the packed latent pass - itts_attention_varlen / itts_attention_varlen_which / itts_gpt_latent_packed
in the header, in both builds of the library and in lib.py; what the two attention entries refuse on the host (one valid call on
host memory, then one argument at a time made invalid: each is refused with ITTS_E_INVALID and a message that begins with the
entry's own name - a HIP call would answer ITTS_E_HIP or touch the host pointers); that the dispatcher's pick never moves with a
length; the chunker of Engine.latent_packed (infer_core.packed_chunks); the precedence of ITTS_PACKED_LATENT over the setter."""
import inspect
import os
import re

import numpy as np
import pytest

from itts_hip import infer_core
from itts_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HOST = np.zeros(4096, dtype=np.float32)
P = (_HOST.ctypes.data + 63) // 64 * 64  # the matrix-core kernel wants 16-byte aligned q, k, v
NO_SWITCH = os.environ.get("ITTS_ATTN_SIMPLE") is None  # read once per process by the library: with it set the dispatcher never names 2


def offsets(*lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


OFF = offsets(40, 1, 17)
# the packed latent pass of a 16-bit engine: fused qkv, 3 heads of 64
VALID = dict(o=P, q=P, k=P, v=P, off=OFF, nseq=3, H=3, dqk=64, dv=64, ldq=576, ldk=576, ldv=576, ldo=192, scale=0.125, dtype=L.BF16, kernel=0)
ORDER = ("q", "k", "v", "off", "nseq", "H", "dqk", "dv", "ldq", "ldk", "ldv", "ldo", "scale", "dtype", "kernel")


def call_args(**kw):
    a = dict(VALID, **kw)
    if isinstance(a["off"], np.ndarray):
        a["off"] = a["off"].ctypes.data
    return a["o"], tuple(a[k] for k in ORDER)


def which(lib, **kw):
    return lib.itts_attention_varlen_which(*call_args(**kw)[1])


def refused(lib, ask=True, **kw):
    """Both entries refuse the call: status -1 and the entry's own message -> the messages"""
    o, args = call_args(**kw)
    st = lib.itts_attention_varlen(o, *args, None)
    msg = lib.itts_last_error()
    assert st == -1 and msg.startswith(b"itts_attention_varlen: "), (kw, st, msg)  # ITTS_E_INVALID, before any HIP call
    if ask:
        assert lib.itts_attention_varlen_which(*args) == -1, kw
        m2 = lib.itts_last_error()
        assert m2.startswith(b"itts_attention_varlen_which: "), (kw, m2)
        msg += b" | " + m2
    return msg


def test_entry_points_header_and_binding():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        h = f.read()
    common = (r"const\s+void\s*\*\s*q\s*,\s*const\s+void\s*\*\s*k\s*,\s*const\s+void\s*\*\s*v\s*,\s*const\s+int32_t\s*\*\s*seq_off_host\s*,\s*int\s+nseq\s*,"
              r"\s*int\s+H\s*,\s*int\s+dqk\s*,\s*int\s+dv\s*,\s*int\s+ldq\s*,\s*int\s+ldk\s*,\s*int\s+ldv\s*,\s*int\s+ldo\s*,\s*float\s+scale\s*,"
              r"\s*int\s+dtype\s*,\s*int\s+kernel\s*")
    assert re.search(r"\bint\s+itts_attention_varlen\s*\(\s*void\s*\*\s*o\s*,\s*" + common + r",\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_attention_varlen_which\s*\(\s*" + common + r"\)\s*;", h)
    assert re.search(r"#define\s+ITTS_VARLEN_MAX_SEQ\s+128\b", h)
    assert re.search(r"\bint\s+itts_gpt_latent_packed\s*\(\s*itts_engine\s*\*\s*e\s*,\s*const\s+float\s*\*\s*cond\s*,\s*const\s+int32_t\s*\*\s*cond_index_host\s*,"
                     r"\s*int\s+n_cond\s*,", h)
    new = {"itts_attention_varlen", "itts_attention_varlen_which", "itts_gpt_latent_packed"}
    assert new <= set(L.exported_symbols())
    for half in ("bf16", "f16"):
        lib = L.load(half)
        for name in new:
            assert getattr(lib, name).restype is L.i32
        assert len(lib.itts_attention_varlen_which.argtypes) == len(lib.itts_attention_varlen.argtypes) - 2
        assert lib.itts_gpt_latent_packed.argtypes == lib.itts_gpt_latent_batch_cond.argtypes  # the same interface
        assert lib.itts_abi_version() == 4  # an addition: the ABI version stays
    assert infer_core.PACKED_MAX_SEQ == 128


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_varlen_entries_refuse_on_the_host(half):
    lib = L.load(half)
    assert which(lib) == (2 if NO_SWITCH else 1)  # the call itself is valid
    assert which(lib, kernel=1) == 1 and which(lib, kernel=2) == 2
    for k in ("q", "k", "v", "off"):
        assert b"null pointer" in refused(lib, **{k: None}), k
    assert b"null pointer" in refused(lib, ask=False, o=None)  # (o is not an argument of itts_attention_varlen_which)
    for bad in (0, -1, 129, 1 << 20):
        assert b"nseq" in refused(lib, nseq=bad), bad
    big = offsets(*([3] * 128))
    assert which(lib, off=big, nseq=128) in (1, 2) and which(lib, nseq=1) in (1, 2)
    assert b"[0] must be 0" in refused(lib, off=OFF + 1)
    for bad in (offsets(40, 0, 17), np.asarray([0, 40, 39, 58], dtype=np.int32), np.asarray([0, 40, 41, 41], dtype=np.int32),
                np.asarray([0, -1, 41, 58], dtype=np.int32)):
        assert b"strictly increasing" in refused(lib, off=bad), bad
    for bad in (0, -1, 65536):
        assert b"H is a grid dimension" in refused(lib, H=bad, ldq=1 << 23, ldk=1 << 23, ldv=1 << 23, ldo=1 << 23), bad
    assert which(lib, H=65535, ldq=65535 * 192, ldk=65535 * 192, ldv=65535 * 192, ldo=65535 * 64) in (1, 2)
    for bad in (L.F16, L.FP8, 2, 3, -1, 6):
        assert b"dtype" in refused(lib, dtype=bad), bad
    for kw in (dict(dqk=0), dict(dqk=-64), dict(dqk=129, ldq=1024, ldk=1024), dict(dv=0), dict(dv=65, ldv=1024, ldo=1024), dict(dv=128, ldv=1024, ldo=1024)):
        assert b"head dims" in refused(lib, **kw), kw
    for k, least in (("ldq", 192), ("ldk", 192), ("ldv", 192), ("ldo", 192)):
        assert b"leading dims" in refused(lib, **{k: least - 1}), k
        assert b"leading dims" in refused(lib, **{k: 0}), k
        assert which(lib, **dict(dict(ldq=192, ldk=192, ldv=192, ldo=192), **{k: least})) in (1, 2)
    assert b"leading dims" in refused(lib, dqk=128, ldq=383)  # H * dqk = 384
    for bad in (-1, 3, 99):
        assert b"unknown kernel" in refused(lib, kernel=bad)
    # kernel 2: whatever its structural rule rejects is refused, the vector kernel does not take its place - and kernels 0 and 1
    # take every one of these calls
    for kw in (dict(dtype=L.F32), dict(dqk=32), dict(dqk=96), dict(dqk=128, ldq=384, ldk=384), dict(dv=32), dict(dv=48), dict(ldq=580), dict(ldk=580),
               dict(ldv=580), dict(q=P + 8), dict(k=P + 8), dict(v=P + 2)):
        assert b"attn_varlen_mfma needs" in refused(lib, kernel=2, **kw), kw
        assert which(lib, **kw) == 1 and which(lib, kernel=1, **kw) == 1, kw


@pytest.mark.parametrize("half", ("bf16", "f16"))
def test_the_dispatchers_pick_never_moves_with_a_length(half):
    """The same pick for every length set, a 1-row sequence and 128 sequences included: type, head dims, leading dims and alignment only."""
    lib = L.load(half)
    mfma = 2 if NO_SWITCH else 1
    sets = ((1,), (15,), (16,), (64,), (65,), (15, 16, 17), (1, 129, 64, 130), (200, 1, 1, 1, 70), tuple(1 + (7 * i) % 37 for i in range(128)))
    for lens in sets:
        off = offsets(*lens)
        kw = dict(off=off, nseq=len(lens))
        assert which(lib, **kw) == mfma, lens
        assert which(lib, kernel=2, **kw) == 2, lens  # the matrix-core kernel takes every length >= 1
        assert which(lib, dtype=L.F32, **kw) == 1 and which(lib, dv=32, **kw) == 1 and which(lib, ldk=580, **kw) == 1 and which(lib, q=P + 8, **kw) == 1, lens
        assert which(lib, ldk=584, **kw) == mfma and which(lib, o=P + 2, ldo=193, **kw) == mfma, lens  # o is stored by elements


def test_packed_chunks():
    pc = infer_core.packed_chunks
    assert pc([5, 5, 5], 100) == [[0, 1, 2]]
    assert pc([5, 5, 5], 10) == [[0, 1], [2]]
    assert pc([5, 50, 5], 10) == [[0], [1], [2]]           # a sequence over the budget is a chunk of its own
    assert pc([50], 10) == [[0]] and pc([], 10) == []
    assert pc([1] * 300, 10 ** 9) == [list(range(128)), list(range(128, 256)), list(range(256, 300))]  # at most 128 sequences
    assert pc([1] * 5, 10 ** 9, max_seqs=2) == [[0, 1], [2, 3], [4]]
    assert pc([3, 3, 4], 10) == [[0, 1, 2]] and pc([3, 3, 5], 10) == [[0, 1], [2]]  # the budget is inclusive
    rng = np.random.default_rng(3)
    for _ in range(50):
        lens = rng.integers(1, 700, size=int(rng.integers(1, 400))).tolist()
        budget = int(rng.integers(1, 5000))
        chunks = pc(lens, budget)
        assert [i for c in chunks for i in c] == list(range(len(lens)))  # order-preserving, every sequence once
        for c in chunks:
            assert 1 <= len(c) <= 128 and (sum(lens[i] for i in c) <= budget or len(c) == 1)
        for a, b in zip(chunks, chunks[1:]):  # greedy: the next sequence did not fit
            assert len(a) == 128 or sum(lens[i] for i in a) + lens[b[0]] > budget
    assert pc(lens) == pc(lens, infer_core.PACKED_MAX_TOKENS, infer_core.PACKED_MAX_SEQ)
    for bad in (dict(lengths=[3, 0]), dict(lengths=[3, -1]), dict(lengths=[3], max_tokens=0), dict(lengths=[3], max_seqs=0)):
        with pytest.raises(ValueError):
            pc(**bad)


def test_switch_precedence(monkeypatch):
    """ITTS_PACKED_LATENT=1 / 0 overrides IndexTTS(packed_latent=..) in both directions; unset or anything else leaves the setter.
    Default off."""
    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["packed_latent"].default is False
    src = inspect.getsource(IndexTTS)
    assert src.count('infer_core.env_switch("ITTS_PACKED_LATENT", self.packed_latent)') == 2  # plain infer_batch and the mixed path
    monkeypatch.delenv("ITTS_PACKED_LATENT", raising=False)
    assert infer_core.env_switch("ITTS_PACKED_LATENT", False) is False and infer_core.env_switch("ITTS_PACKED_LATENT", True) is True
    monkeypatch.setenv("ITTS_PACKED_LATENT", "1")
    assert infer_core.env_switch("ITTS_PACKED_LATENT", False) is True and infer_core.env_switch("ITTS_PACKED_LATENT", True) is True
    monkeypatch.setenv("ITTS_PACKED_LATENT", "0")
    assert infer_core.env_switch("ITTS_PACKED_LATENT", False) is False and infer_core.env_switch("ITTS_PACKED_LATENT", True) is False
    monkeypatch.setenv("ITTS_PACKED_LATENT", "yes")
    assert infer_core.env_switch("ITTS_PACKED_LATENT", False) is False and infer_core.env_switch("ITTS_PACKED_LATENT", True) is True
    from indextts import cli

    assert cli.build_parser().parse_args(["-v", "x.wav", "hello", "--packed-latent"]).packed_latent is True
