"""No GPU: the public surface of the opt-in row admission into a running batched decode (itts_gpt_admit_rows and what goes with
it, the operator entries itts_kv_admit / itts_rows_admit, the slot choice itts_admit_plan), the slot choice on hand-worked cases,
what the operator entries refuse before they touch the device, and the Python scheduler (infer_core.AdmitScheduler) as a pure
function on a simulated stop schedule."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from itts_hip import infer_core, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = ("bf16", "f16")
E_INVALID = -1


def header():
    with open(os.path.join(ROOT, "include", "itts_hip.h")) as f:
        return f.read()


def test_entry_points():
    h = header()
    assert re.search(r"\bint\s+itts_gpt_admit_rows\s*\(\s*itts_engine\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*cond\s*,\s*int\s+cond_rows\s*,"
                     r"\s*const\s+int32_t\s*\*\s*text_ids_host\s*,\s*int\s+n\s*,\s*int\s+L\s*,\s*const\s+itts_row_sampling\s*\*\s*rows_host\s*,"
                     r"\s*const\s+float\s*\*\s*uniforms_host\s*,\s*const\s+int32_t\s*\*\s*forced_host\s*,\s*int\s+n_forced\s*,"
                     r"\s*int32_t\s*\*\s*slots_host\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_gpt_row_status\s*\(\s*itts_engine\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*orig_host\s*,\s*int32_t\s*\*\s*len_host\s*,"
                     r"\s*int32_t\s*\*\s*unfinished_host\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_kv_admit\s*\(\s*void\s*\*\s*kc\s*,\s*void\s*\*\s*vc\s*,\s*const\s+void\s*\*\s*qkv\s*,\s*int\s+n\s*,\s*int\s+S\s*,"
                     r"\s*int\s+H\s*,\s*int\s+dh\s*,\s*int\s+Smax\s*,\s*int\s+Bcache\s*,\s*int\s+tq\s*,\s*int\s+tc\s*,"
                     r"\s*const\s+int\s*\*\s*slots_host\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_rows_admit\s*\(\s*const\s+itts_rows_admit_args\s*\*\s*\w+\s*,\s*itts_stream\s+\w+\s*\)\s*;", h)
    assert re.search(r"\bint\s+itts_admit_plan\s*\(\s*const\s+int\s*\*\s*unfinished_host\s*,\s*const\s+int\s*\*\s*len_host\s*,\s*int\s+B\s*,"
                     r"\s*int\s+max_gen\s*,\s*int\s+n\s*,\s*int\s*\*\s*slots_host\s*,\s*int\s*\*\s*n_free\s*\)\s*;", h)
    for name, nargs in (("itts_gpt_admit_rows", 12), ("itts_gpt_row_status", 5), ("itts_gpt_rows_total", 1), ("itts_gpt_keep_row_table", 2),
                        ("itts_gpt_graph_captures", 1), ("itts_kv_admit", 13), ("itts_rows_admit", 2), ("itts_admit_plan", 7)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
        assert name in lib.exported_symbols()
        for half in HALVES:
            fn = getattr(lib.load(half), name)
            assert callable(fn) and len(fn.argtypes) == nargs and fn.restype is lib.i32
    for half in HALVES:
        assert lib.load(half).itts_abi_version() == 4  # additions: the ABI version stays
    # the argument block of itts_rows_admit: the header's fields in the binding's order
    block = re.search(r"typedef struct \{([^}]*)\} itts_rows_admit_args;", h).group(1)
    names = re.findall(r"\*?\s*\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", block))
    assert names == [n for n, _ in lib.RowsAdmitArgs._fields_], names


def test_python_options():
    from itts_hip import engine as ieng

    assert list(inspect.signature(ieng.Engine.row_status).parameters) == ["self"]
    assert list(inspect.signature(ieng.Engine.admit_rows).parameters) == ["self", "cond", "text_ids", "rows", "uniforms", "forced"]
    g = inspect.signature(ieng.Engine.generate).parameters
    assert g["slots"].default is None and 0.0 < g["admit_min"].default <= 1.0 and g["return_log"].default is False

    from indextts.infer import IndexTTS

    assert inspect.signature(IndexTTS.__init__).parameters["admit_rows"].default is False

    from indextts import cli

    p = cli.build_parser()
    assert p.parse_args(["hello", "-v", "voice.wav"]).admit_rows is False
    assert p.parse_args(["hello", "-v", "voice.wav", "--admit-rows"]).admit_rows is True


def plan(l, unf, lens, max_gen, n):
    B = len(unf)
    u, ln = np.ascontiguousarray(unf, dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int32)
    slots = np.full(max(n, 1), -7, np.int32)
    free = C.c_int(-1)
    assert l.itts_admit_plan(u.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), B, max_gen, n, slots.ctypes.data_as(C.c_void_p),
                             C.byref(free)) == 0
    k = min(n, free.value)
    assert np.all(slots[k:] == -7)  # nothing written behind the list
    return slots[:k].tolist(), free.value


@pytest.mark.parametrize("half", HALVES)
def test_admit_plan_hand_worked(half):
    l = lib.load(half)
    assert plan(l, [1, 1, 1, 1], [3, 3, 3, 3], 32, 2) == ([], 0)                      # none finished
    assert plan(l, [0, 0, 0, 0], [3, 3, 3, 3], 32, 4) == ([0, 1, 2, 3], 4)            # all finished
    assert plan(l, [0, 0, 0, 0], [3, 3, 3, 3], 32, 2) == ([0, 1], 4)                  # the lowest ones
    assert plan(l, [1, 0, 1, 0, 1], [5, 5, 5, 5, 5], 32, 3) == ([1, 3], 2)            # n larger than free: what there is, and the count
    assert plan(l, [1, 1, 1, 0], [32, 31, 40, 2], 32, 4) == ([0, 2, 3], 3)            # rows at (or past) max_gen count as finished
    assert plan(l, [1, 0, 5, -1], [0, 0, 0, 0], 8, 4) == ([1], 1)                     # any non-zero flag is a live row
    assert plan(l, [0, 1, 0], [1, 1, 1], 8, 0) == ([], 2)                             # n = 0: only the count
    assert plan(l, [], [], 8, 0) == ([], 0)
    free = C.c_int()
    assert l.itts_admit_plan(None, None, 4, 8, 1, None, C.byref(free)) == E_INVALID
    assert b"admit_plan" in l.itts_last_error()


def kv_admit(l, kc=0x1000, vc=0x2000, qkv=0x3000, n=2, S=5, H=3, dh=64, Smax=9, Bcache=4, tq=lib.F32, tc=lib.F32, slots=(3, 1)):
    s = None if slots is None else np.asarray(slots, np.int32)
    return l.itts_kv_admit(kc, vc, qkv, n, S, H, dh, Smax, Bcache, tq, tc, None if s is None else s.ctypes.data_as(C.c_void_p), None)


@pytest.mark.parametrize("half", HALVES)
def test_kv_admit_refusals(half):
    """Every one of these is refused with ITTS_E_INVALID before any HIP call: the pointers are not device memory, and no GPU is here."""
    l = lib.load(half)
    for kw, msg in ((dict(kc=None), b"null pointer"), (dict(vc=None), b"null pointer"), (dict(qkv=None), b"null pointer"),
                    (dict(slots=None), b"null pointer"), (dict(n=0), b"1 <= n <= 128"),
                    (dict(n=129, slots=tuple(range(129)), Bcache=200), b"1 <= n <= 128"), (dict(S=0), b"S <= Smax"), (dict(S=10), b"S <= Smax"),
                    (dict(H=0), b"S <= Smax"), (dict(dh=0), b"S <= Smax"), (dict(Smax=0), b"S <= Smax"), (dict(Bcache=0), b"S <= Smax"),
                    (dict(tq=lib.F32, tc=lib.BF16), b"type pair"), (dict(tq=lib.BF16, tc=lib.F32), b"type pair"),
                    (dict(tq=lib.FP8, tc=lib.FP8), b"type pair"), (dict(tq=lib.F16, tc=lib.FP8), b"type pair"),
                    (dict(dh=6), b"multiple of"), (dict(dh=4, tc=lib.FP8), b"multiple of"), (dict(dh=4, tq=lib.BF16, tc=lib.BF16), b"multiple of"),
                    (dict(qkv=0x3008), b"aligned"), (dict(kc=0x1008), b"aligned"), (dict(vc=0x2004, tc=lib.FP8), b"aligned"),
                    (dict(slots=(3, 4)), b"slot outside"), (dict(slots=(-1, 2)), b"slot outside"), (dict(slots=(2, 2)), b"written twice")):
        assert kv_admit(l, **kw) == E_INVALID, kw
        assert msg in l.itts_last_error(), (kw, l.itts_last_error())


@pytest.mark.parametrize("half", HALVES)
def test_rows_admit_refusals(half):
    l = lib.load(half)
    sl, kv = np.asarray([2, 0], np.int32), np.asarray([3, 7], np.int32)
    ok = dict(seen=0x1000, unfinished=0x2000, cur_tok=0x3000, len=0x4000, kv_start=0x5000, ids=0x6000, forced=0x7000, uniforms=0x8000,
              forced_src=None, uniforms_src=None, slots_host=sl.ctypes.data, kv_start_host=kv.ctypes.data, n=2, B=3, V=50, max_gen=8,
              fake_id=1, start_tok=48, stop=49)

    def call(**kw):
        a = lib.RowsAdmitArgs(**dict(ok, **kw))
        return l.itts_rows_admit(C.byref(a), None)

    assert l.itts_rows_admit(None, None) == E_INVALID
    two = np.asarray([1, 1], np.int32)
    far = np.asarray([1, 3], np.int32)
    neg = np.asarray([-1, 70000], np.int32)
    for kw, msg in ((dict(seen=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(slots_host=None), b"null pointer"),
                    (dict(kv_start_host=None), b"null pointer"), (dict(n=0), b"1 <= n <= 128"), (dict(n=129), b"1 <= n <= 128"),
                    (dict(B=0), b"need 1 <= B"), (dict(V=0), b"need 1 <= B"), (dict(max_gen=0), b"need 1 <= B"),
                    (dict(forced=None, forced_src=0x9000), b"without a forced table"),
                    (dict(uniforms=None, uniforms_src=0x9000), b"without a uniforms table"),
                    (dict(slots_host=two.ctypes.data), b"written twice"), (dict(slots_host=far.ctypes.data), b"slot outside"),
                    (dict(kv_start_host=neg.ctypes.data), b"kv_start outside")):
        assert call(**kw) == E_INVALID, kw
        assert msg in l.itts_last_error(), (kw, l.itts_last_error())


# ---- the scheduler -------------------------------------------------------------------------------------------------------------
def simulate(lengths, stops, slots, admit_min, check_every=4, max_gen=64):
    """Drive AdmitScheduler as Engine.generate(slots=..) does, on a stop schedule: request r ends after stops[r] tokens (or at
    max_gen).  -> (the scheduler, [(tokens, slots, requests)], every slot's (request, first token, last token) history)"""
    sched = infer_core.AdmitScheduler(lengths, slots, admit_min)
    held = [[r, 0] for r in sched.first]  # request, tokens it holds
    for h in held:
        h[1] = 1
    log, hist, steps = [], [], 1
    while True:
        fin = [s for s, (r, k) in enumerate(held) if k >= min(stops[r], max_gen)]
        sl, req = sched.take(fin)
        for s, r in zip(sl, req):
            hist.append((s, held[s][0]))
            held[s] = [r, 1]
        if req:
            log.append((steps, sl, req))
        live = [s for s, (r, k) in enumerate(held) if k < min(stops[r], max_gen)]
        if not sched.waiting and not live:
            break
        assert live, "the loop would decode with no live row"
        for s in live:
            held[s][1] += check_every
        steps += check_every
    return sched, log, hist


def test_scheduler_first_rows_and_order():
    lengths = [5, 9, 9, 2, 7, 9, 1, 8]
    s = infer_core.AdmitScheduler(lengths, 3, 0.5)
    assert s.first == [1, 2, 5] and s.waiting == [0, 3, 4, 6, 7] and s.need == 2  # the longest (ties: the earlier), caller's order
    assert min(lengths[i] for i in s.first) >= max(lengths[i] for i in s.waiting)
    assert s.take([]) == ([], []) and s.take([1]) == ([], [])  # one finished slot of the two it waits for, five waiting
    assert s.take([0, 2]) == ([0, 2], [0, 3]) and s.slot_req == [0, 2, 3]
    assert s.take([1, 2]) == ([1, 2], [4, 6]) and s.waiting == [7]
    assert s.take([0]) == ([0], [7])  # the rest of the list fits: no waiting for a second slot
    assert s.take([0, 1, 2]) == ([], []) and s.order() == [1, 2, 5, 0, 3, 4, 6, 7]
    few = infer_core.AdmitScheduler([3, 4], 8, 0.25)  # no more requests than slots: nobody waits
    assert few.first == [0, 1] and few.waiting == [] and few.order() == [0, 1]
    assert infer_core.AdmitScheduler([1] * 30, 12, 5 / 12).need == 5 and infer_core.AdmitScheduler([1] * 30, 64, 1 / 8).need == 8
    for bad in (dict(slots=0, admit_min=0.5), dict(slots=4, admit_min=0.0), dict(slots=4, admit_min=1.5)):
        with pytest.raises(ValueError):
            infer_core.AdmitScheduler([1, 2, 3], **bad)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("slots,admit_min", [(12, 5 / 12), (8, 0.25), (4, 1.0), (7, 0.01)])
def test_scheduler_simulated(seed, slots, admit_min):
    rng = np.random.default_rng(seed)
    N = int(rng.integers(slots + 1, 5 * slots))
    lengths = rng.integers(1, 40, N).tolist()
    stops = rng.integers(2, 90, N).tolist()
    sched, log, hist = simulate(lengths, stops, slots, admit_min)
    order = sched.order()
    assert sorted(order) == list(range(N))  # nothing lost, nothing admitted twice
    admitted = [r for _, _, req in log for r in req]
    assert admitted == sorted(admitted) == [r for r in range(N) if r not in sched.first]  # the waiting list keeps the caller's order
    assert min(lengths[i] for i in sched.first) >= max(lengths[i] for i in admitted)  # longest first: every later text fits L
    for t, sl, req in log:
        assert len(sl) == len(req) and sl == sorted(set(sl)) and all(0 <= s < slots for s in sl)
    need = sched.need
    left = N - slots
    for t, sl, req in log:  # an admission waits for `need` finished slots unless the rest of the list fits
        assert len(req) >= min(need, left) or len(req) == left
        left -= len(req)
    assert left == 0
