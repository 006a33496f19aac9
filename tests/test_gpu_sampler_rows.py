"""GPU: itts_sampler_step_rows - one launch sequence of the one-beam samplers over a batch whose rows carry their own settings
(csrc/decode_sampler.hip sampler_rows_step: sampler2_kernel / sampler_sample_kernel / sampler_wide_kernel<ROWS = true>, a row's block
working in the kernel of its class and returning at once in the others).
Oracle: the existing itts_sampler_step.  For every row r the scalar entry runs with row r's settings over the same batch; row r of
every state array (seen, ids, cur_tok, unfinished, step, h_next) has to carry the same bits - so a row is committed exactly once,
by the right kernel, with its own top_k / top_p / temperature / penalty.  Greedy and narrow rows are checked against
token_choice_ref.greedy_ref / oracle.gpt.sample_pick as well.  Inputs, the device copy of the table and every guard block are
compared after the call."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_sampler_step as S  # noqa: E402  (new_state, run_sampler, same-state helpers)
import token_choice_ref as T  # noqa: E402
import wide_beam_ref as W  # noqa: E402

from itts_hip import lib, prng  # noqa: E402
from oracle import gpt as ogpt  # noqa: E402

F32 = np.float32
B, MAX_GEN = 6, 5
# (mode, top_k, top_p, temperature, penalty)
ENTRIES = {"g10": (0, 0, 1.0, 1.0, 10.0), "g1.5": (0, 0, 1.0, 1.0, 1.5),
           "n1": (1, 1, 1.0, 1.0, 10.0), "n128": (1, 128, 0.8, 0.7, 1.0),
           "w0": (1, 0, 0.9, 1.0, 10.0), "w200": (1, 200, 1.0, 1.3, 1.5)}
TABLES = {"all": ("g10", "g1.5", "n1", "n128", "w0", "w200"),
          "greedy": ("g10", "g1.5", "g1.5", "g10", "g10", "g1.5"),
          "narrow": ("n1", "n128", "n128", "n1", "n128", "n1"),
          "wide": ("w0", "w200", "w200", "w0", "w0", "w200"),
          "no_greedy": ("w200", "n1", "w0", "n128", "n1", "w0"),
          "no_narrow": ("w0", "g10", "g1.5", "w200", "g10", "w0"),
          "no_wide": ("n128", "g1.5", "n1", "g10", "n128", "g1.5")}


@functools.lru_cache(maxsize=None)
def case(V, D):
    """Six rows whose step differs, row 3 finished, row 4 with a forced token at its step; every row has seen its two best tokens."""
    lg = W.gaussian(f"sampler_rows.{V}.{D}", V, (B, V), 2.0)
    seen = np.zeros((B, V), bool)
    for b in range(B):
        seen[b, prng.randint(f"sampler_rows.seen{b}", V, 12, 0, V)] = True
        seen[b, np.argsort(lg[b])[-2:]] = True
        lg[b, 5 + b], seen[b, 5 + b] = 12.0, True  # a seen token that wins at penalty 1.5 (8.0) and loses at penalty 10 (1.2)
    step =[0, 3, 1, 2, 4, 1]
    forced = np.full((B, MAX_GEN), -1, np.int32)
    forced[4, 4] = 17
    cfg = dict(V=V, max_gen=MAX_GEN, stop=V - 2, forced=forced, D=D, pos_rows=MAX_GEN + 1, emb_bf16=0)
    if D:
        cfg["emb"] = prng.uniform(f"sampler_rows.emb.{V}", V, V * D).reshape(V, D)
        cfg["pos"] = prng.uniform(f"sampler_rows.pos.{V}", V, cfg["pos_rows"] * D).reshape(cfg["pos_rows"], D)
    st = S.new_state(B, V, MAX_GEN, D, step=step, unfinished=[1, 1, 1, 0, 1, 1], seen=seen)
    u = prng.uniform(f"sampler_rows.u.{V}", 3, MAX_GEN * B).reshape(MAX_GEN, B).astype(F32)
    return lg, cfg, st, u


@functools.lru_cache(maxsize=None)
def scalar_run(V, D, name):
    """The existing entry with one table entry as the scalar setting, over the whole batch (computed once per case and entry)."""
    lg, cfg, st, u = case(V, D)
    mode, top_k, top_p, temp, pen = ENTRIES[name]
    return S.run_sampler(st, dict(cfg, do_sample=mode, top_k=top_k, top_p=top_p, temperature=temp, penalty=pen), lg, u)


def run_rows(st, cfg, logits, uniforms, table, expect=0):
    """S.run_sampler for itts_sampler_step_rows; the scalar sampling fields of the argument block hold values no row uses."""
    l = lib.load()
    d = T.DevArrays(S.DEV)
    a = lib.SamplerStepArgs()
    for name in S.STATE:
        setattr(a, name, d.put(name, st[name]))
    if not cfg.get("D"):
        a.h_next = None
    a.logits = d.put("logits", logits)
    a.B, a.V, a.max_gen, a.stop = logits.shape[0], logits.shape[1], cfg["max_gen"], cfg["stop"]
    a.do_sample, a.top_k, a.top_p, a.temperature, a.penalty = 1, 7, 0.33, 2.5, 3.0  # ignored
    a.forced = d.put("forced", cfg["forced"].astype(np.int32))
    a.uniforms = d.put("uniforms", np.ascontiguousarray(uniforms, F32))
    if cfg.get("D"):
        a.D, a.pos_rows, a.emb_bf16 = cfg["D"], cfg["pos_rows"], 0
        a.emb, a.pos = d.put("emb", cfg["emb"]), d.put("pos", cfg["pos"])
    rows = (lib.RowSampling * len(table))(*[lib.RowSampling(*e) for e in table])
    scratch = d.put("rows_dev", np.zeros(len(table) * C.sizeof(lib.RowSampling), np.uint8))
    torch.cuda.synchronize()
    status = l.itts_sampler_step_rows(C.byref(a), rows, C.c_void_p(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == expect, (status, l.itts_last_error())
    got = {name: d.get(name) for name in S.STATE}
    assert T.same_bits(d.get("logits"), logits) and T.same_bits(d.get("forced"), cfg["forced"].astype(np.int32))
    assert T.same_bits(d.get("uniforms"), np.ascontiguousarray(uniforms, F32))
    for name in ("emb", "pos"):
        if cfg.get("D"):
            assert T.same_bits(d.get(name), cfg[name])
    assert d.get("rows_dev").tobytes() == bytes(rows)  # the device copy: the host table, between intact guard blocks
    return got


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("V,D", ((66, 0), (66, 64), (8194, 0), (8194, 64)))
def test_every_row_has_the_bits_of_its_scalar_run(V, D, table):
    lg, cfg, st, u = case(V, D)
    names = TABLES[table]
    got = run_rows(st, cfg, lg, u, [ENTRIES[n] for n in names])
    choice = [0] * B
    for r, n in enumerate(names):
        want = scalar_run(V, D, n)
        for arr in S.STATE:
            if arr == "h_next" and not D:
                continue
            assert T.same_bits(got[arr][r], want[arr][r]), (table, r, n, arr)
        mode, top_k, top_p, temp, pen = ENTRIES[n]
        if mode == 0:
            choice[r] = T.greedy_ref(lg[r], st["seen"][r].astype(bool), pen, cfg["stop"], 0)
        elif 1 <= top_k <= 128:
            choice[r] = ogpt.sample_pick(T.processed32(lg[r], st["seen"][r].astype(bool), pen, cfg["stop"], 0), top_k, top_p, temp,
                                         float(u[min(int(st["step"][r]), MAX_GEN - 1), r]))
    ref = T.commit_ref(st, cfg, choice)
    for r, n in enumerate(names):
        if ENTRIES[n][0] == 0 or 1 <= ENTRIES[n][1] <= 128:
            for arr in S.STATE:
                if arr != "h_next" or D:
                    assert T.same_bits(got[arr][r], ref[arr][r]), (table, r, n, arr, "reference")
    # the case itself: the finished row wrote stop, the forced row its token, and two rows of one class differ through their settings
    assert got["cur_tok"][3] == cfg["stop"] and got["unfinished"][3] == 0 and got["cur_tok"][4] == 17
    assert list(got["step"]) == [1, 4, 2, 3, 5, 2]


def test_the_settings_of_a_row_decide_its_token():
    """The oracle runs themselves differ between the entries of one class on some row: a table that mixed two rows up would show."""
    for a, b in (("g10", "g1.5"), ("n1", "n128"), ("w0", "w200")):
        assert any(not np.array_equal(scalar_run(V, 0, a)["cur_tok"], scalar_run(V, 0, b)["cur_tok"]) for V in (66, 8194)), (a, b)
