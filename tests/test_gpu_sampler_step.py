"""GPU: one launch of the one-beam samplers (csrc/decode_sampler.hip sampler2_kernel - greedy - and sampler_sample_kernel - 1 <= top_k
<= 128) with the fused commit and next-step embedding (csrc/itts_sampler_dev.h), through itts_sampler_step on caller-owned state.
Greedy: the arg-max of the fp32 processed scores (one IEEE operation per element, so numpy has the kernel's bits), the lowest id
among equals.  Sampling: oracle/gpt.py sample_pick, as the existing tests of itts_sample_rows.  The bookkeeping:
token_choice_ref.commit_ref, the whole state compared after every launch, every array between guard blocks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import token_choice_ref as T  # noqa: E402
import wide_beam_ref as W  # noqa: E402

from itts_hip import lib, prng  # noqa: E402
from oracle import gpt as ogpt  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
STATE = ("seen", "ids", "cur_tok", "unfinished", "step", "h_next")


def new_state(B, V, max_gen, D=0, step=None, unfinished=None, seen=None):
    return dict(seen=np.zeros((B, V), np.uint8) if seen is None else seen.astype(np.uint8), ids=np.full((B, max_gen), T.SENT_I, np.int32),
                cur_tok=np.full(B, T.SENT_I, np.int32), unfinished=np.ones(B, np.int32) if unfinished is None else np.asarray(unfinished, np.int32),
                step=np.zeros(B, np.int32) if step is None else np.asarray(step, np.int32), h_next=np.full((B, max(D, 1)), T.SENT_F, F32))


def run_sampler(st, cfg, logits, uniforms=None, expect=0):
    l = lib.load()
    d = T.DevArrays(DEV)
    a = lib.SamplerStepArgs()
    for name in STATE:
        setattr(a, name, d.put(name, st[name]))
    if not cfg.get("D"):
        a.h_next = None
    a.logits = d.put("logits", logits)
    a.B, a.V, a.max_gen, a.stop = logits.shape[0], logits.shape[1], cfg["max_gen"], cfg["stop"]
    a.suppress_stop, a.preprocessed, a.penalty = cfg.get("suppress", 0), cfg.get("pre", 0), cfg.get("penalty", 10.0)
    a.do_sample, a.top_k, a.top_p, a.temperature = cfg.get("do_sample", 0), cfg.get("top_k", 0), cfg.get("top_p", 1.0), cfg.get("temperature", 1.0)
    a.input_n = cfg.get("input_n", 0)
    if cfg.get("forced") is not None:
        a.forced = d.put("forced", cfg["forced"].astype(np.int32))
    if uniforms is not None:
        a.uniforms = d.put("uniforms", np.ascontiguousarray(uniforms, F32))
    if cfg.get("D"):
        a.D, a.pos_rows, a.emb_bf16 = cfg["D"], cfg["pos_rows"], int(bool(cfg.get("emb_bf16")))
        for name in ("emb", "pos"):
            raw = torch.from_numpy(cfg[name]).to(torch.bfloat16).view(torch.int16).numpy() if cfg.get("emb_bf16") else cfg[name]
            setattr(a, name, d.put(name, raw))
    torch.cuda.synchronize()
    status = l.itts_sampler_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == expect, (status, l.itts_last_error())
    got = {name: d.get(name) for name in STATE}
    for name in d.t:
        if name not in STATE:
            d.get(name)  # guard blocks of the inputs
    assert T.same_bits(d.get("logits"), logits)
    return got


def same_state(got, want, D):
    for name in STATE:
        if name == "h_next" and not D:
            continue
        assert T.same_bits(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:6])


GREEDY_ROWS = ["plain", "tie_vec_tail", "tie_in_vector", "tie_thread", "tie_lanes", "tie_waves", "all_inf", "stop_best", "pen_pos", "pen_neg", "pen_zero"]


def greedy_case(V):
    """logits [11, V], seen [11, V]: one scenario per row (ids beyond V - 1 are dropped: the small vocabularies keep what fits)."""
    B = len(GREEDY_ROWS)
    lg = (W.gaussian("sampler_step.greedy", V, (B, V), 1.0) - F32(4.0)).astype(F32)  # every background logit below the planted ones
    lg = np.minimum(lg, F32(-0.5))
    seen = np.zeros((B, V), bool)
    nvec8 = (V >> 3) * 8
    put = lambda r, ids, val: lg.__setitem__((r, [i for i in ids if 0 <= i < V]), F32(val))  # noqa: E731
    r = GREEDY_ROWS.index
    put(r("tie_vec_tail"), [nvec8 - 1, nvec8, V - 1], 3.0)     # the last vector element, the first tail element, the last id
    put(r("tie_in_vector"), [2, 5], 3.0)                        # one thread, one 8-vector
    put(r("tie_thread"), [8 * 3 + 1, 8 * (3 + 1024) + 1, nvec8 + 3], 3.0)  # thread 3: its first chunk, its second chunk, its tail id
    put(r("tie_lanes"), [8 * 9 + 4, 8 * 17 + 4, 8 * 40], 3.0)   # lanes 9, 17, 40 of wave 0
    put(r("tie_waves"), [512 * 15 + 6, 512 * 7 + 6, 512 * 2 + 6, 70], 3.0)  # waves 15, 7, 2, 1 (id 70: lane 8 of wave 0 -> the lowest)
    lg[r("all_inf")] = -np.inf
    stop = V - 2
    lg[r("stop_best"), stop] = 3.0
    lg[r("stop_best"), 1] = 2.0
    a, d_ = 3, 4
    lg[r("pen_pos"), a], lg[r("pen_pos"), d_] = 5.0, 0.6       # seen 5.0 / 10 = 0.5 loses to the unseen 0.6
    seen[r("pen_pos"), a] = True
    lg[r("pen_neg"), :] = np.minimum(lg[r("pen_neg")], F32(-1.0))
    lg[r("pen_neg"), a], lg[r("pen_neg"), d_] = -0.01, -0.05    # seen -0.01 * 10 = -0.1 loses to the unseen -0.05
    seen[r("pen_neg"), a] = True
    lg[r("pen_zero"), a], lg[r("pen_zero"), d_] = 0.0, 0.0      # a seen zero stays zero: ties with the unseen zero, the lower id wins
    seen[r("pen_zero"), a] = True
    return lg, seen, stop


@pytest.mark.parametrize("suppress", (0, 1))
@pytest.mark.parametrize("V", (7, 8, 66, 8191, 8194, 16390))
def test_greedy_argmax(V, suppress):
    lg, seen, stop = greedy_case(V)
    B = lg.shape[0]
    cfg = dict(max_gen=3, stop=stop, suppress=suppress, penalty=10.0)
    st = new_state(B, V, 3, seen=seen)
    choice = [T.greedy_ref(lg[b], seen[b], 10.0, stop, suppress) for b in range(B)]
    got = run_sampler(st, cfg, lg)
    same_state(got, T.commit_ref(st, dict(cfg, V=V), choice), 0)
    r = GREEDY_ROWS.index
    assert got["cur_tok"][r("all_inf")] == 0
    assert got["cur_tok"][r("stop_best")] == (1 if suppress else stop) and got["unfinished"][r("stop_best")] == (1 if suppress else 0)
    assert got["cur_tok"][r("pen_pos")] == 4 and got["cur_tok"][r("pen_neg")] == 4 and got["cur_tok"][r("pen_zero")] == 3
    if V > 8:
        assert got["cur_tok"][r("tie_in_vector")] == 2 and got["cur_tok"][r("tie_thread")] == 25
    if V > 8000:
        assert got["cur_tok"][r("tie_waves")] == 70 and got["cur_tok"][r("tie_lanes")] == 76


def bookkeeping_case(V, max_gen, D, bf16, seed):
    """Six rows: step 0 | step 3, forced -1 there | the last step (position clamp) | past the end (writes nothing) | finished | forced >= 0."""
    B = 6
    lg = W.gaussian(f"sampler_step.book.{seed}", V, (B, V), 2.0)
    seen = np.zeros((B, V), bool)
    for b in range(B):
        seen[b, prng.randint(f"sampler_step.book.seen{b}", V, 20, 0, V)] = True
        seen[b, np.argsort(lg[b])[-2:]] = True
    forced = np.full((B, max_gen), -1, np.int32)
    forced[5, 1] = 17
    forced[0, 0] = 9  # an `input_tokens` step (input_n = 1): the given token is fed at position k + 1
    cfg = dict(V=V, max_gen=max_gen, stop=V - 2, penalty=10.0, forced=forced, input_n=1, D=D, pos_rows=max_gen + 1, emb_bf16=bf16)
    if D:
        emb = prng.uniform(f"sampler_step.emb.{seed}", V, V * D).reshape(V, D)
        pos = prng.uniform(f"sampler_step.pos.{seed}", V, cfg["pos_rows"] * D).reshape(cfg["pos_rows"], D)
        if bf16:
            emb, pos = (torch.from_numpy(x).to(torch.bfloat16).float().numpy() for x in (emb, pos))
        cfg["emb"], cfg["pos"] = emb, pos
    st = new_state(B, V, max_gen, D, step=[0, 3, max_gen - 1, max_gen, 2, 1], unfinished=[1, 1, 1, 1, 0, 1], seen=seen)
    return lg, cfg, st


@pytest.mark.parametrize("kernel", ("greedy", "narrow"))
@pytest.mark.parametrize("D,bf16", ((96, 0), (1280, 1)))
def test_bookkeeping(kernel, D, bf16):
    V, max_gen = 8194, 5
    lg, cfg, st = bookkeeping_case(V, max_gen, D, bf16, kernel)
    B = lg.shape[0]
    u = (prng.uniform("sampler_step.book.u", 1, max_gen * B) * F32(0.5) + F32(0.5)).reshape(max_gen, B).astype(F32)
    if kernel == "narrow":
        cfg.update(do_sample=1, top_k=30, top_p=0.8, temperature=0.9)
        choice = [ogpt.sample_pick(T.processed32(lg[b], st["seen"][b].astype(bool), 10.0, cfg["stop"], 0), 30, 0.8, 0.9,
                                   float(u[min(int(st["step"][b]), max_gen - 1), b])) for b in range(B)]
        # the row index of the uniforms matters: another row of the table gives another token somewhere
        other = [ogpt.sample_pick(T.processed32(lg[b], st["seen"][b].astype(bool), 10.0, cfg["stop"], 0), 30, 0.8, 0.9, float(u[0, b])) for b in range(B)]
        assert other[1:3] != choice[1:3]
    else:
        choice = [T.greedy_ref(lg[b], st["seen"][b].astype(bool), 10.0, cfg["stop"], 0) for b in range(B)]
    got = run_sampler(st, cfg, lg, u if kernel == "narrow" else None)
    want = T.commit_ref(st, cfg, choice)
    same_state(got, want, D)
    assert got["cur_tok"][0] == 9 and got["cur_tok"][5] == 17 and got["cur_tok"][4] == cfg["stop"] and got["unfinished"][4] == 0
    assert got["cur_tok"][1] == choice[1] and got["step"][3] == max_gen and got["cur_tok"][3] == T.SENT_I
    assert T.same_bits(got["h_next"][3], st["h_next"][3])  # past the end: no embedding either
    assert T.same_bits(got["h_next"][0], (cfg["emb"][9] + cfg["pos"][1]).astype(F32))  # given token 0 at position 1
    assert T.same_bits(got["h_next"][2], (cfg["emb"][got["cur_tok"][2]] + cfg["pos"][max_gen]).astype(F32))  # k + 2 = 6 clamped to pos_rows - 1 = 5


@pytest.mark.parametrize("kernel", ("greedy", "narrow"))
def test_three_steps_follow_the_written_history(kernel):
    """The same logits three times: the repetition penalty follows the tokens the launches before wrote into `seen`."""
    V, max_gen, B = 1025, 4, 3
    lg = (W.gaussian("sampler_step.seq", V, (B, V), 1.0) + F32(3.0)).astype(F32)
    cfg = dict(V=V, max_gen=max_gen, stop=V - 2, penalty=10.0)
    u = (prng.uniform("sampler_step.seq.u", 2, max_gen * B) * F32(0.5) + F32(0.5)).reshape(max_gen, B).astype(F32)
    if kernel == "narrow":
        cfg.update(do_sample=1, top_k=2, top_p=1.0, temperature=1.0)
    st = new_state(B, V, max_gen)
    toks = []
    for k in range(3):
        proc = [T.processed32(lg[b], st["seen"][b].astype(bool), 10.0, cfg["stop"], 0) for b in range(B)]
        choice = [ogpt.sample_pick(proc[b], 2, 1.0, 1.0, float(u[k, b])) if kernel == "narrow" else int(np.argmax(proc[b])) for b in range(B)]
        got = run_sampler(st, cfg, lg, u if kernel == "narrow" else None)
        same_state(got, T.commit_ref(st, cfg, choice), 0)
        st = got
        toks.append(list(got["cur_tok"]))
    if kernel == "greedy":  # positive logits: a seen token drops to a tenth, so three different tokens per row
        assert all(len({toks[k][b] for k in range(3)}) == 3 for b in range(B))


def test_narrow_sampling_at_its_largest_vocabulary():
    V, B, max_gen = 15360, 3, 2
    lg = W.gaussian("sampler_step.v15360", V, (B, V), 2.5)
    seen = np.zeros((B, V), bool)
    for b in range(B):
        seen[b, np.argsort(lg[b])[-3:]] = True
    u = np.array([[0.0, 0.37, W.U_TOP], [0.5, 0.5, 0.5]], F32)
    for top_k, top_p, temp in ((30, 0.8, 0.9), (128, 1.0, 1.0), (1, 0.5, 1.3)):
        cfg = dict(V=V, max_gen=max_gen, stop=V - 2, penalty=10.0, do_sample=1, top_k=top_k, top_p=top_p, temperature=temp)
        st = new_state(B, V, max_gen, seen=seen)
        choice = [ogpt.sample_pick(T.processed32(lg[b], seen[b], 10.0, V - 2, 0), top_k, top_p, temp, float(u[0, b])) for b in range(B)]
        same_state(run_sampler(st, cfg, lg, u), T.commit_ref(st, cfg, choice), 0)


def test_overflow_of_the_candidates_is_deterministic():
    """More than 128 scores tie with the top_k-th: sampler_sample_kernel keeps the strictly larger ones and the ties of lowest id."""
    V = 8194
    lg = np.zeros((2, V), F32)
    lg[0, 8000] = 2.0                                     # one larger score at a high id, top_k 30: it must be rank 0
    big = 8193 - 61 * np.arange(127)
    tie = np.setdiff1d(17 + 160 * np.arange(51), big)[:50]
    assert tie.size == 50 and tie[0] == 17
    lg[1] = -30.0
    lg[1, big], lg[1, tie] = 9.0, 0.5                     # 127 larger scores + 50 ties at top_k 128
    for top_k, u_row in ((30, [0.0, 0.0]), (128, [0.0, W.U_TOP])):
        cfg = dict(V=V, max_gen=1, stop=V - 2, penalty=1.0, do_sample=1, top_k=top_k, top_p=1.0, temperature=1.0)
        st = new_state(2, V, 1)
        runs = [run_sampler(st, cfg, lg, np.array([u_row], F32)) for _ in range(3)]
        for got in runs[1:]:
            same_state(got, runs[0], 0)
        if top_k == 30:
            assert runs[0]["cur_tok"][0] == 8000  # u = 0: the best token, which the arrival-order gather could lose
        else:
            assert runs[0]["cur_tok"][1] == 17    # u just below 1: the last kept rank is the tie of lowest id, behind the 127
