"""Shared by test_token_choice_api.py (no GPU) and test_gpu_beam_step.py / test_gpu_typical_filter.py / test_gpu_sampler_step.py: what
one launch of the token-choice kernels has to leave behind, stated in numpy fp64 from the fp32 inputs.  No code is shared with the
kernels; the warped rows and draws come from wide_beam_ref.py, the hypothesis bookkeeping from oracle/hf_beam.py BeamSearchScorer
(pinned to transformers by test_beam_scorer_vs_transformers.py).  Nothing here is tuned to what the kernels return.

Tolerances, in units of U = 2^-24 (every fp32 operation rounds by at most U of its result; expf / logf deliver within 2 U).
DELTA_N, the top-p boundary and the draws of the narrow pair (beam_cand_kernel / beam_select_kernel, sampler_sample_kernel).  Z is a
sequential sum of <= 128 exponentials: relative error (127 + 2) U.  A quotient e / Z adds one rounding: 130 U relative.  The tail
is a sequential sum of <= 127 quotients, each addition rounding by U of a partial sum <= 1: the tail mass is off by at most
(130 + 127) U.  The draw compares a prefix sum over <= 10 * 128 live candidates with u * total: both are sequential sums of <= 1280
terms, relative error (1279 + 3) U each.  delta_n(n) = U * the next power of two >= 2 * n + 8 (n = 128 for the tail, nb * 128 for the
draws), the margin wide_beam_ref.delta_b takes.
TYPICAL_D / TYPICAL_E: typical_bounds below."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_beam_ref as W  # noqa: E402

from oracle import hf_beam  # noqa: E402

F32 = np.float32
U = 2.0 ** -24
CAND = 128  # BEAM_MAX_CAND


def delta_n(n=CAND):
    c, p = 2 * n + 8, 1
    while p < c:
        p <<= 1
    return p * U


class NarrowRow(W.Row):
    """wide_beam_ref.Row with the narrow kernels' cap: of the scores >= the k-th largest only the first 128 in (score descending,
    id ascending) order go on to top-p (oracle/hf_beam.py warp_row `[:128]`)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        min_keep = kw.get("min_keep", 2)
        self.n_ties = self.n  # before the cap
        if self.n > CAND:
            n = CAND
            self.order, self.n = self.order[:n], n
            e = np.exp(self.ss[:n] - self.ss[0])
            c = np.cumsum(e)
            self.tail = (c[-1] - np.concatenate([[0.0], c[:-1]])) / c[-1]
            delta = a[9] if len(a) > 9 else kw["delta"]
            top_p = a[7] if len(a) > 7 else kw["top_p"]

            def count(t):
                return min(max(int((self.tail > t).sum()), min_keep), n)

            if top_p >= 1.0:
                self.R = self.R_lo = self.R_hi = n
            else:
                self.R, self.R_lo, self.R_hi = count(self.thr), count(self.thr + delta), count(self.thr - delta)


# ---------------------------------------------------------------------------------------------------------------------------
# beam step: the caller-owned state as numpy arrays and what one call makes of it
# ---------------------------------------------------------------------------------------------------------------------------
SENT_I = -0x5A5A5A5B  # what unwritten int32 / float / byte cells hold
SENT_F = F32(-7.25e30)
SENT_B = 0xA5


class CountingHyps(hf_beam.BeamHypotheses):
    """BeamHypotheses that also counts its insertions (the device keeps that counter as the insertion order of its slots)."""
    added = 0

    def add(self, hyp, sum_logprobs, generated_len):
        score = sum_logprobs / (generated_len ** self.length_penalty)
        if len(self) < self.num_beams or score > self.worst_score:
            self.added += 1
        super().add(hyp, sum_logprobs, generated_len)


def new_scorer(items, nb, length_penalty):
    sc = hf_beam.BeamSearchScorer(items, nb, length_penalty=length_penalty)
    sc.hyps = [CountingHyps(nb, length_penalty) for _ in range(items)]
    return sc


def new_state(items, nb, max_gen, Smax, k, D=0, beam_scores=None, hist=None, anc=None):
    """A generation at step k (every row k tokens long): sentinels everywhere a generation would not have written."""
    rows = items * nb
    st = dict(
        len=np.full(rows, k, np.int32), cur_tok=np.full(rows, SENT_I, np.int32), unfinished=np.ones(rows, np.int32),
        ids=np.full((2, rows, max_gen), SENT_I, np.int32), anc=np.full((2, rows, Smax), SENT_B, np.uint8),
        beam_scores=np.zeros(rows, F32) if beam_scores is None else np.asarray(beam_scores, F32).copy(),
        hyp_tok=np.full((items, nb + 1, max_gen), SENT_I, np.int32), hyp_score=np.full((items, nb + 1), SENT_F, F32),
        hyp_len=np.full((items, nb + 1), SENT_I, np.int32), hyp_order=np.full((items, nb + 1), -1, np.int32),
        hyp_n=np.zeros(items, np.int32), hyp_worst=np.full(items, 1e9, F32), hyp_counter=np.zeros(items, np.int32),
        done=np.zeros(items, np.int32), h_next=np.full((rows, max(D, 1)), SENT_F, F32))
    par = k & 1
    if hist is not None:
        st["ids"][par, :, :k] = np.asarray(hist)[:, :k]
    if anc is not None:
        st["anc"][par] = anc
    return st


def ref_step(st, cfg, picks, scorer):
    """One call.  cfg: items, nb, max_gen, Smax, stop, input_n, forced (int32 [rows, max_gen] or None), prefix0, D, pos_rows, emb, pos
    (fp32 arrays holding the tables' values, or None).  picks: (score f32, tok, beam) [items, 2 nb] in draw order (ignored on a given
    step and for done items).  -> the expected state; the hypotheses live in `scorer` (compare with hyps_of)."""
    items, nb, mg, Smax, stop = cfg["items"], cfg["nb"], cfg["max_gen"], cfg["Smax"], cfg["stop"]
    rows = items * nb
    out = {k: v.copy() for k, v in st.items()}
    k = int(st["len"][0])
    assert (st["len"] == k).all()
    if k >= mg:
        return out
    par = k & 1
    ids_old, anc_old = st["ids"][par], st["anc"][par]
    forced, input_n = cfg.get("forced"), cfg.get("input_n", 0)
    own = np.arange(rows)
    was_done = st["done"].astype(bool)
    if forced is not None and k < input_n:
        tok, src, score, done = forced[:, k].astype(np.int64), own, st["beam_scores"].copy(), was_done.copy()
    else:
        assert [bool(x) for x in was_done] == [bool(x) for x in scorer.done]
        psc, ptok, pbeam = (np.asarray(x) for x in picks)
        order = np.stack([np.argsort(-psc[b].astype(np.float64), kind="stable") for b in range(items)])  # torch.sort, stable
        take = lambda x: np.take_along_axis(x, order, 1)  # noqa: E731
        score, tok, src = scorer.process(ids_old[:, :k], take(psc).astype(F32), take(ptok), take(pbeam), stop, stop, input_n)
        done = np.asarray(scorer.done, dtype=bool)
        for b in np.nonzero(was_done)[0]:  # the kernel keeps a done item's rows where they are (HF points them at row 0)
            src[b * nb:(b + 1) * nb] = own[b * nb:(b + 1) * nb]
        for b in np.nonzero(~was_done)[0]:
            h = scorer.hyps[b]
            out["hyp_n"][b], out["hyp_worst"][b], out["hyp_counter"][b] = len(h), F32(h.worst_score), h.added
        out["done"] = done.astype(np.int32)
    ids_new, anc_new = out["ids"][par ^ 1], out["anc"][par ^ 1]
    pos_next = cfg.get("prefix0", 0) + k + 1
    for dst in range(rows):
        ids_new[dst, :k] = ids_old[src[dst], :k]
        ids_new[dst, k] = tok[dst]
        anc_new[dst] = anc_old[src[dst]]
        if pos_next < Smax:
            anc_new[dst, pos_next] = dst % nb
    out["cur_tok"] = tok.astype(np.int32)
    out["len"][:] = k + 1
    out["beam_scores"] = np.asarray(score, F32)
    out["unfinished"] = (~np.repeat(done, nb)).astype(np.int32)
    if cfg.get("D", 0) and cfg.get("emb") is not None:
        pp = min(k + 1 if k < input_n else k + 2, cfg["pos_rows"] - 1)
        out["h_next"] = (cfg["emb"][tok].astype(F32) + cfg["pos"][pp].astype(F32)[None]).astype(F32)
    return out


def hyps_of(st, b):
    """The device's live hypotheses of item b in insertion order: [(score, tokens)]."""
    live = [q for q in np.argsort(st["hyp_order"][b], kind="stable") if st["hyp_order"][b, q] >= 0]
    return [(st["hyp_score"][b, q], st["hyp_tok"][b, q, :st["hyp_len"][b, q]].copy(), int(st["hyp_len"][b, q])) for q in live]


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


# ---------------------------------------------------------------------------------------------------------------------------
# typical filter
# ---------------------------------------------------------------------------------------------------------------------------
def typical_bounds(V, maglse, nlmax, H, first=None):
    """(d, e): how far the kernel's running mass / its sort keys can lie from the fp64 ones, from its summation structure.
    se = sum expf(s - mx): <= ceil(V / 1024) strided terms per thread, 6 butterfly levels, 16 wave sums: n_se additions, the terms
    within 3 U (the subtraction, expf): relative (n_se + 3) U = the absolute error of log se; logf 2 U |log se|, mx + log se U |lse|:
    d_lse = n_se + 3 + 3 maglse.  A normalised log-prob nl = s - lse rounds at |nl|: d_nl = d_lse + nlmax, nlmax over the ranks that
    can decide (those before the mass point: a token far behind it has a key far above the threshold).  p = expf(nl): relative
    d_nl + 2.  The running mass: a run of <= 16, 6 levels of the wave scan, <= 15 wave sums, the join, <= 16 along the run again = 53
    additions, each rounding by U of a partial mass <= 1: d = 53 + d_nl + 2.  The entropy sum_i nl_i p_i: every term relative
    (d_nl / |nl| + d_nl + 3), summed over i: d_nl (1 + H) + 3 H, the n_se additions U H each.  A key |(-nl) - H| adds the two errors and
    one rounding at |nl| + H: e = d_nl (2 + H) + H (n_se + 3) + nlmax + H.
    first = (maglse0, nlmax0) under log_softmax_first: the scores the filter starts from are themselves lg - lse0 in fp32, off by
    d_lse(maglse0) + nlmax0 (nlmax0 over the deciding ranks again), which adds to d_nl and bounds the kept values.  A seen token's
    error is max(penalty, 1) times that; typical_ref asserts that no seen token comes within that of the threshold band, so it
    decides nothing (its mass is exp(penalty * log p))."""
    n_se = -(-V // 1024) + 6 + 16
    d_in = 0.0
    if first is not None:
        mag0, nl0 = first
        d_in = n_se + 3 + 3 * mag0 + 2 * nl0
    d_nl = n_se + 3 + 3 * maglse + nlmax + d_in
    d = 53 + d_nl + 2
    e = d_nl * (2 + H) + H * (n_se + 3) + nlmax + H
    return d * U, e * U, d_in * U


def processed32(lg, seen, penalty, stop, suppress):
    """The fp32 processed scores without log_softmax_first: one IEEE operation per element, so these are the kernel's bits."""
    v = np.asarray(lg, F32).copy()
    if float(penalty) != 1.0:
        with np.errstate(invalid="ignore"):
            v = np.where(seen, np.where(v < 0, v * F32(penalty), v / F32(penalty)), v).astype(F32)
    if suppress:
        v[stop] = -np.inf
    return v


def typical_ref(lg, seen, penalty, stop, suppress, lsf, mass, min_keep):
    """fp64 side of one row -> dict(s: processed scores fp64, must / may: bool [V], last_lo, last_hi, d, e, d_in, kept64)."""
    lg = np.asarray(lg, F32)
    V = lg.shape[0]
    first = None
    if lsf:
        x = lg.astype(np.float64)
        mx = x.max()
        lse0 = mx + np.log(np.exp(x - mx).sum())
        s = x - lse0
        pre = s.copy()
        if float(penalty) != 1.0:
            p32 = float(F32(penalty))
            s = np.where(seen, np.where(s < 0, s * p32, s / p32), s)
        if suppress:
            s[stop] = -np.inf
    else:
        s = processed32(lg, seen, penalty, stop, suppress).astype(np.float64)
    fin = s > -np.inf
    mx = s[fin].max()
    lse = mx + np.log(np.exp(s[fin] - mx).sum())
    nl = np.where(fin, s - lse, -np.inf)
    p = np.where(fin, np.exp(nl), 0.0)
    H = float(-(p[fin] * nl[fin]).sum())
    key = np.where(fin, np.abs(-nl - H), np.inf)
    order = np.lexsort((np.arange(V), key))
    ks, cum = key[order], np.cumsum(p[order])
    wide = min(int((cum < mass + 0.01).sum()), V - 1)  # the ranks that can decide, generously
    nlmax = float(np.abs(nl[order[:wide + 1]]).max())
    if lsf:
        first = (abs(lse0), float(np.abs(pre[order[:wide + 1]]).max()))
    d, e, d_in = typical_bounds(V, abs(lse), nlmax, H, first)
    last_lo, last_hi = min(int((cum < mass - d).sum()), V - 1), min(int((cum < mass + d).sum()), V - 1)
    must, may = key < ks[last_lo] - e, key <= ks[last_hi] + e
    if min_keep > 1:  # the first min_keep ranks stay whatever the mass says
        may |= key <= ks[min_keep - 1] + 2 * e
        must[[t for t in order[:min_keep] if int((key <= key[t] + 2 * e).sum()) <= min_keep]] = True  # ranks no error can move
    may &= fin
    clear = True
    if lsf and float(penalty) != 1.0:  # a seen token's score carries penalty times the first stage's error: it must decide nothing
        sk, w = key[seen & fin], max(float(penalty), 1.0) * d_in * (2 + H)
        clear = bool(((sk - w > ks[last_hi] + e) | (sk + w < ks[last_lo] - e)).all())
    last = min(int((cum < mass).sum()), V - 1)
    kept64 = key <= ks[last]
    kept64[order[:min_keep]] = True
    return dict(s=s, must=must, may=may, last_lo=last_lo, last_hi=last_hi, d=d, e=e, d_in=d_in, kept64=kept64 & fin, H=H, clear=clear)


TYP_VOCABS = [66, 1023, 1025, 2049, 8194, 16384]
TYP_MASSES = [0.2, 0.7, 0.9]
TYP_ROWS = ["flat", "mid", "wide", "holes", "peaked"]  # std 0.3 / 1.0 / 2.0, std 1.0 with -inf inputs and the stop suppressed, one token 0.97
TYP_STD = {"flat": 0.3, "mid": 1.0, "wide": 2.0, "holes": 1.0, "peaked": 1.0}
TYP_K = 37  # history length of the beam-history source (odd: plane 1)
BAND_RANKS, BAND_TOKENS = 1, 4


def typical_rows(V, source, mass, min_keep):
    """One launch: logits [5, V], seen bool [5, V], hist int32 [5, TYP_K], refs.  source "map" (byte map, no log_softmax) or "beams"
    (id histories + fake_id 1 + start V - 3, log_softmax first).  A row whose ambiguous band is wider than the cap FOR THE REFERENCE
    ALONE takes the next input stream (never skipped); the stream used is part of the case."""
    from itts_hip import prng

    lsf = source == "beams"
    stop, start, fake = V - 2, V - 3, 1
    lgs, seens, hists, refs, salts = [], [], [], [], []
    for r, kind in enumerate(TYP_ROWS):
        for salt in range(32):
            tag = f"typical.{source}.{kind}.{salt}"
            lg = W.gaussian(tag, V, (V,), TYP_STD[kind])
            if kind == "peaked":
                lg[V // 3] = F32(np.log(0.97 / 0.03 * np.exp(lg.astype(np.float64)).sum()))
            if kind == "holes":
                lg[prng.randint(tag + ".h", V, max(V // 8, 1), 0, V)] = -np.inf
            hist = prng.randint(tag + ".seen", V, TYP_K, 0, V).astype(np.int32)
            if kind != "peaked":
                hist[:3] = np.argsort(lg)[-3:]  # the row's best tokens are among the seen ones
            if kind == "peaked":
                hist[hist == V // 3] = fake
            seen = np.zeros(V, bool)
            seen[hist] = True
            if lsf:
                seen[[fake, start]] = True
            ref = typical_ref(lg, seen, 10.0, stop, kind == "holes", lsf, mass, min_keep)
            if ref["clear"] and ref["last_hi"] - ref["last_lo"] <= BAND_RANKS and int(ref["may"].sum()) - int(ref["must"].sum()) <= BAND_TOKENS:
                break
        else:
            raise AssertionError(("no input stream within the band cap", V, source, mass, min_keep, kind))
        lgs.append(lg), seens.append(seen), hists.append(hist), refs.append(ref), salts.append(salt)
    return dict(logits=np.stack(lgs), seen=np.stack(seens), hist=np.stack(hists), refs=refs, salts=salts, stop=stop, start=start,
                fake=fake, lsf=int(lsf), penalty=10.0)


# ---------------------------------------------------------------------------------------------------------------------------
# one-beam samplers
# ---------------------------------------------------------------------------------------------------------------------------
def greedy_ref(lg, seen, penalty, stop, suppress, preprocessed=False):
    """Arg-max of the processed scores, the lowest id among equals, id 0 when nothing is finite (sampler2_kernel starts from
    (-inf, no id) and a score has to be larger - or equal with a lower id - to take over: -inf == -inf hands id 0 the row)."""
    v = np.asarray(lg, F32) if preprocessed else processed32(lg, seen, penalty, stop, suppress)
    return int(np.argmax(v.astype(np.float64)))  # numpy: the first of equal maxima


def commit_ref(st, cfg, choice):
    """sampler_commit + sampler_next_embedding for every row.  st: seen uint8 [B, V], ids [B, max_gen], cur_tok, unfinished, step [B],
    h_next [B, D]; cfg: V, max_gen, stop, forced, input_n, D, pos_rows, emb, pos."""
    out = {k: v.copy() for k, v in st.items()}
    for b in range(st["step"].shape[0]):
        k = int(st["step"][b])
        if k >= cfg["max_gen"]:
            continue
        c = int(choice[b])
        if cfg.get("forced") is not None and cfg["forced"][b, k] >= 0:
            c = int(cfg["forced"][b, k])
        tok = c if st["unfinished"][b] else cfg["stop"]
        tok = min(max(tok, 0), cfg["V"] - 1)
        out["ids"][b, k] = out["cur_tok"][b] = tok
        out["seen"][b, tok] = 1
        out["unfinished"][b] = int(bool(st["unfinished"][b]) and tok != cfg["stop"])
        out["step"][b] = k + 1
        if cfg.get("D", 0) and cfg.get("emb") is not None:
            pp = min(k + 1 if k < cfg.get("input_n", 0) else k + 2, cfg["pos_rows"] - 1)
            out["h_next"][b] = (cfg["emb"][tok].astype(F32) + cfg["pos"][pp].astype(F32)).astype(F32)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# device memory with guard blocks (the GPU tests)
# ---------------------------------------------------------------------------------------------------------------------------
GUARD_BYTES, GUARD_FILL = 256, 0xC3


class DevArrays:
    """numpy arrays copied to the device, each between two guard blocks that no kernel may touch."""

    def __init__(self, dev="cuda:0"):
        self.dev, self.t = dev, {}

    def put(self, name, arr):
        import torch

        a = np.ascontiguousarray(arr)
        raw = a.reshape(-1).view(np.uint8)
        buf = np.full(raw.size + 2 * GUARD_BYTES, GUARD_FILL, np.uint8)
        buf[GUARD_BYTES:GUARD_BYTES + raw.size] = raw
        t = torch.from_numpy(buf).to(self.dev)
        self.t[name] = (t, a.dtype, a.shape)
        return t.data_ptr() + GUARD_BYTES

    def ptr(self, name):
        return self.t[name][0].data_ptr() + GUARD_BYTES

    def get(self, name):
        t, dtype, shape = self.t[name]
        buf = t.cpu().numpy()
        assert (buf[:GUARD_BYTES] == GUARD_FILL).all() and (buf[-GUARD_BYTES:] == GUARD_FILL).all(), f"guard block of {name} overwritten"
        return buf[GUARD_BYTES:-GUARD_BYTES].view(dtype).reshape(shape).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))
