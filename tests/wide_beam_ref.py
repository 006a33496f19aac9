"""Shared by test_wide_beam_host.py and test_gpu_wide_beam.py: what the whole-vocabulary beam sampler (csrc/beam.hip
beam_wide_cand_kernel + beam_wide_pick_kernel) has to satisfy, stated in fp64 from the fp32 inputs, and an fp32 numpy emulation
of the two kernels' summation structure.  Nothing here is tuned to what the kernels return.

Tolerances.
DELTA_B.  The longest chain of dependent fp32 additions behind any sum of the two kernels is chain(V, nb) = L + 6 + 15 + 1 + L
with L = ceil(nb * V / 1024) (beam_wide_pick_kernel's header: a run's own sum, the wave scan, the other waves' sums, the join,
along the run again; beam_wide_cand_kernel's 53 is never longer).  Every addition rounds by at most 2^-24 of the partial mass,
expf delivers its terms within an ulp and the comparison is with a quotient: delta_b = 2^-24 * the next power of two >=
chain + 8, the margin the one-beam predicate (wide_sampler_ref.py) took.  512 * 2^-24 at 10 beams x 16384 tokens.
SCORE_TOL.  A pick's score is log_softmax -> penalty -> / temperature -> + beam score in fp32.  se = sum expf(lg - mx) goes
through n_se = ceil(V / 1024) + 6 + 16 additions of terms that carry the rounding of lg - mx and expf's ulp: (n_se + 3) * 2^-24
relative, which is the absolute error of log(se); logf adds 2 * 2^-24 * |log se|, the sum mx + log(se) 2^-24 * |lse|, lg - lse
2^-24 * |v|; the penalty product and the temperature quotient scale all of that by penalty / temperature and add one rounding of
the result each; the beam-score add one rounding of the sum.  With mag a bound on |lse|, on |lg - lse| and on |beam score| that
the caller takes from the fp64 reference: score_tol = 2^-24 * (max(penalty, 1) / temperature * (n_se + 3 + 6 * mag) + 2 * mag)."""
import numpy as np

F32 = np.float32
NINF = F32(-np.inf)
U = 2.0 ** -24


def chain(V, nb):
    L = -(-nb * V // 1024)
    return L + 6 + 15 + 1 + L


def delta_b(V, nb):
    c, p = chain(V, nb) + 8, 1
    while p < c:
        p <<= 1
    return p * U


def score_tol(V, penalty, temperature, mag):
    n_se = -(-V // 1024) + 6 + 16
    return U * (max(float(penalty), 1.0) / float(temperature) * (n_se + 3 + 6.0 * mag) + 2.0 * mag)


class Row:
    """fp64 side of one beam row - infer_core.host_distribution(log_softmax_first=True, min_keep=2) restated: warped scores by
    token, ranks by (score descending, id ascending) over the finite ones, HF's tie-keeping TopK, tail masses, and the admissible
    range [R_lo, R_hi] of the kept count with the top-p threshold moved by -/+ delta.  min_keep / ties_desc exist for the broken
    samplers of test_wide_beam_host.py."""

    def __init__(self, logits, seen_ids, penalty, stop, suppress_stop, preprocessed, top_k, top_p, temperature, delta,
                 min_keep=2, ties_desc=False):
        lg = np.asarray(logits, dtype=F32).astype(np.float64)
        V = lg.shape[0]
        self.lse = 0.0
        if not preprocessed:
            mx = lg.max()
            self.lse = mx + np.log(np.exp(lg - mx).sum())
            s = lg - self.lse
            self.logp = s.copy()
            ids = np.fromiter(seen_ids, dtype=np.int64)
            ids = ids[(ids >= 0) & (ids < V)]
            if float(penalty) != 1.0 and ids.size:
                p = float(F32(penalty))
                s[ids] = np.where(s[ids] < 0, s[ids] * p, s[ids] / p)
            if suppress_stop:
                s[stop] = -np.inf
        else:
            s = lg.copy()
            self.logp = s.copy()
        if float(temperature) != 1.0:
            s = s / float(F32(temperature))
        s[np.isnan(s)] = -np.inf
        self.s = s
        fin = np.nonzero(s > -np.inf)[0]
        order = fin[np.lexsort((-fin if ties_desc else fin, -s[fin]))]
        ss = s[order]
        n = order.size
        self.kth = None
        if top_k and top_k >= 1 and n:
            kk = min(max(int(top_k), min_keep), V)
            if kk <= n:
                self.kth = ss[kk - 1]
                n = int((ss >= ss[kk - 1]).sum())
        self.order, self.n, self.ss = order[:n], n, ss
        e = np.exp(ss[:n] - ss[0]) if n else np.zeros(0)
        c = np.cumsum(e)
        Z = c[-1] if n else 1.0
        self.tail = (Z - np.concatenate([[0.0], c[:-1]])) / Z
        self.thr = 1.0 - float(F32(top_p))

        def count(t):
            return n if n < min_keep else min(max(int((self.tail > t).sum()), min_keep), n)

        if top_p >= 1.0:
            self.R = self.R_lo = self.R_hi = n
        else:
            self.R, self.R_lo, self.R_hi = count(self.thr), count(self.thr + delta), count(self.thr - delta)

    def boundary_margin(self):
        """Distance of the top-p threshold from the nearest tail mass it separates (ranks >= 2): inf when nothing is near."""
        if self.n <= 2 or self.thr <= 0.0:
            return np.inf
        return float(np.abs(self.tail[2:] - self.thr).min())


class Result:
    def __init__(self, ok, reason="", max_dev=0.0):
        self.ok, self.reason, self.max_dev = ok, reason, max_dev

    def __bool__(self):
        return self.ok


def accepts(rows, beam_scores, V, stop, picks, kept, u, delta, tol):
    """One batch item.  rows: its nb Row objects; picks = (score, token, beam) arrays [2 * nb] in draw order; kept [nb]; u [2 * nb]."""
    nb = len(rows)
    psc, ptok, pbeam = (np.asarray(x) for x in picks)
    F, S = [], []
    for r, row in enumerate(rows):
        if not row.R_lo <= int(kept[r]) <= row.R_hi:
            return Result(False, f"kept[{r}] = {int(kept[r])} outside [{row.R_lo}, {row.R_hi}]")
        toks = np.sort(row.order[:int(kept[r])])
        F.append(r * V + toks)
        S.append(row.s[toks] + float(F32(beam_scores[r])))
    F, S = np.concatenate(F), np.concatenate(S)
    e = np.exp(S - S.max()) if S.size else np.zeros(0)
    alive = np.ones(F.size, dtype=bool)
    dev = 0.0
    for j in range(2 * nb):
        if not alive.any():
            if not (psc[j] == NINF and int(ptok[j]) == stop and int(pbeam[j]) == 0):
                return Result(False, f"draw {j}: no candidate left, the pick is not (-inf, stop, 0)")
            continue
        b, t = int(pbeam[j]), int(ptok[j])
        if not (0 <= b < nb and 0 <= t < V):
            return Result(False, f"draw {j}: ({b}, {t}) out of range")
        f = b * V + t
        pos = int(np.searchsorted(F, f))
        if pos >= F.size or F[pos] != f:
            return Result(False, f"draw {j}: beam {b} token {t} is not a kept candidate")
        if not alive[pos]:
            return Result(False, f"draw {j}: beam {b} token {t} picked twice")
        w = np.where(alive, e, 0.0)
        c = np.cumsum(w)
        T = c[-1]
        lo = (c[pos] - w[pos]) / T - delta
        hi = np.inf if pos == int(np.nonzero(alive)[0][-1]) else c[pos] / T + delta
        if not lo <= float(u[j]) <= hi:
            return Result(False, f"draw {j}: u = {float(u[j])!r} outside [{lo!r}, {hi!r}] of beam {b} token {t}")
        d = abs(float(psc[j]) - S[pos])
        dev = max(dev, d)
        if not d <= tol:
            return Result(False, f"draw {j}: score {float(psc[j])!r} vs {S[pos]!r}: off by {d:.3e} > {tol:.3e}")
        alive[pos] = False
    return Result(True, "", dev)


def draw_margin(rows, beam_scores, V, u):
    """The fp64 sampler's own picks for one item and how far every u_j lies from the nearest edge of its pick's CDF interval (the
    edge at 0 and the open upper edge of the last live candidate do not count)."""
    F, S = [], []
    for r, row in enumerate(rows):
        toks = np.sort(row.order[:row.R])
        F.append(r * V + toks)
        S.append(row.s[toks] + float(F32(beam_scores[r])))
    F, S = np.concatenate(F), np.concatenate(S)
    e = np.exp(S - S.max())
    alive = np.ones(F.size, dtype=bool)
    margin, picks = np.inf, []
    for j in range(len(u)):
        live = np.nonzero(alive)[0]
        if not live.size:
            break
        w = np.where(alive, e, 0.0)
        c = np.cumsum(w) / w.sum()
        hit = np.nonzero(alive & (c >= float(u[j])))[0]
        pos = int(hit[0]) if hit.size else int(live[-1])
        lo = c[pos] - w[pos] / w.sum()
        if lo > 0.0:
            margin = min(margin, float(u[j]) - lo)
        if pos != live[-1]:
            margin = min(margin, c[pos] - float(u[j]))
        alive[pos] = False
        picks.append((int(F[pos] // V), int(F[pos] % V)))
    return picks, margin


def plain(rows, beam_scores, V, stop, u, wrong=None):
    """The step in plain fp64 over Row objects (built with min_keep = 1 / ties_desc = True for those two broken samplers):
    (picks, kept).  wrong: "replacement", "token_major", "no_beam_score", "kept+1" - the other broken samplers."""
    nb = len(rows)
    ent = []
    for r, row in enumerate(rows):
        for t in np.sort(row.order[:row.R]):
            ent.append((r, int(t), row.s[t] + float(F32(beam_scores[r])), row.s[t]))
    ent.sort(key=(lambda x: (x[1], x[0])) if wrong == "token_major" else (lambda x: (x[0], x[1])))
    S = np.array([x[2] for x in ent])
    Wt = np.array([x[3] for x in ent]) if wrong == "no_beam_score" else S
    e = np.exp(Wt - Wt.max())
    alive = np.ones(len(ent), dtype=bool)
    psc = np.full(2 * nb, NINF, dtype=F32)
    ptok = np.full(2 * nb, stop, dtype=np.int32)
    pbeam = np.zeros(2 * nb, dtype=np.int32)
    for j in range(2 * nb):
        live = np.nonzero(alive)[0]
        if not live.size:
            break
        c = np.cumsum(np.where(alive, e, 0.0))
        hit = np.nonzero(alive & (c >= float(u[j]) * c[-1]))[0]
        pos = int(hit[0]) if hit.size else int(live[-1])
        if wrong != "replacement":
            alive[pos] = False
        psc[j], ptok[j], pbeam[j] = S[pos], ent[pos][1], ent[pos][0]
    kept = np.array([row.R for row in rows], dtype=np.int32)
    if wrong == "kept+1":
        kept[0] += 1
    return (psc, ptok, pbeam), kept


# ---- fp32 emulation of the two kernels' sums ----
def _scan(mine, rev):
    """wide_scan_excl over 1024 threads: (the sum of the threads in front of each thread - rev: behind it -, the 16 wave sums)."""
    inc = mine.reshape(16, 64).astype(F32).copy()
    for o in (1, 2, 4, 8, 16, 32):
        new = inc.copy()
        if rev:
            new[:, :-o] = inc[:, :-o] + inc[:, o:]
        else:
            new[:, o:] = inc[:, o:] + inc[:, :-o]
        inc = new
    ex = np.zeros_like(inc)
    wb = np.zeros(16, dtype=F32)
    if rev:
        ex[:, :-1] = inc[:, 1:]
        wsum = inc[:, 0].copy()
        ws = range(15, -1, -1)
    else:
        ex[:, 1:] = inc[:, :-1]
        wsum = inc[:, 63].copy()
        ws = range(16)
    acc = F32(0)
    for w in ws:
        wb[w] = acc
        acc = F32(acc + wsum[w])
    return (wb[:, None] + ex).astype(F32).reshape(1024), wsum


def _block_sum(per_thread):
    """itts_sampler_dev.h block_sum: xor butterfly inside every wave, then the 16 wave sums in order."""
    v = per_thread.reshape(16, 64).astype(F32)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, np.arange(64) ^ o]).astype(F32)
    r = F32(0)
    for w in range(16):
        r = F32(r + v[w, 0])
    return r


def emulate_scores(logits, seen_ids, penalty, stop, suppress_stop, preprocessed, temperature):
    """The fp32 scores beam_wide_cand_kernel sorts (one row)."""
    lg = np.asarray(logits, dtype=F32)
    V = lg.shape[0]
    lse = F32(0)
    if not preprocessed:
        mx = lg.max()
        pad = np.zeros(-(-V // 1024) * 1024, dtype=F32)
        with np.errstate(invalid="ignore"):
            pad[:V] = np.exp((lg - mx).astype(F32)).astype(F32)
        se = np.zeros(1024, dtype=F32)
        for q in range(pad.size // 1024):
            se = (se + pad[q * 1024:(q + 1) * 1024]).astype(F32)
        lse = F32(mx + F32(np.log(_block_sum(se))))
    v = (lg - lse).astype(F32)
    if not preprocessed:
        ids = np.fromiter(seen_ids, dtype=np.int64)
        ids = ids[(ids >= 0) & (ids < V)]
        if float(penalty) != 1.0 and ids.size:
            v[ids] = np.where(v[ids] < 0, v[ids] * F32(penalty), v[ids] / F32(penalty)).astype(F32)
        if suppress_stop:
            v[stop] = NINF
    if float(temperature) != 1.0:
        v = (v / F32(temperature)).astype(F32)
    v[np.isnan(v)] = NINF
    return v


def emulate_cand(v, top_k, top_p, beam_score):
    """beam_wide_cand_kernel behind the scores: (wide_sc row [V], kept)."""
    V = v.shape[0]
    NP = 1024
    while NP < V:
        NP <<= 1
    per = NP // 1024
    ids = np.arange(V)
    order = np.lexsort((ids, -v.astype(np.float64)))
    s = np.full(NP, NINF, dtype=F32)
    s[:V] = v[order]
    kth = s[min(max(int(top_k), 2), V) - 1] if top_k and top_k >= 1 else NINF
    keep = (s >= kth) & (s > NINF)
    n = int(keep.sum())
    with np.errstate(invalid="ignore"):
        e = np.where(keep, np.exp((s - s[0]).astype(F32)).astype(F32), F32(0)).astype(F32).reshape(1024, per)
    r = np.arange(NP).reshape(1024, per)
    R = n
    if top_p < 1.0:
        mine = np.zeros(1024, dtype=F32)
        for q in range(per - 1, -1, -1):
            mine = (mine + e[:, q]).astype(F32)
        c, _ = _scan(mine, True)
        tail = np.zeros((1024, per), dtype=F32)
        for q in range(per - 1, -1, -1):
            c = (c + e[:, q]).astype(F32)
            tail[:, q] = c
        thr = F32(F32(F32(1) - F32(top_p)) * tail[0, 0])
        stay = (r >= 2) & (r < n) & ~(tail <= thr)
        R = min(max(int(r[stay].max()) + 1 if stay.any() else 2, 2), n)
    out = np.full(V, NINF, dtype=F32)
    out[order[:R]] = (s[:R] + F32(beam_score)).astype(F32)
    return out, R


def emulate_pick(sc, nb, V, stop, u):
    """beam_wide_pick_kernel over one item's wide_sc rows [nb, V]: picks in draw order."""
    N = nb * V
    L = -(-N // 1024)
    flat = np.full(1024 * L, NINF, dtype=F32)
    flat[:N] = np.asarray(sc, dtype=F32).reshape(-1)
    flat = flat.reshape(1024, L)
    psc = np.full(2 * nb, NINF, dtype=F32)
    ptok = np.full(2 * nb, stop, dtype=np.int32)
    pbeam = np.zeros(2 * nb, dtype=np.int32)
    if not (flat > NINF).any():
        return psc, ptok, pbeam
    m = flat.max()

    def weights():
        with np.errstate(invalid="ignore"):
            return np.where(flat > NINF, np.exp((flat - m).astype(F32)).astype(F32), F32(0)).astype(F32)

    def run_sums(e):
        mine = np.zeros(1024, dtype=F32)
        for q in range(L):
            mine = (mine + e[:, q]).astype(F32)
        return mine

    e = weights()
    mine = run_sums(e)
    fidx = np.arange(1024 * L).reshape(1024, L)
    for j in range(2 * nb):
        alive = flat > NINF
        if not alive.any():
            break
        base, wsum = _scan(mine, False)
        total = F32(0)
        for w in range(16):
            total = F32(total + wsum[w])
        target = F32(F32(u[j]) * total)
        c = base.copy()
        pre = np.zeros((1024, L), dtype=F32)
        for q in range(L):
            c = (c + e[:, q]).astype(F32)
            pre[:, q] = c
        hit = alive & (pre >= target)
        pick = int(fidx[hit].min()) if hit.any() else int(fidx[alive].max())
        t, q = divmod(pick, L)
        psc[j], ptok[j], pbeam[j] = flat[t, q], pick % V, pick // V
        flat[t, q] = NINF
        e[t, q] = F32(0)
        mine[t] = run_sums(e[t:t + 1])[0]
    return psc, ptok, pbeam


def emulate(logits, seen, beam_scores, penalty, stop, suppress_stop, preprocessed, top_k, top_p, temperature, u):
    """Both kernels for one item: logits [nb, V], seen: nb id collections, u [2 * nb] -> ((score, token, beam), kept)."""
    lg = np.asarray(logits, dtype=F32)
    nb, V = lg.shape
    sc = np.empty((nb, V), dtype=F32)
    kept = np.zeros(nb, dtype=np.int32)
    for r in range(nb):
        v = emulate_scores(lg[r], seen[r], penalty, stop, suppress_stop, preprocessed, temperature)
        sc[r], kept[r] = emulate_cand(v, top_k, top_p, F32(beam_scores[r]))
    return emulate_pick(sc, nb, V, stop, u), kept


# ---- the fp64 side of one batch item ----
def item_rows(logits, seen, penalty, stop, suppress_stop, preprocessed, top_k, top_p, temperature, delta, **kw):
    return [Row(logits[r], seen[r], penalty, stop, suppress_stop, preprocessed, top_k, top_p, temperature, delta, **kw)
            for r in range(len(logits))]


def magnitude(rows, beam_scores):
    """The bound `mag` of score_tol from the fp64 reference: |lse|, the largest kept |log-prob| before the penalty, |beam score|."""
    m = max(abs(float(b)) for b in beam_scores) if len(beam_scores) else 0.0
    for row in rows:
        m = max(m, abs(row.lse))
        fin = row.logp[np.isfinite(row.logp)]
        if fin.size:
            m = max(m, float(np.abs(fin).max()))
    return m


# ---- the operator cases of both test files (inputs from itts_hip/prng.py: the same arrays with and without a GPU) ----
U_TOP = float(np.nextafter(F32(1), F32(0)))  # the largest float below 1: 0.99999994
SHAPES = [(1, 2), (2, 3), (1, 10)]  # (items, nb)
VOCABS = [130, 1025, 8194]  # NP = 1024 with padding; two ranks per thread; the model's vocabulary, the last run partly out of range
VARIANTS = ["gauss", "ties", "few_finite", "seen", "stop"]
COMBOS = [(0, 0.8, 1.0), (0, 1.0, 0.7), (200, 0.8, 1.0), (129, 0.3, 1.3), (5, 0.8, 1.0)]  # (top_k, top_p, temperature)
FAKE_ID = 1


def gaussian(name, seed, shape, std):
    """prng.py has uniforms only: the sum of 12 of them in (-1, 1) has variance 4 and is gaussian enough (Irwin-Hall)."""
    from itts_hip import prng

    n = int(np.prod(shape))
    return (prng.uniform(name, seed, 12 * n).reshape(n, 12).sum(1) * F32(std / 2)).reshape(shape).astype(F32)


# Input streams whose first draw put two different scores within SCORE_TOL of each other at a top-k cut or across a seen /
# unseen pair (assert_separated: the fp64 reference could then not say which of the two the fp32 kernel has to keep) take the
# next stream.  Found with the reference alone, before any kernel existed to be run on them.
CASE_SALT = {("gauss", 1025, 1, 10, 2.5): 1, ("seen", 1025, 1, 10, 2.5): 1, ("gauss", 8194, 2, 3, 2.5): 2, ("seen", 8194, 1, 10, 2.5): 2,
             ("gauss", 1025, 1, 10, 6.0): 1, ("gauss", 8194, 2, 3, 10.0): 1}


def make_case(variant, V, items, nb, std=2.5, salt=None):
    """-> dict: logits [rows, V], hist int32 [rows, stride], k, beam_scores [rows], penalty, stop, start, suppress, pre."""
    from itts_hip import prng

    rows = items * nb
    if salt is None:
        salt = CASE_SALT.get((variant, V, items, nb, std), 0)
    tag = f"wide_beam.{variant}.{items}x{nb}" + (f".{salt}" if salt else "")
    lg = gaussian(tag, V, (rows, V), std)
    c = dict(k=0, penalty=10.0, stop=V - 2, start=V - 3, suppress=0, pre=0, hist=np.zeros((rows, 64), dtype=np.int32))
    # running beam scores as a generation has them: different per beam, best first, within a few nats
    bs = -(np.arange(rows) % nb).astype(F32) * F32(0.75) - (prng.uniform(tag + ".bs", V, rows) * F32(0.5) + F32(0.5)).astype(F32)
    if variant == "ties":
        # multiples of 1/4: ties straddle the top-k cut; the beams of an item share one logits row and one beam score, as at
        # step 0 of a generation: equal scores across beams
        lg = (np.round(lg * 4) / 4).astype(F32)
        for bi in range(items):
            lg[bi * nb:(bi + 1) * nb] = lg[bi * nb]
        bs = np.zeros(rows, dtype=F32)
    elif variant == "few_finite":
        # what a typical pre-pass leaves: 2 - 3 finite log-probs per row (item 0: 2 in every row, so its 2 * nb picks take every
        # candidate there is and the last one is the "last live entry" fallback)
        keep = np.zeros((rows, V), dtype=bool)
        for r in range(rows):
            nfin = 2 if r < nb else 2 + (r % 2)
            keep[r, np.argsort(prng.uniform(f"{tag}.keep{r}", V, V), kind="stable")[:nfin]] = True
        lg = np.where(keep, (lg * F32(0.4) - F32(3.0)).astype(F32), NINF).astype(F32)
        c["pre"] = 1
    elif variant == "seen":
        c["k"] = 60
        for r in range(rows):
            h = prng.randint(f"{tag}.seen{r}", V, 60, 0, V).astype(np.int32)
            h[:3] = np.argsort(lg[r])[-3:]  # the row's best tokens among them
            c["hist"][r, :60] = h
    elif variant == "stop":
        c["stop"] = int(np.argmax(lg[0]))
        if c["stop"] == c["start"]:
            c["start"] = V - 4
        c["suppress"] = 1
    c["logits"], c["beam_scores"] = np.ascontiguousarray(lg), bs
    return c


def case_seen(c, row):
    return {FAKE_ID, int(c["start"])} | {int(t) for t in c["hist"][row, :c["k"]]}


def uniform_sets(variant, V, items, nb):
    """Two sets [items, 2 * nb]; the first holds 0.0 and 0.99999994."""
    from itts_hip import prng

    u = prng.uniform(f"wide_beam.u.{variant}.{items}x{nb}", V, 2 * items * 2 * nb) * F32(0.5) + F32(0.5)  # (-1, 1) -> (0, 1)
    u = np.minimum(u, F32(U_TOP)).astype(F32)
    u = u.reshape(2, items, 2 * nb)
    u[0, 0, 1], u[0, 0, 2], u[0, -1, -1] = 0.0, U_TOP, U_TOP
    return [u[0].copy(), u[1].copy()]


def case_refs(c, items, nb, top_k, top_p, temperature, **kw):
    """-> per item: (rows, delta, tol) of the fp64 side."""
    V = c["logits"].shape[1]
    delta = delta_b(V, nb)
    out = []
    for bi in range(items):
        sl = slice(bi * nb, (bi + 1) * nb)
        rows = item_rows(c["logits"][sl], [case_seen(c, r) for r in range(bi * nb, (bi + 1) * nb)], c["penalty"], c["stop"],
                         c["suppress"], c["pre"], top_k, top_p, temperature, delta, **kw)
        tol = score_tol(V, c["penalty"], temperature, magnitude(rows, c["beam_scores"][sl]))
        out.append((rows, delta, tol))
    return out


def assert_separated(c, row_index, row, tol):
    """fp64, before any GPU work: no two scores on either side of the top-k cut, and no seen / unseen pair, closer than tol
    unless they are exactly equal (the same logit with the same seen flag goes through the same fp32 operations)."""
    s = row.s
    lg = c["logits"][row_index]
    seen = np.zeros(s.shape[0], dtype=bool)
    if not c["pre"]:
        ids = np.fromiter(case_seen(c, row_index), dtype=np.int64)
        seen[ids[ids < s.shape[0]]] = True
    fin = np.nonzero(s > -np.inf)[0]
    if row.kth is not None:
        near = fin[np.abs(s[fin] - row.kth) <= tol]
        at = near[s[near] == row.kth][0]
        same = (lg[near].view(np.uint32) == lg[at].view(np.uint32)) & (seen[near] == seen[at])
        assert same.all(), (row_index, "scores within tol of the top-k cut that are not the same value", near[~same][:4])
    a, b = fin[seen[fin]], fin[~seen[fin]]
    if a.size and b.size:
        sb = np.sort(s[b])
        pos = np.clip(np.searchsorted(sb, s[a]), 1, sb.size - 1)
        gap = np.minimum(np.abs(sb[pos] - s[a]), np.abs(sb[pos - 1] - s[a]))
        assert (gap > tol).all(), (row_index, "a seen and an unseen token closer than tol", a[gap <= tol][:4])


def safe_uniforms(rows, beam_scores, V, nd, margin, name, seed):
    """Uniforms for one item that the fp64 reference ALONE places at least `margin` from every edge of the drawn candidate's CDF
    interval: draw by draw, the first value of a prng stream that does.  A function of the inputs and the reference only."""
    from itts_hip import prng

    stream = np.minimum(prng.uniform(name, seed, 4096) * F32(0.5) + F32(0.5), F32(U_TOP)).astype(F32)
    u, at = [], 0
    for j in range(nd):
        while True:
            assert at < stream.size, "no uniform with the margin asked for: the distribution is too flat for it"
            cand = u + [stream[at]]
            at += 1
            if draw_margin(rows, beam_scores, V, cand)[1] >= margin:
                u = cand
                break
    return np.asarray(u, dtype=F32)
