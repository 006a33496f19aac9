"""Shared by test_wide_sampler_host.py and test_gpu_wide_sampler.py: what the whole-vocabulary sampler
(csrc/decode_sampler.hip sampler_wide_kernel) has to satisfy, stated in fp64, and an fp32 numpy emulation of the kernel's
summation structure.

Tolerance.  The kernel's sums go through at most CHAIN = 53 dependent fp32 additions (a thread's run of <= 16 ranks: 15, the
wave scan: 6, the other waves' sums: 15, joining the two: 1, along the run again: 16) of terms that expf delivers within 1 ulp, so
the relative error of any partial mass stays under DELTA = 64 * 2^-24.  Nothing here is tuned to what the kernel returns."""
import numpy as np

CHAIN = 53
DELTA = 64 * 2.0 ** -24
F32 = np.float32
NINF = F32(-np.inf)


def sampler_scores(logits, seen_ids=(), penalty=1.0, stop=0, suppress_stop=False, preprocessed=False, temperature=1.0):
    """The fp32 scores the sampler sorts: sampler_score (repetition penalty over seen_ids, stop suppression; none of it when
    preprocessed), then / temperature - the device's own fp32 operations."""
    s = np.asarray(logits, dtype=F32).copy()
    if not preprocessed:
        ids = np.fromiter(seen_ids, dtype=np.int64)
        if penalty != 1.0 and ids.size:
            v = s[ids]
            s[ids] = np.where(v < 0, v * F32(penalty), v / F32(penalty)).astype(F32)
        if suppress_stop:
            s[stop] = NINF
    if temperature != 1.0:
        s = (s / F32(temperature)).astype(F32)
    return s


class Ref:
    """fp64 side of one row: ranks by (score descending, id ascending) over the finite scores, the TopK cut as in HF, the
    masses and the admissible range [R_lo, R_hi] of the kept count."""

    def __init__(self, scores, top_k, top_p):
        s = np.asarray(scores, dtype=F32)
        V = s.shape[0]
        fin = np.nonzero(s > NINF)[0]
        order = fin[np.lexsort((fin, -s[fin].astype(np.float64)))]
        ss = s[order].astype(np.float64)
        n = order.size
        if top_k and top_k >= 1 and n:
            kk = min(int(top_k), V)
            if kk <= n:
                n = int((ss >= ss[kk - 1]).sum())  # ties with the k-th value stay (HF masks `scores < kth`)
        self.order, self.n = order[:n], n
        self.rank_of = {int(t): r for r, t in enumerate(self.order)}
        e = np.exp(ss[:n] - ss[0]) if n else np.zeros(0)
        self.c = np.cumsum(e)
        Z = self.c[-1] if n else 1.0
        self.tail = (Z - np.concatenate([[0.0], self.c[:-1]])) / Z
        if top_p >= 1.0:
            self.R_lo = self.R_hi = n
        else:
            thr = 1.0 - float(F32(top_p))
            self.R_lo = max(1, int((self.tail > thr + DELTA).sum()))
            self.R_hi = max(1, int((self.tail > thr - DELTA).sum()))

    def _draw_ok(self, r, R, u):
        if r >= R:
            return False
        T = self.c[R - 1]
        lo = (self.c[r - 1] / T if r > 0 else 0.0) - DELTA
        hi = np.inf if r == R - 1 else self.c[r] / T + DELTA
        return lo <= float(u) <= hi

    def accepts(self, tok, u, kept=None):
        """kept given: R_lo <= kept <= R_hi and the draw is right for R' = kept.  kept None (not visible at the engine level): the
        draw is right for some R' in [R_lo, R_hi]."""
        r = self.rank_of.get(int(tok))
        if r is None:
            return False
        if kept is not None:
            return self.R_lo <= int(kept) <= self.R_hi and self._draw_ok(r, int(kept), u)
        return any(self._draw_ok(r, R, u) for R in range(self.R_lo, self.R_hi + 1))


def pick_fp64(scores, top_k, top_p, u):
    """HF's step in plain fp64: (token, kept)."""
    ref = Ref(scores, top_k, top_p)
    R = ref.n if top_p >= 1.0 else max(1, int((ref.tail > 1.0 - float(F32(top_p))).sum()))
    target = float(F32(u)) * ref.c[R - 1]
    r = min(int(np.searchsorted(ref.c[:R], target, side="left")), R - 1)
    return int(ref.order[r]), R


# ---- fp32 emulation of sampler_wide_kernel's sums ----
def _scan_excl(mine, rev):
    """wide_scan_excl: one value per thread (1024) -> the sum of the threads in front of it (rev: behind it)."""
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
        wsum = inc[:, 0]
        acc = F32(0)
        for w in range(15, -1, -1):
            wb[w] = acc
            acc = F32(acc + wsum[w])
    else:
        ex[:, 1:] = inc[:, :-1]
        wsum = inc[:, 63]
        acc = F32(0)
        for w in range(16):
            wb[w] = acc
            acc = F32(acc + wsum[w])
    return (wb[:, None] + ex).astype(F32).reshape(1024)


def emulate(scores, top_k, top_p, u, wrong=None):
    """(token, kept) as sampler_wide_kernel computes them, sums in its order in fp32.  wrong: one of the broken samplers the
    predicate has to reject - "rank+1", "kept+1", "ties_desc", "desc_cumsum"."""
    s_in = np.asarray(scores, dtype=F32)
    V = s_in.shape[0]
    NP = 1024
    while NP < V:
        NP <<= 1
    per = NP // 1024
    ids = np.arange(V)
    order = np.lexsort((-ids if wrong == "ties_desc" else ids, -s_in.astype(np.float64)))
    s = np.full(NP, NINF, dtype=F32)
    s[:V] = s_in[order]
    kth = s[min(int(top_k), V) - 1] if top_k and top_k >= 1 else NINF
    keep = (s >= kth) & (s > NINF)
    n = max(int(keep.sum()), 1)
    with np.errstate(invalid="ignore"):
        e = np.where(keep, np.exp((s - s[0]).astype(F32)).astype(F32), F32(0)).astype(F32).reshape(1024, per)
    r = np.arange(NP).reshape(1024, per)
    R = n
    if top_p < 1.0:
        mine = np.zeros(1024, dtype=F32)
        for q in range(per - 1, -1, -1):
            mine = (mine + e[:, q]).astype(F32)
        c = _scan_excl(mine, True)
        tail = np.zeros((1024, per), dtype=F32)
        for q in range(per - 1, -1, -1):
            c = (c + e[:, q]).astype(F32)
            tail[:, q] = c
        thr = F32(F32(F32(1) - F32(top_p)) * tail[0, 0])
        stay = (r >= 1) & (r < n) & ~(tail <= thr)
        R = int(r[stay].max()) + 1 if stay.any() else 1
        if wrong == "desc_cumsum":  # the nucleus taken from the inclusive descending cumsum: the boundary token is lost
            cd = np.cumsum(e.reshape(-1), dtype=F32)
            R = max(1, int((cd[:n] <= F32(top_p) * cd[-1]).sum()))
    e = np.where(r >= R, F32(0), e).astype(F32)
    mine = np.zeros(1024, dtype=F32)
    for q in range(per):
        mine = (mine + e[:, q]).astype(F32)
    c = _scan_excl(mine, False)
    pre = np.zeros((1024, per), dtype=F32)
    for q in range(per):
        c = (c + e[:, q]).astype(F32)
        pre[:, q] = c
    target = F32(F32(u) * pre.reshape(-1)[R - 1])
    hit = (r < R) & (pre >= target)
    pick = min(int(r[hit].min()) if hit.any() else R - 1, R - 1)
    if wrong == "rank+1":
        pick += 1
    if wrong == "kept+1":
        R += 1
    return int(order[min(pick, V - 1)]), R
