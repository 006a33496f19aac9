"""Host-side integer logic of the `IndexTTS.infer` / `infer_fast` orchestration (product code, numpy only).

Mirrors /root/reference/indextts/infer.py: `remove_long_silence` (:244-298), `bucket_sentences` (:303-315),
`pad_tokens_cat` (:316-318).  Parity with the reference's own function is pinned by
tests/golden/silence_cases.npz (tests/test_host_logic.py)."""
from __future__ import annotations

import os

from typing import Dict, List, Sequence, Tuple

import numpy as np


def remove_long_silence(codes: np.ndarray, stop_mel_token: int, silent_token: int = 52,
                        max_consecutive: int = 30) -> Tuple[np.ndarray, np.ndarray]:
    """codes int [B, T] -> (codes', code_lens[B]).  Each row is cut at its first stop token; a row holding more
    than `max_consecutive` silent tokens in total keeps at most 10 consecutive ones (infer.py:262-280); ragged
    rows are right-padded with the stop token (:287) and the batch is clipped to the longest kept row (:294-296)."""
    codes = np.asarray(codes)
    assert codes.ndim == 2
    lens: List[int] = []
    rows: List[np.ndarray] = []
    fixed = False
    for code in codes:
        hit = np.nonzero(code == stop_mel_token)[0]
        n = int(hit[0]) if len(hit) else code.shape[0]
        if int((code == silent_token).sum()) > max_consecutive:
            body = code[:n]
            is_sil = body == silent_token
            # run position of each silent token inside its run (0-based); non-silent tokens reset the run
            idx = np.arange(n)
            last_non = np.maximum.accumulate(np.where(~is_sil, idx, -1))
            run_pos = idx - last_non - 1
            keep = (~is_sil) | (run_pos < 10)
            rows.append(body[keep])
            n = int(keep.sum())
            fixed = True
        else:
            rows.append(code[:n])
        lens.append(n)
    if fixed:
        width = max(r.shape[0] for r in rows)
        out = np.full((len(rows), width), stop_mel_token, dtype=codes.dtype)
        for i, r in enumerate(rows):
            out[i, : r.shape[0]] = r
        codes = out
    m = max(lens)
    if m < codes.shape[1]:
        codes = codes[:, :m]
    return codes, np.asarray(lens, dtype=np.int64)


def bucket_sentences(sentences: Sequence[Sequence], bucket_max_size: int = 4) -> List[List[Dict]]:
    """infer.py:303-315: keep order if everything fits one bucket, else sort by length into buckets."""
    outputs = [{"idx": i, "sent": s, "len": len(s)} for i, s in enumerate(sentences)]
    if len(outputs) <= bucket_max_size:
        return [outputs]
    buckets: List[List[Dict]] = []
    for item in sorted(outputs, key=lambda x: x["len"]):
        if not buckets or len(buckets[-1]) >= bucket_max_size:
            buckets.append([item])
        else:
            buckets[-1].append(item)
    return buckets


def pad_tokens_cat(tokens: Sequence[np.ndarray], stop_text_token: int) -> np.ndarray:
    """infer.py:316-318: right-pad id rows with the stop text token into [B, Lmax]."""
    rows = [np.asarray(t).reshape(-1) for t in tokens]
    width = max(r.shape[0] for r in rows)
    out = np.full((len(rows), width), stop_text_token, dtype=np.int32)
    for i, r in enumerate(rows):
        out[i, : r.shape[0]] = r
    return out


def ragged_groups(lengths: Sequence[int], max_pad: float, cap: int) -> List[List[int]]:
    """Vocoder batches over latents of unequal length (Engine.bigvgan_grouped(ragged=True)): indices sorted by length, longest
    first (ties: lower index first); a group opens with the longest remaining row and takes the following rows while the share of
    padded frames of the [n, Tmax] batch, 1 - sum(len) / (n * Tmax), stays <= max_pad and n <= cap.  Rows only get shorter, so the
    first row that does not fit closes the group.  max_pad = 0: groups of equal length, at most cap rows each."""
    if cap < 1 or not 0.0 <= max_pad < 1.0:
        raise ValueError(f"ragged_groups: cap >= 1 and 0 <= max_pad < 1 expected, not cap={cap!r}, max_pad={max_pad!r}")
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    groups: List[List[int]] = []
    tmax = total = 0
    for i in order:
        n = int(lengths[i])
        if n < 1:
            raise ValueError(f"ragged_groups: length {n} of row {i}")
        g = groups[-1] if groups else None
        # (integers: padded = cells - frames <= max_pad * cells, compared without a division)
        if g is not None and len(g) < cap and (len(g) + 1) * tmax - (total + n) <= max_pad * (len(g) + 1) * tmax:
            g.append(i)
            total += n
        else:
            groups.append([i])
            tmax, total = n, n
    return groups


def sampling_kwargs(do_sample, num_beams, top_k, top_p, temperature, typical_sampling=False, typical_mass=0.9,
                    length_penalty=0.0) -> dict:
    """HF `generate` kwargs (infer.py:116-124) -> Engine.generate keywords; every mode runs on the device:
      do_sample, num_beams > 1       beam_sample (the reference default: 3 beams)
      do_sample, num_beams == 1      multinomial sampling
      not do_sample, num_beams > 1   beam_search (deterministic)
      not do_sample, num_beams == 1  greedy
      typical_sampling               the reference's TypicalLogitsWarper(typical_mass) behind the repetition penalty - a logits
                                     PROCESSOR in the reference (model.py:690-697), so greedy and beam search run it too
    Limits of the device samplers (the web UI offers num_beams 1..10 and top_k 0..100): num_beams <= 10; at most 128 kept
    candidates per row in the narrow samplers.  top_k = 0 / None (HF: TopK warper off) or > 128 is exact all the same: by default
    the token choice then runs on the host over the whole vocabulary (host_sample_step / host_beam_step below, one logits
    read-back per token) - with one beam or several.  With one beam, Engine.generate(wide_sampler="device") / ITTS_WIDE_SAMPLER=device
    runs it on the whole-vocabulary device sampler instead (no read-back; the same distribution, parallel fp32 sums: top-p
    boundary and draw within 64 * 2^-24 of the mass of torch's); with several beams wide_beam_sampler="device" /
    ITTS_WIDE_BEAM_SAMPLER=device does the same on the whole-vocabulary beam sampler (within 512 * 2^-24).  The seed is drawn from torch's global RNG so that torch.manual_seed governs the run as it does for
    the reference's torch.multinomial."""
    import warnings

    import torch

    nb = 1 if num_beams is None else max(1, int(num_beams))
    if typical_sampling and not (0.0 < float(typical_mass) < 1.0):
        raise ValueError(f"`typical_mass` has to be a float > 0 and < 1, but is {typical_mass}")  # model.py:692-693
    if nb > 10:
        warnings.warn(f"itts_hip: num_beams={nb} > 10 is not supported; using 10", RuntimeWarning)
        nb = 10
    lp = float(length_penalty or 0.0)
    tm = float(typical_mass) if typical_sampling else 0.0
    if not do_sample:
        kw = dict(num_beams=nb, length_penalty=lp) if nb > 1 else {}
        if tm:
            kw["typical_mass"] = tm
        return kw
    k = int(top_k) if top_k else 0
    if k < 1:
        k = 0  # HF: TopK warper off - exact on the host (Engine.generate takes the host-sampling path, with or without beams)
    p = 1.0 if top_p is None else float(top_p)
    return dict(do_sample=True, top_k=k, top_p=min(max(p, 1e-6), 1.0), temperature=float(temperature or 1.0), num_beams=nb,
                typical_mass=tm, length_penalty=lp,
                seed=int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))


# ---- mixed decode batches: which utterances may share a generation, and the per-row table of one ----
MIXED_SHARED = ("num_beams", "typical_sampling", "typical_mass", "length_penalty", "max_mel_tokens")
MIXED_PER_ROW = ("do_sample", "top_k", "top_p", "temperature", "repetition_penalty")


def _is_seq(x) -> bool:
    return isinstance(x, (list, tuple, np.ndarray))


def mixed_groups(settings: Sequence[dict]) -> List[List[int]]:
    """Index lists of the utterances that may share one generation (IndexTTS.infer_batch, mixed_batch): settings[u] holds the
    generation kwargs of utterance u (IndexTTS._gen_kwargs).  A generation has one num_beams, one typical filter, one
    length_penalty and one max_mel_tokens, so those are the key; do_sample / top_k / top_p / temperature / repetition_penalty
    are per row - except under beams or typical filtering, which have no per-row form: there the key holds them as well.
    The voice never is part of the key.  Groups in the order of their first utterance, indices ascending."""
    groups: Dict[tuple, List[int]] = {}
    for u, g in enumerate(settings):
        nb = max(1, int(g.get("num_beams") or 1))
        typical = bool(g.get("typical_sampling", False))
        key = (nb, typical, float(g.get("typical_mass", 0.9)) if typical else 0.0, float(g.get("length_penalty") or 0.0),
               int(g.get("max_mel_tokens", 600)))
        if nb > 1 or typical:
            key += row_sampling_table(1, *(g.get(k, d) for k, d in zip(MIXED_PER_ROW, (True, 30, 0.8, 1.0, 10.0))))[0]
        groups.setdefault(key, []).append(u)
    return list(groups.values())


def row_sampling_table(B: int, do_sample, top_k, top_p, temperature, repetition_penalty) -> List[tuple]:
    """The per-row table of a mixed batch of B rows: every argument a scalar (all rows) or a sequence of length B.
    -> [(mode, top_k, top_p, temperature, penalty)] * B in the form of itts_row_sampling, normalised as sampling_kwargs does it:
    mode 1 = sample, 0 = greedy; top_k None / < 1 -> 0 (TopK warper off); top_p None -> 1, clipped to [1e-6, 1]; temperature
    None / 0 -> 1.  A greedy row reads none of the three, so it carries (0, 1.0, 1.0): equal rows compare equal."""
    cols = []
    for name, v in zip(MIXED_PER_ROW, (do_sample, top_k, top_p, temperature, repetition_penalty)):
        v = list(v) if _is_seq(v) else [v] * B
        if len(v) != B:
            raise ValueError(f"row_sampling_table: {name} has {len(v)} entries for {B} rows")
        cols.append(v)
    table = []
    for ds, k, p, t, pen in zip(*cols):
        pen = float(pen)
        t = float(t or 1.0)
        if not pen > 0.0 or not t > 0.0:
            raise ValueError(f"row_sampling_table: temperature and repetition_penalty have to be > 0, not {t!r}, {pen!r}")
        if not ds:
            table.append((0, 0, 1.0, 1.0, pen))
            continue
        k = int(k) if k else 0
        p = 1.0 if p is None else float(p)
        table.append((1, k if k >= 1 else 0, min(max(p, 1e-6), 1.0), t, pen))
    return table


def row_uniforms(seeds: Sequence, max_gen: int) -> np.ndarray:
    """Draws [max_gen, B] of a batch whose row b has its own seed: column b is default_rng(seeds[b]).random(max_gen) - what the
    request would draw alone, whoever shares its batch and whichever row it sits in."""
    return np.stack([np.random.default_rng(s).random(max_gen, dtype=np.float32) for s in seeds], axis=1)


class AdmitScheduler:
    """Which requests of one call start a generation of `slots` rows and which wait for a finished row's slot (row admission,
    Engine.generate(slots=..)).  Pure bookkeeping, no engine: the longest `slots` texts start - so every later text fits the
    generation's text length - in the caller's order; the others wait in the caller's order.  take(finished) hands the head
    of the waiting list to the lowest finished slots once at least ceil(admit_min * slots) slots are finished, or as soon as the
    rest of the list fits into the finished ones.  slot_req[s]: the request slot s holds; log: (slots, requests) per admission."""

    def __init__(self, lengths: Sequence[int], slots: int, admit_min: float):
        n, slots = len(lengths), int(slots)
        if slots < 1 or not 0.0 < float(admit_min) <= 1.0:
            raise ValueError(f"AdmitScheduler: slots >= 1 and 0 < admit_min <= 1, not {slots!r}, {admit_min!r}")
        order = sorted(range(n), key=lambda i: (-int(lengths[i]), i))
        self.first = sorted(order[:slots])
        self.waiting = sorted(order[slots:])
        self.need = max(1, int(np.ceil(float(admit_min) * slots - 1e-9)))
        self.slot_req = list(self.first)
        self.log: List[tuple] = []

    def take(self, finished: Sequence[int]):
        """finished: the slots whose row has finished, ascending.  -> (slots, requests) to admit now (both empty: not yet)."""
        f = len(finished)
        if not self.waiting or f == 0 or (f < self.need and len(self.waiting) > f):
            return [], []
        k = min(f, len(self.waiting))
        req, self.waiting = self.waiting[:k], self.waiting[k:]
        sl = [int(s) for s in finished[:k]]
        for s, r in zip(sl, req):
            self.slot_req[s] = r
        self.log.append((sl, req))
        return sl, req

    def order(self) -> List[int]:
        """The request of every original row of the generation: the first rows, then the admitted ones in admission order."""
        return self.first + [r for _, req in self.log for r in req]


# ---- packed latent pass (Engine.latent_packed): chunks and the A/B switch ----
PACKED_MAX_SEQ = 128       # ITTS_VARLEN_MAX_SEQ: the sequence offsets travel in the kernel's argument block
PACKED_MAX_TOKENS = 65536  # default token budget of one pass: about 33 KiB (16-bit) / 55 KiB (fp32) of scratch per token row at D = 1280


def packed_chunks(lengths: Sequence[int], max_tokens: int = PACKED_MAX_TOKENS, max_seqs: int = PACKED_MAX_SEQ) -> List[List[int]]:
    """Consecutive runs of sequence indices for one packed pass each: order-preserving, at most max_seqs sequences and at most
    max_tokens token rows a chunk; a sequence longer than the budget is a chunk of its own.  (Any chunking gives the same bits -
    a sequence's latent does not depend on its companions - so this only bounds the scratch.)"""
    if max_tokens < 1 or max_seqs < 1:
        raise ValueError(f"packed_chunks: max_tokens {max_tokens} / max_seqs {max_seqs} must be >= 1")
    chunks, cur, tok = [], [], 0
    for i, n in enumerate(lengths):
        n = int(n)
        if n < 1:
            raise ValueError(f"packed_chunks: sequence {i} has length {n}")
        if cur and (len(cur) >= max_seqs or tok + n > max_tokens):
            chunks.append(cur)
            cur, tok = [], 0
        cur.append(i)
        tok += n
    if cur:
        chunks.append(cur)
    return chunks


# ---- packed vocoder (Engine.bigvgan_packed): the gap rule and the chunks ----
PACKED_VOCODER_MAX_SEQ = 128        # SEG_MAX: offsets and lengths travel in the kernels' argument block
PACKED_VOCODER_MAX_FRAMES = 16384   # default frame budget of one pass, see packed_vocoder_plan


def packed_vocoder_gap(up_rates: Sequence[int], up_kernels: Sequence[int], res_kernels: Sequence[int],
                       res_dils: Sequence[Sequence[int]]) -> int:
    """Zero frames a packed sentence needs behind its signal: the largest reach of any convolution of the generator, in latent
    frames, rounded up - conv_pre (k = 7: 3 frames), every ups[i] at its INPUT rate (polyphase: output q * u + ph reads
    x[q + (ph + p) // u - m], m < k // u, p = (k - u) // 2), every AMP conv at its stage's rate ((k * d - d) // 2 rows, and
    (k - 1) // 2 for the undilated second conv), conv_post (3 rows at the output rate).  The rule of csrc/model_vocoder.hip
    bigvgan_packed_gap, which checks every call against it again."""
    ceil_div = lambda a, b: -(-int(a) // int(b))  # noqa: E731
    gap, U = 3, 1
    for u, k in zip(up_rates, up_kernels):
        u, k = int(u), int(k)
        p, taps = (k - u) // 2, k // u
        gap = max(gap, ceil_div(max((u - 1 + p) // u, taps - 1 - p // u), U))
        U *= u
        for ks, dils in zip(res_kernels, res_dils):
            for d in dils:
                gap = max(gap, ceil_div(max((int(ks) * int(d) - int(d)) // 2, (int(ks) - 1) // 2), U))
    return max(gap, ceil_div(3, U))


def packed_vocoder_plan(lengths: Sequence[int], gap: int, max_frames: int = PACKED_VOCODER_MAX_FRAMES,
                        max_seqs: int = PACKED_VOCODER_MAX_SEQ) -> Tuple[List[List[int]], List[List[int]], List[int]]:
    """Chunks of one packed vocoder pass each: -> (chunks, offsets, frames).  chunks[k]: a consecutive run of sentence indices
    (order-preserving); offsets[k]: len(chunks[k]) + 1 frame offsets, sentence j of the chunk owns [offsets[k][j], offsets[k][j + 1]),
    a capacity of exactly len + gap; frames[k] = offsets[k][-1], the frames the pass computes - at most max_frames, except that a
    sentence whose len + gap is over the budget is a chunk of its own; at most max_seqs sentences a chunk.  Pure.  (Any chunking
    gives the same samples - a sentence does not depend on its companions - so this only bounds the scratch.)
    The default budget, 16384 frames, is sized from the pass's scratch: the bump allocator keeps six tensors of every stage, at
    full dims 6 * (4 * 768 + 16 * 384 + 64 * 192 + 3 * 24576) elements per latent frame - about 1.2 MiB (16-bit) / 2.4 MiB (fp32)
    a frame, so about 19 / 38 GiB a pass; the batched form already runs 64 x 480 = 30720 frames in one pass."""
    gap, max_frames, max_seqs = int(gap), int(max_frames), int(max_seqs)
    if gap < 0 or max_frames < 1 or max_seqs < 1:
        raise ValueError(f"packed_vocoder_plan: gap {gap} >= 0, max_frames {max_frames} >= 1 and max_seqs {max_seqs} >= 1 expected")
    chunks, offsets, frames = [], [], []
    cur, off = [], [0]
    for i, n in enumerate(lengths):
        n = int(n)
        if n < 1:
            raise ValueError(f"packed_vocoder_plan: sentence {i} has length {n}")
        if cur and (len(cur) >= max_seqs or off[-1] + n + gap > max_frames):
            chunks.append(cur), offsets.append(off), frames.append(off[-1])
            cur, off = [], [0]
        cur.append(i)
        off.append(off[-1] + n + gap)
    if cur:
        chunks.append(cur), offsets.append(off), frames.append(off[-1])
    return chunks, offsets, frames


# ---- streaming synthesis (Engine.bigvgan_stream, IndexTTS.infer_stream) ----
STREAM_CHUNK_FRAMES = 48        # default frames per chunk (about 2 s of audio): unmeasured, see tools/bench_stream.py
STREAM_FIRST_CHUNK_FRAMES = 24  # default frames of a sentence's first chunk (about 1 s)
ACT1D_REACH = 5                 # Activation1d, one side, in samples of its own rate (derived below)


def vocoder_reach(up_rates: Sequence[int], up_kernels: Sequence[int], res_kernels: Sequence[int],
                  res_dils: Sequence[Sequence[int]]) -> int:
    """The accumulated one-sided reach R of the whole generator in latent frames: frame t of the latent changes no output sample
    outside frames [t - R, t + R], and whatever lies outside a window [a - R, b + R) changes nothing inside [a, b).  Pure.
    Unlike packed_vocoder_gap - the LARGEST reach of one layer, enough to keep a neighbour's signal out of one convolution - this
    is the SUM over the cascade: a layer that reaches e samples to a side at up-sampling rate m adds e / m frames, the sum is
    rounded up once (a perturbed frame is m whole samples at rate m, so the fractions of the layers add before they are cut).
      conv_pre (k = 7, pad 3)                                3 samples at rate 1
      ups[i] (ConvTranspose1d k, stride u, pad p = (k - u) // 2: input i feeds outputs i * u - p .. i * u - p + k - 1)
                                                             max(p, k - u - p) samples at its OUTPUT rate
      Activation1d (replicate pad 5 / 5, 12-tap transposed conv stride 2, crop 15 / 15; SnakeBeta; replicate pad 5 / 6, 12-tap conv
      stride 2): x[i] feeds the 2x samples 2i - 5 .. 2i + 6, and y[t] reads the 2x samples 2t - 5 .. 2t + 6, so x[i] reaches
      y[i - 5 .. i + 5]                                      5 samples at the stage rate; the replicate clamp at a segment's own end
                                                             copies the edge sample into those pads, which reaches no further
      AMP block, kernel ks, per dilation d: Activation1d, conv (ks, dilation d), Activation1d, conv (ks), plus the skip - the
      longest path                                           sum over d of 5 + d * (ks - 1) / 2 + 5 + (ks - 1) / 2; per stage the
                                                             deepest branch, i.e. the largest such sum over the kernels
      activation_post, conv_post (k = 7)                     5 + 3 samples at the output rate
    IndexTTS-1.5 (rates 4 4 4 4 2 2, kernels 8 8 4 4 4 4, AMP kernels 3 7 11, dilations 1 3 5): 3 + 2/4 + 90/4 + 2/16 + 90/16 +
    90/64 + 90/256 + 1/512 + 90/512 + 1/1024 + 90/1024 + 8/1024 = 33.8 -> R = 34 frames."""
    from fractions import Fraction

    reach, rate = Fraction(3), 1
    for u, k in zip(up_rates, up_kernels):
        u, k = int(u), int(k)
        p = (k - u) // 2
        rate *= u
        reach += Fraction(max(p, k - u - p, 0), rate)
        amp = 0
        for ks, dils in zip(res_kernels, res_dils):
            ks = int(ks)
            amp = max(amp, sum(2 * ACT1D_REACH + int(d) * (ks - 1) // 2 + (ks - 1) // 2 for d in dils))
        reach += Fraction(amp, rate)
    reach += Fraction(ACT1D_REACH + 3, rate)
    return int(-(-reach.numerator // reach.denominator))


class StreamWindow:
    """The emit and hold-back arithmetic of one streamed sentence (Engine.bigvgan_stream).  Frames arrive in pieces; a vocoder
    window is the frames [lo, have) held so far, and frame f of it is FINAL when it lies R frames away from every artificial
    window edge: f >= lo + R unless lo = 0 (the sentence's true left edge), f < have - R unless the sentence has ended (its true
    right edge).  lo = max(0, sent - R) keeps exactly the left context the next window needs.
    push(n, last) -> (lo, a, b): n more frames arrived; run the window [lo, have) and emit frames [a, b) - or nothing (b == a) while
    fewer than `chunk` frames (`first_chunk` for the sentence's first emission) are final; last=True emits everything left.
    Everything emitted is final; the emissions are consecutive and, after last, cover [0, have).  Pure host arithmetic."""

    def __init__(self, R: int, chunk: int = 1, first_chunk: int = None):
        self.R, self.chunk = int(R), max(1, int(chunk))
        self.first = self.chunk if first_chunk is None else max(1, int(first_chunk))
        self.have = self.sent = self.lo = 0
        self.ended = False

    def push(self, n: int, last: bool = False) -> Tuple[int, int, int]:
        if self.ended or int(n) < 0:
            raise ValueError("StreamWindow.push: the sentence has ended" if self.ended else "StreamWindow.push: n < 0")
        self.have += int(n)
        self.ended = bool(last)
        lo, a = self.lo, self.sent
        b = self.have if last else max(a, self.have - self.R)
        if not last and b - a < (self.first if a == 0 else self.chunk):
            b = a  # hold back: not a whole chunk yet
        self.sent = b
        self.lo = max(0, b - self.R)
        return lo, a, b


def stream_clean(codes, stop_mel_token: int, silent_token: int = 52, max_consecutive: int = 30, state: dict = None):
    """The causal form of remove_long_silence for ONE row that arrives in pieces: -> (kept codes of this piece, state).  Pass the
    returned state with the next piece (None = a fresh row).  The row ends at its first stop token (nothing from there on is kept).
    Silent code i at 0-based position r of its run of silent codes is dropped iff r >= 10 and the silent codes seen so far, itself
    included, number more than max_consecutive - a decision that needs nothing behind code i, so what was kept stays kept.
    Where it differs from remove_long_silence: that rule first counts the silent codes of the WHOLE row and, if there are more than
    max_consecutive, drops every silent code with r >= 10 - also one that came among the row's first max_consecutive silent codes,
    which the causal rule has already passed on.  So the two differ only for a silent code with r >= 10 among a row's first
    max_consecutive silent codes, in a row that ends with more than max_consecutive; they agree on every row with at most
    max_consecutive silent codes and on every row whose runs longer than 10 begin after its max_consecutive-th silent code."""
    st = dict(state) if state else dict(run=0, silent=0, stopped=False)
    keep = []
    for c in np.asarray(codes).reshape(-1):
        c = int(c)
        if st["stopped"]:
            break
        if c == stop_mel_token:
            st["stopped"] = True
            break
        if c == silent_token:
            r = st["run"]
            st["run"] += 1
            st["silent"] += 1
            if r >= 10 and st["silent"] > max_consecutive:
                continue
        else:
            st["run"] = 0
        keep.append(c)
    return np.asarray(keep, dtype=np.int64), st


def env_switch(name: str, setting: bool) -> bool:
    """An A/B switch of IndexTTS: the environment variable overrides the constructor's setting in both directions ("1" on, "0" off);
    unset or anything else leaves the setting."""
    return {"1": True, "0": False}.get(os.environ.get(name, ""), bool(setting))


# ---- host-side token choice (HF GenerationMixin.sample over the whole vocabulary) ----
def host_distribution(scores: np.ndarray, seen_ids, penalty: float, temperature: float, top_k: int, top_p: float,
                      typical_mass: float, stop: int, suppress_stop: bool, min_keep: int = 1, log_softmax_first: bool = False,
                      return_scores: bool = False):
    """One row of HF 4.36.2 `sample()`'s score pipeline, in the order generate() builds it for infer.py:116-124 /
    model.py:688-703: RepetitionPenaltyLogitsProcessor over every id seen so far (fake prefix id, start token, generated
    codes) -> [TypicalLogitsWarper] -> TemperatureLogitsWarper -> TopKLogitsWarper (off when top_k < 1) -> TopPLogitsWarper.
    Returns (kept token ids in descending-score order - ties: lower id first -, un-normalised weights exp(s - s_max)).  fp32.
    Beams (beam_sample): log_softmax_first (the processors see log-probabilities), min_keep = 2 (min_tokens_to_keep of every
    warper and of the typical filter, model.py:693-694); return_scores: the warped scores instead of the weights."""
    # The kept SET is computed with torch's CPU ops in the order and form of the HF 4.36.2 classes (sort -> softmax -> cumsum,
    # topk's k-th value, log_softmax): with thousands of kept tokens the top-p boundary depends on the last bits of a
    # cumulative sum, and the reference's arithmetic IS torch's - a numpy restatement parts from it once in a few hundred steps.
    import torch

    s = torch.from_numpy(np.asarray(scores, dtype=np.float32).copy())
    V = s.shape[0]
    if log_softmax_first:
        s = torch.log_softmax(s, dim=-1)
    ids = torch.from_numpy(np.fromiter(seen_ids, dtype=np.int64))
    if penalty != 1.0 and ids.numel():
        v = s[ids]
        s[ids] = torch.where(v < 0, v * float(penalty), v / float(penalty))  # RepetitionPenaltyLogitsProcessor
    if suppress_stop:
        s[stop] = -float("inf")
    if typical_mass and 0.0 < typical_mass < 1.0:
        s = torch.from_numpy(_typical_filter(s.numpy(), float(typical_mass), min_keep))
    if temperature != 1.0:
        s = s / float(temperature)  # TemperatureLogitsWarper
    if top_k and top_k >= 1:  # TopKLogitsWarper: top_k = max(top_k, min_tokens_to_keep), ties with the k-th value stay
        kk = min(max(int(top_k), min_keep), V)
        s = s.masked_fill(s < torch.topk(s, kk)[0][-1], -float("inf"))
    if top_p is not None and top_p < 1.0:  # TopPLogitsWarper
        sorted_logits, sorted_idx = torch.sort(s, descending=False)
        remove = sorted_logits.softmax(dim=-1).cumsum(dim=-1) <= (1 - float(top_p))
        remove[-min_keep:] = False
        s[sorted_idx[remove]] = -float("inf")
    s = s.numpy()
    keep = np.nonzero(np.isfinite(s))[0]
    order = np.lexsort((keep, -s[keep].astype(np.float64)))
    idx = keep[order]
    e = np.exp((s[idx] - s[idx[0]]).astype(np.float32)).astype(np.float32)
    n = idx.size
    return (idx[:n], s[idx[:n]]) if return_scores else (idx[:n], e[:n])


def host_beam_step(logits: np.ndarray, ids_hist: np.ndarray, k: int, beam_scores: np.ndarray, done: np.ndarray, nb: int,
                   penalty: float, temperature: float, top_k: int, top_p: float, typical_mass: float, u: np.ndarray, stop: int,
                   suppress_stop: bool, start_tok: int, fake_id: int = 1):
    """One step of HF 4.36.2 `beam_sample` up to (not including) BeamSearchScorer.process, for every batch item, on the host:
    per beam log_softmax -> RepetitionPenalty over the beam's own ids (the fake prompt id, the start token, its k generated
    codes) -> [Typical] -> Temperature -> TopK -> TopP (min_tokens_to_keep = 2) -> + running beam score; the kept candidates
    of an item's beams in flat (beam-major, token-ascending) order = next_token_scores.view(batch, beams * vocab); 2 * nb
    draws without replacement as sequential inverse-CDF look-ups of the caller's uniforms u [items, 2 * nb] (the convention
    of the device sampler, beam.hip beam_select_kernel: fp32 running sums in flat order).
    logits [items * nb, V], ids_hist [items * nb, >= k], beam_scores [items * nb], done [items].
    -> (scores, tokens, beams) each [items, 2 * nb], in DRAW order (itts_gpt_commit_beams sorts them and runs the scorer)."""
    lg = np.asarray(logits, dtype=np.float32)
    items = lg.shape[0] // nb
    nd = 2 * nb
    psc = np.zeros((items, nd), dtype=np.float32)
    ptok = np.full((items, nd), stop, dtype=np.int32)
    pbeam = np.zeros((items, nd), dtype=np.int32)
    for bi in range(items):
        if done[bi]:
            continue
        fs, ft, fb = [], [], []
        for r in range(nb):
            row = bi * nb + r
            seen = {int(fake_id), int(start_tok)} | {int(t) for t in ids_hist[row, :k]}
            idx, sc = host_distribution(lg[row], seen, penalty, temperature, top_k, top_p, typical_mass, stop, suppress_stop,
                                        min_keep=2, log_softmax_first=True, return_scores=True)
            o = np.argsort(idx, kind="stable")
            fs.append((sc[o] + np.float32(beam_scores[row])).astype(np.float32))
            ft.append(idx[o])
            fb.append(np.full(idx.size, r, dtype=np.int32))
        fs, ft, fb = np.concatenate(fs), np.concatenate(ft), np.concatenate(fb)
        e = np.exp((fs - fs.max()).astype(np.float32)).astype(np.float32)
        alive = np.ones(e.size, dtype=bool)
        for j in range(nd):
            c = np.cumsum(np.where(alive, e, np.float32(0.0)), dtype=np.float32)  # sequential fp32 sums; a dead entry adds 0.0 (exact)
            target = np.float32(np.float32(u[bi, j]) * c[-1])
            hit = np.nonzero(alive & (c >= target))[0]
            live = np.nonzero(alive)[0]
            if live.size == 0:
                break  # fewer live candidates than picks (cannot happen with min_tokens_to_keep = 2): the stop-token defaults stay
            pick = int(hit[0]) if hit.size else int(live[-1])
            alive[pick] = False
            psc[bi, j], ptok[bi, j], pbeam[bi, j] = fs[pick], ft[pick], fb[pick]
        if live.size == 0:
            psc[bi, j:] = -np.inf
    return psc, ptok, pbeam


def host_sample_step(logits: np.ndarray, seen: Sequence[set], penalty: float, temperature: float, top_k: int, top_p: float,
                     typical_mass: float, u: np.ndarray, stop: int, suppress_stop: bool) -> np.ndarray:
    """One multinomial draw per row over host_distribution, taken as the inverse-CDF lookup of the caller's uniform u[row]
    over the kept tokens in descending-score order - the convention of the device samplers."""
    lg = np.asarray(logits, dtype=np.float32)
    out = np.empty(lg.shape[0], dtype=np.int32)
    for r in range(lg.shape[0]):
        idx, e = host_distribution(lg[r], seen[r], penalty, temperature, top_k, top_p, typical_mass, stop, suppress_stop)
        c = np.cumsum(e, dtype=np.float32)
        target = np.float32(np.float32(u[r]) * c[-1])
        out[r] = int(idx[min(int(np.searchsorted(c, target, side="left")), idx.size - 1)])
    return out


def _typical_filter(s: np.ndarray, mass: float, min_keep: int = 1) -> np.ndarray:
    """The reference's TypicalLogitsWarper (indextts/utils/typical_sampling.py:9-30) on one fp32 row; min_keep =
    min_tokens_to_keep (2 under beams, model.py:693-694)."""
    m = s.max()
    z = np.exp((s - m).astype(np.float32)).astype(np.float32)
    normalized = ((s - m) - np.float32(np.log(z.sum(dtype=np.float32)))).astype(np.float32)
    p = np.exp(normalized).astype(np.float32)
    with np.errstate(invalid="ignore"):
        ent = -np.nansum(normalized * p, dtype=np.float32)
    shifted = np.abs((-normalized) - ent).astype(np.float32)
    order = np.argsort(shifted, kind="stable")
    so = s[order]
    eo = np.exp((so - so.max()).astype(np.float32)).astype(np.float32)
    cum = np.cumsum(eo / eo.sum(dtype=np.float32), dtype=np.float32)
    last = min(int((cum < np.float32(mass)).sum()), s.size - 1)
    out = s.copy()
    remove = shifted[order] > shifted[order][last]
    if min_keep > 1:
        remove[:min_keep] = False
    out[order[remove]] = -np.inf
    return out
