"""CPU: what the selector of the launch path's bf16 decode GEMV (csrc/decode_gemv.hip gemv_bf16_pick, exported as itts_gemv_which)
decides - whether gemv_bf16 takes a call, and which instantiation (batch rows compiled in, weight rows per wave, 512-column
chunks per lane, waves per workgroup) the call gets.  Pure host code, no device is touched.

The expectations were written down from the commit BEFORE the selector existed, where the table was stated twice:
`gemv_bf16_supported()` (restated here as parent_supported) and the if-ladder `dispatch_gemv_bf16<NB>()` (PINNED).  One corner
the two did not agree on, kept as it was: fp32 input with prologue 3 passes the gate (K <= 1536) although no kernel is
instantiated for it - gemv_bf16 answers "no instantiation for this shape"; no caller builds that call.  It is part of the
acceptance sweep and left out of PINNED.

One thing the selector changed on purpose since: the block-cooperative kernel masks only its last 512-column chunk, so a call
is taken only when K reaches that chunk, K >= (NCH - 1) * 512.  parent_supported stays the parent's table; the sweep expects it
less exactly those calls (test_dropped_calls_are_the_two_unmasked_ranges)."""
import itertools

import pytest

from itts_hip import lib as L

D = 1280  # model width of the full-size GPT: c_attn 3D x D, c_fc 4D x D, c_proj D x D, mlp.c_proj D x 4D, head 8194 x D


@pytest.fixture(scope="module")
def which():
    f = L.load().itts_gemv_which

    def call(B, N, K, pro, xbf, ybf, w5=0):
        v = int(f(B, N, K, pro, xbf, ybf, w5))
        return None if v < 0 else (v & 15, (v >> 4) & 15, (v >> 8) & 255, v >> 16)

    return call


def parent_supported(B, K, pro, xbf, ybf):
    """gemv_bf16_supported() of the parent, line for line (prologue 3 with both partial buffers present)."""
    nch = (K + 511) // 512
    if not (1 <= B <= 4 and K % 8 == 0 and K >= 64 and nch <= 10):
        return False
    if xbf and pro == 3:
        return (not ybf) and K % 64 == 0 and (nch <= 1 or nch == 3)
    if xbf:
        return pro == 0 and (not ybf) and (nch <= 1 or nch == 3 or nch == 4 or 4 < nch <= 10)
    if pro == 0 or nch > 3:
        return False
    return not (pro == 2 and ybf)


# (name, N, K, prologue, x_bf16, y_bf16, w5) -> (rpw, nch, waves) at 1-2 rows, at 3-4 rows; read off the parent's ladder
W4 = {
    "c_attn": (2, 3, 4), "c_fc": (2, 3, 4), "c_proj": (2, 3, 4), "c_proj split": (2, 3, 4), "mlp.c_proj": (2, 10, 4),
    "head": (4, 3, 4), "K=2048": (2, 4, 4),
}
CALLS = {
    "c_attn": (3 * D, D, 1, 0, 0), "c_fc": (4 * D, D, 1, 0, 1), "c_proj": (D, D, 0, 1, 0), "c_proj split": (D, D, 3, 1, 0),
    "mlp.c_proj": (D, 4 * D, 0, 1, 0), "head": (8194, D, 2, 0, 0), "K=2048": (D, 2048, 0, 1, 0),
}
# the ITTS_GEMV_W5 rows of the ladder sit behind `NB <= 2`: 3 and 4 rows keep the 4-wave pick; head and K=2048 have no such row
W5 = {"c_attn": (3, 3, 5), "c_fc": (4, 3, 5), "c_proj": (1, 3, 5), "c_proj split": (1, 3, 5), "mlp.c_proj": (1, 10, 5)}
PINNED = [(nm, B, w5, (W5[nm] if w5 and B <= 2 and nm in W5 else W4[nm])) for nm in CALLS for B in (1, 2, 3, 4) for w5 in (0, 1)]


@pytest.mark.parametrize("name,B,w5,want", PINNED)
def test_pinned_picks(which, name, B, w5, want):
    N, K, pro, xbf, ybf = CALLS[name]
    assert which(B, N, K, pro, xbf, ybf, w5) == (B,) + want


def test_w5_rows_need_their_own_width(which):
    """The 5-wave rows name their N (256 workgroups x 5 waves x RPW rows): any other width keeps the 4-wave pick."""
    for B in (1, 2):
        assert which(B, 3 * D + 8, D, 1, 0, 0, 1) == (B, 2, 3, 4)
        assert which(B, 3 * D, D, 1, 0, 1, 1) == (B, 2, 3, 4)  # c_attn's width with c_fc's output type
        assert which(B, 2 * D, D, 0, 1, 0, 1) == (B, 2, 3, 4)
        assert which(B, 2 * D, 4 * D, 0, 1, 0, 1) == (B, 2, 10, 4)
        assert which(B, D, 4 * D - 512, 0, 1, 0, 1) == (B, 2, 10, 4)  # 9 chunks: the row asks for exactly 10
        assert which(B, 8194, D, 2, 0, 0, 1) == (B, 4, 3, 4)


def test_micro_sizes(which):
    """K <= 512: every prologue / type combination the ladder has a row for runs one weight row per wave, one chunk, 4 waves."""
    combos = [(1, 0, 1), (1, 0, 0), (2, 0, 0), (0, 1, 0), (3, 1, 0)]  # (prologue, x_bf16, y_bf16): the five rows of the ladder
    for K in (64, 96, 256, 448, 504, 512):
        for (pro, xbf, ybf), B, N, w5 in itertools.product(combos, (1, 2, 3, 4), (96, 384, D), (0, 1)):
            if pro == 3 and K % 64:
                continue  # the merged attention output comes in whole heads
            assert parent_supported(B, K, pro, xbf, ybf)
            assert which(B, N, K, pro, xbf, ybf, w5) == (B, 1, 1, 4), (K, pro, xbf, ybf, B, N, w5)


KS = list(range(56, 5129, 8)) + [57, 66, 127, 516, 1284, 2047, 5116]
NS = (96, D, 3 * D, 4 * D, 8194)


@pytest.fixture(scope="module")
def sweep(which):
    """Every call of the acceptance set once: (B, N, K, prologue, x_bf16, y_bf16) -> pick or None."""
    return {c: which(*c) for c in itertools.product(range(6), NS, KS, range(4), (0, 1), (0, 1))}


def ladder_nch(K):
    """The chunk count compiled into the kernel a call gets, as the ladder states it: 1, 3, 4 or 10 chunks of 512 columns."""
    nch = (K + 511) // 512
    return 1 if nch <= 1 else 3 if nch <= 3 else 4 if nch <= 4 else 10


def test_acceptance_set_unchanged(sweep):
    """What the parent accepted, less the calls whose K does not reach the kernel's last chunk: gemv_bf16_kernel masks only chunk
    NCH - 1, so every earlier chunk has to lie inside K (K >= (NCH - 1) * 512)."""
    assert len(sweep) == 6 * len(NS) * len(KS) * 4 * 2 * 2
    want = {c: parent_supported(c[0], c[2], c[3], c[4], c[5]) and c[2] >= (ladder_nch(c[2]) - 1) * 512 for c in sweep}
    wrong = [c for c, got in sweep.items() if (got is not None) != want[c]]
    assert not wrong, (len(wrong), wrong[:8])
    assert sum(got is not None for got in sweep.values()) > 10000  # the sweep does reach the accepted side


def test_dropped_calls_are_the_two_unmasked_ranges(sweep):
    """Relative to the parent exactly two K ranges left the acceptance set: fp32 x at two chunks (512 < K < 1024, which ran the
    3-chunk kernel) and bf16 x at 2048 < K < 4608 (5 to 9 chunks, which ran the 10-chunk kernel).  Nothing was added."""
    dropped = {c for c, got in sweep.items() if got is None and parent_supported(c[0], c[2], c[3], c[4], c[5])}
    added = [c for c, got in sweep.items() if got is not None and not parent_supported(c[0], c[2], c[3], c[4], c[5])]
    assert not added, added[:8]
    fp32_two_chunks = {c for c in sweep if parent_supported(c[0], c[2], c[3], c[4], c[5]) and not c[4] and 512 < c[2] < 1024}
    bf16_mid = {c for c in sweep if parent_supported(c[0], c[2], c[3], c[4], c[5]) and c[4] and 2048 < c[2] < 4608}
    assert dropped == fp32_two_chunks | bf16_mid
    assert fp32_two_chunks and bf16_mid and not (fp32_two_chunks & bf16_mid)
    assert {(c[2] + 511) // 512 for c in fp32_two_chunks} == {2} and {(c[2] + 511) // 512 for c in bf16_mid} == {5, 6, 7, 8, 9}
    assert {c[2] for c in fp32_two_chunks} == {K for K in KS if K % 8 == 0 and 512 < K < 1024}
    assert {c[2] for c in bf16_mid} == {K for K in KS if K % 8 == 0 and 2048 < K < 4608}
    assert {c[3] for c in fp32_two_chunks} == {1, 2, 3} and {c[3] for c in bf16_mid} == {0}  # (bf16 x, prologue 3 never had 5+ chunks)


def test_acceptance_does_not_depend_on_w5(which, sweep):
    for c in itertools.product((1, 2, 4), NS, range(56, 5129, 64), range(4), (0, 1), (0, 1)):
        assert (which(*c, 1) is not None) == (sweep[c] is not None), c


def test_prologue_3_takes_whole_heads(which):
    """itts_gemv_which passes partial buffers for prologue 3, as a real call has them; whole heads only."""
    assert which(2, D, D, 3, 1, 0) == (2, 2, 3, 4)
    assert which(2, D, D - 32, 3, 1, 0) is None and which(2, D, D - 32, 0, 1, 0) == (2, 2, 3, 4)


def test_row_count(sweep):
    """Rows compiled into the kernel: B for 1-3 rows and 4 for 4 rows, on every accepted call."""
    wrong = [c for c, got in sweep.items() if got is not None and got[0] != c[0]]
    assert not wrong, wrong[:8]
    assert {c[0] for c, got in sweep.items() if got is not None} == {1, 2, 3, 4}
