"""GPU, full IndexTTS-1.5 sizes, the "smooth" checkpoint (fixture smooth_decode_b1): what the opt-in fp8 (e4m3) K/V cache costs
in accuracy, by the procedure of tests/test_gpu_bf16_accuracy.py::test_bf16_forced_logits - teacher-forced on the reference ids at
2 rows (1024-thread attention form, GEMV projections) and at 32 rows (32 x 20 heads >= 512: the 256-thread form, MFMA
projections), top-8 logits' relative RMS against the fp32 reference by sequence length S, up to S = 619.  The 16-bit-cache engine
runs the same rows in the same test, so both numbers are in one record (keys smooth_kv_fp8_* of the accuracy fixture; copied to
profiles/kv_fp8.txt)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from itts_hip import engine as ieng  # noqa: E402
from test_gpu_bf16_accuracy import CFG, S0, forced_trace, mel, rms_rel, sd_smooth, top8_err  # noqa: E402,F401

# e4m3 keeps 3 mantissa bits: a K or V element moves by up to 2^-4 relative (bf16: 2^-9), as an fp8 weight does (BOUND_FP8 = 0.045
# there).  Measured on one MI355X (profiles/kv_fp8.txt): top-8 logits relative RMS, worst over the 12 traced steps, 3.73e-3 at 2 rows
# and 4.24e-3 at 32 rows (16-bit cache, same rows in the same test: 3.05e-3 and 3.07e-3), flat in S (early / late means 2.6e-3 /
# 2.9e-3 and 2.8e-3 / 2.8e-3), the arg-max equal to the reference's at 12 of the 12 traced steps.  The bound is 2 x the worst
# measurement - the margin the fp8-weight bound has; it leaves room for another summation order in later kernels.
BOUND_KV_FP8 = 8.5e-3


@pytest.fixture(scope="module")
def eng16(sd_smooth):  # noqa: F811
    return ieng.build_engine(CFG, "bf16", parts=("gpt",), state_dicts={"gpt": sd_smooth})


@pytest.mark.parametrize("nrows", [2, 32])
def test_kv_fp8_forced_logits(eng16, mel, gold, accuracy, monkeypatch, nrows):  # noqa: F811
    monkeypatch.delenv("ITTS_KV_FP8", raising=False)
    g = gold("smooth_decode_b1")
    cond = eng16.conditioning(mel)
    res = {}
    for tag, on in (("bf16_cache", False), ("fp8_cache", True)):
        eng16.set_kv_fp8(on)
        try:
            lgs = forced_trace(eng16, cond, g, nrows)
            mode = eng16.decode_mode()
        finally:
            eng16.set_kv_fp8(False)
        assert not on or mode == 0  # the fp8 cache keeps the launch path
        for k, lg in lgs.items():  # (a) identical rows of a batch: identical logits
            for r in range(1, nrows):
                assert np.array_equal(lg[r], lg[0]), (tag, k, r)
        res[tag] = top8_err(lgs, g)
        agree = [int(lgs[int(k)][0].argmax()) == int(g["top_idx"][i][0]) for i, k in enumerate(g["trace_steps"])]
        accuracy[f"smooth_kv_fp8_{tag}_forced_rows{nrows}_top8_logits_rel_rms_by_S"] = res[tag]
        accuracy[f"smooth_kv_fp8_{tag}_forced_rows{nrows}_argmax_equal_to_reference"] = f"{sum(agree)} of {len(agree)} traced steps"
        print(f"kv_fp8 accuracy rows={nrows} {tag}: worst {max(res[tag].values()):.4e} by S " +
              " ".join(f"{S}:{v:.3e}" for S, v in sorted(res[tag].items())) + f"; argmax {sum(agree)} of {len(agree)}")
    r8 = res["fp8_cache"]
    assert r8 != res["bf16_cache"], "the fp8 cache did not engage"
    early = np.mean([v for S, v in r8.items() if S < 300])
    late = np.mean([v for S, v in r8.items() if S >= 400])
    print(f"kv_fp8 accuracy rows={nrows}: early {early:.4e} late {late:.4e}")
    assert late < 1.5 * early + 0.02, (early, late)  # (b) no growth with the sequence length
    assert max(r8.values()) < BOUND_KV_FP8, r8  # (c)
