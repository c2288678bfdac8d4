"""The candidate window of upsample_bwd4_kernel against the launcher's rule that admits it (CPU, numpy float32: no device).

The float4 adjoint of the bilinear up-sampling gathers, per axis, the NW = 8 outputs oy_lo .. oy_lo + 7 and nothing else.  Whether
eight are enough is decided on the host: tmg_upsample_bwd takes that kernel only while 2 (ho - 1) <= 5 (hi - 1) + 2 on both axes
and hi > 1.  The two statements live in different places (a device constant and a host inequality); this test restates the kernel's
window arithmetic with its fp32 roundings and asserts, for every 2 <= hi <= 64 and EVERY ho the rule admits, that every output
with a non-zero hat weight on an input row lies inside that row's window - and that the rule is not vacuous: (hi, ho) = (2, 9),
the first ho beyond it, needs a ninth candidate.  An edit of either side that breaks the agreement fails here."""
import numpy as np

F32 = np.float32
NW = 8                  # csrc/tmg_pointwise.hip, upsample_bwd4_kernel: constexpr int NW = 8


def rule_admits(hi, ho):
    """csrc/tmg_pointwise.hip, tmg_upsample_bwd: win_ok, one axis ((dims[3] - 1) * 2 <= (dims[1] - 1) * 5 + 2 && dims[1] > 1)."""
    return (ho - 1) * 2 <= (hi - 1) * 5 + 2 and hi > 1


def ratio(hi, ho):
    """upsample_bwd4_kernel: ry = ho > 1 ? (float)(hi - 1) / (float)(ho - 1) : 0.f"""
    return F32(hi - 1) / F32(ho - 1) if ho > 1 else F32(0)


def window_lo(r, hi):
    """upsample_bwd4_kernel: oy_lo = 0; if (ry > 0.f) oy_lo = max(0, (int)floorf((iy - 1) / ry) - 1), for every iy at once."""
    iy = np.arange(hi)
    if not r > 0:
        return np.zeros(hi, dtype=np.int64)
    q = (iy - 1).astype(F32) / r                            # int -> float conversion, then the fp32 division
    return np.maximum(0, np.floor(q).astype(np.int64) - 1)


def hat(r, ho, hi):
    """upsample_hat(r, o, idx, n_in) for every (idx, o): sv = r * o; i0 = min((int)sv, n_in - 1); i1 = min(i0 + 1, n_in - 1);
    f = sv - i0; (i0 == idx ? 1 - f : 0) + (i1 == idx ? f : 0), every operation rounded to fp32."""
    o = np.arange(ho)
    sv = (r * o.astype(F32)).astype(F32)
    i0 = np.minimum(sv.astype(np.int64), hi - 1)            # (int) truncates; sv >= 0
    i1 = np.minimum(i0 + 1, hi - 1)
    f = (sv - i0.astype(F32)).astype(F32)
    idx = np.arange(hi)[:, None]
    w = np.where(i0[None] == idx, (F32(1) - f)[None], F32(0)) + np.where(i1[None] == idx, f[None], F32(0))
    return w.astype(F32)                                    # [hi, ho]


def outside_window(hi, ho):
    """(iy, o) pairs with a non-zero weight outside [oy_lo(iy), oy_lo(iy) + NW)."""
    r = ratio(hi, ho)
    lo = window_lo(r, hi)[:, None]
    o = np.arange(ho)[None]
    w = hat(r, ho, hi)
    return np.argwhere((w != 0) & ((o < lo) | (o >= lo + NW)))


def test_emulation_is_a_partition_of_unity():
    """The restated hat weights are the forward's interpolation weights: every output's weights over the inputs sum to 1."""
    for hi, ho in ((2, 4), (5, 12), (64, 128), (33, 80), (7, 1), (9, 4)):
        s = hat(ratio(hi, ho), ho, hi).astype(np.float64).sum(0)
        assert np.all(np.abs(s - 1) <= 2.0 ** -23), (hi, ho)


def test_every_admitted_size_fits_the_eight_candidate_window():
    checked = 0
    for hi in range(2, 65):
        ho = 1
        while rule_admits(hi, ho):
            bad = outside_window(hi, ho)
            assert bad.size == 0, "hi %d ho %d: (iy, o) %s outside the window" % (hi, ho, bad[:4].tolist())
            checked += 1
            ho += 1
        assert ho - 1 == (5 * (hi - 1) + 2) // 2 + 1        # the largest admitted ho, from the inequality itself
    assert checked == sum((5 * (hi - 1) + 2) // 2 + 1 for hi in range(2, 65))


def test_rule_is_not_vacuous():
    """Just beyond the rule a ninth candidate is needed, so neither NW nor the inequality has slack to give away at hi = 2."""
    assert rule_admits(2, 4) and not rule_admits(2, 5)
    assert not rule_admits(2, 9) and outside_window(2, 9).tolist() == [[1, 8]]
    assert not rule_admits(1, 1) and not rule_admits(1, 2)  # hi == 1 (r == 0) always takes the gather kernel
