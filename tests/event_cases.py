"""Case tables, reference and named defects of the ensemble event verification (tests/test_events_cpu.py, tests/test_events_gpu.py).

Definitions (include/tmglow_hip_event.h, tmg_ops.EnsembleEvents).  Event k = (channel, value, ">" | "<"), strict; the raw threshold
thr[b, k] = float32((value / u[b, c] - out_mu[c]) / out_std[c]), formed in fp64.  Per pixel n = #{m : x_m <> thr} and o = [y <> thr] on
the float32 values: comparisons have no rounding, so every integer output of the device must EQUAL this reference, on integer and on
real data alike.

The reference never uses prefix sums or tiles: counts by direct comparison, box sums as the sum of the w^2 shifted slices of the
zero-padded field, tables by bincount.  The derived float outputs come from other formulas than tmg_ops.event_table_scores':
  brier       the direct pixel sum of (n - S o)^2 in int64, divided once by S^2 HW
  brier_rel   the pixel mean of (n / S - obar_{n(p)})^2, brier_res the pixel mean of (obar_{n(p)} - obar)^2 (obar_j looked up per pixel)
  roc_area    the Mann-Whitney statistic over the (event pixel, non-event pixel) pairs with ties counted half, in integers:
              sum_e (2 #{q : n_q < n_e} + #{q : n_q = n_e}) / (2 N1 N0); NaN when N1 or N0 is 0
  fss         1 - sum_p (f - g)^2 / (sum_p f^2 + sum_p g^2) on the fractions f = Nf / (S w^2), g = No / w^2 in fp64
The time aggregates pool the pixels of the timed steps.

Float tolerance (the issue's): |got - ref| <= 2^-24 |ref| + 2^-40: the one final rounding to float32 plus the fp64 formulas' own
rounding (at most 1026 terms of magnitude <= 1: under 2^-42; the reference's pixel sums are numpy's pairwise sums of at most
3 * 33123 terms <= 1: under 17 * 2^-53 of their value)."""
import functools

import numpy as np
import torch

import structure_cases as SC

F32 = np.float32
T = 3
U24 = 2.0 ** -24
TOL_ABS = 2.0 ** -40
DEFAULT_SCALES = (1, 3, 5, 9, 17, 33)
EIGHT = (1, 3, 5, 7, 9, 17, 25, 33)
STEP_KEYS = ("brier", "brier_rel", "brier_res", "brier_unc", "base_rate", "fcst_rate", "roc_area")
TIME_TABLE_KEYS = ("time_brier", "time_brier_rel", "time_brier_res", "time_brier_unc", "time_base_rate", "time_roc_area",
                   "time_fss_uniform")
INT_KEYS = ("rel_count", "rel_hit", "fss_raw", "time_rel_count", "time_rel_hit", "time_event_count", "time_obs_count")
FLOAT_KEYS = STEP_KEYS + ("fss",) + TIME_TABLE_KEYS + ("time_fss", "time_rel_obs_freq", "time_roc_hit_rate", "time_roc_false_rate",
                                                        "time_brier_map")
ALL_KEYS = INT_KEYS + FLOAT_KEYS + ("event_scales",)
DEFECTS = ("non_strict", "target_member", "even_window", "wrap", "hit_ungated", "s_plus_one", "drop_last")
SD = SC.SD
MU = [0.2, -0.1, 0.4, 0.05]


def int_events(Cc, K):
    """Thresholds ON values of the integer data (-3..3): both directions on channel 0, then the other channels."""
    return (((0, 1.0, ">"), (0, 1.0, "<"), (1, -2.0, "<"), (Cc - 1, 0.0, ">")))[:K]


# (S, B, C, (H, W), t_start, chunk kind, padded, K, scales)
INT_TABLE = [
    (1, 1, 2, (1, 2), 0, 0, False, 1, (1,)), (2, 3, 3, (2, 1), 1, 2, True, 2, (1, 3)), (1024, 1, 2, (1, 5), 0, 2, False, 1, (1, 3, 5)),
    (5, 3, 3, (7, 9), 1, 1, True, 4, (33, 1, 5)), (17, 3, 4, (5, 13), 1, 1, True, 3, EIGHT), (64, 1, 3, (16, 17), 0, 2, False, 2, DEFAULT_SCALES),
    (130, 1, 2, (16, 33), 0, 1, True, 2, DEFAULT_SCALES), (5, 1, 3, (50, 58), 1, 2, False, 4, EIGHT), (17, 3, 2, (3, 70), 0, 1, True, 2, (3, 9)),
    (2, 1, 4, (66, 3), 1, 0, False, 3, (5,)), (5, 1, 2, (66, 130), 0, 2, True, 2, (1, 9, 33)), (1024, 1, 3, (7, 9), 0, 1, False, 2, (1, 3, 33)),
    (64, 3, 2, (16, 33), 1, 0, True, 1, (17,)),
]
LONG_CASE = (2, 1, 2, (181, 183), 0, 2, False, 1, (1, 33))                    # 6 x 6 tiles, two steps
# (S, B, C, (H, W), kind, with_u, events, scales)
REAL_TABLE = [
    (5, 3, 3, (7, 9), "gauss", True, ((0, 0.0, "<"), (2, 1.5, ">")), (1, 3, 33)),
    (16, 1, 4, (16, 17), "smooth", False, ((0, 0.0, "<"), (3, 0.5, ">"), (0, 2.0, ">")), DEFAULT_SCALES),
    (17, 3, 2, (5, 13), "biased", True, ((0, 0.0, "<"), (1, 0.3, ">")), (1, 5)),
    (64, 1, 3, (16, 33), "gauss", False, ((1, 0.0, "<"), (1, 0.0, ">"), (2, 1.0, ">"), (0, -0.5, "<")), EIGHT),
    (130, 1, 2, (50, 58), "smooth", True, ((0, 0.0, "<"),), DEFAULT_SCALES),
    (2, 3, 3, (50, 58), "biased", False, ((2, 0.0, "<"), (0, 1.0, ">")), (3,)),
    (5, 1, 2, (3, 70), "smooth", True, ((0, 0.0, "<"), (1, 0.0, ">")), (1, 3, 5)),
    (7, 3, 3, (66, 3), "gauss", True, ((0, 0.5, ">"),), (1, 9)),
    (1, 3, 3, (16, 17), "gauss", True, ((0, 0.0, "<"), (2, 0.5, ">")), (1, 3)),
]
FIELDS = {(1, 2), (2, 1), (1, 5), (7, 9), (5, 13), (16, 17), (16, 33), (50, 58), (3, 70), (66, 3), (66, 130), (181, 183)}


def int_case_inputs(case, idx):
    S, B, Cc, hw, t_start, kind, padded, K, scales = case
    steps = 2 if case is LONG_CASE else T
    xs, tgt = SC.int_inputs("small", S, B, Cc, hw, 9000 + idx, steps)
    return xs, tgt, int_events(Cc, K), min(t_start, steps - 1)


def real_case_inputs(idx):
    S, B, Cc, hw, kind, with_u, events, scales = REAL_TABLE[idx]
    xs, tgt = SC.real_inputs(S, B, Cc, hw, kind, 9500 + idx)
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))) if with_u else None
    return xs, tgt, u


def thresholds(events, B, Cc, mu=None, sd=None, u=None):
    """thr [B, K] float32: (value / u - mu) / sd in fp64 from the fp32 factors, rounded once."""
    m = np.zeros(Cc) if mu is None else np.asarray(mu, F32)[:Cc].astype(np.float64)
    s = np.ones(Cc) if sd is None else np.asarray(sd, F32)[:Cc].astype(np.float64)
    sc = np.ones((B, Cc)) if u is None else np.asarray(u, F32).reshape(B, Cc).astype(np.float64)
    return np.stack([((float(v) / sc[:, ch] - m[ch]) / s[ch]).astype(F32) for ch, v, _ in events], 1)


def counts(xs, tgt, thr, events, defect=None):
    """xs [T, S, B, C, H, W], tgt [T, B, C, H, W], thr [B, K] -> n, o [T, B, K, H, W] int64 by direct comparison (in the dtype of xs)."""
    n, o = [], []
    for k, (ch, _, d) in enumerate(events):
        th = thr[:, k].astype(xs.dtype).reshape(1, 1, -1, 1, 1)
        x, y = xs[:, :, :, ch], tgt[:, :, ch]
        if defect == "non_strict":
            cx, cy = (x >= th, y >= th[:, 0]) if d == ">" else (x <= th, y <= th[:, 0])
        else:
            cx, cy = (x > th, y > th[:, 0]) if d == ">" else (x < th, y < th[:, 0])
        nk, ok = cx.sum(1).astype(np.int64), cy.astype(np.int64)
        if defect == "target_member":
            nk = nk + ok
        n.append(nk)
        o.append(ok)
    return np.stack(n, 2), np.stack(o, 2)


def box_sums(f, w, defect=None):
    """f [.., H, W] int64 -> the sums over the w x w box centred on every pixel, zeros outside the field: the sum of the w^2 shifted
    slices of the zero-padded field."""
    r = w // 2
    hi = r + 1 if defect == "even_window" else r
    Hh, Ww = f.shape[-2:]
    if defect == "wrap":
        return sum(np.roll(f, (-dy, -dx), (-2, -1)) for dy in range(-r, hi + 1) for dx in range(-r, hi + 1))
    pad = np.zeros(f.shape[:-2] + (Hh + r + hi, Ww + r + hi), np.int64)
    pad[..., r:r + Hh, r:r + Ww] = f
    out = np.zeros(f.shape, np.int64)
    for dy in range(r + hi + 1):
        for dx in range(r + hi + 1):
            out += pad[..., dy:dy + Hh, dx:dx + Ww]
    return out


def tables(n, o, S, defect=None):
    """-> rel_count, rel_hit [.., S + 1] int64 by bincount over the last two axes of n, o [.., H, W]."""
    lead = n.shape[:-2]
    nf, of = n.reshape(-1, n.shape[-2] * n.shape[-1]), o.reshape(-1, n.shape[-2] * n.shape[-1])
    nb = S + 2 if defect == "target_member" else S + 1
    cnt = np.stack([np.bincount(a, minlength=nb)[:S + 1] for a in nf])
    hit = cnt.copy() if defect == "hit_ungated" else np.stack([np.bincount(a[b == 1], minlength=nb)[:S + 1] for a, b in zip(nf, of)])
    return cnt.reshape(lead + (S + 1,)).astype(np.int64), hit.reshape(lead + (S + 1,)).astype(np.int64)


def raw_fss(boxes, defect=None, tile=32):
    """boxes: per width (Nf, No) [.., H, W] -> [.., NS, 3] int64 = (sum Nf^2, sum Nf No, sum No^2) over the pixels."""
    n = boxes[0][0]
    keep = np.ones(n.shape[-2:], np.int64)
    if defect == "drop_last":                                                 # the last row and column of every tile are not summed
        keep[tile - 1::tile, :] = 0
        keep[:, tile - 1::tile] = 0
    out = []
    for nf, no in boxes:
        out.append(np.stack([(nf * nf * keep).sum((-2, -1)), (nf * no * keep).sum((-2, -1)), (no * no * keep).sum((-2, -1))], -1))
    return np.stack(out, -2)


def _roc_area(n, o):
    """Mann-Whitney with half ties over flat n, o; NaN without an event or a non-event."""
    e, q = np.sort(n[o == 1]), np.sort(n[o == 0])
    if e.size == 0 or q.size == 0:
        return float("nan")
    less = np.searchsorted(q, e, side="left").astype(np.int64)
    leq = np.searchsorted(q, e, side="right").astype(np.int64)
    return float(int((less + leq).sum())) / (2.0 * e.size * q.size)


def _pixel_scores(n, o, S):
    """n, o flat int64 (the pooled pixels) -> dict of fp64 scalars, obs_freq [S + 1] and the ROC curve [S + 2]."""
    N = n.size
    Sf = float(S)
    out = {"brier": float(int(((n - S * o) ** 2).sum())) / (Sf * Sf * N)}
    ob = float(int(o.sum())) / N
    cnt, hit = np.bincount(n, minlength=S + 1)[:S + 1], np.bincount(n[o == 1], minlength=S + 1)[:S + 1]
    oj = np.where(cnt > 0, hit / np.maximum(cnt, 1), np.nan)
    nn = np.minimum(n, S)
    out["brier_rel"] = float(((n / Sf - oj[nn]) ** 2).mean())
    out["brier_res"] = float(((oj[nn] - ob) ** 2).mean())
    out["brier_unc"] = ob * (1.0 - ob)
    out["base_rate"] = ob
    out["fcst_rate"] = float(int(n.sum())) / (Sf * N)
    out["roc_area"] = _roc_area(n, o)
    out["obs_freq"] = oj
    n1, n0 = int(o.sum()), N - int(o.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        out["roc_hit_rate"] = np.array([float(((n >= j) & (o == 1)).sum()) for j in range(S + 2)]) / np.float64(n1)
        out["roc_false_rate"] = np.array([float(((n >= j) & (o == 0)).sum()) for j in range(S + 2)]) / np.float64(n0)
    return out


def _fss_fractions(boxes, idx, S, scales):
    """boxes: per width (Nf, No); idx selects the planes -> fss [NS] in fp64 from the fractions, the sums over all selected pixels."""
    out = []
    for w, (nf, no) in zip(scales, boxes):
        f = nf[idx] / float(S * w * w)
        g = no[idx] / float(w * w)
        den = (f * f).sum() + (g * g).sum()
        out.append(1.0 - ((f - g) ** 2).sum() / den if den > 0 else float("nan"))
    return np.array(out)


def reference(xs, tgt, thr, events, scales, t_start, defect=None):
    """-> dict shaped as EnsembleEvents' outputs (case axis first), integers int64, floats fp64, plus n, o [T, B, K, H, W] and
    tsum_steps [T, 4, B, K, H, W] (the running per-pixel sums after every step; steps before t_start hold zeros)."""
    Tn, S, B = xs.shape[:3]
    K, NS = len(events), len(scales)
    n, o = counts(xs, tgt, thr, events, defect)
    Sd = S + 1 if defect == "s_plus_one" else S
    cnt, hit = tables(n, o, S, defect)                                        # [T, B, K, S + 1]
    boxes = [(box_sums(n, w, defect), box_sums(o, w, defect)) for w in scales]
    raw = raw_fss(boxes, defect)                                              # [T, B, K, NS, 3]
    ref = {"n": n, "o": o, "rel_count": cnt.transpose(1, 0, 2, 3), "rel_hit": hit.transpose(1, 0, 2, 3),
           "fss_raw": raw.transpose(1, 0, 2, 3, 4)}
    for key in STEP_KEYS:
        ref[key] = np.zeros((B, Tn, K))
    ref["fss"] = np.zeros((B, Tn, K, NS))
    nm = np.minimum(n, S)                                                     # (target_member: the count S + 1 scores as S)
    for t in range(Tn):
        for b in range(B):
            for k in range(K):
                sc = _pixel_scores(nm[t, b, k].ravel(), o[t, b, k].ravel(), Sd)
                for key in STEP_KEYS:
                    ref[key][b, t, k] = sc[key]
                ref["fss"][b, t, k] = _fss_fractions(boxes, (t, b, k), Sd, scales)
    tt = slice(t_start, Tn)
    Tw = Tn - t_start
    ref["time_rel_count"], ref["time_rel_hit"] = ref["rel_count"][:, tt].sum(1), ref["rel_hit"][:, tt].sum(1)
    for key in TIME_TABLE_KEYS:
        ref[key] = np.zeros((B, K))
    ref["time_fss"] = np.zeros((B, K, NS))
    ref["time_rel_obs_freq"] = np.zeros((B, K, S + 1))
    ref["time_roc_hit_rate"], ref["time_roc_false_rate"] = np.zeros((B, K, S + 2)), np.zeros((B, K, S + 2))
    for b in range(B):
        for k in range(K):
            sc = _pixel_scores(nm[tt, b, k].ravel(), o[tt, b, k].ravel(), Sd)
            for key in ("brier", "brier_rel", "brier_res", "brier_unc", "base_rate", "roc_area"):
                ref["time_" + key][b, k] = sc[key]
            ref["time_fss_uniform"][b, k] = 0.5 + sc["base_rate"] / 2
            ref["time_rel_obs_freq"][b, k] = sc["obs_freq"][:S + 1]
            ref["time_roc_hit_rate"][b, k], ref["time_roc_false_rate"][b, k] = sc["roc_hit_rate"][:S + 2], sc["roc_false_rate"][:S + 2]
            ref["time_fss"][b, k] = _fss_fractions(boxes, (tt, b, k), Sd, scales)
    ref["time_event_count"], ref["time_obs_count"] = n[tt].sum(0), o[tt].sum(0)
    ref["time_brier_map"] = ((n[tt] - Sd * o[tt]) ** 2).sum(0) / (float(Sd) * float(Sd) * Tw)
    steps = np.zeros((Tn, 4, B, K) + n.shape[-2:], np.int64)
    for t in range(t_start, Tn):
        w = slice(t_start, t + 1)
        steps[t] = np.stack([n[w].sum(0), o[w].sum(0), (n[w] * n[w]).sum(0), (n[w] * o[w]).sum(0)])
    ref["tsum_steps"] = steps
    ref["event_scales"] = np.array(scales, np.int64)
    return ref


@functools.lru_cache(maxsize=None)
def int_reference(idx):
    case = LONG_CASE if idx == len(INT_TABLE) else INT_TABLE[idx]
    xs, tgt, events, t_start = int_case_inputs(case, idx)
    return reference(xs, tgt, thresholds(events, case[1], case[2]), events, case[8], t_start)


@functools.lru_cache(maxsize=None)
def real_reference(idx):
    S, B, Cc, hw, kind, with_u, events, scales = REAL_TABLE[idx]
    xs, tgt, u = real_case_inputs(idx)
    thr = thresholds(events, B, Cc, MU, SD, None if u is None else u.numpy())
    return reference(xs, tgt, thr, events, scales, idx % 2)


def simulate(n, o, S, scales, plan, defect=None):
    """The device scheme in numpy, driven by the launch plan: per tile the region tile + halo of n and o (zeros outside the field)
    into tables of `rows` x `pitch` int32 with a zero row and column, a row prefix pass, a column prefix pass, every box sum from
    four entries, int64 sums over the tiles; the tables from the tiles' own pixels.  n, o [H, W] int64 -> (rel_count, rel_hit
    [S + 1], fss_raw [NS, 3])."""
    Hh, Ww = n.shape
    TH, TW, R = plan["TH"], plan["TW"], plan["halo"]
    assert plan["rows"] == TH + 2 * R + 1 and plan["pitch"] == TW + 2 * R + 1 and R == max(scales) // 2
    cnt, hit = np.zeros(S + 1, np.int64), np.zeros(S + 1, np.int64)
    raw = np.zeros((len(scales), 3), np.int64)
    seen = np.zeros((Hh, Ww), np.int64)
    for ty in range(plan["NTY"]):
        for tx in range(plan["NTX"]):
            tabs = []
            for f in (n, o):
                tab = np.zeros((plan["rows"], plan["pitch"]), np.int64)
                for ry in range(TH + 2 * R):
                    gy = ty * TH - R + ry
                    if 0 <= gy < Hh:
                        x0, x1 = max(0, tx * TW - R), min(Ww, tx * TW + TW + R)
                        tab[ry + 1, x0 - (tx * TW - R) + 1:x1 - (tx * TW - R) + 1] = f[gy, x0:x1]
                tab = tab.cumsum(1).cumsum(0)
                assert int(tab.max()) < 2 ** 31
                tabs.append(tab.astype(np.int32).astype(np.int64))
            th_, tw_ = min(TH, Hh - ty * TH), min(TW, Ww - tx * TW)
            if defect == "drop_last":
                th_, tw_ = th_ - (th_ == TH), tw_ - (tw_ == TW)
            ys, xs_ = np.arange(th_).reshape(-1, 1), np.arange(tw_).reshape(1, -1)
            seen[ty * TH:ty * TH + th_, tx * TW:tx * TW + tw_] += 1
            tn_, to_ = n[ty * TH:ty * TH + th_, tx * TW:tx * TW + tw_], o[ty * TH:ty * TH + th_, tx * TW:tx * TW + tw_]
            cnt += np.bincount(tn_.ravel(), minlength=S + 1)
            hit += np.bincount(tn_[to_ == 1].ravel(), minlength=S + 1)
            for s, w in enumerate(scales):
                r = w // 2
                y0, y1, x0, x1 = ys + R - r, ys + R + r + 1, xs_ + R - r, xs_ + R + r + 1
                nf, no = [tb[y1, x1] - tb[y0, x1] - tb[y1, x0] + tb[y0, x0] for tb in tabs]
                raw[s] += [(nf * nf).sum(), (nf * no).sum(), (no * no).sum()]
    return cnt, hit, raw, seen


def check_floats(got, ref, what):
    """Every float32 output within 2^-24 |ref| + 2^-40 of the reference, NaNs where the reference has them -> the worst share."""
    worst = 0.0
    for key in FLOAT_KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key], np.float64)
        assert g.dtype == F32 and g.shape == r.shape, "%s %s: %s %s against %s" % (what, key, g.dtype, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s %s: NaNs differ" % (what, key)
        ok = ~np.isnan(r)
        share = np.abs(g.astype(np.float64)[ok] - r[ok]) / (U24 * np.abs(r[ok]) + TOL_ABS)
        if share.size:
            assert float(share.max()) <= 1.0, "%s %s: worst error is %.3f of its bound" % (what, key, float(share.max()))
            worst = max(worst, float(share.max()))
    return worst


def check_integers(got, ref, what):
    for key in INT_KEYS + ("event_scales",):
        g = np.asarray(got[key])
        assert g.dtype == np.int64 and g.shape == ref[key].shape and np.array_equal(g, ref[key]), "%s %s" % (what, key)


def check_identities(got, S, scales, hw, what):
    """fss_raw at w = 1 against the tables (A - 2 S Bx + S^2 Cc = S^2 HW brier, in integers) and brier = rel - res + unc."""
    j = np.arange(S + 1, dtype=np.int64)
    cnt, hit = np.asarray(got["rel_count"]), np.asarray(got["rel_hit"])
    num = (cnt * j * j - 2 * S * hit * j + S * S * hit).sum(-1)
    if 1 in scales:
        raw = np.asarray(got["fss_raw"])[..., list(scales).index(1), :]
        assert np.array_equal(raw[..., 0] - 2 * S * raw[..., 1] + S * S * raw[..., 2], num), "%s: the Brier identity at w = 1" % what
        assert np.array_equal(raw[..., 0], (cnt * j * j).sum(-1)) and np.array_equal(raw[..., 2], hit.sum(-1)), what
    assert np.array_equal(cnt.sum(-1), np.full(cnt.shape[:-1], hw[0] * hw[1])), "%s: the table does not hold every pixel once" % what
    for pre in ("", "time_"):
        g = {k: np.asarray(got[pre + k]).astype(np.float64) for k in ("brier", "brier_rel", "brier_res", "brier_unc")}
        assert float(np.abs(g["brier"] - (g["brier_rel"] - g["brier_res"] + g["brier_unc"])).max()) <= 2.0 ** -22, "%s %sbrier" % (what, pre)
