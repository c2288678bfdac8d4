"""The cases and the references of the distance-map verification tests (test_edt_cpu.py, test_edt_gpu.py).

The int64 reference is written from the definitions of include/tmglow_hip_edt.h: the distance along each row to the nearest set pixel
by broadcasting, then the minimum over the rows of drow^2 + g^2, math.isqrt for the fixed-point distance w, bincount for the
histograms.  It has two second statements: the all-pairs minimum over the set's pixels, and scipy.ndimage.distance_transform_edt
with the squared distance recomputed in integers from the indices it returns, where scipy imports.  The fp64 formulas of every host
output are restated here on numpy arrays.  Named mutations of the reference are the ways a kernel of this shape can go wrong; the
comparison the GPU test uses must catch each of them.

Two of the mutations one would name change no output, so no comparison can catch them; they are kept as EQUIVALENT and
test_edt_cpu.py shows the equivalence over every d2 up to 255^2 + 1 and every cutoff instead:
  hist_w8     the histogram bin formed as w >> 8 where min(floor(sqrt(d2)), c) is specified: below the cutoff w = floor(256 x) with
              x = sqrt(d2) and floor(floor(256 x) / 256) = floor(x); from the cutoff on w = 256 c.
  cutoff_gt   the cutoff compared with > where >= is specified: they part only at d2 = c^2, where isqrt(65536 c^2) = 256 c is the cut
              value itself."""
import fractions
import functools
import math

import numpy as np

U24 = 2.0 ** -24
TOL_ABS = 2.0 ** -40
INF = 1 << 30
NONE = 32768                                                                  # the row distance of a row without a set pixel: NONE^2 = INF
TIMED = (False, True, True)                                                   # the steps of every case: the first one is not timed
TILE = (64, 64)                                                               # the kernel's band of rows and strip of columns
QUANTILES = (0.5, 0.75, 0.9, 1.0)
PAIR = ("nA", "nO", "nAO", "sOA1", "sOA2", "sAO1", "sAO2", "sD1", "sD2", "hOA", "hAO")
SUMMARY = ("dist_med_miss", "dist_med_false", "dist_med", "dist_hausdorff", "dist_baddeley", "dist_csi")
FLOAT_KEYS = ("dist_med_miss", "dist_med_false", "dist_rms_miss", "dist_rms_false", "dist_med", "dist_hausdorff_miss",
              "dist_hausdorff_false", "dist_hausdorff", "dist_hausdorff_q", "dist_baddeley", "dist_baddeley1", "dist_csi", "dist_mean",
              "dist_std")
RAW_KEYS = ("dist_pair_raw", "dist_hist_raw")
STEP_KEYS = RAW_KEYS + FLOAT_KEYS + ("dist_valid",)
MAP_INT_KEYS = ("time_dist_member_sum", "time_dist_target_sum")
MAP_FLOAT_KEYS = ("time_dist_mean_map", "time_dist_bias_map")
META_KEYS = ("dist_cutoff", "dist_quantiles")
ALL_KEYS = STEP_KEYS + tuple("time_" + k for k in STEP_KEYS) + MAP_INT_KEYS + MAP_FLOAT_KEYS + META_KEYS
INT_KEYS = RAW_KEYS + ("dist_valid",) + tuple("time_" + k for k in RAW_KEYS + ("dist_valid",)) + MAP_INT_KEYS
ALL_FLOAT_KEYS = FLOAT_KEYS + tuple("time_" + k for k in FLOAT_KEYS) + MAP_FLOAT_KEYS
MUTATIONS = ("cityblock", "round_w", "swapped", "border_set", "nonstrict")
EQUIVALENT = ("cutoff_gt", "hist_w8")

# (S, B, C, (H, W), K, cutoff, kind, padded): padded feeds channel slices at offset 1 of 4-channel NaN-filled storage.  The fields sit
# on the edges of the 64-column strip (one word of the indicator) and of the 64-row band: 1, 2, 3 and 5 strips, 1 to 4 bands.
TABLE = [
    (1, 2, 2, (1, 1), 1, 1, "int", False),
    (2, 2, 3, (1, 7), 2, 5, "int", True),
    (5, 2, 3, (3, 130), 2, 5, "edges", True),
    (5, 1, 4, (2, 300), 1, 255, "corners", False),
    (5, 2, 3, (64, 64), 3, 5, "smooth", False),
    (2, 2, 2, (65, 63), 2, 1, "checker", True),
    (5, 2, 3, (70, 70), 2, 5, "empty", False),
    (2, 1, 4, (70, 70), 4, 255, "blobs", False),
    (2, 2, 3, (70, 70), 1, 5, "cutoff", True),
    (3, 2, 3, (70, 70), 2, 5, "nonfinite", False),
    (5, 1, 2, (200, 70), 1, 255, "corners", False),
    (2, 1, 3, (130, 130), 1, 5, "edges", False),
    (3, 2, 3, (70, 70), 2, 255, "int", False),
    (2, 1, 3, (70, 70), 1, 5, "sparse", False),
]
SHAPES = ((1, 1), (1, 7), (3, 130), (64, 64), (65, 63), (70, 70), (2, 300))      # of the statements' agreement
DENSITIES = (0.0, 0.0005, 0.02, 0.5, 1.0)


def chunk_sizes(S, kind):
    """0: one chunk; 1: one member per chunk; 2: an uneven split (2, 3 for five members)."""
    if kind == 0 or S == 1:
        return [S]
    if kind == 1:
        return [1] * S
    return [S // 2, S - S // 2]


def events_for(Cc, K):
    """K events on distinct channels, not in storage order, the directions alternating, the values on multiples of 0.5 (exact in
    float32: with out_mu = 0, out_std = 1, u = 1 the raw thresholds are the values)."""
    assert K <= Cc
    return tuple((Cc - 1 - e, 0.5 * e - 0.5, "<" if e % 2 == 0 else ">") for e in range(K))


def thresholds(case):
    S, B, Cc, hw, K, c, kind, _ = case
    return np.array(np.broadcast_to(np.array([v for _, v, _ in events_for(Cc, K)], np.float32), (B, K)))


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------------
def edge_pixels(hw, side):
    """A pixel on one side (0: the last of a word or band, 1: the first of the next) of every 64-column word edge and every 64-row band
    edge inside the field, as a boolean mask; empty for a field of one strip and one band."""
    Hh, Ww = hw
    m = np.zeros(hw, bool)
    for col in range(TILE[1] - 1 + side, Ww, TILE[1]):
        if side or col + 1 < Ww:
            m[(3 * col) % Hh, col] = True
    for row in range(TILE[0] - 1 + side, Hh, TILE[0]):
        if side or row + 1 < Hh:
            m[row, (5 * row) % Ww] = True
    return m


def set_mask(kind, hw, t, r, S, b, e, c, rng):
    """The event set of row r (S: the target) of step t, case b, event e, for the kinds that are given as sets."""
    Hh, Ww = hw
    i, j = np.mgrid[0:Hh, 0:Ww]
    m = np.zeros(hw, bool)
    if kind == "checker":
        return (i + j + r + t) % 2 == 0
    if kind == "corners":                                                     # one set pixel, in a corner: no early exit, the far diagonal
        q = (r + t + b + e) % 4
        m[(Hh - 1) * (q // 2), (Ww - 1) * (q % 2)] = True
        return m
    if kind == "blobs":                                                       # from (r, 0) the nearest along the row is far, along the column near
        m[r % Hh, Ww - 1 - (r + t) % 3] = True
        m[min(Hh - 1, 5 + t + e):min(Hh, 7 + t + e), 0:2] = True
        if r == S:
            m[Hh - 3:Hh - 1, Ww // 2:Ww // 2 + 3] = True
        return m
    if kind == "cutoff":                                                      # a pair of pixels exactly the cutoff apart, and one short of it
        if r == S:
            m[10, 10] = True
            return m
        di, dj = [(3, 4), (0, 5), (5, 0), (4, 3), (4, 2)][(r + t + b) % 5] if c == 5 else [(0, c), (c, 0), (c - 1, 0)][(r + t + b) % 3]
        m[min(Hh - 1, 10 + di), min(Ww - 1, 10 + dj)] = True
        return m
    if kind == "empty":                                                       # empty, sparse, dense and full sets against each other
        how = ("empty", "sparse", "full")[t % 3] if r == S else ("empty", "half", "full", "rare", "empty")[(r + b) % 5]
        if how == "empty":
            return m
        if how == "full":
            return ~m
        return rng.random(hw) < {"sparse": 0.02, "half": 0.5, "rare": 0.0005}[how]
    if kind == "edges":                                                       # a set pixel on each side of every word edge and band edge
        if r == S:
            return edge_pixels(hw, 0) | edge_pixels(hw, 1)
        m = edge_pixels(hw, (r + t) % 2)
        return np.roll(m, r, axis=0) if Hh > 1 and r % 3 == 2 else m
    if kind == "sparse":
        return rng.random(hw) < (0.0005 if (r + t) % 2 == 0 else 0.02)
    raise ValueError(kind)


def make_inputs(case, seed):
    """-> (xs [Tk, S, B, C, H, W], tgt [Tk, B, C, H, W]) float32.  The kinds given as sets put the event's value minus / plus one
    inside and, outside, the value itself (strictness shows) or the value plus / minus one, in a checkerboard."""
    S, B, Cc, hw, K, c, kind, _ = case
    Hh, Ww = hw
    Tk = len(TIMED)
    rng = np.random.default_rng(seed)
    ev = events_for(Cc, K)
    i, j = np.mgrid[0:Hh, 0:Ww]
    if kind == "int":                                                         # multiples of 0.5, the events' values among them
        full = rng.integers(-2, 3, (Tk, S + 1, B, Cc, Hh, Ww)).astype(np.float32) * 0.5
    elif kind == "smooth":
        ph = rng.uniform(0, 2 * np.pi, (Tk, S + 1, B, Cc, 1, 1))
        kx = rng.integers(1, 3, (Tk, S + 1, B, Cc, 1, 1))
        full = (1.5 * np.sin(2 * np.pi * (kx * j / max(Ww, 2) + i / max(Hh, 2)) + ph)).astype(np.float32)
    elif kind == "nonfinite":
        full = rng.normal(0, 1, (Tk, S + 1, B, Cc, Hh, Ww)).astype(np.float32)
        where = rng.random(full.shape)
        full[where < 0.02] = np.nan
        full[(where >= 0.02) & (where < 0.04)] = np.inf
        full[(where >= 0.04) & (where < 0.06)] = -np.inf
    else:
        full = np.zeros((Tk, S + 1, B, Cc, Hh, Ww), np.float32)
        for t in range(Tk):
            for r in range(S + 1):
                for b in range(B):
                    for e, (ch, v, d) in enumerate(ev):
                        m = set_mask(kind, hw, t, r, S, b, e, c, rng)
                        sg = -1.0 if d == "<" else 1.0
                        full[t, r, b, ch] = np.where(m, v + sg, np.where((i + j) % 2 == 0, v, v - sg))
    return np.ascontiguousarray(full[:, :S]), np.ascontiguousarray(full[:, S])


@functools.lru_cache(maxsize=None)
def inputs(idx):
    xs, tgt = make_inputs(TABLE[idx], 4200 + idx)
    xs.setflags(write=False)
    tgt.setflags(write=False)
    return xs, tgt


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def in_event(x, v, d, mutation=None):
    """The indicator of the event (value v, direction d) on the array x: strict, a non-finite value on the wrong side or NaN is out."""
    with np.errstate(invalid="ignore"):
        if mutation == "nonstrict":
            return x >= v if d == ">" else x <= v
        return x > v if d == ">" else x < v


def edt2(mask, mutation=None):
    """The squared Euclidean distance of every pixel to the set `mask` [H, W], int64: g by broadcasting, then the minimum over the
    rows of drow^2 + g^2; INF for an empty set."""
    Hh, Ww = mask.shape
    if mutation == "border_set":                                              # the field's border counted as set: a frame around it
        return edt2(np.pad(mask, 1, constant_values=True))[1:-1, 1:-1]
    cols = np.arange(Ww, dtype=np.int64)
    far = np.where(mask[:, None, :], np.abs(cols[None, :, None] - cols[None, None, :]), NONE)          # [H, j, set column]
    g = far.min(-1) if Ww else np.full((Hh, 0), NONE)                          # [H, W]
    rows = np.arange(Hh, dtype=np.int64)
    dr = np.abs(rows[:, None] - rows[None, :])[:, :, None]                     # [i, i', 1]
    if mutation == "cityblock":
        d = (dr + g[None]).min(1)
        return np.minimum(d * d, INF)
    return np.minimum((dr * dr + (g * g)[None]).min(1), INF)


def edt2_all_pairs(mask):
    """The second statement: the minimum over the set's pixels of the squared distance, row by row."""
    Hh, Ww = mask.shape
    si, sj = np.nonzero(mask)
    if si.size == 0:
        return np.full(mask.shape, INF, np.int64)
    si, sj = si.astype(np.int64)[:, None], sj.astype(np.int64)[:, None]
    cols = np.arange(Ww, dtype=np.int64)[None]
    return np.stack([((i - si) ** 2 + (cols - sj) ** 2).min(0) for i in range(Hh)])


def edt2_scipy(mask):
    """The third statement: scipy's transform for the nearest set pixel, the squared distance recomputed from its indices in integers."""
    from scipy import ndimage
    if not mask.any():
        return np.full(mask.shape, INF, np.int64)
    _, idx = ndimage.distance_transform_edt(~mask, return_indices=True)
    i, j = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
    return (i - idx[0].astype(np.int64)) ** 2 + (j - idx[1].astype(np.int64)) ** 2


def fixed(d2, c, mutation=None):
    """w = 256 c if d2 >= c^2 else isqrt(65536 d2), int64, elementwise."""
    d2 = np.asarray(d2, np.int64)
    vals, inv = np.unique(d2, return_inverse=True)
    if mutation == "round_w":
        w = np.array([int(round(256.0 * math.sqrt(int(v)))) for v in vals], np.int64)
    else:
        w = np.array([math.isqrt(65536 * int(v)) for v in vals], np.int64)
    cut = vals > c * c if mutation == "cutoff_gt" else vals >= c * c
    return np.where(cut, 256 * c, w)[inv].reshape(d2.shape)


def whole(d2, c, mutation=None):
    """min(floor(sqrt(d2)), c), int64, elementwise."""
    d2 = np.asarray(d2, np.int64)
    if mutation == "hist_w8":
        return fixed(d2, c) >> 8
    vals, inv = np.unique(d2, return_inverse=True)
    return np.minimum(np.array([math.isqrt(int(v)) for v in vals], np.int64), c)[inv].reshape(d2.shape)


def pair_of(dA, dO, c, mutation=None):
    """The eleven integers and the two histograms of one member's d2_A against the target's d2_O."""
    if mutation == "swapped":
        dA, dO = dO, dA
    a, o = dA == 0, dO == 0
    wA, wO = fixed(dA, c, mutation), fixed(dO, c, mutation)
    df = np.abs(wA - wO)
    pair = [a.sum(), o.sum(), (a & o).sum(), wA[o].sum(), (wA[o] ** 2).sum(), wO[a].sum(), (wO[a] ** 2).sum(), df.sum(), (df ** 2).sum(),
            dA[o].max() if o.any() else -1, dO[a].max() if a.any() else -1]
    if mutation == "swapped":
        pair[0], pair[1] = pair[1], pair[0]
    hist = [np.bincount(whole(dA[o], c, mutation), minlength=c + 1), np.bincount(whole(dO[a], c, mutation), minlength=c + 1)]
    return np.array(pair, np.int64), np.array(hist, np.int64)


def reference(xs, tgt, thr, events, c, mutation=None):
    """xs [Tk, S, B, C, H, W], tgt [Tk, B, C, H, W], thr [B, K] -> pair [B, Tk, K, S, 11], hist [B, Tk, K, S, 2, c + 1], d2_target
    [B, Tk, K, H, W], w_members [B, Tk, K, H, W] (the sum over the members of w_A) and w_target [B, Tk, K, H, W], int64."""
    Tk, S, B, Cc, Hh, Ww = xs.shape
    K = len(events)
    out = {"pair": np.zeros((B, Tk, K, S, len(PAIR)), np.int64), "hist": np.zeros((B, Tk, K, S, 2, c + 1), np.int64),
           "d2_target": np.zeros((B, Tk, K, Hh, Ww), np.int64), "w_members": np.zeros((B, Tk, K, Hh, Ww), np.int64),
           "w_target": np.zeros((B, Tk, K, Hh, Ww), np.int64)}
    for b in range(B):
        for t in range(Tk):
            for e, (ch, _, d) in enumerate(events):
                dO = edt2(in_event(tgt[t, b, ch], thr[b, e], d, mutation), mutation)
                out["d2_target"][b, t, e] = dO
                out["w_target"][b, t, e] = fixed(dO, c, mutation)
                for m in range(S):
                    dA = edt2(in_event(xs[t, m, b, ch], thr[b, e], d, mutation), mutation)
                    out["pair"][b, t, e, m], out["hist"][b, t, e, m] = pair_of(dA, dO, c, mutation)
                    out["w_members"][b, t, e] += fixed(dA, c, mutation)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(idx, mutation=None):
    S, B, Cc, hw, K, c, kind, _ = TABLE[idx]
    xs, tgt = inputs(idx)
    return reference(xs, tgt, thresholds(TABLE[idx]), events_for(Cc, K), c, mutation)


# ---- the host outputs in fp64 ---------------------------------------------------------------------------------------------------------------
def outputs_reference(pair, hist, S, Hh, Ww, c, quantiles, steps):
    """pair [..., S, 11], hist [..., S, 2, c + 1] int64 -> the keys of tmg_ops.dist_outputs, floats in fp64."""
    nA, nO, nAO, sOA1, sOA2, sAO1, sAO2, sD1, sD2, hOA, hAO = (pair[..., i].astype(np.float64) for i in range(len(PAIR)))
    P = float(Hh * Ww * steps)
    with np.errstate(invalid="ignore", divide="ignore"):
        o = {"dist_med_miss": sOA1 / (256.0 * nO), "dist_med_false": sAO1 / (256.0 * nA),
             "dist_rms_miss": np.sqrt(sOA2 / nO) / 256.0, "dist_rms_false": np.sqrt(sAO2 / nA) / 256.0}
        o["dist_med"] = np.maximum(o["dist_med_miss"], o["dist_med_false"])      # NaN when either is
        one, both = (nA == 0) ^ (nO == 0), (nA == 0) & (nO == 0)
        for key, h in (("dist_hausdorff_miss", hOA), ("dist_hausdorff_false", hAO)):
            o[key] = np.where(both, 0.0, np.where(one | (h >= INF), np.inf, np.sqrt(np.maximum(h, 0.0))))
        o["dist_hausdorff"] = np.maximum(o["dist_hausdorff_miss"], o["dist_hausdorff_false"])
        cum = np.cumsum(hist, -1)
        n = cum[..., -1]
        hq = np.full(n.shape + (len(quantiles),), np.nan)
        for pos in np.ndindex(*n.shape):
            for qi, q in enumerate(quantiles):
                if n[pos] > 0:
                    need = math.ceil(fractions.Fraction(q) * int(n[pos]))
                    hq[pos + (qi,)] = next(j for j in range(c + 1) if cum[pos + (j,)] >= need)
        o["dist_hausdorff_q"] = hq
        o["dist_baddeley"] = np.sqrt(sD2 / P) / 256.0
        o["dist_baddeley1"] = sD1 / (256.0 * P)
        o["dist_csi"] = nAO / (nA + nO - nAO)
        st = np.stack([o[k] for k in SUMMARY], -1)                             # [..., S, 6]
        ok = np.isfinite(st)
        cnt = ok.sum(-2)
        mean = np.where(ok, st, 0.0).sum(-2) / cnt
        dev = np.where(ok, st - mean[..., None, :], 0.0)
        o["dist_mean"] = mean
        o["dist_std"] = np.sqrt((dev * dev).sum(-2) / cnt)
    o["dist_valid"] = cnt.astype(np.int64)
    return o


def pooled(pair, hist, steps):
    """The tables [B, Tk, ...] pooled over `steps` (indices): sums added, the two maxima maxed."""
    p = pair[:, steps]
    return np.concatenate([p[..., :9].sum(1), p[..., 9:].max(1)], -1), hist[:, steps].sum(1)


def full_reference(ref, S, Hh, Ww, c, quantiles, timed=TIMED):
    """The reference's tables -> every key of EnsembleDistance.finalize."""
    out = {"dist_pair_raw": ref["pair"], "dist_hist_raw": ref["hist"], "dist_cutoff": np.int64(c), "dist_quantiles": np.array(quantiles, np.float64)}
    out.update(outputs_reference(ref["pair"], ref["hist"], S, Hh, Ww, c, quantiles, 1))
    on = [t for t, f in enumerate(timed) if f]
    tp, th = pooled(ref["pair"], ref["hist"], on)
    out["time_dist_pair_raw"], out["time_dist_hist_raw"] = tp, th
    for k, v in outputs_reference(tp, th, S, Hh, Ww, c, quantiles, len(on)).items():
        out["time_" + k] = v
    out["time_dist_member_sum"] = ref["w_members"][:, on].sum(1)
    out["time_dist_target_sum"] = ref["w_target"][:, on].sum(1)
    mean = out["time_dist_member_sum"].astype(np.float64) / (256.0 * S * len(on))
    out["time_dist_mean_map"] = mean
    out["time_dist_bias_map"] = mean - out["time_dist_target_sum"].astype(np.float64) / (256.0 * len(on))
    return out


def mismatches(got, want, keys):
    """The keys whose arrays are not equal bit for bit."""
    return [k for k in keys if not (np.asarray(got[k]).shape == np.asarray(want[k]).shape and np.array_equal(got[k], want[k]))]


def check_floats(got, want, keys, what):
    """Every float32 output within 2^-24 |ref| + 2^-40 of the fp64 formula, NaN where it is NaN and the same infinity where it is
    infinite -> the worst share of that tolerance."""
    worst = 0.0
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k], np.float64)
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (what, k)
        err, tol = np.abs(g[fin].astype(np.float64) - w[fin]), U24 * np.abs(w[fin]) + TOL_ABS
        assert bool((err <= tol).all()), "%s: %s off by %.3e of its tolerance" % (what, k, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()) if err.size else 0.0)
    return worst
