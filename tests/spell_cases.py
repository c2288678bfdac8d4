"""Cases and references of the ensemble event durations (tmg_spell.hip / tmg_ops.EnsembleSpells / utils.modelPredSpells).

The reference is written from the definitions in int64 numpy: the indicator series of every (row, case, event, pixel), run-length
encoded by np.diff on the series padded with the complement of its ends, every run classed as complete, left, right or both.  A
second, independent statement (`regex_tables`) matches 1+ / 0+ on the series written as a string; tests/test_spells_cpu.py holds
the two against each other, so the reference itself is tested.  `host_reference` restates tmg_ops.spell_outputs with loops in fp64.

MUTATIONS names the defects the comparison must see: each changes at least one compared table on the case set (test_spells_cpu.py).

Data: integer-valued fields with the thresholds ON data values (ties: strictness shows), AR(1)-in-time real fields (run lengths
vary), and planted pixels in member 0 and in the target of event 0: always in, never in, alternating every step, and one interior
spell each of length L - 1, L and L + 1 where the window holds them."""
import functools
import re

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
TOL_ABS = 2.0 ** -40
TABLE_KEYS = ("spell_hist", "spell_len", "spell_cens", "spell_cens_len")
MAP_KEYS = ("time_in_count", "time_spell_count", "time_longest_sum", "time_longest_max", "target_in_count", "target_spell_count",
            "target_longest")
INT_HOST_KEYS = ("spell_mean_below", "spell_mean_equal", "spell_mean_valid")
FLOAT_HOST_KEYS = ("spell_mean", "spell_survival", "spell_p11", "spell_p01", "spell_markov_mean", "spell_w1", "spell_w1_pooled")
FLOAT_MAP_KEYS = ("time_longest_mean", "time_mean_duration", "target_mean_duration")
ALL_KEYS = TABLE_KEYS + MAP_KEYS + INT_HOST_KEYS + FLOAT_HOST_KEYS + FLOAT_MAP_KEYS + ("spell_bins",)
MUTATIONS = ("censored_complete", "non_strict", "length_off_by_one", "overflow_dropped", "left_right_swapped", "nan_in_event",
             "longest_complete_only")
COMPLETE, LEFT, RIGHT, BOTH = 0, 1, 2, 3


def group(K, L):
    """The member group size of tmg_ens_spell_plan: the rows whose LDS table [K][2][L + 3] int32 stays within 16 KiB, at most 8."""
    return min(8, 16384 // (4 * K * 2 * (L + 3)))


def events_for(Cc, K):
    """K = 1: reverse flow; K = 4: both directions, thresholds on integer data values, every channel of 2..4 reached."""
    return ((0, 0.0, "<"),) if K == 1 else ((0, 0.0, "<"), (1, 1.0, ">"), (Cc - 1, 0.0, ">"), (0, 1.0, "<"))


# (S, B, C, (H, W), K, Tn, L, kind, padded): HW 35, 256, 257, 561; S 1, 2 and G - 1, G, G + 1, 2 G + 1 (G = 8 at L = 4, 7 at K = 4 and
# L = 64); B 1 and 3; C 2, 3, 4; padded: the chunk and the target are channel slices at offset 1 of 4-channel storage
TABLE = [
    (1, 1, 2, (5, 7), 1, 2, 4, "int", False),
    (2, 3, 3, (5, 7), 4, 3, 4, "int", True),
    (7, 1, 3, (16, 16), 4, 9, 4, "ar1", False),
    (8, 3, 4, (1, 257), 1, 9, 4, "int", False),
    (9, 1, 2, (17, 33), 4, 9, 4, "ar1", True),
    (17, 3, 3, (5, 7), 4, 9, 4, "int", True),
    (5, 1, 3, (16, 16), 1, 9, 1, "ar1", True),
    (15, 1, 4, (5, 7), 4, 9, 64, "int", False),
    (3, 3, 3, (1, 257), 4, 3, 4, "ar1", False),
    (2, 1, 2, (17, 33), 1, 2, 4, "int", False),
]
LONG_CASE = (1, 1, 2, (5, 7), 1, 300, 32, "ar1", False)                        # a window beyond 8 bits of run length
NONFINITE_CASE = (4, 3, 3, (5, 7), 4, 9, 4, "ar1", True)


def chunk_sizes(S, kind):
    """kind 0: one chunk; 1: one member per chunk; 2: an uneven split."""
    if kind == 0 or S == 1:
        return [S]
    if kind == 1:
        return [1] * S
    a = max(1, S // 3)
    return [a, S - a] if S - a <= a + 1 or S < 4 else [a, 1, S - a - 1]


def plant(xs, tgt, events, L):
    """Planted pixels 0..5 of channel events[0] in member 0 of every case and in the target: always in, never in, alternating, and
    an interior spell of length L - 1, L, L + 1 from step 1 on (the ones of length >= 1 that end before the last step)."""
    Tn = xs.shape[0]
    ch, val, d = events[0]
    vin, vout = (val - 1.5, val + 1.5) if d == "<" else (val + 1.5, val - 1.5)   # (off every threshold of events_for)
    for field in (xs[:, 0], tgt):                                              # [Tn, B, C, H, W]
        flat = field.reshape(Tn, field.shape[1], field.shape[2], -1)
        flat[:, :, ch, 0] = vin
        flat[:, :, ch, 1] = vout
        flat[:, :, ch, 2] = np.where(np.arange(Tn) % 2 == 0, vin, vout).reshape(Tn, 1)
        for i, n in enumerate((L - 1, L, L + 1)):
            if n >= 1 and 1 + n <= Tn - 1:
                s = np.full(Tn, vout)
                s[1:1 + n] = vin
                flat[:, :, ch, 3 + i] = s.reshape(Tn, 1)


def make_inputs(case, seed):
    """-> xs [Tn, S, B, C, H, W], tgt [Tn, B, C, H, W] float32 (raw normalised values; the tests use out_mu = 0, out_std = 1)."""
    S, B, Cc, (Hh, Ww), K, Tn, L, kind, _ = case
    rs = np.random.RandomState(seed)
    shape = (Tn, S + 1, B, Cc, Hh, Ww)
    if kind == "int":
        x = rs.randint(-2, 3, size=shape).astype(F32)
    else:
        a = 0.8
        x = np.empty(shape, np.float64)
        x[0] = rs.standard_normal(shape[1:])
        for t in range(1, Tn):
            x[t] = a * x[t - 1] + np.sqrt(1 - a * a) * rs.standard_normal(shape[1:])
        x = (x + 0.3).astype(F32)
    xs, tgt = np.ascontiguousarray(x[:, :S]), np.ascontiguousarray(x[:, S])
    plant(xs, tgt, events_for(Cc, K), L)
    return xs, tgt


def plant_nonfinite(xs, tgt, seed):
    """NaN, +Inf and -Inf at one entry in sixteen of the members and of the target, in place."""
    rs = np.random.RandomState(seed)
    for v in (xs, tgt):
        r = rs.randint(0, 48, size=v.shape)
        v[r == 0] = np.nan
        v[r == 1] = np.inf
        v[r == 2] = -np.inf


@functools.lru_cache(maxsize=None)
def inputs(idx):
    xs, tgt = make_inputs(TABLE[idx], 100 + idx)
    xs.setflags(write=False)
    tgt.setflags(write=False)
    return xs, tgt


def thresholds(events, B):
    """thr [B, K] float32 for out_mu = 0, out_std = 1 and no u: the values themselves."""
    return np.array([[v for _, v, _ in events]] * B, dtype=F32)


def indicators(xs, tgt, thr, events, mutate=None):
    """-> e [R, B, K, HW, Tn] bool: rows 0..S-1 the members, row S the target; strict float32 comparisons."""
    x = np.concatenate([xs, tgt[:, None]], axis=1)                             # [Tn, R, B, C, H, W]
    Tn, R, B = x.shape[:3]
    out = []
    for k, (ch, _, d) in enumerate(events):
        v = x[:, :, :, ch].reshape(Tn, R, B, -1)
        th = np.asarray(thr)[:, k].reshape(1, 1, B, 1)
        with np.errstate(invalid="ignore"):
            if mutate == "non_strict":
                e = v >= th if d == ">" else v <= th
            else:
                e = v > th if d == ">" else v < th
        if mutate == "nan_in_event":
            e = e | np.isnan(v)
        out.append(e)
    return np.ascontiguousarray(np.stack(out, 0).transpose(2, 3, 0, 4, 1))     # [K, Tn, R, B, HW] -> [R, B, K, HW, Tn]


def run_list(E):
    """E [N, Tn] bool -> (series, start, length, polarity, class) of every run, int64: np.diff on the series padded with the
    complement of its ends marks a boundary before step 0, after step Tn - 1 and at every change."""
    N, Tn = E.shape
    e = E.astype(np.int8)
    pad = np.concatenate([1 - e[:, :1], e, 1 - e[:, -1:]], axis=1)
    n, i = np.nonzero(np.diff(pad, axis=1))                                    # boundaries i in 0..Tn, sorted within a series
    first = i < Tn                                                             # every boundary but a series' last starts a run
    series, start = n[first], i[first]
    end = i[np.flatnonzero(first) + 1]                                         # the series' next boundary ends it
    assert np.array_equal(n[np.flatnonzero(first) + 1], series)
    length = (end - start).astype(np.int64)
    pol = e[series, start].astype(np.int64)
    cls = np.where((start == 0) & (end == Tn), BOTH, np.where(start == 0, LEFT, np.where(end == Tn, RIGHT, COMPLETE)))
    return series.astype(np.int64), start.astype(np.int64), length, pol, cls.astype(np.int64)


def tables_from_runs(series, length, pol, cls, shape, L, mutate=None):
    """shape = (R, B, K, HW): the run list -> the four tables [B, K, R, 2, ..] int64."""
    R, B, K, HW = shape
    r, b, k, _ = np.unravel_index(series, shape)
    if mutate == "length_off_by_one":
        length = length + 1
    if mutate == "censored_complete":
        cls = np.zeros_like(cls)
    if mutate == "left_right_swapped":
        cls = np.where(cls == LEFT, RIGHT, np.where(cls == RIGHT, LEFT, cls))
    hist = np.zeros((B, K, R, 2, L), np.int64)
    slen = np.zeros((B, K, R, 2), np.int64)
    cens = np.zeros((B, K, R, 2, 3), np.int64)
    clen = np.zeros((B, K, R, 2, 3), np.int64)
    c = cls == COMPLETE
    keep = c & (length < L) if mutate == "overflow_dropped" else c
    np.add.at(hist, (b[keep], k[keep], r[keep], pol[keep], np.minimum(length[keep], L) - 1), 1)
    np.add.at(slen, (b[c], k[c], r[c], pol[c]), length[c])
    z = ~c
    np.add.at(cens, (b[z], k[z], r[z], pol[z], cls[z] - 1), 1)
    np.add.at(clen, (b[z], k[z], r[z], pol[z], cls[z] - 1), length[z])
    return {"spell_hist": hist, "spell_len": slen, "spell_cens": cens, "spell_cens_len": clen}


def reference(xs, tgt, thr, events, L, mutate=None):
    """The device's outputs from the definitions -> dict of int64 arrays: TABLE_KEYS and MAP_KEYS ([B, K, H, W])."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    K, HW = len(events), Hh * Ww
    E = indicators(xs, tgt, thr, events, mutate)                               # [R, B, K, HW, Tn]
    shape = E.shape[:4]
    series, start, length, pol, cls = run_list(E.reshape(-1, Tn))
    out = tables_from_runs(series, length, pol, cls, shape, L, mutate)
    N = int(np.prod(shape))
    sp = pol == 1
    nsp = np.bincount(series[sp], minlength=N).astype(np.int64).reshape(shape)
    lsel = sp & (cls == COMPLETE) if mutate == "longest_complete_only" else sp
    longest = np.zeros(N, np.int64)
    np.maximum.at(longest, series[lsel], length[lsel])
    longest = longest.reshape(shape)
    cin = E.sum(-1).astype(np.int64)
    m = lambda v: np.ascontiguousarray(v).reshape(B, K, Hh, Ww)                # noqa: E731
    out["time_in_count"], out["time_spell_count"] = m(cin[:S].sum(0)), m(nsp[:S].sum(0))
    out["time_longest_sum"], out["time_longest_max"] = m(longest[:S].sum(0)), m(longest[:S].max(0))
    out["target_in_count"], out["target_spell_count"], out["target_longest"] = m(cin[S]), m(nsp[S]), m(longest[S])
    return out


@functools.lru_cache(maxsize=None)
def case_reference(idx):
    S, B, Cc, hw, K, Tn, L, kind, _ = TABLE[idx]
    xs, tgt = inputs(idx)
    ev = events_for(Cc, K)
    return reference(xs, tgt, thresholds(ev, B), ev, L)


def regex_tables(xs, tgt, thr, events, L):
    """The second statement: every series as a string of 0 / 1, its runs the matches of 1+|0+ -> the four tables and the maps."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    K, HW = len(events), Hh * Ww
    E = indicators(xs, tgt, thr, events)
    R = S + 1
    out = {"spell_hist": np.zeros((B, K, R, 2, L), np.int64), "spell_len": np.zeros((B, K, R, 2), np.int64),
           "spell_cens": np.zeros((B, K, R, 2, 3), np.int64), "spell_cens_len": np.zeros((B, K, R, 2, 3), np.int64)}
    maps = {key: np.zeros((B, K, HW), np.int64) for key in MAP_KEYS}
    for r in range(R):
        for b in range(B):
            for k in range(K):
                for p in range(HW):
                    s = "".join("1" if v else "0" for v in E[r, b, k, p])
                    longest = nsp = 0
                    for mt in re.finditer(r"1+|0+", s):
                        a, z = mt.span()
                        pol, n = int(s[a]), z - a
                        if a > 0 and z < Tn:
                            out["spell_hist"][b, k, r, pol, min(n, L) - 1] += 1
                            out["spell_len"][b, k, r, pol] += n
                        else:
                            c = 2 if (a == 0 and z == Tn) else (0 if a == 0 else 1)
                            out["spell_cens"][b, k, r, pol, c] += 1
                            out["spell_cens_len"][b, k, r, pol, c] += n
                        if pol:
                            nsp += 1
                            longest = max(longest, n)
                    if r < S:
                        maps["time_in_count"][b, k, p] += s.count("1")
                        maps["time_spell_count"][b, k, p] += nsp
                        maps["time_longest_sum"][b, k, p] += longest
                        maps["time_longest_max"][b, k, p] = max(maps["time_longest_max"][b, k, p], longest)
                    else:
                        maps["target_in_count"][b, k, p] = s.count("1")
                        maps["target_spell_count"][b, k, p] = nsp
                        maps["target_longest"][b, k, p] = longest
    for key, v in maps.items():
        out[key] = v.reshape(B, K, Hh, Ww)
    return out


def transitions(xs, tgt, thr, events):
    """n_xy [B, K, R, 2, 2] int64: the steps t in 0..Tn-2 with (e_t, e_t+1) = (x, y), counted directly."""
    E = indicators(xs, tgt, thr, events).astype(np.int64)                      # [R, B, K, HW, Tn]
    a, z = E[..., :-1], E[..., 1:]
    n = np.stack([np.stack([((a == x) & (z == y)).sum((-2, -1)) for y in (0, 1)], -1) for x in (0, 1)], -2)   # [R, B, K, 2, 2]
    return n.transpose(1, 2, 0, 3, 4)


def check_identities(t, Tn, HW, n_xy=None):
    """The four identities of the tables, per (case, event, row); with n_xy also against the directly counted transitions."""
    runs = t["spell_hist"].sum(-1) + t["spell_cens"].sum(-1)
    steps = t["spell_len"] + t["spell_cens_len"].sum(-1)
    assert np.array_equal(steps.sum(-1), np.full(steps.shape[:-1], Tn * HW))
    n11, n00 = steps[..., 1] - runs[..., 1], steps[..., 0] - runs[..., 0]
    c = t["spell_cens"]
    n01 = runs[..., 1] - c[..., 1, 0] - c[..., 1, 2]
    n10 = runs[..., 1] - c[..., 1, 1] - c[..., 1, 2]
    assert (n11 >= 0).all() and (n00 >= 0).all() and (n01 >= 0).all() and (n10 >= 0).all()
    assert np.array_equal(n11 + n00 + n01 + n10, np.full(n11.shape, (Tn - 1) * HW))
    # a gap that starts after step 0 follows a spell, and the other way round
    assert np.array_equal(n10, runs[..., 0] - c[..., 0, 0] - c[..., 0, 2]) and np.array_equal(n01, runs[..., 0] - c[..., 0, 1] - c[..., 0, 2])
    if n_xy is not None:
        assert np.array_equal(n_xy[..., 1, 1], n11) and np.array_equal(n_xy[..., 0, 0], n00)
        assert np.array_equal(n_xy[..., 0, 1], n01) and np.array_equal(n_xy[..., 1, 0], n10)


def host_reference(t, S, maps=None):
    """tmg_ops.spell_outputs restated with loops over (case, event) in fp64 -> dict of float64 / int64 arrays."""
    hist, slen, cens, clen = (t[k] for k in TABLE_KEYS)
    B, K, R, _, L = hist.shape
    nan = float("nan")
    o = {"spell_mean": np.full((B, K, R, 2), nan), "spell_survival": np.full((B, K, R, 2, L), nan), "spell_p11": np.full((B, K, R), nan),
         "spell_p01": np.full((B, K, R), nan), "spell_markov_mean": np.full((B, K, R), nan), "spell_w1": np.full((B, K, S, 2), nan),
         "spell_w1_pooled": np.full((B, K, 2), nan), "spell_mean_below": np.zeros((B, K, 2), np.int64),
         "spell_mean_equal": np.zeros((B, K, 2), np.int64), "spell_mean_valid": np.zeros((B, K, 2), np.int64)}

    def w1(p, q):
        if p.sum() == 0 or q.sum() == 0:
            return nan
        fp, fq = np.cumsum(p.astype(np.float64) / p.sum()), np.cumsum(q.astype(np.float64) / q.sum())
        return float(np.abs(fp - fq).sum())

    for b in range(B):
        for k in range(K):
            for r in range(R):
                for pol in (0, 1):
                    h = hist[b, k, r, pol]
                    n = int(h.sum())
                    if n:
                        o["spell_mean"][b, k, r, pol] = float(slen[b, k, r, pol]) / n
                        for j in range(L):
                            o["spell_survival"][b, k, r, pol, j] = float(h[j:].sum()) / n
                ns = int(hist[b, k, r, 1].sum() + cens[b, k, r, 1].sum())
                ng = int(hist[b, k, r, 0].sum() + cens[b, k, r, 0].sum())
                n11 = int(slen[b, k, r, 1] + clen[b, k, r, 1].sum()) - ns
                n00 = int(slen[b, k, r, 0] + clen[b, k, r, 0].sum()) - ng
                n01 = ns - int(cens[b, k, r, 1, 0]) - int(cens[b, k, r, 1, 2])
                n10 = ns - int(cens[b, k, r, 1, 1]) - int(cens[b, k, r, 1, 2])
                if n11 + n10:
                    p11 = n11 / float(n11 + n10)
                    o["spell_p11"][b, k, r] = p11
                    o["spell_markov_mean"][b, k, r] = float("inf") if n10 == 0 else 1.0 / (1.0 - p11)
                if n01 + n00:
                    o["spell_p01"][b, k, r] = n01 / float(n01 + n00)
            for pol in (0, 1):
                ht = hist[b, k, S, pol]
                for m in range(S):
                    o["spell_w1"][b, k, m, pol] = w1(hist[b, k, m, pol], ht)
                o["spell_w1_pooled"][b, k, pol] = w1(hist[b, k, :S, pol].sum(0), ht)
                cT, lT = int(ht.sum()), int(slen[b, k, S, pol])
                for m in range(S):
                    cm, lm = int(hist[b, k, m, pol].sum()), int(slen[b, k, m, pol])
                    if cm:
                        o["spell_mean_valid"][b, k, pol] += 1
                        if cT:
                            o["spell_mean_below"][b, k, pol] += lm * cT < lT * cm
                            o["spell_mean_equal"][b, k, pol] += lm * cT == lT * cm
    if maps is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            o["time_longest_mean"] = maps["time_longest_sum"] / float(S)
            o["time_mean_duration"] = np.where(maps["time_spell_count"] > 0, maps["time_in_count"] / maps["time_spell_count"].astype(np.float64), nan)
            o["target_mean_duration"] = np.where(maps["target_spell_count"] > 0,
                                                 maps["target_in_count"] / maps["target_spell_count"].astype(np.float64), nan)
    return o


def mismatches(got, ref, keys):
    """The keys whose arrays are not the reference's bit for bit (dtype, shape, values)."""
    bad = []
    for key in keys:
        g, r = got.get(key), ref[key]
        if g is None or g.dtype != r.dtype or g.shape != r.shape or not np.array_equal(g, r):
            bad.append(key)
    return bad


def check_floats(got, ref, keys, what):
    """float32 outputs within 2^-24 |ref| + 2^-40 of the fp64 reference, NaN and infinities where it has them -> worst share."""
    worst = 0.0
    for key in keys:
        g, r = np.asarray(got[key]), np.asarray(ref[key], dtype=np.float64)
        assert g.dtype == F32 and g.shape == r.shape, "%s: %s is %s %s, expected float32 %s" % (what, key, g.dtype, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s: %s NaN pattern" % (what, key)
        inf = np.isinf(r)
        assert np.array_equal(g[inf].astype(np.float64), r[inf]), "%s: %s infinities" % (what, key)
        ok = np.isfinite(r)
        if ok.any():
            err = np.abs(g[ok].astype(np.float64) - r[ok])
            tol = U24 * np.abs(r[ok]) + TOL_ABS
            assert bool((err <= tol).all()), "%s: %s error %.3e of tolerance" % (what, key, float((err / tol).max()))
            worst = max(worst, float((err / tol).max()))
    return worst
