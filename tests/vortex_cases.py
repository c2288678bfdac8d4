"""Cases, references and named mutations of the ensemble vortex census (tests/test_vortices_cpu.py, tests/test_vortices_gpu.py).

Definitions (include/tmglow_hip_vortex.h, tmg_ops.EnsembleVortices).  fl() is one fp32 rounding.
  physical    fl(sc fl(fl(sd y) + mu)), zero outside the field; Sx, Sy the un-scaled 3x3 stencils in the summation order of
              pdf_cases._ddx / _ddy; ux = fl(Sx(u) rdx), uy = fl(Sy(u) rdy), vx, vy alike, rdx = fl(0.125 / fl(dx))
  w = fl(vx - uy) (pdf_cases.derived's vorticity), sn = fl(ux - vy), ss = fl(vx + uy), ow = fl(fl(fl(w w) - fl(sn sn)) - fl(ss ss))
  qf = fl(w qscale[b]), q = rint(qf); class sign(w) when the pixel is off the one-pixel frame, ow > thr[b], |qf| <= 2^31 and q != 0
  rejected    interior pixels with a NaN ow, or with ow > thr whose |qf| <= 2^31 fails
  component   maximal 4-connected set of one non-zero class, labelled by its smallest linear index; background -1
  measures    root, n, sum w, sum h, sum q, sum q w, sum q h, max |q| in int64
  table       the components with n >= min_area in increasing root order, the first K; found (+, -) counts them all; empty slot -1, 0..
  occupancy   per sign, the pixels of components with n >= min_area (truncated ones included)

The references use none of the device's means: the classes from shifted slices of a padded array (float32: the mirror; float64:
the restatement), the labels from a queue flood fill in row-major order (the first pixel of a component met is its smallest index),
the measures from np.add.at on int64, the finalize from explicit loops over the slots.

Near-threshold pixels (real data).  Each derivative d carries at most 12 u A_d (A_d the sum of its absolute stencil terms times rd,
a term taken as u0 (sd |x| + |mu|); 3 roundings per term, 6 additions, the product, 2 for rd: pdf_cases.near_bound's count without
the final difference).  w, sn, ss are one more rounding each: 13 u A with A_w = A_ss = A_vx + A_uy, A_sn = A_ux + A_vy, and |w| <= A_w.
A square then errs by 2 * 13 u A^2 + u A^2 = 27 u A^2, the two subtractions by u (A_w^2 + A_sn^2 + A_ss^2) each at most:
|ow32 - ow64| <= 29 u (A_w^2 + A_sn^2 + A_ss^2) + O(u^2); NEAR_OW = 30 covers the second order."""
import collections
import functools

import numpy as np

import pdf_cases as P

F32 = np.float32
U24 = 2.0 ** -24
NEAR_OW = 30 * U24
NEAR_CAP = 0.02                 # at most 2 % of the interior pixels of a real case may lie that near the threshold
WORDS = 8
AREA_BINS = 19
SD = [1.6, 0.7, 2.2]
MU = [0.4, -0.1, 0.25]
GRID = (0.5, 0.25)
CHUNKINGS = {1: [(1,)], 3: [(3,), (1, 2)], 5: [(5,), (2, 2, 1), (1,) * 5]}
MUTATIONS = ("conn8", "nosign", "ge", "frame", "area_after")
FLOAT_KEYS = ("count_mean", "count_std", "target_count", "area_frac_mean", "area_frac_std", "target_area_frac", "circ_sum_mean",
              "circ_sum_std", "target_circ_sum", "time_area_w1", "time_circ_w1", "time_member_circ_w1", "match_dist_mean",
              "match_miss_frac", "core_prob", "target_core_freq")
INT_KEYS = ("target_vortex_table", "vortex_found", "vortex_rejected", "vortex_truncated", "area_hist", "circ_hist")
META_KEYS = ("vortex_threshold", "vortex_qscale", "vortex_circ_edges", "vortex_args")
NEW_KEYS = FLOAT_KEYS + INT_KEYS + META_KEYS


# ---- classification -------------------------------------------------------------------------------------------------------------------
def gradients(x, mu, sd, u, grid, dtype):
    """x [.., B, C, H, W] -> (ux, uy, vx, vy) [.., B, H, W] in dtype, every operation rounded on its own (mu, sd None: 0, 1)."""
    mu = [0.0] * x.shape[-3] if mu is None else mu
    sd = [1.0] * x.shape[-3] if sd is None else sd
    ph = P.physical(x[..., :2, :, :], np.asarray(mu)[:2], np.asarray(sd)[:2], None if u is None else np.asarray(u)[:, :2], dtype)
    rdx, rdy = P.rd_of(grid, dtype)
    pu, pv = P._pad(ph[..., 0, :, :], False), P._pad(ph[..., 1, :, :], False)
    return P._ddx(pu) * rdx, P._ddy(pu) * rdy, P._ddx(pv) * rdx, P._ddy(pv) * rdy


def classify(x, mu, sd, u, grid, thr, qscale, dtype=F32, mutation=None):
    """-> dict: om, ow, qf [.., B, H, W] in dtype, cls int8, rej bool.  thr, qscale [B].  Mutations: "ge" (ow >= thr), "frame"
    (the frame is classified as well)."""
    with np.errstate(all="ignore"):
        ux, uy, vx, vy = gradients(x, mu, sd, u, grid, dtype)
        om = vx - uy
        sn = ux - vy
        ss = vx + uy
        ow = om * om - sn * sn
        ow = ow - ss * ss
        B = x.shape[-4]
        t = np.asarray(thr, F32).astype(dtype).reshape(B, 1, 1)
        qf = om * np.asarray(qscale, F32).astype(dtype).reshape(B, 1, 1)
        inner = np.zeros(x.shape[-2:], bool)
        inner[1:-1, 1:-1] = True
        if mutation == "frame":
            inner[:] = True
        over = (ow >= t) if mutation == "ge" else (ow > t)
        fits = np.abs(qf) <= dtype(2.0 ** 31)
        q = np.rint(qf)
        on = inner & over & fits & (q != 0)
        cls = np.where(on, np.where(om > 0, 1, -1), 0).astype(np.int8)
        rej = inner & (np.isnan(ow) | (over & ~fits))
    return dict(om=om, ow=ow, qf=qf, cls=cls, rej=rej)


def near_bound(x, mu, sd, u, grid):
    """NEAR_OW (A_w^2 + A_sn^2 + A_ss^2) [.., B, H, W] in fp64."""
    B, Cc = x.shape[-4], x.shape[-3]
    m, s = np.abs(np.asarray(mu, F32).astype(np.float64)).reshape(Cc, 1, 1), np.asarray(sd, F32).astype(np.float64).reshape(Cc, 1, 1)
    a = P._scale(u, B, Cc, np.float64).reshape(B, Cc, 1, 1) * (s * np.abs(x.astype(np.float64)) + m)
    au, av = P._pad(a[..., 0, :, :], False), P._pad(a[..., 1, :, :], False)
    sx = lambda p: 2 * p[..., 1:-1, 2:] + p[..., :-2, 2:] + p[..., 2:, 2:] + 2 * p[..., 1:-1, :-2] + p[..., :-2, :-2] + p[..., 2:, :-2]   # noqa: E731
    sy = lambda p: 2 * p[..., 2:, 1:-1] + p[..., 2:, :-2] + p[..., 2:, 2:] + 2 * p[..., :-2, 1:-1] + p[..., :-2, :-2] + p[..., :-2, 2:]   # noqa: E731
    rdx, rdy = P.rd_of(grid, np.float64)
    aw, an = sx(av) * rdx + sy(au) * rdy, sx(au) * rdx + sy(av) * rdy
    return NEAR_OW * (2 * aw * aw + an * an)


def defaults(tp, grid):
    """tp [B, T, 2.., H, W] physical fp64 -> (thr, qscale) [B]: 0.2 std of ow over the interior and the steps, 2^(20 - ceil(log2 max |w|))."""
    B = tp.shape[0]
    r = classify(tp.transpose(1, 0, 2, 3, 4), [0, 0, 0][:tp.shape[2]], [1, 1, 1][:tp.shape[2]], None, grid, np.zeros(B), np.ones(B), np.float64)
    ow = r["ow"][:, :, 1:-1, 1:-1].transpose(1, 0, 2, 3).reshape(B, -1)
    om = np.abs(r["om"][:, :, 1:-1, 1:-1]).transpose(1, 0, 2, 3).reshape(B, -1).max(1)
    return 0.2 * ow.std(1), 2.0 ** (20 - np.ceil(np.log2(om)))


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def label(cls, mutation=None):
    """cls [H, W] int8 -> label [H, W] int32: queue flood fill in row-major order.  Mutations: "conn8", "nosign"."""
    Hh, Ww = cls.shape
    c = np.abs(cls) if mutation == "nosign" else cls
    c = c.tolist()
    lab = [[-1] * Ww for _ in range(Hh)]
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if mutation == "conn8" else [])
    for h in range(Hh):
        for w in range(Ww):
            k = c[h][w]
            if k == 0 or lab[h][w] >= 0:
                continue
            root = h * Ww + w
            lab[h][w] = root
            queue = collections.deque([(h, w)])
            while queue:
                i, j = queue.popleft()
                for di, dj in nb:
                    a, b = i + di, j + dj
                    if 0 <= a < Hh and 0 <= b < Ww and lab[a][b] < 0 and c[a][b] == k:
                        lab[a][b] = root
                        queue.append((a, b))
    return np.array(lab, np.int32)


def scipy_label(cls):
    """The same labels through scipy.ndimage.label (None when scipy is not installed): per sign, 4-connectivity, then every label
    replaced by its component's smallest linear index."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    out = np.full(cls.shape, -1, np.int32)
    idx = np.arange(cls.size).reshape(cls.shape)
    for sgn in (1, -1):
        lab, n = ndimage.label(cls == sgn)
        if n:
            roots = ndimage.minimum(idx, lab, np.arange(1, n + 1)).astype(np.int32)
            out[lab > 0] = roots[lab[lab > 0] - 1]
    return out


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def census(lab, cls, om, qscale, K, min_area, mutation=None):
    """One plane: lab, cls, om [H, W], qscale a float -> (table [K, 8] int64, found [2] int32, core [2, H, W] int32).  Mutation
    "area_after": the first K components are taken before the min_area filter."""
    Hh, Ww = lab.shape
    HW = Hh * Ww
    on = lab >= 0
    l = lab[on].astype(np.int64)
    hh, ww = np.nonzero(on)
    with np.errstate(all="ignore"):
        q = np.rint(om.astype(F32)[on] * F32(qscale)).astype(np.int64)
    sums = np.zeros((7, HW), np.int64)
    for row, v in enumerate((np.ones_like(q), ww, hh, q, q * ww, q * hh)):
        np.add.at(sums[row], l, v)
    np.maximum.at(sums[6], l, np.abs(q))
    roots = np.unique(l)
    sign_neg = cls.reshape(-1)[roots] < 0
    big = sums[0, roots] >= min_area
    found = np.array([np.sum(big & ~sign_neg), np.sum(big & sign_neg)], np.int32)
    if mutation == "area_after":
        kept = roots[:K]
        kept = kept[sums[0, kept] >= min_area]
    else:
        kept = roots[big][:K]
    table = np.zeros((K, WORDS), np.int64)
    table[:, 0] = -1
    table[:len(kept), 0] = kept
    table[:len(kept), 1:] = sums[:, kept].T
    core = np.zeros((2, Hh, Ww), np.int32)
    ok = np.zeros(HW, bool)
    ok[roots[big]] = True
    inside = on & ok[np.where(on, lab, 0)]
    core[0][inside & (cls > 0)] = 1
    core[1][inside & (cls < 0)] = 1
    return table, found, core


def reference(xs, mu, sd, u, grid, thr, qscale, K, min_area, timed, mutation=None):
    """xs [steps, S + 1, B, C, H, W] float32 (the target last) -> the integer state over the timed steps: table [B, S + 1, T, K, 8],
    found [B, S + 1, T, 2], rejected [B, S + 1, T], core [2, B, 2, H, W] (members, target), cls, lab [T, S + 1, B, H, W], om."""
    timed = list(timed)
    R, B, Hh, Ww = xs.shape[1], xs.shape[2], xs.shape[-2], xs.shape[-1]
    S, T = R - 1, len(timed)
    r = classify(xs[timed], mu, sd, u, grid, thr, qscale, F32, mutation)
    table = np.zeros((B, R, T, K, WORDS), np.int64)
    found, rejected = np.zeros((B, R, T, 2), np.int32), np.zeros((B, R, T), np.int32)
    core = np.zeros((2, B, 2, Hh, Ww), np.int32)
    lab = np.zeros((T, R, B, Hh, Ww), np.int32)
    for t in range(T):
        for row in range(R):
            for b in range(B):
                lab[t, row, b] = label(r["cls"][t, row, b], mutation)
                table[b, row, t], found[b, row, t], c = census(lab[t, row, b], r["cls"][t, row, b], r["om"][t, row, b], float(np.asarray(qscale)[b]),
                                                               K, min_area, mutation)
                core[1 if row == S else 0, b] += c
                rejected[b, row, t] = r["rej"][t, row, b].sum()
    return dict(table=table, found=found, rejected=rejected, core=core, cls=r["cls"], lab=lab, om=r["om"])


# ---- finalize ---------------------------------------------------------------------------------------------------------------------------
def _w1(p, q, h):
    """Mass at the bin centres: the mean |difference| of the two quantile functions, as the integral of |F - G| between centres."""
    if p.sum() == 0 or q.sum() == 0:
        return np.nan
    F, G = np.cumsum(p) / p.sum(), np.cumsum(q) / q.sum()
    return float(sum(abs(F[j] - G[j]) for j in range(len(p) - 1)) * h)


def finalize(table, found, core, S, hw, grid, qscale, nb, circ_range, T):
    """The finalize of tmg_ops.EnsembleVortices from the integer state, slot by slot, in fp64 -> dict of numpy arrays."""
    B, R, _, K = table.shape[:4]
    Hh, Ww = hw
    dx, dy = float(grid[0]), float(grid[1])
    vort = [[[[] for _ in range(T)] for _ in range(R)] for _ in range(B)]     # (sign, n, gamma, cx, cy) of every kept vortex
    for b in range(B):
        for r in range(R):
            for t in range(T):
                for k in range(K):
                    root, n, sw, sh, sq, sqw, sqh, pk = [int(v) for v in table[b, r, t, k]]
                    if root >= 0:
                        vort[b][r][t].append((0 if sq > 0 else 1, n, sq * dx * dy / float(qscale[b]), sqw / sq * dx, sqh / sq * dy))
    o = {}
    cr = np.zeros((B, 2))
    for b in range(B):
        if circ_range is None:
            top = max([abs(v[2]) for t in range(T) for v in vort[b][S][t]] + [0.0])
            cr[b] = (0.0, 1.25 * top if top > 0 else 1.0)
        else:
            cr[b] = np.asarray(circ_range, np.float64).reshape(-1, 2)[b if np.asarray(circ_range).ndim == 2 else 0]
    o["vortex_circ_edges"] = np.stack([cr[b, 0] + (cr[b, 1] - cr[b, 0]) * np.arange(nb + 1) / nb for b in range(B)])
    rows = {k: np.zeros((B, R, T, 2)) for k in ("count", "area_frac", "circ_sum")}
    rows["count"] = found.astype(np.float64)
    ah, ch = np.zeros((B, R, 2, AREA_BINS), np.int64), np.zeros((B, R, 2, nb), np.int64)
    for b in range(B):
        for r in range(R):
            for t in range(T):
                for s, n, gm, cx, cy in vort[b][r][t]:
                    rows["area_frac"][b, r, t, s] += n / float((Hh - 2) * (Ww - 2))
                    rows["circ_sum"][b, r, t, s] += gm
                    ah[b, r, s, n.bit_length() - 1] += 1
                    j = int(np.floor((abs(gm) - cr[b, 0]) / (cr[b, 1] - cr[b, 0]) * nb))
                    ch[b, r, s, min(max(j, 0), nb - 1)] += 1
    for key, v in rows.items():
        o[key + "_mean"], o[key + "_std"], o["target_" + key] = v[:, :S].mean(1), v[:, :S].std(1), v[:, S]
    o["area_hist"], o["circ_hist"] = ah, ch
    o["time_area_w1"], o["time_circ_w1"] = np.zeros((B, 2)), np.zeros((B, 2))
    o["time_member_circ_w1"] = np.zeros((B, S, 2))
    for b in range(B):
        h = (cr[b, 1] - cr[b, 0]) / nb
        for s in range(2):
            o["time_area_w1"][b, s] = _w1(ah[b, :S, s].sum(0), ah[b, S, s], 1.0)
            o["time_circ_w1"][b, s] = _w1(ch[b, :S, s].sum(0), ch[b, S, s], h)
            for m in range(S):
                o["time_member_circ_w1"][b, m, s] = _w1(ch[b, m, s], ch[b, S, s], h)
    md, mf = np.full((B, T, 2), np.nan), np.full((B, T, 2), np.nan)
    for b in range(B):
        for t in range(T):
            for s in range(2):
                tv = [v for v in vort[b][S][t] if v[0] == s]
                if not tv:
                    continue
                dist, miss = [], 0
                for m in range(S):
                    mv = [v for v in vort[b][m][t] if v[0] == s]
                    for v in tv:
                        if mv:
                            dist.append(min(np.hypot(v[3] - w[3], v[4] - w[4]) for w in mv))
                        else:
                            miss += 1
                md[b, t, s] = np.mean(dist) if dist else np.nan
                mf[b, t, s] = miss / float(S * len(tv))
    o["match_dist_mean"], o["match_miss_frac"] = md, mf
    o["core_prob"] = core[0].astype(np.float64) / float(S * T)
    o["target_core_freq"] = core[1].astype(np.float64) / float(T)
    o["vortex_truncated"] = (found.astype(np.int64).sum(-1) > K).sum((1, 2))
    return o


def check_floats(got, ref, what, keys=FLOAT_KEYS):
    """|got - ref| <= 2^-23 |ref| + 2^-40 max(1, max |ref|): the final rounding to float32 (2^-24) with room for a fp64 result that
    sits on a float32 tie, plus the two fp64 evaluations' own rounding (sums of at most K T terms)."""
    for key in keys:
        g, r = np.asarray(got[key], np.float64), np.asarray(ref[key], np.float64)
        assert g.shape == r.shape, (what, key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, key)
        fin = ~np.isnan(r)
        scale = max(1.0, float(np.abs(r[fin]).max())) if fin.any() else 1.0
        err = np.abs(g[fin] - r[fin]) - (2.0 ** -23 * np.abs(r[fin]) + 2.0 ** -40 * scale)
        assert not (err > 0).any(), (what, key, float(err.max()))


def check_identities(f, table, found, S, hw, K, what):
    """The histograms sum to the kept counts; area_frac follows from the tables; count is found."""
    kept = (table[..., 0] >= 0)
    pos, neg = kept & (table[..., 4] > 0), kept & (table[..., 4] < 0)
    per = np.stack((pos.sum((2, 3)), neg.sum((2, 3))), -1)                    # [B, R, 2]
    assert np.array_equal(f["area_hist"].sum(-1), per) and np.array_equal(f["circ_hist"].sum(-1), per), what
    assert np.array_equal(np.minimum(found.sum(-1), K), kept.sum(-1)), what
    frac = np.stack(((table[..., 1] * pos).sum(-1), (table[..., 1] * neg).sum(-1)), -1) / float((hw[0] - 2) * (hw[1] - 2))
    assert np.allclose(f["target_area_frac"], frac[:, S], rtol=1e-12, atol=0) and np.allclose(f["area_frac_mean"], frac[:, :S].mean(1), rtol=1e-12, atol=1e-300), what
    assert np.array_equal(f["target_count"], found[:, S].astype(np.float64)), what


# ---- masks ------------------------------------------------------------------------------------------------------------------------------
def mask_shapes(TH, TW):
    return [(5, 7), (TH - 1, TW + 1), (2 * TH + 3, 3 * TW + 1)]


def masks(hw, TH, TW, big=False):
    """name -> int8 [H, W] with classes in {-1, 0, 1}: the adversarial masks of the labelling kernel for a field of hw and a tile
    (TH, TW).  big: only those a 256 x 256 field is meant for (and the rest are cheap enough to keep)."""
    Hh, Ww = hw
    hh, ww = np.mgrid[0:Hh, 0:Ww]
    m = {}
    m["empty"] = np.zeros(hw, np.int8)
    m["all_one"] = np.ones(hw, np.int8)
    m["checkerboard"] = ((hh + ww) % 2).astype(np.int8)
    m["sign_stripes"] = np.where(ww % 2 == 0, 1, -1).astype(np.int8)
    s = np.zeros(hw, np.int8)                                                 # serpentine: full rows joined at alternating ends
    s[0::2, :] = 1
    for i, h in enumerate(range(1, Hh - 1, 2)):
        s[h, Ww - 1 if i % 2 == 0 else 0] = 1
    m["serpentine"] = s
    vs = np.zeros(hw, np.int8)                                                # the same along the columns
    vs[:, 0::2] = -1
    for i, w in enumerate(range(1, Ww - 1, 2)):
        vs[Hh - 1 if i % 2 == 0 else 0, w] = -1
    m["serpentine_columns"] = vs
    c = np.zeros(hw, np.int8)                                                 # comb: a spine along the bottom, teeth up every other column
    c[Hh - 1, :] = 1
    c[:, 0::2] = 1
    m["comb"] = c
    ch, cw = min(TH, Hh - 1), min(TW, Ww - 1)                                 # a tile corner (or the nearest interior point)
    d = np.zeros(hw, np.int8)
    d[max(0, ch - 3):ch, max(0, cw - 3):cw] = 1
    d[ch:ch + 3, cw:cw + 3] = 1
    m["diagonal_touch"] = d
    o = np.zeros(hw, np.int8)
    o[:, max(0, cw - 3):cw] = 1
    o[:, cw:cw + 3] = -1
    m["opposite_signs_on_border"] = o
    ring = np.minimum(np.minimum(hh, Hh - 1 - hh), np.minimum(ww, Ww - 1 - ww))
    m["nested_rings"] = np.where(ring % 2 == 0, np.where(ring % 4 == 0, 1, -1), 0).astype(np.int8)
    rng = np.random.default_rng(1234 + Hh * 1000 + Ww)
    for dens in (0.3, 0.5, 0.6):
        r = rng.random(hw)
        m["random_%.1f" % dens] = np.where(r < dens / 2, 1, np.where(r < dens, -1, 0)).astype(np.int8)
    return m


# ---- fields -----------------------------------------------------------------------------------------------------------------------------
def gauss_field(hw, vortices, noise=0.0, seed=0):
    """Sum of Gaussian stream functions psi = g exp(-r^2 / 2 s^2) at (cy, cx): u = d psi / dy, v = -d psi / dx -> [3, H, W] float32."""
    Hh, Ww = hw
    y, x = np.mgrid[0:Hh, 0:Ww].astype(np.float64)
    u, v = np.zeros(hw), np.zeros(hw)
    for cy, cx, g, s in vortices:
        psi = g * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * s * s))
        u += -(y - cy) / (s * s) * psi
        v += (x - cx) / (s * s) * psi
    out = np.stack((u, v, np.zeros(hw)))
    if noise:
        out[:2] += np.random.default_rng(seed).normal(0.0, noise, (2,) + tuple(hw))
    return out.astype(F32)


STREET = tuple((14, 10 + 22 * i, 5.0, 3.0) for i in range(4)) + tuple((34, 21 + 22 * i, -5.0, 3.0) for i in range(4))   # staggered
# (field, vortices, noise, counts (+, -), areas (+ then -, in root order within a sign), centres)
KNOWN = [
    ((24, 40), ((12, 12, 5.0, 3.0), (12, 28, -5.0, 3.0)), 0.0, (1, 1), ((25,), (25,))),
    ((24, 40), ((12, 12, 5.0, 3.0), (12, 28, -5.0, 3.0)), 0.05, (1, 1), ((25,), (25,))),
    ((40, 72), ((32, 32, 5.0, 4.0), (10, 60, -3.0, 2.5)), 0.0, (1, 1), ((45,), (21,))),
    ((48, 96), STREET, 0.0, (4, 4), ((25,) * 4, (25,) * 4)),
]


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, hw, steps, seed):
    """Drifting Gaussian vortices plus noise, normalised -> (xs [steps, S + 1, B, 3, H, W] float32 raw, sd, mu, u [B, 3]).  The
    members are the target's vortices displaced and rescaled, some dropped, so that counts, areas and matches all vary."""
    rng = np.random.default_rng(seed)
    Hh, Ww = hw
    u = (0.75 + 0.5 * rng.random((B, 1))).astype(F32) * np.array([1.0, 1.0, 1.0], F32)
    u[:, 2] = u[:, 0] ** 2
    xs = np.zeros((steps, S + 1, B, 3, Hh, Ww), F32)
    nv = max(2, (Hh * Ww) // 300)
    for b in range(B):
        base = [(rng.uniform(min(3, Hh / 2 - 1), max(Hh - 4, Hh / 2)), rng.uniform(min(3, Ww / 2 - 1), max(Ww - 4, Ww / 2)),
                 rng.choice([-1.0, 1.0]) * rng.uniform(2, 5), rng.uniform(1.5, 3.0))
                for _ in range(nv)]
        for r in range(S + 1):
            mine = base if r == S else [(cy + rng.normal(0, 1.0), cx + rng.normal(0, 1.0), g * rng.uniform(0.7, 1.3), s)
                                        for cy, cx, g, s in base if rng.random() > 0.2]
            for t in range(steps):
                f = gauss_field(hw, [(cy, cx + 0.7 * t, g, s) for cy, cx, g, s in mine]).astype(np.float64)
                f[:2] += rng.normal(0.0, 0.05, (2, Hh, Ww))
                f[2] = rng.normal(0.0, 1.0, (Hh, Ww))
                phys = f                                                       # physical; raw = (phys / u - mu) / sd
                xs[t, r, b] = ((phys / u[b].astype(np.float64).reshape(3, 1, 1) - np.array(MU).reshape(3, 1, 1)) / np.array(SD).reshape(3, 1, 1)).astype(F32)
    return xs, SD, MU, u


def real_defaults(xs, sd, mu, u, grid, timed):
    """thr, qscale of the target rows of xs over the timed steps, from their fp64 physical values."""
    S = xs.shape[1] - 1
    tp = P.physical(xs[list(timed), S], mu, sd, u, np.float64).transpose(1, 0, 2, 3, 4)
    return defaults(tp, grid)


def int_inputs(S, B, hw, steps, seed, vmax=3):
    """Integer velocities in -vmax .. vmax (unit scales, dx = dy = 1, qscale 8: the vorticity is a multiple of 1 / 8) -> xs float32."""
    rng = np.random.default_rng(seed)
    return rng.integers(-vmax, vmax + 1, (steps, S + 1, B, 3) + tuple(hw)).astype(F32)


# (S, B, field, padded, Tn); one untimed step comes first.  33 x 65: one more than a tile both ways (2 x 3 tiles); 40 x 72 as the issue
CASES = [(1, 1, (5, 7), False, 2), (3, 2, (31, 33), True, 2), (5, 1, (33, 65), False, 3), (5, 2, (40, 72), True, 2)]
MAX_CASE = (1024, 1, (6, 7), False, 2)                                        # chunks (1024,) and (64,) * 16
