"""Case tables, the fp64 / int64 reference, the rounding bounds, a float32 simulation and named defects of the ensemble structure
functions and variogram score (csrc/tmg_sfun.hip, tmg_ops.EnsembleStructure), shared by tests/test_structure_cpu.py (no device) and
tests/test_structure_gpu.py.

Definitions (case b, kept step t, channel c; rows x_0..x_{S-1} the raw normalised members, x_S = y the normalised target, R = S + 1;
a_c = u[b, c] out_std[c] in fp64 from the fp32 factors).  A lag l = (dx, dy), dx along W, dy along H; its pairs are the pixels
p = (i, j) with p' = (i + dy, j + dx) in the field, N_l = (H - |dy|) (W - dx); D_m(p) = x_m(p') - x_m(p).
  M_q[m] = sum_p D_m^q, q = 2, 3, 4;  s_m = sqrt|D_m|, sbar = mean_{m<S} s_m, V_l = sum_p (s_S - sbar)^2
  sf_q = a^q M_q / N_l; sf2_mean / sf2_std over the members; vario_lag = w_l a V_l / N_l; vario_score = sum_l vario_lag;
  time_sf_q = a^q sum_t M_q / (T N_l); time_skew = time_sf3 / time_sf2^1.5; time_flat = time_sf4 / time_sf2^2; time_vario_*.
The REFERENCE slices the field directly (numpy, fp64; integer data: int64, exact) and never walks pixel slices.

The bounds (u = 2^-24; Lc and P from tmg_hip.ens_sfun_plan: Lc fp32 additions along the longest path inside one partial, P partials
added in slice order).  A term of M_q is formed as D = fl(x' - x), D2 = fl(D D), then D2, fl(D2 D), fl(D2 D2):
  |M_q - ref| <= (Lc + P + k_q) u sum_p |D|^q,  k_q = q + (q - 1) + 1:  the operand's rounding enters q times, q - 1 products (D^4
  as a square of a square: 2 (2 d + 1) + 1 = 4 d + 3, the same), one for all second-order terms ((Lc + P + k_q) u < 1e-3)
  k_2 = 4, k_3 = 6, k_4 = 8.
Variogram: s_m = sqrtf(fl|D|) carries 1.5 u (half the operand's rounding, one for the root); the sequential sum of S of them S - 1
more; fl(1 / S) and the product 2: sbar is off by (S + 2.5) u sbar, s_S by 1.5 u s_S, their difference rounds once, u |s_S - sbar|:
  |e - (s_S - sbar)| <= E := (S + 4) u (s_S + sbar) per pair;  |e^2 - ref^2| <= 2 |ref| E + E^2
  |V_l - ref| <= sum_p (2 |s_S - sbar| E + E^2) + (Lc + P + 2) u V_l  (the square's rounding and the second order: 2)
tmom / tvar after j timed steps: the sum of the steps' bounds plus one rounding per step, j u (sum_t sum_p |D|^q + the bounds).
Physical outputs: the same bounds scaled as the outputs are, plus the final rounding to float32, u (|ref| + bound); sf2_std is
1-Lipschitz in the root mean square of the members' errors; time_skew / time_flat are propagated over the interval of time_sf2 and
compared only where time_sf2's reference exceeds its own bound tenfold (check() returns the count).
No bound is fitted to what the kernels give; the GPU tests print the share of it that they reach."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
KQ = {2: 4, 3: 6, 4: 8}
F32 = np.float32
T = 3
RAW_KEYS = ("mom", "vsum")
SF_KEYS = ("sf2", "sf3", "sf4")
STEP_KEYS = SF_KEYS + ("sf2_mean", "sf2_std", "vario_lag", "vario_score")
TIME_KEYS = ("time_sf2", "time_sf3", "time_sf4", "time_skew", "time_flat", "time_vario_lag", "time_vario_score")
DEFECTS = ("drop_last", "dy_flip", "target_in_sbar", "s_minus_one", "abs_cube", "n_hw")

# ---- lag lists by field -----------------------------------------------------------------------------------------------------------------
ALL16 = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (0, 1), (0, 2), (0, 4), (0, 8), (0, 15), (3, -2), (1, 1), (5, -15), (16, 15), (7, 3),
         (2, -1))
LAGS = {
    (1, 2): ((1, 0),),                                                       # N = 1
    (2, 1): ((0, 1),),
    (1, 5): ((1, 0), (2, 0), (4, 0)),                                        # H = 1: only dy = 0 fits; dx = W - 1
    (7, 9): ((1, 0), (8, 0), (0, 6), (3, -2), (1, -6), (0, 1)),              # dx = W - 1, dy = +-(H - 1), a diagonal with dy < 0
    (8, 8): ((1, 1),),                                                       # a single lag
    (5, 13): ((12, 0), (0, 4), (2, -4), (1, 0), (3, 2)),                     # five lags: the eight-lag instance
    (16, 17): ALL16,                                                         # all 16 lags at once
    (16, 33): ((32, 0), (0, 15), (5, -15), (1, 0), (0, 1), (2, 2), (4, -3)),
    (50, 58): ((1, 0), (0, 16), (3, -2), (57, 0), (0, 49), (10, -49), (32, 5), (0, 1), (64 - 7, 49)),   # (0, 16): 928 pixels, wider than a slice of 512
    (3, 70): ((64, 0), (1, 2), (0, 2)),
    (66, 3): ((0, 64), (2, -64), (1, 0)),
    (181, 183): ((1, 0), (0, 1), (3, -2)),
}
# (mode, S, B, C, (H, W), t_start, chunking, padded): chunking 0: one member per chunk, 1: three, 2: all at once
INT_TABLE = [
    ("small", 1, 1, 2, (1, 2), 0, 0, False), ("binary", 2, 3, 3, (2, 1), 1, 2, True), ("binary", 1024, 1, 2, (1, 5), 0, 2, False),
    ("small", 5, 3, 3, (7, 9), 1, 1, True), ("binary", 16, 1, 4, (8, 8), 0, 0, False), ("small", 17, 3, 2, (5, 13), 1, 1, True),
    ("binary", 64, 1, 3, (16, 17), 0, 2, False), ("small", 130, 1, 2, (16, 33), 0, 1, True), ("binary", 64, 1, 2, (50, 58), 1, 2, False),
    ("small", 2, 3, 4, (50, 58), 0, 2, True), ("small", 5, 1, 3, (3, 70), 0, 0, False), ("binary", 17, 3, 2, (66, 3), 1, 1, True),
    ("binary", 5, 1, 3, (16, 17), 0, 0, True), ("binary", 16, 3, 2, (16, 33), 1, 1, False),
]
# three pixels per thread: a slice of 768 pixels needs H W > 512 * 768 / (B C)
LONG_CASE = ("binary", 2, 3, 4, (181, 183), 0, 2, False)
REAL_TABLE = [  # (S, B, C, (H, W), kind, with_u)
    (5, 3, 3, (7, 9), "gauss", True), (16, 1, 4, (16, 17), "smooth", False), (17, 3, 2, (5, 13), "biased", True),
    (64, 1, 3, (16, 33), "gauss", False), (130, 1, 2, (50, 58), "smooth", True), (2, 3, 3, (50, 58), "biased", False),
    (5, 1, 2, (3, 70), "smooth", True), (7, 3, 3, (66, 3), "gauss", True), (1, 3, 3, (16, 17), "smooth", True),
]
SD = [1.7, 0.6, 2.5, 0.9]
GRID = (0.25, 0.5)


def chunk_sizes(S, kind):
    per = (1, 3, S)[kind]
    return [min(per, S - m0) for m0 in range(0, S, per)]


def weights_of(L):
    return [0.5 + 0.25 * (l % 5) for l in range(L)]


def plan_branch(plan):
    """-> (the kernel instance of a case: the lags it holds accumulators for; the plan's branch: more than one slice, pixels per
    thread)."""
    return 4 if plan["L"] <= 4 else 8 if plan["L"] <= 8 else 16, (plan["P"] > 1, plan["SL"] // 256)


INSTANCES = {4, 8, 16}
# one slice of 256 or of 512 pixels (H W <= 512); several slices of 512; several longer ones (the grid is full: LONG_CASE)
PLAN_BRANCHES = {(False, 1), (False, 2), (True, 2), (True, 3)}


@functools.lru_cache(maxsize=None)
def int_inputs(mode, S, B, Cc, hw, seed, steps=T):
    """small: members and target integers in -3..3 (|D| <= 6, D^4 <= 1296: every moment sum is exact in fp32 for H W <= 12 900);
    binary: values in {0, 1} (|D| in {0, 1}: sqrtf exact).  -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W]) float32."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-3, 4) if mode == "small" else (0, 2)
    xs = torch.randint(lo, hi, (steps, S, B, Cc) + tuple(hw), generator=g)
    tgt = torch.randint(lo, hi, (steps, B, Cc) + tuple(hw), generator=g)
    return xs.float().numpy(), tgt.float().numpy()


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, Cc, hw, kind, seed, steps=T):
    """gauss: members and target N(0.3, 1); smooth: a double cumulative sum of N(0, 1) (over H, then W) shared by the members and
    the target plus 1e-3 N(0, 1) of member noise: the field is large and the increments cancel; biased: members 5 +- 0.1, target
    0 +- 1."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, *hw, generator=g)                          # noqa: E731
    if kind == "gauss":
        xs, tgt = n(steps, S, B, Cc) + 0.3, n(steps, B, Cc) + 0.3
    elif kind == "biased":
        xs, tgt = 5.0 + 0.1 * n(steps, S, B, Cc), n(steps, B, Cc)
    else:
        base = n(steps, B, Cc).cumsum(-2).cumsum(-1)
        xs, tgt = base[:, None] + 1e-3 * n(steps, S, B, Cc), base + 1e-3 * n(steps, B, Cc)
    return xs.numpy().astype(F32), tgt.numpy().astype(F32)


def scales(sd, u, B, Cc):
    """a [B, C] fp64 = u out_std from the fp32 factors."""
    sd = np.ones(Cc, F32) if sd is None else np.asarray(sd, F32)[:Cc]
    a = np.broadcast_to(sd.astype(np.float64), (B, Cc)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, Cc)
    return a


def pair_counts(lags, hw):
    return np.array([(hw[0] - abs(dy)) * (hw[1] - dx) for dx, dy in lags], dtype=np.float64)


def rows_of(xs, tgt):
    """[T, S, B, C, H, W], [T, B, C, H, W] -> the R = S + 1 rows [T, B, C, R, H, W] (the dtype of xs)."""
    x = np.concatenate([xs, tgt[:, None]], 1)
    return np.ascontiguousarray(np.moveaxis(x, 1, 3))


def increments(x, lag, defect=None):
    """x [.., H, W] -> D = x(p') - x(p) over the pairs of the lag, [.., H - |dy|, W - dx]."""
    dx, dy = lag
    if defect == "dy_flip":
        dy = -dy
    H, W = x.shape[-2:]
    a = x[..., max(0, -dy):H - max(0, dy), 0:W - dx]
    b = x[..., max(0, dy):H + min(0, dy), dx:W]
    d = b - a
    if defect == "drop_last":                                                # the last column of pairs, or the last row when dx = 0
        d = d[..., :, :-1] if dx > 0 else d[..., :-1, :]
    return d


def reference(xs, tgt, lags, integer=False, eps=None):
    """-> mom, abs [T, 3, B, C, L, R] (sum D^q and sum |D|^q), vsum [T, B, C, L], vpair [T, B, C, L] (sum_p 2 |s_S - sbar| E + E^2) in
    fp64 by direct slicing.  integer: D and the moment sums in int64 (exact); binary data also gives vint = S^2 V_l in int64.
    eps (broadcastable to D's [T, B, C, R, h, w]): every increment of the inputs is itself known only to +-eps (end to end): abs is
    taken over |D| + eps, xmom = sum (|D| + eps)^q - |D|^q is the reference's own uncertainty, and E grows by 2 sqrt(eps)
    (|sqrt|D + d| - sqrt|D|| <= sqrt|d|, for s_S and for sbar)."""
    S = xs.shape[1]
    x = rows_of(xs, tgt)
    x = x.astype(np.int64) if integer else x.astype(np.float64)
    mom, ab, vs, vp, vi, xm = [], [], [], [], [], []
    ep = 0.0 if eps is None else eps
    for lag in lags:
        d = increments(x, lag)                                               # [T, B, C, R, h, w]
        mom.append(np.stack([(d ** q).sum((-1, -2)) for q in (2, 3, 4)], 1))
        ab.append(np.stack([((np.abs(d) + ep) ** q).sum((-1, -2)) for q in (2, 3, 4)], 1))
        xm.append(np.stack([((np.abs(d) + ep) ** q - np.abs(d) ** q).sum((-1, -2)) for q in (2, 3, 4)], 1))
        s = np.sqrt(np.abs(d).astype(np.float64))
        sbar = s[:, :, :, :S].mean(3)
        e = s[:, :, :, S] - sbar
        E = (S + 4) * U24 * (s[:, :, :, S] + sbar) + 2.0 * np.sqrt(ep if eps is None else np.broadcast_to(ep, d.shape)[:, :, :, 0])
        vs.append((e * e).sum((-1, -2)))
        vp.append((2 * np.abs(e) * E + E * E).sum((-1, -2)))
        if integer and np.abs(d).max() <= 1:
            ad = np.abs(d)
            vi.append(((S * ad[:, :, :, S] - ad[:, :, :, :S].sum(3)) ** 2).sum((-1, -2)))
    out = {"mom": np.stack(mom, 4).astype(np.float64), "abs": np.stack(ab, 4).astype(np.float64), "vsum": np.stack(vs, 3),
           "vpair": np.stack(vp, 3), "xmom": np.stack(xm, 4).astype(np.float64)}
    if len(vi) == len(lags):
        out["vint"] = np.stack(vi, 3)
    return out


def derive(mom, vsum, a, w, N, t_start, S, tmom=None, tvar=None, defect=None, hw=None):
    """The physical outputs in fp64 from raw sums mom [T, 3, B, C, L, R], vsum [T, B, C, L] (tmom / tvar: the accumulated sums, else
    the plain sums over the timed steps), shaped as EnsembleStructure's."""
    mom, vsum = np.asarray(mom, np.float64), np.asarray(vsum, np.float64)
    Tn, _, B, Cc, L, R = mom.shape
    N = np.full(L, float(hw[0] * hw[1])) if defect == "n_hw" else np.asarray(N, np.float64)
    w = np.asarray(w, np.float64)
    nT = Tn - t_start
    tmom = mom[t_start:].sum(0) if tmom is None else np.asarray(tmom, np.float64)
    tvar = vsum[t_start:].sum(0) if tvar is None else np.asarray(tvar, np.float64)
    o = {}
    for q in (2, 3, 4):
        o["sf%d" % q] = np.moveaxis((a ** q).reshape(1, B, Cc, 1, 1) * mom[:, q - 2] / N.reshape(1, 1, 1, L, 1), 0, 1)
        o["time_sf%d" % q] = (a ** q).reshape(B, Cc, 1, 1) * tmom[q - 2] / (nT * N.reshape(1, 1, L, 1))
    mem = o["sf2"][..., :S]
    o["sf2_mean"] = mem.mean(-1)
    o["sf2_std"] = np.sqrt(((mem - o["sf2_mean"][..., None]) ** 2).mean(-1))
    o["vario_lag"] = np.moveaxis(w.reshape(1, 1, 1, L) * a.reshape(1, B, Cc, 1) * vsum / N.reshape(1, 1, 1, L), 0, 1)
    o["vario_score"] = o["vario_lag"].sum(-1)
    s2 = o["time_sf2"]
    with np.errstate(divide="ignore", invalid="ignore"):
        o["time_skew"] = np.where(s2 != 0, o["time_sf3"] / s2 ** 1.5, 0.0)
        o["time_flat"] = np.where(s2 != 0, o["time_sf4"] / s2 ** 2, 0.0)
    o["time_vario_lag"] = w.reshape(1, 1, L) * a.reshape(B, Cc, 1) * tvar / (nT * N.reshape(1, 1, L))
    o["time_vario_score"] = o["time_vario_lag"].sum(-1)
    return o


def bounds(ref, phys, plan, a, w, N, t_start, S):
    """The bounds of the module docstring: raw (mom, vsum, tmom_cum, tvar_cum after every timed step) and physical."""
    Tn, _, B, Cc, L, R = ref["mom"].shape
    lp = plan["Lc"] + plan["P"]
    bm = np.stack([(lp + KQ[q]) * U24 * ref["abs"][:, q - 2] + ref["xmom"][:, q - 2] for q in (2, 3, 4)], 1)
    bv = ref["vpair"] + (lp + 2) * U24 * ref["vsum"]
    nT = Tn - t_start
    steps = np.arange(1, nT + 1)
    cb = np.cumsum(bm[t_start:], 0)
    cabs = np.cumsum(ref["abs"][t_start:], 0)
    tb = cb + steps.reshape(-1, 1, 1, 1, 1, 1) * U24 * (cabs + cb)
    cvb = np.cumsum(bv[t_start:], 0)
    tvb = cvb + steps.reshape(-1, 1, 1, 1) * U24 * (np.cumsum(ref["vsum"][t_start:], 0) + cvb)
    out = {"mom": bm, "vsum": bv, "tmom_cum": tb, "tvar_cum": tvb}
    N = np.asarray(N, np.float64)
    w = np.asarray(w, np.float64)
    rnd = lambda name, b: b + U24 * (np.abs(phys[name]) + b)                  # noqa: E731
    raw = {}
    for q in (2, 3, 4):
        raw["sf%d" % q] = np.moveaxis((a ** q).reshape(1, B, Cc, 1, 1) * bm[:, q - 2] / N.reshape(1, 1, 1, L, 1), 0, 1)
        raw["time_sf%d" % q] = (a ** q).reshape(B, Cc, 1, 1) * tb[-1][q - 2] / (nT * N.reshape(1, 1, L, 1))
    raw["sf2_mean"] = raw["sf2"][..., :S].mean(-1)
    raw["sf2_std"] = np.sqrt((raw["sf2"][..., :S] ** 2).mean(-1))
    raw["vario_lag"] = np.moveaxis(w.reshape(1, 1, 1, L) * a.reshape(1, B, Cc, 1) * bv / N.reshape(1, 1, 1, L), 0, 1)
    raw["vario_score"] = raw["vario_lag"].sum(-1)
    raw["time_vario_lag"] = w.reshape(1, 1, L) * a.reshape(B, Cc, 1) * tvb[-1] / (nT * N.reshape(1, 1, L))
    raw["time_vario_score"] = raw["time_vario_lag"].sum(-1)
    s2, b2 = phys["time_sf2"], raw["time_sf2"]
    ok = s2 > 10 * b2
    lo = np.where(ok, s2 - b2, 1.0)
    s2s = np.where(ok, s2, 1.0)
    raw["time_skew"] = raw["time_sf3"] / lo ** 1.5 + np.abs(phys["time_sf3"]) * (lo ** -1.5 - s2s ** -1.5)
    raw["time_flat"] = raw["time_sf4"] / lo ** 2 + np.abs(phys["time_sf4"]) * (lo ** -2.0 - s2s ** -2.0)
    for name, b in raw.items():
        out[name] = rnd(name, b)
    out["qualifies"] = ok
    return out


def check(got, ref, phys, bnd, t_start, what):
    """Every output of `got` (EnsembleStructure's dict as numpy plus the raw buffers: mom [T, 3, B, C, L, R], vsum, and tmom_steps /
    tvar_steps after every step) against the reference within the bounds -> (the worst share of a bound reached, the number of
    time_skew / time_flat entries compared)."""
    worst = 0.0

    def within(name, g, r, b, mask=None):
        nonlocal worst
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == np.shape(r), "%s %s: shape %s, expected %s" % (what, name, g.shape, np.shape(r))
        err = np.abs(g - r)
        share = np.where(err > 0, err / np.maximum(b, 1e-300), 0.0)
        if mask is not None:
            share = np.where(mask, share, 0.0)
        share = float(share.max())
        assert not np.isnan(g).any() and share <= 1.0, "%s %s: worst error is %.3g of its bound" % (what, name, share)
        worst = max(worst, share)

    within("mom", got["mom"], ref["mom"], bnd["mom"])
    within("vsum", got["vsum"], ref["vsum"], bnd["vsum"])
    cm, cv = np.cumsum(ref["mom"][t_start:], 0), np.cumsum(ref["vsum"][t_start:], 0)
    for j in range(cm.shape[0]):
        within("tmom after timed step %d" % j, got["tmom_steps"][t_start + j], cm[j], bnd["tmom_cum"][j])
        within("tvar after timed step %d" % j, got["tvar_steps"][t_start + j], cv[j], bnd["tvar_cum"][j])
    for name in STEP_KEYS + TIME_KEYS:
        assert got[name].dtype == F32, name
        within(name, got[name], phys[name], bnd[name], bnd["qualifies"] if name in ("time_skew", "time_flat") else None)
    return worst, int(bnd["qualifies"].sum())


def vario_exact(mode, S, ref, t_start):
    """Integer mode: is every variogram sum, and every accumulated one, exact in fp32?  Binary data, S a power of two 2^j, and the
    largest accumulated S^2 V under 2^24."""
    if mode != "binary" or S & (S - 1) or "vint" not in ref:
        return False
    return int(np.cumsum(ref["vint"][t_start:], 0).max()) < 2 ** 24 and int(ref["vint"].max()) < 2 ** 24


def check_integer(got, ref, mode, S, t_start, what):
    """Integer mode: the raw buffers EQUAL the int64 reference after every step, and tmom / tvar the cumulative integer sums after
    every timed step.  -> whether the variogram sums were compared for equality (else they are checked by the bound only)."""
    Tn = ref["mom"].shape[0]
    assert np.abs(np.cumsum(ref["abs"][t_start:], 0)).max() < 2 ** 24 and ref["abs"].max() < 2 ** 24
    vex = vario_exact(mode, S, ref, t_start)
    for t in range(Tn):
        assert np.array_equal(got["mom_steps"][t], ref["mom"][t].astype(F32)), "%s: mom after step %d" % (what, t)
        if vex:
            assert np.array_equal(got["vsum_steps"][t], (ref["vint"][t] / float(S * S)).astype(F32)), "%s: vsum after step %d" % (what, t)
    assert np.array_equal(got["mom"], ref["mom"].astype(F32)) and (not vex or np.array_equal(got["vsum"], (ref["vint"] / float(S * S)).astype(F32)))
    cm = np.cumsum(ref["mom"][t_start:], 0)
    for j in range(Tn - t_start):
        assert np.array_equal(got["tmom_steps"][t_start + j], cm[j].astype(F32)), "%s: tmom after timed step %d" % (what, j)
        if vex:
            cv = np.cumsum(ref["vint"][t_start:], 0)[j] / float(S * S)
            assert np.array_equal(got["tvar_steps"][t_start + j], cv.astype(F32)), "%s: tvar after timed step %d" % (what, j)
    return vex


# ---- the scheme in numpy float32 (the sums in another order than the device's: exact on integer data, inside the bound otherwise) -----
def _slice_sums(term, lag, hw, plan, defect):
    """term [.., h, w] float32 over the pairs of the lag -> its sum [..]: the terms laid out at their pixel p in the field, every slice
    summed by numpy's pairwise float32 sum, the slices in slice order."""
    dx, dy = lag
    if defect == "dy_flip":
        dy = -dy
    H, W = hw
    full = np.zeros(term.shape[:-2] + (H, W), F32)
    i0 = max(0, -dy)
    full[..., i0:i0 + term.shape[-2], 0:term.shape[-1]] = term
    flat = full.reshape(term.shape[:-2] + (H * W,))
    acc = None
    for s in range(plan["P"]):
        part = flat[..., s * plan["SL"]:(s + 1) * plan["SL"]].sum(-1, dtype=F32)
        acc = part if acc is None else (acc + part).astype(F32)
    return acc


def simulate(xs, tgt, lags, plan, a, w, N, t_start, defect=None):
    """The kernels' scheme in float32, with a named defect put in:
      drop_last       the last column of pairs (the last row when dx = 0) is not counted
      dy_flip         dy taken with the wrong sign
      target_in_sbar  the target counted into sbar (S + 1 terms, times fl(1 / (S + 1)))
      s_minus_one     fl(1 / (S - 1)) for fl(1 / S) (S > 1)
      abs_cube        q = 3 taken as |D|^3
      n_hw            N_l = H W in the physical outputs
    -> the dict check() and check_integer() take."""
    Tn, S, B, Cc, H, W = xs.shape
    x = rows_of(xs, tgt)                                                     # float32 [T, B, C, R, H, W]
    mom, vs = [], []
    for lag in lags:
        d = increments(x, lag, defect).astype(F32)
        d2 = (d * d).astype(F32)
        d3 = (d2 * (np.abs(d) if defect == "abs_cube" else d)).astype(F32)
        d4 = (d2 * d2).astype(F32)
        mom.append(np.stack([_slice_sums(t, lag, (H, W), plan, defect) for t in (d2, d3, d4)], 1))
        s = np.sqrt(np.abs(d)).astype(F32)
        nm = S + 1 if defect == "target_in_sbar" else S
        acc = s[:, :, :, 0]
        for m in range(1, nm):
            acc = (acc + s[:, :, :, m]).astype(F32)
        den = S - 1 if defect == "s_minus_one" and S > 1 else nm
        sbar = (acc * F32(1.0 / den)).astype(F32)
        e = (s[:, :, :, S] - sbar).astype(F32)
        vs.append(_slice_sums((e * e).astype(F32), lag, (H, W), plan, defect))
    mom, vs = np.stack(mom, 4), np.stack(vs, 3)                              # [T, 3, B, C, L, R], [T, B, C, L]
    tm_steps, tv_steps = np.full(mom.shape, np.nan, F32), np.full(vs.shape, np.nan, F32)
    tm = tv = None
    for t in range(t_start, Tn):
        tm = mom[t].copy() if tm is None else (tm + mom[t]).astype(F32)
        tv = vs[t].copy() if tv is None else (tv + vs[t]).astype(F32)
        tm_steps[t], tv_steps[t] = tm, tv
    out = {k: v.astype(F32) for k, v in derive(mom, vs, a, w, N, t_start, S, tmom=tm, tvar=tv, defect=defect, hw=(H, W)).items()}
    out.update(mom=mom, vsum=vs, mom_steps=mom, vsum_steps=vs, tmom_steps=tm_steps, tvar_steps=tv_steps)
    return out
