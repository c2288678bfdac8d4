"""Case tables, the fp64 reference, the rounding bound and a float32 simulation of the ensemble energy score (csrc/tmg_gram.hip,
tmg_ops.EnsembleEnergy), shared by tests/test_energy_cpu.py (no device) and tests/test_energy_gpu.py.

Definitions (case b, kept step t; rows x_0..x_{S-1} the raw normalised members, x_S = y the normalised target, R = S + 1;
a_c = u[b, c] out_std[c] in fp64 from the fp32 factors; groups g of channels):
  d2_g[m, n] = sum_{c in g} a_c^2 sum_p (x_m - x_n)^2        the REFERENCE takes these direct differences in fp64 (integer data: in
                                                              int64) and never goes through a Gram matrix
  dist = sqrt(d2); target_dist_mean = (1/S) sum_{m<S} dist[m, S]; pair_dist_mean = (2/S^2) sum_{m<n<S} dist[m, n];
  energy_score = target_dist_mean - pair_dist_mean / 2; energy_score_fair: 1 / (S (S - 1)) for 1 / S^2 (S = 1: the pair term is 0);
  medoid = argmin_{m<S} sum_{n<S} dist[m, n]; nearest = argmin_{m<S} dist[m, S] (ties: lowest index); traj_dist2 = sum of d2 over the
  timed steps, traj_* the same formulas on sqrt(traj_dist2); time_* the plain means of the per-step scores over the timed steps.

The bound (u = 2^-24).  The kernel forms e_m = fl(x_m - r) about its own mean plane r and G_c[m, n] = sum_p e_m e_n in fp32: P slices,
each a sum of at most L terms (L and P from tmg_hip.ens_gram_plan: the four waves' fmaf chains of L / 4 end to end, three additions
in wave order, then P - 1 additions in slice order), then d2 = sum_c a2_c ((G_mm + G_nn) - 2 G_mn).  The identity
sum_p (e_m - e_n)^2 = G_mm + G_nn - 2 G_mn is exact for ANY r, so the error of d2 is the rounding alone:
  cnt = L + P + C_ROUND, C_ROUND = 10: 2 operand roundings (x - r), 2 combining additions (the doubling is exact), 2 for the scale (a_c^2
  rounded once from fp64, one product), up to 3 additions over the channels of a group, 1 for all second-order terms (cnt u < 1e-3)
  A_c = |e| |e|^T in fp64 about the kernel's own r
  beta[m, n] = sum_{c in g} cnt u (A_mm + A_nn + 2 A_mn) a_c^2 >= |d2 - ref|
  a distance gets min(sqrt(beta), beta / dist_ref) (|sqrt a - sqrt b| <= |a - b| / sqrt b and <= sqrt |a - b|); a mean of distances
  the mean of those bounds; energy_score the target term's plus half the pair term's; nearest_dist the largest bound of its column;
  traj_dist2 the sum of the steps' beta plus one rounding per step, Tn u (traj_ref + sum beta).
An argmin is compared by value: with E_m the bound of candidate m's sum, ref[returned] <= min ref + E_returned + E_argmin-of-ref.
The bound is never fitted to what the kernel gives; the GPU tests print the share of it that they reach."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
C_ROUND = 10
F32 = np.float32
STEP_KEYS = ("energy_score", "energy_score_fair", "target_dist_mean", "pair_dist_mean", "nearest_dist")
TRAJ_KEYS = ("traj_energy_score", "traj_energy_score_fair")
T = 3

# ---- case tables: (S, B, C, (H, W), groups, t_start, chunking, padded) ---------------------------------------------------------------
# R = S + 1 at every edge of the launch plan: 2; 15, 16 (the one-tile instance's last), 17 (one row alone in a second tile); 48, 63, 64
# (a full macro-tile), 65 (a second macro-tile: the off-diagonal instance); 131 (three macro-tiles, six pairs); HW 1, 63, 64, 65 (one
# wave's chunk and its neighbours), 272 (a little over one slice of 256: two slices), 528 (three slices, HW a multiple of 4: the float4
# loads with a ragged end); B 1 and 3, C 2..4, groups that reorder and omit channels; chunking 0: one member per chunk, 1: three, 2: all
HWS = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 272: (16, 17), 528: (16, 33)}
G2, G3, G4 = ((0, 1),), ((0, 1), (2,)), ((3, 1), (0,))
INT_TABLE = [
    (1, 1, 2, HWS[1], G2, 0, 0, False), (1, 3, 3, HWS[272], G3, 1, 2, True),
    (14, 1, 2, HWS[63], ((1,), (0,)), 0, 1, False), (15, 3, 3, HWS[64], ((2, 0),), 1, 0, True), (16, 1, 4, HWS[65], G4, 0, 2, False),
    (47, 3, 2, HWS[272], G2, 1, 1, True), (62, 1, 3, HWS[65], G3, 0, 2, False), (63, 1, 4, HWS[528], ((0, 1, 2, 3),), 0, 1, True),
    (63, 3, 2, HWS[1], ((1, 0),), 1, 2, False), (64, 1, 3, HWS[272], ((2,), (1, 0)), 0, 2, True), (64, 3, 2, HWS[63], G2, 1, 1, False),
    (130, 1, 2, HWS[272], G2, 0, 2, False), (130, 3, 4, HWS[64], G4, 1, 1, True), (4, 1, 3, HWS[528], G3, 0, 0, False),
    (8, 3, 3, HWS[272], G3, 1, 1, True), (32, 1, 3, HWS[528], G3, 0, 2, True),
]
# the longest wave loop: a slice of 512 pixels (two chunks per wave) needs HW > 256 * 768 / (B C NP): six pairs, twelve (case, channel)s
LONG_CASE = (130, 3, 4, (50, 58), ((0, 1), (2, 3)), 0, 2, False)
# the largest member count: 17 macro-tiles, 153 pairs
MAX_CASE = (1024, 1, 2, (1, 5), G2, 0, 2, False)
REAL_TABLE = [  # (S, B, C, (H, W), groups, kind, with_u)
    (7, 3, 3, HWS[272], G3, "gauss", True), (7, 3, 3, HWS[272], G3, "biased", False), (33, 1, 4, HWS[528], G4, "gauss", False),
    (33, 3, 2, HWS[65], G2, "biased", True), (64, 1, 3, HWS[272], G3, "near", True), (130, 1, 2, HWS[63], G2, "biased", True),
    (15, 3, 3, HWS[528], G3, "near", False), (9, 3, 3, HWS[65], G3, "centred", True),
]
SD = [1.7, 0.6, 2.5, 0.9]


def chunk_sizes(S, kind):
    per = (1, 3, S)[kind]
    return [min(per, S - m0) for m0 in range(0, S, per)]


@functools.lru_cache(maxsize=None)
def int_inputs(S, B, Cc, hw, seed, steps=T):
    """Integer data whose products and partial sums are exact in fp32 -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W], k [T, B, C, H, W])
    float32: per pixel the members are k + z with an integer mean k and z in -3..3 that cancels in pairs (an odd member out holds
    0); the target is an integer in -4..4.  The mean plane is fl(fl(S k) fl(1 / S)) = fl(k (1 + d)), |d| <= 2^-24, which is k for
    every k only when S is a power of two (d = 0); otherwise k is drawn from those of -2..2 for which this float32 product IS k
    (0 always is; a d < 0 leaves only 0, since below a power of two the spacing halves).  |e| <= 6 and HW <= 2900: every Gram
    entry stays under 2^24."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    ks = torch.tensor([v for v in range(-2, 3) if float(F32(F32(S * v) * F32(1.0 / S))) == v])
    k = ks[torch.randint(0, len(ks), (steps, 1, B, Cc, Hh, Ww), generator=g)]
    half = S // 2
    z = torch.zeros((steps, S, B, Cc, Hh, Ww), dtype=torch.int64)
    if half:
        zz = torch.randint(-3, 4, (steps, half, B, Cc, Hh, Ww), generator=g)
        perm = torch.randperm(S, generator=g)
        z[:, perm[:half]] = zz
        z[:, perm[half:2 * half]] = -zz
    tgt = torch.randint(-4, 5, (steps, B, Cc, Hh, Ww), generator=g)
    return (k + z).float().numpy(), tgt.float().numpy(), k[:, 0].float().numpy()


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, Cc, hw, kind, seed, steps=T):
    """gauss: members and target N(0.3, 1); biased: members 5 +- 0.1, target 0 +- 1; near: members 2 + 1e-3 N(0, 1) around a common
    N(0, 1) field, the target that field; centred: members 0.5 N(0, 1) around the target (the target is nearer to the members than
    they are to each other)."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    n = lambda *s: torch.randn(*s, Hh, Ww, generator=g)                       # noqa: E731
    if kind == "gauss":
        xs, tgt = n(steps, S, B, Cc) + 0.3, n(steps, B, Cc) + 0.3
    elif kind == "biased":
        xs, tgt = 5.0 + 0.1 * n(steps, S, B, Cc), n(steps, B, Cc)
    elif kind == "centred":
        tgt = n(steps, B, Cc)
        xs = tgt[:, None] + 0.5 * n(steps, S, B, Cc)
    else:
        tgt = n(steps, B, Cc)
        xs = tgt[:, None] + 2.0 + 1e-3 * n(steps, S, B, Cc)
    return xs.numpy().astype(F32), tgt.numpy().astype(F32)


def scales(sd, u, B, Cc):
    """a [B, C] fp64 = u out_std from the fp32 factors, and the float32 a^2 the kernel is handed."""
    sd = np.ones(Cc, F32) if sd is None else np.asarray(sd, F32)[:Cc]
    a = np.broadcast_to(sd.astype(np.float64), (B, Cc)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, Cc)
    return a, (a * a).astype(F32)


def rows_of(xs, tgt):
    """[T, S, B, C, H, W], [T, B, C, H, W] -> the R = S + 1 rows [T, B, C, R, HW] (torch, the dtype of xs)."""
    Tn, S, B, Cc = xs.shape[:4]
    x = torch.from_numpy(np.concatenate([xs, tgt[:, None]], 1)).reshape(Tn, S + 1, B, Cc, -1)
    return x.permute(0, 2, 3, 1, 4).contiguous()


def pair_d2(x):
    """x [R, HW] fp64 or int64 -> sum_p (x_m - x_n)^2 [R, R] by direct differences, a block of rows at a time."""
    R, HW = x.shape
    out = torch.empty((R, R), dtype=x.dtype)
    step = max(1, (1 << 23) // max(1, R * HW))
    for m0 in range(0, R, step):
        d = x[m0:m0 + step, None, :] - x[None, :, :]
        out[m0:m0 + step] = (d * d).sum(-1)
    return out


def derive(d2, S, defect=None):
    """d2 [.., R, R] fp64 -> the scores and argmins over the last two axes (numpy fp64 / int64)."""
    dist = np.sqrt(d2)
    mem = dist[..., :S, :S]
    tcol = dist[..., :S, S]
    rs = mem.sum(-1)
    tdm = tcol.mean(-1)
    pair = rs.sum(-1) / 2.0
    pdm = 2.0 * pair / (S * S)
    den = S * S if defect == "fair_s" else S * (S - 1)
    fair = tdm - 0.5 * (2.0 * pair / den if S > 1 else 0.0)
    cand = dist[..., :, :S].sum(-1) if defect == "target_medoid" else rs
    return {"dist": dist, "rowsum": rs, "target_dist_mean": tdm, "pair_dist_mean": pdm, "energy_score": tdm - 0.5 * pdm,
            "energy_score_fair": fair, "medoid": cand.argmin(-1), "nearest": tcol.argmin(-1), "nearest_dist": tcol.min(-1)}


def _finish(d2, S, groups, t_start, defect=None):
    """d2 [T, B, Gn, R, R] -> the whole output dict, arrays shaped as EnsembleEnergy's."""
    per = derive(d2, S, defect)
    out = {k: np.moveaxis(per[k], 0, 1) for k in STEP_KEYS + ("medoid", "nearest")}            # [B, T, Gn]
    out["d2"], out["dist"], out["rowsum"] = d2, per["dist"], per["rowsum"]
    traj = d2[t_start:].sum(0)
    tr = derive(traj, S, defect)
    out["traj_dist2"] = traj
    out["traj_cum"] = np.cumsum(d2[t_start:], 0)
    out["traj_dist"], out["traj_rowsum"] = tr["dist"], tr["rowsum"]
    out["traj_energy_score"], out["traj_energy_score_fair"] = tr["energy_score"], tr["energy_score_fair"]
    out["traj_medoid"], out["traj_nearest"] = tr["medoid"], tr["nearest"]
    out["time_energy_score"] = out["energy_score"][:, t_start:].mean(1)
    out["time_energy_score_fair"] = out["energy_score_fair"][:, t_start:].mean(1)
    return out


def reference(xs, tgt, a, groups, t_start, integer=False):
    """The fp64 reference from direct differences (integer: the squared differences summed in int64, exact)."""
    Tn, S, B, Cc = xs.shape[:4]
    x = rows_of(xs, tgt)
    x = x.to(torch.int64) if integer else x.double()
    dc = torch.stack([torch.stack([torch.stack([pair_d2(x[t, b, c]) for c in range(Cc)]) for b in range(B)]) for t in range(Tn)])
    dc = dc.double().numpy()                                                 # [T, B, C, R, R]
    a2 = (a * a).reshape(1, B, Cc, 1, 1)
    d2 = np.stack([sum(a2[:, :, c] * dc[:, :, c] for c in g) for g in groups], 2)
    return _finish(d2, S, groups, t_start)


def bounds(xs, tgt, r, a, groups, plan, ref, t_start, r_slack=0.0, extra_dist=None):
    """The bounds of the module docstring for every output, about the kernel's mean planes r [T, B, C, HW].  r_slack: added to |e| (a
    mean plane known only to that accuracy); extra_dist [T, B, Gn, R, R]: an error of the REFERENCE distances, added to every
    distance's bound."""
    Tn, S, B, Cc = xs.shape[:4]
    cnt = plan["L"] + plan["P"] + C_ROUND
    e = (rows_of(xs, tgt).double() - torch.from_numpy(np.asarray(r, dtype=np.float64)).reshape(Tn, B, Cc, 1, -1)).abs() + r_slack
    A = (e @ e.transpose(-1, -2)).numpy()                                    # [T, B, C, R, R]
    dg = np.diagonal(A, axis1=-2, axis2=-1)
    A3 = dg[..., :, None] + dg[..., None, :] + 2.0 * A
    a2 = (a * a).reshape(1, B, Cc, 1, 1)
    beta = np.stack([sum(cnt * U24 * a2[:, :, c] * A3[:, :, c] for c in g) for g in groups], 2)          # [T, B, Gn, R, R]

    def dist_bound(bt, dist, extra):
        with np.errstate(divide="ignore", invalid="ignore"):
            db = np.where(dist > 0, np.minimum(np.sqrt(bt), bt / dist), np.sqrt(bt))
        return db if extra is None else db + extra

    def score_bounds(db):
        tb = db[..., :S, S].mean(-1)
        pb = db[..., :S, :S].sum((-1, -2)) / (S * S)
        fb = tb + 0.5 * (db[..., :S, :S].sum((-1, -2)) / (S * (S - 1)) if S > 1 else 0.0)
        return {"target_dist_mean": tb, "pair_dist_mean": pb, "energy_score": tb + 0.5 * pb, "energy_score_fair": fb,
                "nearest_dist": db[..., :S, S].max(-1), "rowsum": db[..., :S, :S].sum(-1), "tcol": db[..., :S, S]}

    db = dist_bound(beta, ref["dist"], extra_dist)
    out = {k: (np.moveaxis(v, 0, 1) if k in STEP_KEYS else v) for k, v in score_bounds(db).items()}
    out["beta"] = beta
    cum = np.cumsum(beta[t_start:], 0)
    nst = np.arange(1, Tn - t_start + 1).reshape(-1, 1, 1, 1, 1)
    out["traj_cum"] = cum + nst * U24 * (ref["traj_cum"] + cum)
    ex = None if extra_dist is None else np.sqrt((extra_dist[t_start:] ** 2).sum(0))
    tdb = dist_bound(out["traj_cum"][-1], ref["traj_dist"], ex)
    tb = score_bounds(tdb)
    out["traj_energy_score"], out["traj_energy_score_fair"] = tb["energy_score"], tb["energy_score_fair"]
    out["traj_rowsum"], out["traj_tcol"] = tb["rowsum"], tb["tcol"]
    out["time_energy_score"] = out["energy_score"][:, t_start:].mean(1)
    out["time_energy_score_fair"] = out["energy_score_fair"][:, t_start:].mean(1)
    return out


def _argmin_ok(idx, refv, bnd):
    """ref[returned] <= min ref + bound[returned] + bound[argmin ref], over the last axis."""
    best = refv.argmin(-1)
    take = lambda v, i: np.take_along_axis(v, i[..., None], -1)[..., 0]      # noqa: E731
    return bool((take(refv, idx) <= refv.min(-1) + take(bnd, idx) + take(bnd, best)).all())


def check(got, ref, bnd, S, t_start, what, d2=True):
    """Every output of `got` (EnsembleEnergy's dict as numpy, plus traj_steps [T, B, Gn, R, R]: traj_dist2 after every step) against the
    reference within the bounds -> the worst share of a bound that was reached.  d2: also the squared distances step by step."""
    worst = 0.0

    def within(name, g, r, b):
        nonlocal worst
        err = np.abs(np.asarray(g, dtype=np.float64) - r)
        share = float(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0).max())
        assert not np.isnan(np.asarray(g, dtype=np.float64)).any() and share <= 1.0, \
            "%s %s: worst error is %.3g of its bound" % (what, name, share)
        worst = max(worst, share)

    for name in STEP_KEYS + TRAJ_KEYS + ("time_energy_score", "time_energy_score_fair"):
        assert got[name].dtype == F32, name
        within(name, got[name], ref[name], bnd[name])
    if d2:
        for j in range(ref["traj_cum"].shape[0]):
            within("traj_dist2 after timed step %d" % j, got["traj_steps"][t_start + j], ref["traj_cum"][j], bnd["traj_cum"][j])
    within("traj_dist2", got["traj_dist2"], ref["traj_dist2"], bnd["traj_cum"][-1])
    tr = got["traj_dist2"]
    assert tr.dtype == F32 and np.array_equal(tr, np.swapaxes(tr, -1, -2)) and not np.diagonal(tr, axis1=-2, axis2=-1).any(), what
    for name in ("medoid", "nearest", "traj_medoid", "traj_nearest"):
        assert got[name].dtype == np.int64 and got[name].min() >= 0 and got[name].max() < S, "%s %s" % (what, name)
    mv = lambda v: np.moveaxis(v, 0, 1)                                      # noqa: E731
    assert _argmin_ok(got["medoid"], mv(ref["rowsum"]), mv(bnd["rowsum"])), "%s medoid" % what
    assert _argmin_ok(got["nearest"], mv(ref["dist"][..., :S, S]), mv(bnd["tcol"])), "%s nearest" % what
    assert _argmin_ok(got["traj_medoid"], ref["traj_rowsum"], bnd["traj_rowsum"]), "%s traj_medoid" % what
    assert _argmin_ok(got["traj_nearest"], ref["traj_dist"][..., :S, S], bnd["traj_tcol"]), "%s traj_nearest" % what
    return worst


def check_integer(got, ref, k, t_start, what):
    """Integer mode: the mean plane is k, and traj_dist2 after every timed step (the first one: d2 itself) is the integer reference bit
    for bit."""
    Tn = got["r"].shape[0]
    assert np.array_equal(got["r"], k.reshape(got["r"].shape)), "%s: the mean plane is not the integer mean" % what
    for j in range(Tn - t_start):
        cum = ref["traj_cum"][j]
        assert cum.max() < 2 ** 24
        assert np.array_equal(got["traj_steps"][t_start + j], cum.astype(F32)), "%s: traj_dist2 after timed step %d" % (what, j)
    assert np.array_equal(got["traj_dist2"], ref["traj_dist2"].astype(F32)), what


# ---- the scheme in numpy float32 (the sums in another order than the device's: exact on integer data, inside the bound otherwise) -----
def simulate(xs, tgt, a2, groups, plan, t_start, defect=None):
    """The kernels' scheme operation by operation in float32, with a named defect put in:
      drop_run        the last run of 16 pixels is not contracted
      target_in_mean  the target is counted into the mean plane
      no_factor_two   G_mm + G_nn - G_mn
      fair_s          S for S - 1 in the fair term
      target_medoid   the target's column counted into the medoid's sums
    -> the dict check() takes (with r [T, B, C, HW] and traj_steps)."""
    Tn, S, B, Cc = xs.shape[:4]
    R, Gn = S + 1, len(groups)
    x = rows_of(xs, tgt).numpy()                                             # [T, B, C, R, HW] float32
    HW = x.shape[-1]
    acc = x[:, :, :, 0].copy()
    for m in range(1, S + (1 if defect == "target_in_mean" else 0)):
        acc = (acc + x[:, :, :, m]).astype(F32)
    r = (acc * F32(1.0 / (S + (1 if defect == "target_in_mean" else 0)))).astype(F32)
    e = (x - r[:, :, :, None]).astype(F32)
    if defect == "drop_run":
        e = e[..., :max(0, (HW - 1) // 16 * 16)]
    SL = plan["SL"]
    G = np.zeros(e.shape[:3] + (R, R), F32)
    for s in range(plan["P"]):
        part = np.zeros_like(G)
        for w in range(4):                                                   # the waves' chunks of the slice, then wave order
            cols = [c for c0 in range(s * SL + 64 * w, min(HW, (s + 1) * SL), 256) for c in range(c0, min(c0 + 64, e.shape[-1]))]
            ew = e[..., cols]
            part = (part + np.matmul(ew, np.swapaxes(ew, -1, -2)).astype(F32)).astype(F32)
        G = (G + part).astype(F32)
    dg = np.diagonal(G, axis1=-2, axis2=-1)
    d2 = np.zeros((Tn, B, Gn, R, R), F32)
    two = F32(1.0 if defect == "no_factor_two" else 2.0)
    for gi, g in enumerate(groups):
        d = None
        for c in g:
            q = ((dg[:, :, c, :, None] + dg[:, :, c, None, :]).astype(F32) - (two * G[:, :, c]).astype(F32)).astype(F32)
            v = (a2[None, :, c, None, None] * q).astype(F32)
            d = v if d is None else (d + v).astype(F32)
        d2[:, :, gi] = np.where(d < 0, F32(0), d)
    idx = np.arange(R)
    d2[..., idx, idx] = 0
    traj = np.zeros((B, Gn, R, R), F32)
    steps = np.full((Tn, B, Gn, R, R), np.nan, F32)
    for t in range(t_start, Tn):
        traj = (traj + d2[t]).astype(F32) if t > t_start else d2[t].copy()
        steps[t] = traj
    per = _finish(np.sqrt(d2).astype(np.float64) ** 2, S, groups, t_start, defect)   # dist = sqrtf(d2), then fp64 sums
    per_t = derive(np.sqrt(traj).astype(np.float64) ** 2, S, defect)
    out = {k: per[k].astype(F32) for k in STEP_KEYS}
    out.update(medoid=per["medoid"], nearest=per["nearest"], traj_dist2=traj, traj_steps=steps, r=r,
               traj_energy_score=per_t["energy_score"].astype(F32), traj_energy_score_fair=per_t["energy_score_fair"].astype(F32),
               traj_medoid=per_t["medoid"], traj_nearest=per_t["nearest"],
               time_energy_score=out["energy_score"][:, t_start:].astype(np.float64).mean(1).astype(F32),
               time_energy_score_fair=out["energy_score_fair"][:, t_start:].astype(np.float64).mean(1).astype(F32))
    return out
