"""Case tables, the float32 mirror of the labelling, the integer and fp64 references of the raw sums, the derived formulas and the
counted rounding bound of the ensemble phase averages (csrc/tmg_phase.hip, tmg_ops.EnsemblePhase), shared by tests/test_phase_cpu.py
(no device) and tests/test_phase_gpu.py.

Labels (case b, row = a member or the target at a kept step; raw_i, raw_j the row's raw coefficient sums on the pair's modes, g [B, 2]
the fp32 factors 1 / (HW sqrt(lam)), tab the 8 fp32 values of tmg_ops.phase_table: the gate, then the tangents):
  x = fl(g_i raw_i), y = fl(g_j raw_j); label -1 when fl(fl(x x) + fl(y y)) < tab[0]; else the quadrant from the signs (x > 0, y >= 0: 0;
  x <= 0, y > 0: 1; x < 0, y <= 0: 2; x >= 0, y < 0: 3) times NB / 4 plus the count of the tangents t_q with fl(t_q |x|) <= |y|
  (quadrants 0, 2) or fl(t_q |y|) <= |x| (quadrants 1, 3).  A point exactly on an edge belongs to the higher sector; (0, 0) with a
  gate of 0 is sector 0.  label_mirror does this in numpy float32, operation by operation; label_atan2 is the fp64 binning of
  atan2(y, x), which agrees away from the edges.

Raw sums (a [B, C] and m [B, C, H, W] as the kernel is handed them, fp32; rows the raw normalised members / target at the TIMED steps):
  d_c = a_c (x_c - m_c)                                  the REFERENCE forms d in fp64 (integer data: int64)
  raw[b, n] = sum over the rows of case b with label n of (d_0 .. d_{C-1}, d_0^2 .. d_{C-1}^2, d_0 d_1)      [B, NB, Q = 2 C + 1, HW]
grouped with boolean masks and summed directly, never through the kernel's tiling.

Derived outputs (fp64; n_k the rows of sector k, w_k = n_k / sum n, empty sectors NaN and left out of the aggregates):
  dev_k = raw_d / n_k, phase_mean = mean_phys + dev_k, phase_var = raw_dd / n_k - dev_k^2, phase_uv = raw_uv / n_k - dev_k0 dev_k1,
  coh_k = dev_k - sum_k w_k dev_k, coh_var = sum_k w_k coh_k^2, coh_uv = sum_k w_k coh_k0 coh_k1, incoh_var = sum_k w_k phase_var_k,
  incoh_uv = sum_k w_k phase_uv_k, coh_tke_frac = sum_{c < 2, p} coh_var / sum_{c < 2, p} (coh_var + incoh_var),
  phase_mean_rmse = sqrt(mean_p (dev_k - target dev_k)^2), coh_corr = sum coh_k tcoh_k / sqrt(sum coh_k^2 sum tcoh_k^2) over c < 2 and p,
  phase_speed = mean over consecutive timed steps of the increment of atan2(coef_j / sqrt(lam_j), coef_i / sqrt(lam_i)) wrapped to
  (-pi, pi].

The bound (u = 2^-24) of an accumulator element that received n rows.  The kernel loads the running value (0 at first), adds the n
terms one by one in fp32 and stores: n additions, each of relative error u on a partial sum of magnitude at most sum |term|.  A term
itself carries the roundings of its factors: d = fl(a fl(x - m)) is d (1 + e), |e| <= 2 u to first order, so
  a linear plane's term d:            2 u                      C_ROUND_LIN  = 2 + 1 = 3   (d's two roundings, 1 for all second-order terms)
  a product plane's term fl(d d'):    2 u + 2 u + u            C_ROUND_PROD = 4 + 1 + 1 = 6   (d's two roundings in EACH of the two factors,
                                                               the product's own rounding, 1 for all second-order terms: (n + 6) u < 1e-4)
  |acc - ref| <= (n + C_ROUND) u sum |term|
The counts come from the arithmetic above, never from what the kernel gives; the GPU tests print the share of the bound they reach.
Host-derived outputs are held to 2^-24 |ref| + 2^-40 against the formulas above applied to the device's own raw sums and labels."""
import functools
import math

import numpy as np
import torch

U24 = 2.0 ** -24
C_ROUND_LIN = 3
C_ROUND_PROD = 6
F32 = np.float32
BINS = (4, 8, 16, 32)
FIELD_KEYS = ("phase_mean", "phase_var", "phase_uv", "coh_var", "coh_uv", "incoh_var", "incoh_uv", "coh_tke_frac")
COUNT_KEYS = ("phase_bin", "target_phase_bin", "phase_count", "member_phase_count", "target_phase_count", "phase_skipped", "target_phase_skipped")
NEW_KEYS = COUNT_KEYS + FIELD_KEYS + tuple("target_" + k for k in FIELD_KEYS) + ("phase_mean_rmse", "coh_corr", "phase_speed",
                                                                                 "target_phase_speed", "phase_edges")

# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# The plan's tiles: 1024 pixels on the vector path (dense rows, HW % 4 == 0), 256 on the scalar path.  H x W: 1x1; 5x7 (ragged, scalar);
# 32x32 (exactly one vector tile) and 16x16 padded (exactly one scalar tile); 1x257 (one pixel over a scalar tile) and 4x257 (one
# thread's four pixels over a vector tile); 17x31 (three ragged scalar tiles) and 2x1030 (three vector tiles, the last of 12 pixels).
HWS = {1: (1, 1), 35: (5, 7), 256: (16, 16), 257: (1, 257), 527: (17, 31), 1024: (32, 32), 1028: (4, 257), 2060: (2, 1030)}
T = 4
# (S, B, C, (H, W), NB, chunking, padded, pattern); chunking 0: one member per chunk, 1: uneven, 2: all; padded: the rows are channel
# slices of a wider NaN-filled NHWC buffer (always the scalar path); pattern: "one" every row in one sector, "never" one sector never
# gets a row, "alt" the sectors in turn, "skip" as alt with step 2 wholly skipped.  Step 0 is never timed (t_start = 1).
INT_TABLE = [
    (1, 1, 2, HWS[1], 4, 2, False, "alt"), (17, 3, 3, HWS[35], 8, 1, False, "skip"), (70, 1, 4, HWS[1024], 32, 1, False, "alt"),
    (17, 1, 3, HWS[256], 8, 0, True, "never"), (5, 3, 2, HWS[257], 4, 2, False, "one"), (17, 1, 4, HWS[1028], 16, 1, False, "skip"),
    (70, 3, 3, HWS[527], 32, 2, True, "alt"), (3, 1, 3, HWS[2060], 8, 0, False, "never"), (17, 3, 2, HWS[1024], 4, 2, True, "alt"),
    (1, 3, 4, HWS[527], 16, 2, False, "one"), (70, 1, 2, HWS[2060], 8, 1, False, "skip"), (5, 1, 3, HWS[256], 32, 0, False, "alt"),
]
MAX_CASE = (1024, 1, 2, (2, 4), 32, 1, False, "alt")
REAL_TABLE = [  # (S, B, C, (H, W), NB, chunking, padded, with_u)
    (7, 3, 3, HWS[527], 8, 1, False, True), (33, 1, 4, HWS[1028], 16, 0, False, False), (17, 3, 2, HWS[256], 4, 2, True, True),
    (70, 1, 3, HWS[2060], 32, 1, False, True),
]
LABEL_TABLE = [(4, 1, 1), (8, 3, 17), (32, 1, 70), (32, 3, 17), (4, 3, 70), (8, 1, 1)]      # (NB, B, S)
SD = [1.7, 0.6, 2.5, 0.9]


def chunk_sizes(S, kind):
    if kind == 2:
        return [S]
    if kind == 0:
        return [1] * S
    out, pat, i = [], (1, 3, 2, 5, 18), 0
    while sum(out) < S:
        out.append(min(pat[i % len(pat)], S - sum(out)))
        i += 1
    return out


def table(NB, min_amp):
    """The 8 fp32 values of the label kernel, formed here on their own: fp64, rounded once."""
    tab = [F32(2.0 * float(min_amp) * float(min_amp))] + [F32(math.tan(2.0 * math.pi * q / NB)) for q in range(1, NB // 4)]
    return np.array(tab + [F32(0)] * (8 - len(tab)), dtype=F32)


def gains(lam, HW):
    """g [B, 2] = 1 / (HW sqrt(lam)) in fp64, rounded to fp32 once."""
    return (1.0 / (HW * np.sqrt(np.asarray(lam, dtype=np.float64)))).astype(F32)


def label_mirror(raw_i, raw_j, g_i, g_j, tab, NB):
    """The float32 mirror of tmg_ens_phase_label: every operation a numpy float32 operation of its own -> int32 labels."""
    ri, rj = np.asarray(raw_i, dtype=F32), np.asarray(raw_j, dtype=F32)
    x = (np.asarray(g_i, dtype=F32) * ri).astype(F32)
    y = (np.asarray(g_j, dtype=F32) * rj).astype(F32)
    r2 = ((x * x).astype(F32) + (y * y).astype(F32)).astype(F32)
    ax, ay = np.abs(x), np.abs(y)
    nq = NB // 4
    q0, q1, q2, q3 = (x > 0) & (y >= 0), (x <= 0) & (y > 0), (x < 0) & (y <= 0), (x >= 0) & (y < 0)
    base = np.where(q0, 0, np.where(q1, nq, np.where(q2, 2 * nq, np.where(q3, 3 * nq, -1))))
    mirrored = q1 | q3
    p, q = np.where(mirrored, ay, ax).astype(F32), np.where(mirrored, ax, ay).astype(F32)
    cnt = np.zeros(x.shape, dtype=np.int64)
    for i in range(nq - 1):
        cnt += ((F32(tab[1 + i]) * p).astype(F32) <= q)
    out = np.where(base >= 0, base + cnt, 0)
    return np.where(r2 < F32(tab[0]), -1, out).astype(np.int32)


def label_atan2(x, y, NB):
    """fp64: the sector of atan2(y, x) counted from the positive x axis towards positive y (valid away from the edges)."""
    th = np.mod(np.arctan2(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)), 2 * np.pi)
    return (np.floor(th / (2 * np.pi / NB)).astype(np.int64) % NB).astype(np.int32)


def pattern_labels(pattern, S, B, NB, steps=T):
    """The wanted labels [B, S, steps] of a pattern (-1: a skipped row)."""
    s, b, t = np.meshgrid(np.arange(S), np.arange(B), np.arange(steps), indexing="ij")
    s, b, t = s.transpose(1, 0, 2), b.transpose(1, 0, 2), t.transpose(1, 0, 2)
    if pattern == "one":
        lab = np.full((B, S, steps), NB - 1)
    elif pattern == "never":
        lab = (s + t + b) % (NB - 1)                                         # sector NB - 1 never gets a row
    else:
        lab = (s + 3 * t + b) % NB
        if pattern == "skip":
            lab = np.where(t == 2, -1, lab)
            lab = np.where((s % 5 == 4) & (t == 3), -1, lab)                     # and single skipped rows inside a chunk
    return lab.astype(np.int64)


def coefs_for(lab, NB, HW, seed):
    """Raw coefficient pairs [.., 2] float32 whose labels are `lab` with lam = 1 (g = 1 / HW): radius 1.5 at the sector's centre plus
    up to a quarter sector of jitter; a skipped row has radius 0.1 (under the default gate 0.25 sqrt(2))."""
    rng = np.random.RandomState(seed)
    th = (np.maximum(lab, 0) + 0.5 + 0.25 * (2 * rng.rand(*lab.shape) - 1)) * (2 * np.pi / NB)
    r = np.where(lab >= 0, 1.5, 0.1) * HW
    return np.stack([r * np.cos(th), r * np.sin(th)], -1).astype(F32)


@functools.lru_cache(maxsize=None)
def int_inputs(S, B, Cc, hw, seed, steps=T):
    """Integer data -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W], m [B, C, H, W]) float32, integers in -8..8; a = 1: |d| <= 16, a
    term at most 256, so 2^7 rows per sector keep every sum under 2^15."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    xs = torch.randint(-8, 9, (steps, S, B, Cc, Hh, Ww), generator=g)
    tgt = torch.randint(-8, 9, (steps, B, Cc, Hh, Ww), generator=g)
    m = torch.randint(-8, 9, (B, Cc, Hh, Ww), generator=g)
    return xs.float().numpy(), tgt.float().numpy(), m.float().numpy()


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, Cc, hw, with_u, seed, steps=T):
    """Gaussian members, target and mean -> (xs, tgt, m float32, sd [C], u [B, C] or None)."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    sd = torch.tensor(SD[:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=g)) if with_u else None
    tgt = torch.randn(steps, B, Cc, Hh, Ww, generator=g) + 0.3
    xs = torch.randn(steps, S, B, Cc, Hh, Ww, generator=g) + 0.3
    m = 0.3 + 0.5 * torch.randn(B, Cc, Hh, Ww, generator=g)
    return (xs.numpy().astype(F32), tgt.numpy().astype(F32), m.numpy().astype(F32), sd.numpy(), None if u is None else u.numpy())


def scales(sd, u, B, Cc):
    """a [B, C]: u out_std in fp64 from the fp32 factors, rounded to fp32 once (what the kernel is handed), as fp64."""
    sd = np.ones(Cc, F32) if sd is None else np.asarray(sd, F32)[:Cc]
    a = np.broadcast_to(sd.astype(np.float64), (B, Cc)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, Cc)
    return a.astype(F32).astype(np.float64)


def reference(rows, lab, timed, a, m, NB, integer=False):
    """The raw sums by boolean masks.  rows [T, S, B, C, H, W] (the target: S = 1), lab [B, S, T], timed: the timed steps, a [B, C],
    m [B, C, H, W] -> dict: raw [B, NB, Q, HW] (int64 or fp64), abs (the sums of the terms' magnitudes), n [B, NB] the rows."""
    dt = np.int64 if integer else np.float64
    x = np.asarray(rows).astype(dt)
    Tn, S, B, Cc = x.shape[:4]
    HW = x.shape[4] * x.shape[5]
    d = (np.asarray(a).astype(dt)[None, None, :, :, None, None] * (x - np.asarray(m).astype(dt)[None, None])).reshape(Tn, S, B, Cc, HW)
    on = np.zeros(Tn, dtype=bool)
    on[list(timed)] = True
    raw, ab, n = np.zeros((B, NB, 2 * Cc + 1, HW), dtype=dt), np.zeros((B, NB, 2 * Cc + 1, HW), dtype=dt), np.zeros((B, NB), dtype=np.int64)
    for b in range(B):
        db = d[:, :, b]                                                      # [T, S, C, HW]
        terms = np.concatenate([db, db * db, db[:, :, :1] * db[:, :, 1:2]], axis=2)
        for k in range(NB):
            mask = (np.asarray(lab)[b].T == k) & on[:, None]                 # [T, S]
            n[b, k] = int(mask.sum())
            raw[b, k] = terms[mask].sum(0)
            ab[b, k] = np.abs(terms[mask]).sum(0)
    return {"raw": raw, "abs": ab, "n": n}


def check_integer(acc, ref, what):
    assert ref["n"].max() <= 2 ** 7 and np.abs(ref["abs"]).max() < 2 ** 24, "%s: %d rows in a sector" % (what, ref["n"].max())
    assert acc.dtype == F32 and np.array_equal(acc, ref["raw"].astype(F32)), "%s: the accumulators are not the integer sums" % what


def check_bound(acc, ref, Cc, what):
    """Every accumulator element inside (n + C_ROUND) u sum |term| -> the worst share of the bound that is reached."""
    cr = np.array([C_ROUND_LIN] * Cc + [C_ROUND_PROD] * (Cc + 1), dtype=np.float64).reshape(1, 1, -1, 1)
    bound = (ref["n"].astype(np.float64)[:, :, None, None] + cr) * U24 * ref["abs"]
    err = np.abs(acc.astype(np.float64) - ref["raw"])
    assert acc.dtype == F32 and not np.isnan(acc).any(), what
    share = float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())
    assert share <= 1.0, "%s: worst error is %.3g of its bound" % (what, share)
    return share


def counts(lab, timed, NB):
    """lab [B, S, T] -> (member counts [B, S, NB], skipped [B]) over the timed steps."""
    lt = np.asarray(lab)[:, :, list(timed)]
    return np.stack([(lt == k).sum(2) for k in range(NB)], -1), (lt < 0).sum((1, 2))


def fields(n, raw, Cc):
    """n [B, NB], raw [B, NB, Q, P] -> the derived fields (fp64) by the formulas of the module docstring."""
    n = np.asarray(n, dtype=np.float64)
    raw = np.asarray(raw, dtype=np.float64)
    B, NB = n.shape
    P = raw.shape[-1]
    nan = np.nan
    dev, var, uv = np.full((B, NB, Cc, P), nan), np.full((B, NB, Cc, P), nan), np.full((B, NB, P), nan)
    coh = np.full((B, NB, Cc, P), nan)
    out = {k: np.full((B, Cc, P), nan) for k in ("coh_var", "incoh_var")}
    out.update({k: np.full((B, P), nan) for k in ("coh_uv", "incoh_uv")})
    out["coh_tke_frac"] = np.full((B,), nan)
    for b in range(B):
        ks = [k for k in range(NB) if n[b, k] > 0]
        for k in ks:
            dev[b, k] = raw[b, k, :Cc] / n[b, k]
            var[b, k] = raw[b, k, Cc:2 * Cc] / n[b, k] - dev[b, k] * dev[b, k]
            uv[b, k] = raw[b, k, 2 * Cc] / n[b, k] - dev[b, k, 0] * dev[b, k, 1]
        if not ks:
            continue
        w = n[b] / n[b].sum()
        mbar = sum(w[k] * dev[b, k] for k in ks)
        for k in ks:
            coh[b, k] = dev[b, k] - mbar
        out["coh_var"][b] = sum(w[k] * coh[b, k] ** 2 for k in ks)
        out["coh_uv"][b] = sum(w[k] * coh[b, k, 0] * coh[b, k, 1] for k in ks)
        out["incoh_var"][b] = sum(w[k] * var[b, k] for k in ks)
        out["incoh_uv"][b] = sum(w[k] * uv[b, k] for k in ks)
        num = out["coh_var"][b, :2].sum()
        out["coh_tke_frac"][b] = num / (num + out["incoh_var"][b, :2].sum())
    out.update(dev=dev, var=var, uv=uv, coh=coh)
    return out


def speed(coef, lam, pair, timed):
    """coef [.., T, K], lam [B, 2] fp64 -> the mean wrapped increment of the angle over consecutive timed steps."""
    c = np.asarray(coef, dtype=np.float64)[..., list(timed), :]
    if c.shape[-2] < 2:
        return np.full(c.shape[:-2], np.nan)
    s = np.sqrt(np.asarray(lam, dtype=np.float64))
    s = s.reshape((s.shape[0],) + (1,) * (c.ndim - 2) + (2,))
    th = np.arctan2(c[..., pair[1]] / s[..., 1], c[..., pair[0]] / s[..., 0])
    dth = np.diff(th, axis=-1)
    dth = dth - 2 * np.pi * np.ceil((dth - np.pi) / (2 * np.pi))
    return dth.mean(-1)


def derive(got, acc, tacc, Cc, hw, mean_phys, lam, pair, timed):
    """Every host-derived output (fp64) from the device's own raw sums acc, tacc [B, NB, Q, HW] and labels."""
    NB = acc.shape[1]
    B = acc.shape[0]
    Hh, Ww = hw
    mc, skipped = counts(got["phase_bin"], timed, NB)
    tc, tskipped = counts(got["target_phase_bin"][:, None], timed, NB)
    out = {"member_phase_count": mc, "phase_count": mc.sum(1), "target_phase_count": tc[:, 0], "phase_skipped": skipped,
           "target_phase_skipped": tskipped}
    fe, ft = fields(out["phase_count"], acc, Cc), fields(out["target_phase_count"], tacc, Cc)
    mp = np.asarray(mean_phys, dtype=np.float64).reshape(B, 1, Cc, -1)
    for pre, f in (("", fe), ("target_", ft)):
        out[pre + "phase_mean"] = (mp + f["dev"]).reshape(B, NB, Cc, Hh, Ww)
        out[pre + "phase_var"] = f["var"].reshape(B, NB, Cc, Hh, Ww)
        out[pre + "phase_uv"] = f["uv"].reshape(B, NB, Hh, Ww)
        for k in ("coh_var", "incoh_var"):
            out[pre + k] = f[k].reshape(B, Cc, Hh, Ww)
        for k in ("coh_uv", "incoh_uv"):
            out[pre + k] = f[k].reshape(B, Hh, Ww)
        out[pre + "coh_tke_frac"] = f["coh_tke_frac"]
    diff = fe["dev"] - ft["dev"]
    out["phase_mean_rmse"] = np.sqrt((diff * diff).mean(-1))
    ce, ct = fe["coh"][:, :, :2].reshape(B, NB, -1), ft["coh"][:, :, :2].reshape(B, NB, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["coh_corr"] = (ce * ct).sum(-1) / np.sqrt((ce * ce).sum(-1) * (ct * ct).sum(-1))
    out["phase_speed"] = speed(got["coef"], lam, pair, timed)
    out["target_phase_speed"] = speed(got["target_coef"], lam, pair, timed)
    out["phase_edges"] = 2 * np.pi * np.arange(NB + 1) / NB
    return out


def check_derived(got, ref, what):
    """Counts equal; every float output within 2^-24 |ref| + 2^-40 of the formulas, NaN exactly where the reference is."""
    for name in NEW_KEYS:
        if name in ("phase_bin", "target_phase_bin"):
            continue
        g, r = np.asarray(got[name]), np.asarray(ref[name])
        assert g.shape == r.shape, "%s %s: %s, not %s" % (what, name, g.shape, r.shape)
        if r.dtype.kind == "i":
            assert g.dtype == np.int64 and np.array_equal(g, r), "%s %s" % (what, name)
            continue
        assert g.dtype == (np.float64 if name == "phase_edges" else F32), "%s %s: %s" % (what, name, g.dtype)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin), "%s %s: NaN pattern" % (what, name)
        err = np.abs(g.astype(np.float64)[fin] - r[fin])
        assert bool((err <= U24 * np.abs(r[fin]) + 2.0 ** -40).all()), "%s %s: off by %.3g" % (what, name, float(err.max()))
