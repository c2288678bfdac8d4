"""Case tables, the float32 mirror of the state, the int64 reference, the fp64 reference by direct definition, the fp64 host
restatement of the finalize formulas and the counted rounding bounds of the ensemble two-point space-time correlations
(csrc/tmg_corr.hip, tmg_ops.EnsembleCorrelation), shared by tests/test_corr_cpu.py (no device) and tests/test_corr_gpu.py.

Rows are the S members plus the target as row S.  a [B, 3] and m [B, 3, H, W] are the fp32 tables the kernels are handed, x the raw
normalised rows; t = 0, 1, .. numbers the TIMED steps, lag l has n_l = T - tau_l pairs (probe at t - tau_l, field at t).

THE ORDER of the state (stated once here, once in the kernel's header comment), every operation a float32 operation of its own:
  d_c = fl(a_c fl(x_c - m_c));  series[row, b, t, p, c] = d_c at probe p
  X[p,q,l] at plane (p Q + q) L + l:          term = fl(series[row, b, t - tau_l, p, ci_q] * d_{cj_q}(x, t))
  F[j,l]   at plane P Q L + j L + l:          term = d_j(x, t)                 (J = the sorted distinct cj)
  G[j,l]   at plane P Q L + |J| L + j L + l:  term = fl(d_j d_j)
  a plane of lag l holds the term of t == tau_l, then fl(raw + term) per timed step t > tau_l in step order; it is untouched before.

The reference by direct definition (fp64, per row, case, probe, pair and lag): with d = a (x - m) exactly, n = T - tau,
probe = d_ci(x0, 0 .. n - 1) and field = d_cj(x, tau .. T - 1),
  cov = mean((probe - mean probe) (field - mean field)),  rho = cov / (std probe  std field)      (population std), NaN for n < 2
written with numpy's mean and std on the two slices: no planes, no shift formula.  The host restatement applies the kernel's formulas
to a given raw state and series in fp64:  mf = F / n, vf = G / n - mf^2, cov = X / n - pm mf, rho = cov / sqrt(pv vf).

The bounds (u = 2^-24, e = 2^-53), counted from the arithmetic, never from what the kernel gives:
  d, series   the subtraction and the multiplication: |d32 - d| <= e_d = 2 u |d|   (+ u pad, where the test's own inputs are uncertain)
  X  the two factors carry e_s and e_d, the product one rounding, and n - 1 additions of relative error u on partial sums of at most
     A_X = sum |s| |d|:   dX <= sum (|s| e_d + |d| e_s) + u A_X + (n - 1) u A_X            = (n - 1 + 5) u A_X without pad
  F  dF <= sum e_d + (n - 1) u A_F, A_F = sum |d|                                          = (n - 1 + 2) u A_F
  G  dG <= sum 2 |d| e_d + u A_G + (n - 1) u A_G, A_G = sum d^2                            = (n - 1 + 5) u A_G
  the probe sums (fp64 on the host from the fp32 series):  d(sum s) <= sum e_s,  d(sum s^2) <= sum 2 |s| e_s
  first-order propagation, with the definition's own mf, pm, vf, pv:
     dmf = dF / n,  dpm = d(sum s) / n,  dvf = dG / n + 2 |mf| dmf,  dpv = d(sum s^2) / n + 2 |pm| dpm
     dcov = dX / n + |mf| dpm + |pm| dmf
     drho = dcov / sqrt(pv vf) + |rho| (dpv / (2 pv) + dvf / (2 vf))
  doubled for the second order, which holds while dpv / pv and dvf / vf stay under 1 / 4; beyond that nothing can be said and the
  bound is infinite (the synthetic cases are drawn so that this never happens: nothing is excluded there).  The fp64 evaluation adds
  C_FIN = 8 roundings e on the operand magnitudes, the fp32 output u |ref|:
     |cov - ref| <= u |ref| + 2 dcov + C_FIN e (A_X / n + |pm| |mf|)
     |rho - ref| <= u |ref| + 2 drho + C_FIN e (A_X / n + |pm| |mf|) / sqrt(pv vf) + C_FIN e |rho|
  The Welford mean over the members moves by at most the largest member bound; so does the population std (1-Lipschitz in the
  largest change of a value), whose own fp64 roundings dq = 2 (C_FIN + 4 S) e max|v|^2 of the variance move it by at most
  min(sqrt(dq), dq / std).
  Same raw (device against the host restatement): both sides evaluate the same fp64 formula; |got - ref| <= u |ref| + 2^-40.
Real test data stays in the normal fp32 range."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
E53 = 2.0 ** -53
C_D, C_X, C_F, C_G = 2, 5, 2, 5
C_FIN = 8
SAME_RAW_ABS = 2.0 ** -40
F32 = np.float32
FIELD_KEYS = ("tp_cov_mean", "tp_cov_std", "tp_rho_mean", "tp_rho_std", "target_tp_cov", "target_tp_rho")
DERIVED_KEYS = ("tp_len", "tp_len_mean", "tp_len_std", "target_tp_len", "tp_shift", "tp_speed", "tp_speed_mean", "tp_speed_std",
                "target_tp_speed")
NEW_KEYS = FIELD_KEYS + ("member_tp_rho", "tp_line_x", "tp_line_y") + DERIVED_KEYS + ("tp_probes", "tp_pairs", "tp_lags")

# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# (S, B, (H, W), padded, T timed steps); FRONT[i] untimed steps come first; padded: the rows are channel slices of a wider NaN-filled
# buffer.  5x7: scalar path, one block; 19x15: scalar path, 285 pixels cross a block of 256; 8x12: vector path; 6x256: vector path,
# 1536 pixels cross a block of 1024; the last case is the member limit.
CASES = [(3, 2, (5, 7), False, 6), (2, 1, (19, 15), True, 5), (4, 2, (8, 12), True, 7), (2, 1, (6, 256), False, 5)]
MAX_CASE = (1024, 1, (3, 4), False, 3)
FRONT = [1, 2, 1, 2]
CHUNKINGS = {1024: [(1024,), (64,) * 16], 2: [(2,), (1, 1)], 3: [(3,), (1, 1, 1), (2, 1)], 4: [(4,), (1, 1, 1, 1), (1, 3)]}
PAIRS = ((0, 0), (1, 1), (0, 1), (2, 2))                                     # J = (0, 1, 2)
SD = [1.7, 0.6, 2.5]
MU = [0.4, -0.1, 0.25]
GRID = (0.5, 0.25)


def probes_of(hw):
    """The four corners (the last of them is the last pixel), an interior pixel and a duplicate of probe 1."""
    Hh, Ww = hw
    return ((0, 0), (0, Ww - 1), (Hh - 1, 0), (Hh - 1, Ww - 1), (Hh // 2, Ww // 2), (0, Ww - 1))


DUPLICATE = (1, 5)


def lags_of(T):
    """The distinct values of (0, 1, T - 2, T - 1, T + 1): n = 2, n = 1 and a lag whose planes are never written."""
    return tuple(sorted({0, 1, T - 2, T - 1, T + 1}))


def jset(pairs):
    return tuple(sorted({cj for _ci, cj in pairs}))


def planes(P, pairs, L):
    return P * len(pairs) * L + 2 * len(jset(pairs)) * L


@functools.lru_cache(maxsize=None)
def int_inputs(S, B, hw, steps, seed):
    """Integer data -> (xs [steps, S + 1, B, 3, H, W] (row S: the target), m [B, 3, H, W]) float32; x in -3..3, m in -1..1, a = 1:
    |d| <= 4, a term at most 16 and at most 8 steps keep every sum under 2^8: exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(-3, 4, (steps, S + 1, B, 3) + tuple(hw), generator=g)
    m = torch.randint(-1, 2, (B, 3) + tuple(hw), generator=g)
    return xs.float().numpy(), m.float().numpy()


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, hw, steps, seed):
    """Normal noise plus a smooth part -> (xs [steps, S + 1, B, 3, H, W], m [B, 3, H, W] float32, sd [3], mu [3], u [B, 3]).  The
    smooth part is a ramp in time whose slope varies smoothly over the field with a magnitude in 1..1.5 and a sign per row and
    channel; with noise of std 0.12 two consecutive steps never come close, so that even the n = 2 lags keep their variances away
    from zero (test_corr_cpu checks pv * vf > 1e-3 of its median on every case)."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    yy, xx = torch.meshgrid(torch.arange(Hh, dtype=torch.float32), torch.arange(Ww, dtype=torch.float32), indexing="ij")
    ph = 6.28 * torch.rand(1, S + 1, B, 3, 1, 1, generator=g)
    slope = 1.25 + 0.25 * torch.sin(0.7 * xx + 0.9 * yy + ph)
    sign = torch.where(torch.rand(1, S + 1, B, 3, 1, 1, generator=g) < 0.5, -1.0, 1.0)
    tt = torch.arange(steps, dtype=torch.float32).view(steps, 1, 1, 1, 1, 1) - 0.5 * (steps - 1)
    m = 0.3 + 0.5 * torch.randn(B, 3, Hh, Ww, generator=g)
    xs = m[None, None] + sign * slope * tt + 0.12 * torch.randn(steps, S + 1, B, 3, Hh, Ww, generator=g)
    u = 0.5 + torch.rand(B, 3, generator=g)
    return xs.numpy().astype(F32), m.numpy().astype(F32), np.array(SD, F32), np.array(MU, F32), u.numpy().astype(F32)


def scales(sd, u, B):
    """a [B, 3]: u out_std in fp64 from the fp32 factors, rounded to fp32 once (what the kernels are handed)."""
    a = np.broadcast_to(np.asarray(sd, F32).astype(np.float64), (B, 3)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, 3)
    return a.astype(F32)


# ---- 1: the float32 mirror --------------------------------------------------------------------------------------------------------------
def mirror(xs, a, m, timed, probes, pairs, lags):
    """The state after every step: xs [steps, R, B, 3, H, W] -> list of (series [R, B, steps, P, 3], raw [R, B, NPL, HW]) float32
    snapshots; what no launch has written is NaN (the tests pre-fill the device's state with NaN)."""
    xs, a = np.asarray(xs), np.asarray(a)
    assert xs.dtype == F32 and a.dtype == F32 and (m is None or m.dtype == F32)
    steps, R, B = xs.shape[:3]
    Hh, Ww = xs.shape[-2:]
    P, Q, L, J = len(probes), len(pairs), len(lags), jset(pairs)
    series = np.full((R, B, steps, P, 3), np.nan, F32)
    raw = np.full((R, B, planes(P, pairs, L), Hh * Ww), np.nan, F32)
    offf, offg = P * Q * L, P * Q * L + len(J) * L
    snaps, t = [], 0
    for step in range(steps):
        if step in timed:
            d = a[None, :, :, None, None] * (xs[step] - (np.zeros_like(xs[0, 0]) if m is None else m)[None])   # [R, B, 3, H, W]
            assert d.dtype == F32
            for p, (h, w) in enumerate(probes):
                series[:, :, t, p] = d[:, :, :, h, w]
            df = d.reshape(R, B, 3, -1)
            for l, tau in enumerate(lags):
                if tau > t:
                    continue
                terms = []
                for p in range(P):
                    for q, (ci, cj) in enumerate(pairs):
                        terms.append(((p * Q + q) * L + l, series[:, :, t - tau, p, ci][:, :, None] * df[:, :, cj]))
                for j, ch in enumerate(J):
                    terms.append((offf + j * L + l, df[:, :, ch]))
                    terms.append((offg + j * L + l, df[:, :, ch] * df[:, :, ch]))
                for pl, term in terms:
                    assert term.dtype == F32
                    raw[:, :, pl] = term if tau == t else raw[:, :, pl] + term
            t += 1
        snaps.append((series.copy(), raw.copy()))
    return snaps


def int_reference(xs, m, timed, probes, pairs, lags):
    """Integer data, a = 1: the sums of the planes in int64, summed directly -> ([R, B, NPL, HW] int64, written [NPL] bool)."""
    x = np.asarray(xs)[list(timed)].astype(np.int64)
    d = x - np.asarray(m).astype(np.int64)[None, None]                        # [T, R, B, 3, H, W]
    T, R, B = d.shape[:3]
    P, Q, L, J = len(probes), len(pairs), len(lags), jset(pairs)
    out = np.zeros((R, B, planes(P, pairs, L), d.shape[-2] * d.shape[-1]), np.int64)
    written = np.zeros(out.shape[2], bool)
    df = d.reshape(T, R, B, 3, -1)
    offf, offg = P * Q * L, P * Q * L + len(J) * L
    for l, tau in enumerate(lags):
        if tau >= T:
            continue
        for p, (h, w) in enumerate(probes):
            for q, (ci, cj) in enumerate(pairs):
                out[:, :, (p * Q + q) * L + l] = (d[:T - tau, :, :, ci, h, w][..., None] * df[tau:, :, :, cj]).sum(0)
                written[(p * Q + q) * L + l] = True
        for j, ch in enumerate(J):
            out[:, :, offf + j * L + l] = df[tau:, :, :, ch].sum(0)
            out[:, :, offg + j * L + l] = (df[tau:, :, :, ch] ** 2).sum(0)
            written[offf + j * L + l] = written[offg + j * L + l] = True
    assert np.abs(out).max() < 2 ** 24
    return out, written


# ---- 2: the definition and the restatement -------------------------------------------------------------------------------------------------
def fluct(xs, a, m, timed):
    """d = a (x - m) in fp64 from the fp32 tables at the timed steps -> [T, R, B, 3, H, W]."""
    x = np.asarray(xs, dtype=np.float64)[list(timed)]
    a64 = np.asarray(a, dtype=np.float64)[None, None, :, :, None, None]
    return a64 * (x - (0.0 if m is None else np.asarray(m, dtype=np.float64)[None, None]))


def definition(d, probes, pairs, lags, mut=None, pad=None):
    """The reference by direct definition on d [T, R, B, 3, H, W] fp64 -> dict: cov, rho [R, B, P, Q, L, H, W] (NaN for n < 2), and
    the bounds bcov, brho of the module docstring (without the output's u |ref|), pvvf = pv * vf.  pad [T, R, B, 3, H, W]: what d
    is uncertain by beyond its own two roundings, in units of u.  mut: one deliberate mistake (the sensitivity test): "lag" tau + 1
    in place of tau, "n" the sums divided by T in place of n, "window" the variances of the whole window in place of those of the
    paired samples, "swap" ci and cj exchanged."""
    T, R, B = d.shape[:3]
    Hh, Ww = d.shape[-2:]
    P, Q, L = len(probes), len(pairs), len(lags)
    shape = (R, B, P, Q, L, Hh, Ww)
    out = {k: np.full(shape, np.nan) for k in ("cov", "rho", "bcov", "brho", "pvvf")}
    ed = U24 * (C_D * np.abs(d) + (0.0 if pad is None else np.asarray(pad, dtype=np.float64)))
    for l, tau in enumerate(lags):
        n = T - tau
        if n < 2:
            continue
        tl = tau + 1 if mut == "lag" and tau + 1 < T else tau
        nn = T - tl
        for p, (h, w) in enumerate(probes):
            for q, (ci, cj) in enumerate(pairs):
                if mut == "swap":
                    ci, cj = cj, ci
                probe = d[:nn, :, :, ci, h, w][..., None, None]              # [n, R, B, 1, 1]
                field = d[tl:, :, :, cj]                                     # [n, R, B, H, W]
                pm, mf = probe.mean(0), field.mean(0)
                cov = ((probe - pm[None]) * (field - mf[None])).mean(0)
                if mut == "n":
                    cov = cov * nn / T
                sp, sf = probe.std(0), field.std(0)
                if mut == "window":
                    sp, sf = d[:, :, :, ci, h, w].std(0)[..., None, None], d[:, :, :, cj].std(0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rho = cov / (sp * sf)
                out["cov"][:, :, p, q, l], out["rho"][:, :, p, q, l] = cov, rho
                if mut is not None:
                    continue
                # the bound, from this lag's own samples
                es, edf = ed[:n, :, :, ci, h, w][..., None, None], ed[tau:, :, :, cj]
                ap, af = np.abs(probe), np.abs(field)
                AX, AF, AG = (ap * af).sum(0), af.sum(0), (field * field).sum(0)
                dX = (ap * edf + af * es).sum(0) + U24 * AX + (n - 1) * U24 * AX
                dF = edf.sum(0) + (n - 1) * U24 * AF
                dG = (2.0 * af * edf).sum(0) + U24 * AG + (n - 1) * U24 * AG
                dS, dS2 = es.sum(0), (2.0 * ap * es).sum(0)
                pv, vf = sp * sp, sf * sf
                dmf, dpm = dF / n, dS / n
                dvf, dpv = dG / n + 2.0 * np.abs(mf) * dmf, dS2 / n + 2.0 * np.abs(pm) * dpm
                dcov = dX / n + np.abs(mf) * dpm + np.abs(pm) * dmf
                mag = AX / n + np.abs(pm) * np.abs(mf)
                with np.errstate(divide="ignore", invalid="ignore"):
                    sig = np.sqrt(pv * vf)
                    drho = dcov / sig + np.abs(rho) * (dpv / (2.0 * pv) + dvf / (2.0 * vf))
                    brho = 2.0 * drho + C_FIN * E53 * mag / sig + C_FIN * E53 * np.abs(rho)
                    brho = np.where((dpv < 0.25 * pv) & (dvf < 0.25 * vf), brho, np.inf)
                out["bcov"][:, :, p, q, l] = 2.0 * dcov + C_FIN * E53 * mag
                out["brho"][:, :, p, q, l] = brho
                out["pvvf"][:, :, p, q, l] = pv * vf
    return out


def probe_stats(series, pairs, lags, T):
    """pm, pv [R, B, P, Q, L] fp64: the mean and the population variance of the probe's first n_l values, NaN for n_l < 1."""
    s = np.asarray(series, dtype=np.float64)
    R, B, _, P, _ = s.shape
    pm = np.full((R, B, P, len(pairs), len(lags)), np.nan)
    pv = pm.copy()
    for q, (ci, _cj) in enumerate(pairs):
        for l, tau in enumerate(lags):
            n = T - tau
            if n >= 1:
                v = s[:, :, :n, :, ci]
                pm[:, :, :, q, l] = v.sum(2) / n
                pv[:, :, :, q, l] = ((v - pm[:, :, None, :, q, l]) ** 2).sum(2) / n
    return pm, pv


def restate(raw, series, T, hw, probes, pairs, lags):
    """The finalize formulas in fp64 on a raw state and its series -> (cov, rho) [R, B, P, Q, L, H, W]; NaN for n_l < 2, whose planes
    are not read."""
    raw = np.asarray(raw)
    R, B = raw.shape[:2]
    P, Q, L, J = len(probes), len(pairs), len(lags), jset(pairs)
    offf, offg = P * Q * L, P * Q * L + len(J) * L
    pm, pv = probe_stats(series, pairs, lags, T)
    cov = np.full((R, B, P, Q, L) + tuple(hw), np.nan)
    rho = cov.copy()
    for l, tau in enumerate(lags):
        n = T - tau
        if n < 2:
            continue
        for q, (ci, cj) in enumerate(pairs):
            j = J.index(cj)
            F = raw[:, :, offf + j * L + l].astype(np.float64).reshape((R, B) + tuple(hw))
            G = raw[:, :, offg + j * L + l].astype(np.float64).reshape((R, B) + tuple(hw))
            mf = F / n
            vf = G / n - mf * mf
            for p in range(P):
                X = raw[:, :, (p * Q + q) * L + l].astype(np.float64).reshape((R, B) + tuple(hw))
                pmv, pvv = pm[:, :, p, q, l][..., None, None], pv[:, :, p, q, l][..., None, None]
                c = X / n - pmv * mf
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where((pvv > 0) & (vf > 0), c / np.sqrt(pvv * vf), np.nan)
                cov[:, :, p, q, l], rho[:, :, p, q, l] = c, r
    return cov, rho


def outputs_from_rows(cov, rho):
    """Per-row cov, rho [S + 1, B, P, Q, L, H, W] -> the dict of the published fields (fp64)."""
    return {"tp_cov_mean": cov[:-1].mean(0), "tp_cov_std": cov[:-1].std(0), "tp_rho_mean": rho[:-1].mean(0), "tp_rho_std": rho[:-1].std(0),
            "target_tp_cov": cov[-1], "target_tp_rho": rho[-1], "member_tp_rho": np.ascontiguousarray(np.moveaxis(rho[:-1], 0, 1))}


def lines_from_rows(rho, probes):
    """rho [S + 1, B, P, Q, L, H, W] -> (tp_line_x [B, S + 1, P, Q, L, W], tp_line_y [B, S + 1, P, Q, L, H])."""
    lx = np.stack([rho[:, :, p, :, :, h, :] for p, (h, w) in enumerate(probes)], axis=2)
    ly = np.stack([rho[:, :, p, :, :, :, w] for p, (h, w) in enumerate(probes)], axis=2)
    return np.moveaxis(lx, 0, 1), np.moveaxis(ly, 0, 1)


# ---- 3: the checks ----------------------------------------------------------------------------------------------------------------------
def _share(err, bound, what, nan_free=None):
    """err against bound, NaN on both sides at the same places (nan_free: places where either may be NaN: an infinite bound)."""
    en, bn = np.isnan(err), np.isnan(bound)
    if nan_free is not None:
        en, bn = en & ~nan_free, bn & ~nan_free
    assert np.array_equal(en, bn), "%s: NaN pattern" % what
    fin = np.isfinite(bound) & ~np.isnan(err)
    share = float(np.where(err[fin] > 0, err[fin] / np.maximum(bound[fin], 1e-300), 0.0).max()) if fin.any() else 0.0
    assert share <= 1.0, "%s: off by %.3g of its bound" % (what, share)
    return share


def check_same_raw(got, rows, probes, what):
    """The published fields `got` (numpy fp32) against the host restatement rows = (cov, rho) of the device's own state:
    |got - ref| <= 2^-24 |ref| + 2^-40 -> the worst share reached."""
    ref = outputs_from_rows(*rows)
    ref["tp_line_x"], ref["tp_line_y"] = lines_from_rows(rows[1], probes)
    worst = 0.0
    for name in FIELD_KEYS + ("tp_line_x", "tp_line_y") + (("member_tp_rho",) if "member_tp_rho" in got else ()):
        g, r = got[name].astype(np.float64), ref[name]
        assert got[name].dtype == F32 and g.shape == r.shape, (what, name, g.shape, r.shape)
        worst = max(worst, _share(np.abs(g - r), np.where(np.isnan(r), np.nan, U24 * np.abs(r) + SAME_RAW_ABS), "%s %s" % (what, name)))
    return worst


def check_definition(got, ref, S, what):
    """The published fields against the direct definition `ref` (definition()) inside the propagated bounds -> the worst share."""
    cov, rho, bcov, brho = ref["cov"], ref["rho"], ref["bcov"], ref["brho"]
    worst = 0.0
    loose = ~np.isfinite(brho) & ~np.isnan(brho)                             # an infinite bound: the device may give NaN there
    cw = (C_FIN + 4 * S) * E53

    def std_bound(v, b):
        r, big = v[:-1].std(0), np.abs(v[:-1]).max(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            dq = 2.0 * cw * big * big
            own = np.minimum(np.sqrt(dq), np.where(r > 0, dq / np.maximum(r, 1e-300), np.inf))
        return r, U24 * np.abs(r) + b[:-1].max(0) + cw * big + own

    for v, b, base in ((cov, bcov, "cov"), (rho, brho, "rho")):
        free = loose if base == "rho" else None
        mfree = None if free is None else free[:-1].any(0)
        g = got["tp_%s_mean" % base].astype(np.float64)
        r = v[:-1].mean(0)
        worst = max(worst, _share(np.abs(g - r), U24 * np.abs(r) + b[:-1].max(0) + cw * np.abs(v[:-1]).max(0), "%s tp_%s_mean" % (what, base), mfree))
        r, bs = std_bound(v, b)
        worst = max(worst, _share(np.abs(got["tp_%s_std" % base].astype(np.float64) - r), bs, "%s tp_%s_std" % (what, base), mfree))
        g = got["target_tp_%s" % base].astype(np.float64)
        worst = max(worst, _share(np.abs(g - v[-1]), U24 * np.abs(v[-1]) + b[-1], "%s target_tp_%s" % (what, base), None if free is None else free[-1]))
    if "member_tp_rho" in got:
        g = np.moveaxis(got["member_tp_rho"].astype(np.float64), 1, 0)
        worst = max(worst, _share(np.abs(g - rho[:-1]), U24 * np.abs(rho[:-1]) + brho[:-1], "%s member_tp_rho" % what, loose[:-1]))
    return worst


# ---- known answer: a frozen pattern ------------------------------------------------------------------------------------------------------
KAT_SHIFT, KAT_T, KAT_HW, KAT_PROBE, KAT_LAGS = 2, 8, (5, 24), (2, 3), (0, 1, 2, 4)


@functools.lru_cache(maxsize=None)
def frozen(S=3, B=2, seed=7):
    """A frozen random pattern of every row, convected by KAT_SHIFT pixels along W per step and cut from a wider array, so that there
    is no wrap: x(h, w, step) = pat(h, w + off - KAT_SHIFT step).  One untimed step first -> (xs [T + 1, S + 1, B, 3, H, W], m) fp32."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = KAT_HW
    steps = KAT_T + 1
    off = KAT_SHIFT * (steps - 1)
    pat = torch.randn(S + 1, B, 3, Hh, Ww + off, generator=g)
    xs = torch.stack([pat[..., off - KAT_SHIFT * t:off - KAT_SHIFT * t + Ww] for t in range(steps)])
    m = 0.2 * torch.randn(B, 3, Hh, Ww, generator=g)
    return np.ascontiguousarray(xs.numpy().astype(F32)), m.numpy().astype(F32)
