"""Case tables, the integer and fp64 references and the counted rounding bound of the ensemble POD projection (csrc/tmg_pod.hip,
tmg_ops.EnsembleModes / pod_basis), shared by tests/test_modes_cpu.py (no device) and tests/test_modes_gpu.py.

Definitions (case b, kept step t; rows: the S raw normalised members and the normalised target; channels the Cg channels of the inner
product; the tables a [B, Cg], m [B, Cg, H, W], psi [B, K, Cg, H, W] as the kernel is handed them, fp32):
  d = a_c (x_c - m_c)                                   the REFERENCE forms d explicitly in fp64 (integer data: in int64)
  coef_raw[k] = sum_c sum_p d psi_k,  en_raw = sum_c sum_p d d      by direct einsum, never through the kernel's slicing
  coef = coef_raw / HW, fluct_energy = en_raw / HW; over the timed steps, in fp64 from the per-step outputs:
  time_mode_energy = mean_t coef^2, time_mode_mean = mean_t coef, time_coef_cov = mean_t (coef - mean)(coef - mean)^T,
  time_captured_frac = sum_k time_mode_energy / mean_t fluct_energy, time_resid_energy = mean_t fluct_energy - sum_k time_mode_energy,
  target_time_* the same of the target's row, mode_energy_ratio_mean / _std = mean / population std over the members of
  time_mode_energy / lam_k (lam: pod_basis' energies where the accumulator was given them, else target_time_mode_energy).

The bound (u = 2^-24).  The kernel forms d = fl(a fl(x - m)): two roundings, so its d is d (1 + e), |e| <= 2 u to first order.  It
then sums the HW Cg terms d psi_k in fp32 in P slices (P, SL and L = SL Cg from tmg_hip.ens_pod_plan): inside a slice four waves'
fmaf chains of L / 4 terms each, added in wave order (3 additions), then P - 1 additions in slice order.  However the terms are
grouped, a term takes part in at most L + P additions (L / 4 + 3 + P - 1 for a coefficient; the energy's lane chains are L / 16 long and
are joined by 3 + 3 additions: L / 16 + 6 + P - 1, below L + P since L >= 256), each of relative error u on a partial sum that is
at most sum |d| |psi|.  Hence
  cnt = L + P + C_ROUND,  C_ROUND = 6: the roundings of d (2 for a coefficient, 4 for d d in the energy), 1 for the host's division by
        HW (fp64, rounded to fp32 once), 1 for all second-order terms (cnt u < 1e-3)
  |coef_raw - ref| <= cnt u sum_c sum_p |d| |psi_k|,   |en_raw - ref| <= cnt u sum_c sum_p d d
and the same over HW for coef / fluct_energy.  Host-derived outputs are held to 2^-24 |ref| + 2^-40 against these formulas applied to
the device's own per-step outputs.  The bound is never fitted to what the kernel gives; the GPU tests print the share they reach."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
C_ROUND = 6
F32 = np.float32
T = 3
STEP_KEYS = ("coef", "fluct_energy", "target_coef", "target_fluct_energy")
TIME_KEYS = ("time_mode_energy", "time_mode_mean", "time_coef_cov", "time_captured_frac", "time_resid_energy")
DERIVED_KEYS = TIME_KEYS + tuple("target_" + k for k in TIME_KEYS) + ("mode_energy_ratio_mean", "mode_energy_ratio_std")

# ---- case tables: (S, B, C, channels, (H, W), K, t_start, chunking, padded) ------------------------------------------------------------
# H x W: 1x1, 5x7 (one ragged chunk), 16x16 (one slice exactly: P = 1 at its largest), 1x257 (one pixel over the slice boundary SL = 256
# of the plan: P = 2, the second slice holds one pixel; HW not a multiple of 4: the scalar loads of psi), 17x31 (three slices, ragged);
# S 1, 15, 16 (a full tile, the one-tile instance's last), 17 (one member alone in a second tile: the four-tile instance), 33, 70 (a
# second block of 64 members); K 1, 5, 16; B 1 and 3; channel sets that omit and reorder channels; chunking 0: one member per chunk,
# 1: uneven, 2: all; padded: the rows are channel slices of a wider NaN-filled NHWC buffer
HWS = {1: (1, 1), 35: (5, 7), 256: (16, 16), 257: (1, 257), 527: (17, 31)}
INT_TABLE = [
    (1, 1, 2, (0,), HWS[1], 1, 0, 2, False), (15, 3, 3, (0, 1), HWS[35], 5, 1, 1, True), (16, 1, 3, (0, 2), HWS[256], 16, 0, 0, False),
    (17, 3, 3, (0, 1, 2), HWS[527], 5, 1, 1, True), (33, 1, 4, (1, 3), HWS[257], 16, 0, 1, False), (33, 3, 2, (0, 1), HWS[256], 1, 1, 2, True),
    (17, 1, 3, (0, 1), HWS[257], 5, 0, 0, True), (1, 3, 4, (1, 3), HWS[527], 16, 0, 2, True), (15, 1, 2, (0,), HWS[527], 1, 1, 0, False),
    (16, 3, 3, (0, 2), HWS[35], 5, 0, 1, False), (33, 1, 3, (0, 1, 2), HWS[35], 16, 0, 2, False), (70, 1, 3, (2, 0), HWS[257], 5, 1, 2, True),
]
# two chunks per wave: a slice of 512 pixels needs HW > 32 * 256
LONG_CASE = (3, 1, 3, (0, 1), (91, 91), 2, 0, 2, False)
# the largest member count: 16 blocks of 64 members
MAX_CASE = (1024, 1, 2, (0, 1), (1, 5), 3, 0, 1, False)
REAL_TABLE = [  # (S, B, C, channels, (H, W), K, kind, with_u)
    (7, 3, 3, (0, 1), HWS[527], 3, "pod", True), (33, 1, 4, (1, 3), HWS[257], 16, "random", False), (17, 3, 3, (0, 1, 2), HWS[256], 5, "random", True),
    (70, 1, 2, (1, 0), HWS[527], 16, "random", True), (5, 3, 3, (0, 2), HWS[35], 2, "pod", False), (16, 1, 3, (0, 1), (40, 52), 3, "pod", True),
]
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


@functools.lru_cache(maxsize=None)
def int_inputs(S, B, Cc, channels, hw, K, seed, steps=T):
    """Integer data whose products and partial sums are exact in fp32 -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W], m [B, Cg, H, W],
    psi [B, K, Cg, H, W]) float32: x and m integers in -8..8, psi in -2..2, a = 1.  |d| <= 16, so a coefficient's terms are at most 32
    and the energy's at most 256 in magnitude: every sum of absolute values is asserted to stay under 2^24."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    Cg = len(channels)
    xs = torch.randint(-8, 9, (steps, S, B, Cc, Hh, Ww), generator=g)
    tgt = torch.randint(-8, 9, (steps, B, Cc, Hh, Ww), generator=g)
    m = torch.randint(-8, 9, (B, Cg, Hh, Ww), generator=g)
    psi = torch.randint(-2, 3, (B, K, Cg, Hh, Ww), generator=g)
    assert Hh * Ww * Cg * 256 < 2 ** 24
    return xs.float().numpy(), tgt.float().numpy(), m.float().numpy(), psi.float().numpy()


def wave_series(B, Tn, Cc, hw, seed, noise=1e-2):
    """A normalised series [B, Tn, C, H, W] fp64 of three travelling waves with well-separated amplitudes (3, 1, 0.3: three pairs of
    modes) plus small noise and a steady part."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    yy, xx = torch.meshgrid(torch.arange(Hh, dtype=torch.float64), torch.arange(Ww, dtype=torch.float64), indexing="ij")
    t = torch.arange(Tn, dtype=torch.float64).view(1, Tn, 1, 1, 1)
    ph = 2 * np.pi * torch.rand(B, 1, Cc, 1, 1, generator=g, dtype=torch.float64)
    s = 0.4 * torch.randn(B, 1, Cc, Hh, Ww, generator=g, dtype=torch.float64)
    for amp, kx, ky, om in ((3.0, 1, 0, 0.9), (1.0, 2, 1, 1.7), (0.3, 3, 2, 2.9)):
        s = s + amp * torch.sin(2 * np.pi * (kx * xx / max(Ww, 2) + ky * yy / max(Hh, 2)) - om * t + ph)
    return s + noise * torch.randn(B, Tn, Cc, Hh, Ww, generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, Cc, channels, hw, K, kind, with_u, seed, steps=4):
    """pod: the target is a wave series, the tables are pod_basis' of it (fp32), the members the target plus N(0, 0.5) noise and a
    bias; random: Gaussian members, target and tables.  -> (xs, tgt, m, psi float32, sd [C], u [B, C] or None)."""
    import tmg_ops as ops
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    Cg = len(channels)
    sd = torch.tensor(SD[:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=g)) if with_u else None
    if kind == "pod":
        series = wave_series(B, steps, Cc, hw, seed).float()
        a = (sd.double().view(1, Cc) * (u.double() if with_u else 1.0)).expand(B, Cc)
        m, psi, _, _, _ = ops.pod_basis(series, a, channels, K)
        tgt = series.permute(1, 0, 2, 3, 4)
        xs = tgt[:, None] + 0.2 + 0.5 * torch.randn(steps, S, B, Cc, Hh, Ww, generator=g)
    else:
        tgt = torch.randn(steps, B, Cc, Hh, Ww, generator=g) + 0.3
        xs = torch.randn(steps, S, B, Cc, Hh, Ww, generator=g) + 0.3
        m = 0.5 * torch.randn(B, Cg, Hh, Ww, generator=g)
        psi = torch.randn(B, K, Cg, Hh, Ww, generator=g)
    return (xs.numpy().astype(F32), tgt.numpy().astype(F32), m.numpy().astype(F32), psi.numpy().astype(F32), sd.numpy(),
            None if u is None else u.numpy())


def scales(sd, u, B, Cc, channels):
    """a [B, Cg]: u out_std in fp64 from the fp32 factors, rounded to fp32 once (what the kernel is handed), as fp64."""
    sd = np.ones(Cc, F32) if sd is None else np.asarray(sd, F32)[:Cc]
    a = np.broadcast_to(sd.astype(np.float64), (B, Cc)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, Cc)
    return a[:, list(channels)].astype(F32).astype(np.float64)


def reference(xs, tgt, a, m, psi, channels, integer=False):
    """The reference from explicitly formed d by direct einsum (integer: in int64, exact) -> dict of fp64 / int64 arrays: coef_raw
    [B, S, T, K], en_raw [B, S, T], tcoef_raw [B, T, K], ten_raw [B, T], and the sums of absolute values abs_coef, abs_tcoef (the
    energies are their own)."""
    dt = np.int64 if integer else np.float64
    ch = list(channels)
    x = np.asarray(xs)[:, :, :, ch].astype(dt)                               # [T, S, B, Cg, H, W]
    y = np.asarray(tgt)[:, :, ch].astype(dt)                                 # [T, B, Cg, H, W]
    mm, pp, aa = np.asarray(m).astype(dt), np.asarray(psi).astype(dt), np.asarray(a).astype(dt)
    d = aa[None, None, :, :, None, None] * (x - mm[None, None])
    dtg = aa[None, :, :, None, None] * (y - mm[None])
    return {"coef_raw": np.einsum("tsbchw,bkchw->bstk", d, pp), "en_raw": np.einsum("tsbchw,tsbchw->bst", d, d),
            "tcoef_raw": np.einsum("tbchw,bkchw->btk", dtg, pp), "ten_raw": np.einsum("tbchw,tbchw->bt", dtg, dtg),
            "abs_coef": np.einsum("tsbchw,bkchw->bstk", np.abs(d), np.abs(pp)),
            "abs_tcoef": np.einsum("tbchw,bkchw->btk", np.abs(dtg), np.abs(pp))}


def count(plan):
    return plan["L"] + plan["P"] + C_ROUND


def pairs(got, ref, plan, hw):
    """(name, device value, reference, bound) of the four per-step outputs, over HW."""
    n = float(hw[0] * hw[1])
    c = count(plan) * U24 / n
    return [("coef", got["coef"], ref["coef_raw"] / n, c * ref["abs_coef"]), ("fluct_energy", got["fluct_energy"], ref["en_raw"] / n, c * ref["en_raw"]),
            ("target_coef", got["target_coef"], ref["tcoef_raw"] / n, c * ref["abs_tcoef"]),
            ("target_fluct_energy", got["target_fluct_energy"], ref["ten_raw"] / n, c * ref["ten_raw"])]


def check_bound(got, ref, plan, hw, what, extra=None):
    """Every per-step output inside the counted bound (extra: {name: an uncertainty of the reference itself, added to the bound})
    -> the worst share of a bound that was reached."""
    worst = 0.0
    for name, g, r, b in pairs(got, ref, plan, hw):
        assert g.dtype == F32 and g.shape == r.shape, "%s %s: %s %s" % (what, name, g.dtype, g.shape)
        b = np.asarray(b, dtype=np.float64) + (0.0 if extra is None else extra[name])
        err = np.abs(g.astype(np.float64) - r)
        share = float(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0).max())
        assert not np.isnan(g).any() and share <= 1.0, "%s %s: worst error is %.3g of its bound" % (what, name, share)
        worst = max(worst, share)
    return worst


def check_integer(got, ref, hw, what):
    """Integer mode: the raw sums are the int64 reference bit for bit, and the outputs its quotient by HW rounded once."""
    n = float(hw[0] * hw[1])
    for raw, out, key in (("coef_raw", "coef", "coef_raw"), ("en_raw", "fluct_energy", "en_raw"), ("tcoef_raw", "target_coef", "tcoef_raw"),
                          ("ten_raw", "target_fluct_energy", "ten_raw")):
        r = ref[key]
        assert np.abs(r).max() < 2 ** 24 and ref["abs_coef"].max() < 2 ** 24 and ref["abs_tcoef"].max() < 2 ** 24
        assert got[raw].dtype == F32 and np.array_equal(got[raw], r.astype(F32)), "%s: %s is not the integer sum" % (what, raw)
        assert np.array_equal(got[out], (r.astype(np.float64) / n).astype(F32)), "%s: %s" % (what, out)


def time_stats(coef, en):
    """coef [.., T, K], en [.., T] fp64 over the timed steps -> the time aggregates (fp64), by the formulas of the module docstring."""
    mean = coef.mean(-2)
    dev = coef - mean[..., None, :]
    energy = (coef * coef).mean(-2)
    cov = np.einsum("...tk,...tl->...kl", dev, dev) / coef.shape[-2]
    fl = en.mean(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = energy.sum(-1) / fl
    return {"time_mode_energy": energy, "time_mode_mean": mean, "time_coef_cov": cov, "time_captured_frac": frac,
            "time_resid_energy": fl - energy.sum(-1)}


def derive(got, t_start, lam=None):
    """The host-derived outputs from the device's own per-step outputs, in fp64.  lam [B, K]: the energies the mode-energy ratio is
    taken against (None: the target's own time_mode_energy, EnsembleModes' default)."""
    f = lambda k: got[k].astype(np.float64)                                  # noqa: E731
    tm = time_stats(f("coef")[:, :, t_start:], f("fluct_energy")[:, :, t_start:])
    tt = time_stats(f("target_coef")[:, t_start:], f("target_fluct_energy")[:, t_start:])
    out = dict(tm)
    out.update({"target_" + k: v for k, v in tt.items()})
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = tm["time_mode_energy"] / (tt["time_mode_energy"] if lam is None else np.asarray(lam, dtype=np.float64))[:, None]
    out["mode_energy_ratio_mean"], out["mode_energy_ratio_std"] = ratio.mean(1), ratio.std(1)
    return out


def check_derived(got, t_start, what, lam=None):
    """Host-derived outputs within 2^-24 |ref| + 2^-40 of the formulas applied to the device's per-step outputs (a reference that
    is not finite, an energy of zero in a denominator, must be met by the same non-finite value)."""
    ref = derive(got, t_start, lam)
    for name in DERIVED_KEYS:
        g, r = got[name], ref[name]
        assert g.dtype == F32 and g.shape == r.shape, "%s %s: %s %s" % (what, name, g.dtype, g.shape)
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin), "%s %s" % (what, name)
        err = np.abs(g.astype(np.float64)[fin] - r[fin])
        assert bool((err <= U24 * np.abs(r[fin]) + 2.0 ** -40).all()), "%s %s: off by %.3g" % (what, name, float(err.max()))


def shapes(got, S, B, Tn, K):
    want = {"coef": (B, S, Tn, K), "fluct_energy": (B, S, Tn), "target_coef": (B, Tn, K), "target_fluct_energy": (B, Tn),
            "time_mode_energy": (B, S, K), "time_mode_mean": (B, S, K), "time_coef_cov": (B, S, K, K), "time_captured_frac": (B, S),
            "time_resid_energy": (B, S), "target_time_mode_energy": (B, K), "target_time_mode_mean": (B, K),
            "target_time_coef_cov": (B, K, K), "target_time_captured_frac": (B,), "target_time_resid_energy": (B,),
            "mode_energy_ratio_mean": (B, K), "mode_energy_ratio_std": (B, K)}
    for k, s in want.items():
        assert tuple(got[k].shape) == s, "%s: %s, not %s" % (k, tuple(got[k].shape), s)
