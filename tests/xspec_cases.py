"""Case tables and references of the ensemble spectral skill (tests/test_xspec_cpu.py, tests/test_xspec_gpu.py): synthetic fields
with a known coherence step, the fp64 statement of the raw shell sums (numpy fft2 of the windowed, centred fields, a shell map
computed here, the modal quantities written out from the definitions), a plain fp32 torch restatement of the matrix DFT (the
yardstick of the comparison, as _f32_E of tests/test_spectrum_gpu.py), the host formulas restated in numpy, the named mutations of
the reference and the comparison rule.  No device, no project code.

The rule, taken over from tests/test_spectrum_gpu.py::_check: an element of a raw sum may differ from fp64 by at most
max(1e-5 |ref| + 2e-6 Etot, 3 e32); e32: the largest error of the fp32 restatement on that output; Etot: the largest total of P_T
over the shells of any case and step."""
import math

import numpy as np
import torch

RAW_KEYS = ("xs_target_power", "xs_sum", "xs_mean_field", "xs_time_member", "xs_time_target", "xs_time_mean_field")
STEP_FORMS = ("spec_corr", "mean_field_corr", "err_spec", "mean_err_spec", "spread_spec", "spread_skill", "power_ratio", "rel_err")
DERIVED_KEYS = STEP_FORMS + tuple("time_" + n for n in STEP_FORMS) + (
    "time_member_corr", "time_corr_mean", "time_corr_std", "cutoff_k", "cutoff_len", "cutoff_k_mean", "cutoff_k_std", "xs_k")
MUTATIONS = ("noconj", "nohalf", "dsum", "bar_s1", "shift", "tcen")

MU = np.array([0.3, -0.2, 0.5], dtype=np.float32)
SD = np.array([1.7, 0.6, 2.5], dtype=np.float32)
U = np.array([[1.3, 0.7, 1.69], [0.8, 1.2, 0.64]], dtype=np.float32)

# (H, W, dx, dy): one tile; separate operands, fewer column tiles than waves; five column tiles, so a wave takes two; five row tiles;
# stretched shells; one tile stretched fourfold, which leaves shells empty (r = sqrt(16 p^2 + q^2) skips 15, 19 .. 23, ...)
SHAPES = [(16, 16, 1.0, 1.0), (16, 48, 0.05, 0.07), (32, 80, 0.05, 0.075), (80, 16, 0.05, 0.07), (64, 64, 1.0, 0.5), (16, 16, 1.0, 0.25)]
# (shape, S, B, T, window, u given, centred, t_start, channel-slice view of stride 4, shell k0 of the coherence step)
CASES = [
    (0, 1, 1, 2, "hann", False, True, 0, False, 3),
    (0, 3, 2, 3, None, True, False, 1, True, 4),
    (1, 5, 1, 2, "hann", True, True, 0, False, 4),
    (1, 3, 2, 3, None, False, True, 1, False, 3),
    (2, 3, 2, 2, "hann", True, True, 0, True, 6),
    (2, 5, 1, 2, None, False, False, 0, False, 5),
    (3, 3, 1, 3, "hann", False, True, 1, False, 4),
    (3, 1, 2, 2, None, True, True, 0, True, 3),
    (4, 5, 2, 2, "hann", True, True, 0, False, 8),
    (4, 3, 1, 2, None, False, False, 1, False, 6),
    (5, 3, 2, 2, "hann", True, True, 0, False, 6),
]


def signed(n):
    m = np.arange(n, dtype=np.float64)
    return np.where(m <= n // 2, m, m - n)


def bins(Hh, Ww, dx, dy):
    """(bins int64 [H, W], k [NK]) of the shell definition; asserts that no r sits within 1e-6 of a shell edge."""
    Lx, Ly = Ww * dx, Hh * dy
    Lmax = max(Lx, Ly)
    r = np.sqrt((signed(Hh)[:, None] * Lmax / Ly) ** 2 + (signed(Ww)[None, :] * Lmax / Lx) ** 2)
    assert float(np.abs(r + 0.5 - np.round(r + 0.5)).min()) > 1e-6
    b = np.floor(r + 0.5).astype(np.int64)
    return b, np.arange(b.max() + 1) * 2 * math.pi / Lmax


def hann(n):
    w = 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n, dtype=np.float64) / n)
    return w / np.sqrt(np.mean(w * w))


def window2(Hh, Ww, window):
    return hann(Hh)[:, None] * hann(Ww)[None, :] if window == "hann" else np.ones((Hh, Ww))


def synthetic(T, S, B, Hh, Ww, slope, seed, k0, grid=(1.0, 1.0)):
    """(members [T, S, B, 3, H, W], target [T, B, 3, H, W]) fp64: u, v of the target with random phases and amplitude
    ~ r^(-slope / 2 - 1 / 2), rms 0.3, plus a mean flow of 1 in u.  A member copies the target's modes on the shells below k0 of the
    grid's shell map and draws independent phases on the others, so that its coherence with the target steps from 1 to about 0 at
    shell k0.  The third channel is noise."""
    rng = np.random.default_rng(seed)
    r = np.sqrt(signed(Hh)[:, None] ** 2 + signed(Ww)[None, :] ** 2)
    amp = np.where(r > 0, np.maximum(r, 1.0) ** (-slope / 2 - 0.5), 0.0)
    low = bins(Hh, Ww, *grid)[0] < k0
    mem, tgt = np.empty((T, S, B, 3, Hh, Ww)), np.empty((T, B, 3, Hh, Ww))
    for c in (0, 1):
        at = amp * np.exp(1j * rng.uniform(0, 2 * math.pi, (T, B, Hh, Ww)))
        am = amp * np.exp(1j * rng.uniform(0, 2 * math.pi, (T, S, B, Hh, Ww)))
        am = np.where(low, at[:, None], am)
        xt, xm = np.fft.ifft2(at).real, np.fft.ifft2(am).real
        scale = 0.3 / np.sqrt((xt ** 2).mean(axis=(-2, -1), keepdims=True))
        tgt[:, :, c], mem[:, :, :, c] = scale * xt, scale[:, None] * xm
    tgt[:, :, 0] += 1.0
    mem[:, :, :, 0] += 1.0
    tgt[:, :, 2] = rng.standard_normal((T, B, Hh, Ww))
    mem[:, :, :, 2] = rng.standard_normal((T, S, B, Hh, Ww))
    return mem, tgt


def normalised(f, u):
    """The fp32 model-side array whose un-normalisation u[b, c] (sd y + mu) gives f [..., B, 3, H, W]."""
    y = f if u is None else f / u.astype(np.float64)[:, :, None, None]
    return ((y - MU.astype(np.float64)[:, None, None]) / SD.astype(np.float64)[:, None, None]).astype(np.float32)


def fields(y32, u, mu=MU, sd=SD):
    """(fp64, fp32) un-normalised velocity [..., B, 2, H, W] of the fp32 array y32 [..., B, C, H, W]: the fp64 statement and a plain
    fp32 form."""
    y = y32[..., :2, :, :]
    m, s = mu[:2, None, None], sd[:2, None, None]
    f64 = s.astype(np.float64) * y.astype(np.float64) + m.astype(np.float64)
    f32 = s * y + m
    if u is not None:
        f64 = f64 * u[:, :2, None, None].astype(np.float64)
        f32 = f32 * u[:, :2, None, None]
    return f64, f32.astype(np.float32)


def centre(ft64, t_start):
    """The target's time mean over the steps from t_start on, formed in fp64 and rounded once: ft64 [T, B, 2, H, W] -> fp32."""
    return ft64[t_start:].mean(0).astype(np.float32)


def make_case(idx):
    """-> dict of a case of CASES: the fp32 model-side members ym [T, S, B, 3, H, W] and target yt [T, B, 3, H, W], u, the centre
    plane cen (fp32 [B, 2, H, W] or None) and the case's parameters."""
    si, S, B, T, window, u_given, centred, t_start, padded, k0 = CASES[idx]
    Hh, Ww, dx, dy = SHAPES[si]
    u = U[:B] if u_given else None
    mem, tgt = synthetic(T, S, B, Hh, Ww, 5 / 3 if idx % 2 else 3.0, 300 + idx, k0, (dx, dy))
    ym, yt = normalised(mem, u), normalised(tgt, u)
    cen = centre(fields(yt, u)[0], t_start) if centred else None
    return dict(ym=ym, yt=yt, u=u, cen=cen, S=S, B=B, T=T, H=Hh, W=Ww, grid=(dx, dy), window=window, t_start=t_start, padded=padded, k0=k0)


# ---- the fp64 statement of the raw sums ----------------------------------------------------------------------------------------------
def _shell(a, b, NK):
    """a [..., H, W] -> its sums over the shells of the map b: [..., NK]."""
    flat = a.reshape(-1, b.size)
    out = np.stack([np.bincount(b.ravel(), weights=row, minlength=NK) for row in flat])
    return out.reshape(a.shape[:-2] + (NK,))


def modal(fm, ft, cen, window, mutate=None):
    """fm [T, S, B, 2, H, W], ft [T, B, 2, H, W] fp64 un-normalised, cen [B, 2, H, W] or None -> per mode (PT [T, B, H, W],
    member (P, X, D) [T, S, B, H, W] each, mean field (P, X, D) [T, B, H, W] each) in fp64."""
    Hh, Ww = fm.shape[-2:]
    S = fm.shape[1]
    g = window2(Hh, Ww, window)
    c = 0.0 if cen is None else cen.astype(np.float64)
    fmc, ftc = fm - c, ft - (0.0 if mutate == "tcen" else c)
    fb = fmc.sum(1) / (S - 1 if mutate == "bar_s1" else S)
    tr = lambda f: np.fft.fft2(g * (f[..., 0, :, :] + 1j * f[..., 1, :, :]))      # noqa: E731
    Zm, Zt, Zb = tr(fmc), tr(ftc), tr(fb)
    sc = (1.0 if mutate == "nohalf" else 0.5) / float(Hh * Ww) ** 2

    def pxd(Z, ZT):
        P, PT = sc * np.abs(Z) ** 2, sc * np.abs(ZT) ** 2
        X = sc * ((Z * ZT).real if mutate == "noconj" else (np.conj(Z) * ZT).real)
        D = P + PT + 2 * X if mutate == "dsum" else sc * np.abs(Z - ZT) ** 2
        return P, X, D
    return sc * np.abs(Zt) ** 2, pxd(Zm, Zt[:, None]), pxd(Zb, Zt)


def raw_sums(PT, mem, bar, b, NK, t_start):
    """Shell sums per mode -> the raw outputs in the layout of the device (fp64)."""
    sh = lambda a: _shell(a, b, NK)                                            # noqa: E731
    pt = sh(PT)                                                                # [T, B, NK]
    m = np.stack([sh(a) for a in mem], axis=3)                                 # [T, S, B, 3, NK]
    br = np.stack([sh(a) for a in bar], axis=2)                                # [T, B, 3, NK]
    return {"xs_target_power": pt.transpose(1, 0, 2), "xs_sum": m.sum(1).transpose(1, 0, 2, 3), "xs_mean_field": br.transpose(1, 0, 2, 3),
            "xs_time_member": m[t_start:].sum(0).transpose(1, 0, 2, 3), "xs_time_target": pt[t_start:].sum(0),
            "xs_time_mean_field": br[t_start:].sum(0)}


def reference(fm, ft, cen, grid, window, t_start, mutate=None):
    """The fp64 statement of the six raw outputs."""
    Hh, Ww = fm.shape[-2:]
    b, k = bins(Hh, Ww, *grid)
    if mutate == "shift":
        b = np.roll(b, 1, axis=1)
    PT, mem, bar = modal(fm, ft, cen, window, mutate)
    return raw_sums(PT, mem, bar, b, k.size, t_start)


# ---- the fp32 yardstick ---------------------------------------------------------------------------------------------------------------
def operand32(n, window):
    """fp64-built (re, im) of T[x][m] = w[x] exp(-2 pi i ((x m) mod n) / n), rounded once to fp32."""
    i = np.arange(n, dtype=np.int64)
    ang = ((i[:, None] * i[None, :]) % n).astype(np.float64) * (-2 * math.pi / n)
    w = hann(n) if window == "hann" else np.ones(n)
    return (torch.from_numpy((w[:, None] * np.cos(ang)).astype(np.float32)), torch.from_numpy((w[:, None] * np.sin(ang)).astype(np.float32)))


def f32_raw(fm32, ft32, cen, grid, window, t_start):
    """The raw outputs as a plain fp32 torch restatement of the matrix DFT (CPU matmul with the fp64-built operands rounded to fp32,
    index_add_ over the shell map, fp32 sums): fm32 [T, S, B, 2, H, W], ft32 [T, B, 2, H, W] fp32 -> dict of fp64 arrays."""
    Hh, Ww = fm32.shape[-2:]
    S = fm32.shape[1]
    b, k = bins(Hh, Ww, *grid)
    NK = k.size
    wr, wi = operand32(Ww, window)
    hr, hi = operand32(Hh, window)
    fm, ft = torch.from_numpy(fm32), torch.from_numpy(ft32)
    if cen is not None:
        fm, ft = fm - torch.from_numpy(cen), ft - torch.from_numpy(cen)
    fb = fm.sum(1) / torch.tensor(float(S))

    def tr(f):
        u, v = f[..., 0, :, :], f[..., 1, :, :]
        yr, yi = u @ wr - v @ wi, u @ wi + v @ wr
        return hr.T @ yr - hi.T @ yi, hr.T @ yi + hi.T @ yr
    sc = torch.tensor(0.5 / float(Hh * Ww) ** 2, dtype=torch.float32)
    bt = torch.from_numpy(b.ravel())

    def sh(a):
        flat = a.reshape(-1, Hh * Ww)
        out = torch.zeros(flat.shape[0], NK, dtype=torch.float32)
        out.index_add_(1, bt, flat)
        return out.reshape(tuple(a.shape[:-2]) + (NK,)).numpy()

    def pxd(z, t):
        (zr, zi), (tr_, ti) = z, t
        dr, di = zr - tr_, zi - ti
        return sh(sc * (zr * zr + zi * zi)), sh(sc * (zr * tr_ + zi * ti)), sh(sc * (dr * dr + di * di))
    zt = tr(ft)
    pt = sh(sc * (zt[0] * zt[0] + zt[1] * zt[1]))
    m = np.stack(pxd(tr(fm), (zt[0][:, None], zt[1][:, None])), axis=3)
    br = np.stack(pxd(tr(fb), zt), axis=2)
    f32sum = lambda a, ax: np.add.reduce(a.astype(np.float32), axis=ax, dtype=np.float32)     # noqa: E731
    out = {"xs_target_power": pt.transpose(1, 0, 2), "xs_sum": f32sum(m, 1).transpose(1, 0, 2, 3), "xs_mean_field": br.transpose(1, 0, 2, 3),
           "xs_time_member": f32sum(m[t_start:], 0).transpose(1, 0, 2, 3), "xs_time_target": f32sum(pt[t_start:], 0),
           "xs_time_mean_field": f32sum(br[t_start:], 0)}
    return {key: v.astype(np.float64) for key, v in out.items()}


def etot(ref):
    return float(ref["xs_target_power"].sum(-1).max())


def mismatches(got, ref, y32, report=None, keys=RAW_KEYS):
    """The raw outputs of `got` (those of `keys`) that break the rule against the fp64 `ref` with the yardstick y32 -> list of keys
    (missing, wrongly shaped or non-finite ones included)."""
    bad = [key for key in keys if key not in got]
    E = etot(ref)
    for key in keys:
        if key in bad:
            continue
        g, r = np.asarray(got[key], dtype=np.float64), ref[key]
        if g.shape != r.shape or not np.isfinite(g).all():
            bad.append(key)
            continue
        e32 = float(np.abs(y32[key] - r).max())
        err = np.abs(g - r)
        bound = np.maximum(1e-5 * np.abs(r) + 2e-6 * E, 3 * e32)
        if report is not None:
            i = int((err - bound).argmax())
            report("%s: max err %.3e (%.3e Etot), e32 %.3e Etot, tightest: err %.3e bound %.3e"
                   % (key, float(err.max()), float(err.max()) / E, e32 / E, float(err.ravel()[i]), float(bound.ravel()[i])))
        if not bool((err <= bound).all()):
            bad.append(key)
    return bad


# ---- the host formulas, restated ------------------------------------------------------------------------------------------------------
def _ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, 1.0), np.nan)


def _forms(P, X, D, Pb, Xb, Db, PT, S, pre):
    spread = D - Db
    arg = _ratio((S + 1.0) / S * spread, Db)
    with np.errstate(invalid="ignore"):
        ss = np.sqrt(np.where(arg >= 0, arg, np.nan))
    return {pre + "spec_corr": _ratio(X, np.sqrt(P * PT)), pre + "mean_field_corr": _ratio(Xb, np.sqrt(Pb * PT)), pre + "err_spec": D,
            pre + "mean_err_spec": Db, pre + "spread_spec": spread, pre + "spread_skill": ss, pre + "power_ratio": _ratio(P, PT),
            pre + "rel_err": _ratio(D, PT)}


def cutoff_shell(row, level):
    """(the finite shell before s*, s*) of one row of time correlations: s* the first shell >= 1 with a finite corr under level, None
    when there is none."""
    prev = None
    for s in range(1, len(row)):
        if not math.isfinite(row[s]):
            continue
        if row[s] < level:
            return prev, s
        prev = s
    return prev, None


def cutoff(corr, k, level):
    out = np.full(corr.shape[:-1], np.inf)
    for idx in np.ndindex(*corr.shape[:-1]):
        row = corr[idx]
        prev, s = cutoff_shell(row, level)
        if s is not None:
            out[idx] = k[s] if prev is None else k[prev] + (row[prev] - level) / (row[prev] - row[s]) * (k[s] - k[prev])
    return out


def derived(raw, S, k, level, Tn):
    """The derived outputs from raw sums (any float dtype, taken to fp64), written out from the definitions."""
    PT, sm, bar, tm, tT, tb = (np.asarray(raw[key], dtype=np.float64) for key in RAW_KEYS)
    o = _forms(sm[:, :, 0] / S, sm[:, :, 1] / S, sm[:, :, 2] / S, bar[:, :, 0], bar[:, :, 1], bar[:, :, 2], PT, S, "")
    ms = tm.sum(1)
    o.update(_forms(ms[:, 0] / S / Tn, ms[:, 1] / S / Tn, ms[:, 2] / S / Tn, tb[:, 0] / Tn, tb[:, 1] / Tn, tb[:, 2] / Tn, tT / Tn, S, "time_"))
    mc = _ratio(tm[:, :, 1], np.sqrt(tm[:, :, 0] * tT[:, None]))
    o["time_member_corr"], o["time_corr_mean"], o["time_corr_std"] = mc, mc.mean(1), mc.std(1)
    bc = _ratio(tb[:, 1], np.sqrt(tb[:, 0] * tT))
    cut = cutoff(np.concatenate((mc, bc[:, None]), axis=1), k, level)
    o["cutoff_k"] = cut
    with np.errstate(divide="ignore"):
        o["cutoff_len"] = 2 * math.pi / cut
    mean, std = np.full(cut.shape[0], np.nan), np.full(cut.shape[0], np.nan)
    for n in range(cut.shape[0]):
        v = cut[n, :S][np.isfinite(cut[n, :S])]
        if v.size:
            mean[n], std[n] = v.mean(), v.std()
    o["cutoff_k_mean"], o["cutoff_k_std"] = mean, std
    o["xs_k"] = np.asarray(k, dtype=np.float64)
    return o


def derived_mismatches(got, ref):
    """Keys of DERIVED_KEYS whose fp64 values differ by more than 2^-40 + 2^-50 |ref| (NaN and inf must sit in the same places)."""
    bad = []
    for key in DERIVED_KEYS:
        if key not in got:
            bad.append(key)
            continue
        g, r = np.asarray(got[key]), ref[key]
        if g.dtype != np.float64 or g.shape != r.shape:
            bad.append(key)
            continue
        same = (np.isnan(g) & np.isnan(r)) | (np.isinf(r) & (g == r))
        fin = np.isfinite(g) & np.isfinite(r)
        gf, rf = np.where(fin, g, 0.0), np.where(fin, r, 0.0)
        ok = same | (fin & (np.abs(gf - rf) <= 2.0 ** -40 + 2.0 ** -50 * np.abs(rf)))
        if not bool(ok.all()):
            bad.append(key)
    return bad
