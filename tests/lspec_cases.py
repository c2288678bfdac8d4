"""What the line-spectrum tests share (tests/test_lspec_cpu.py, tests/test_lspec_gpu.py): the fp64 reference, its second statement, a
float32 mirror of the device arithmetic, synthetic fields and the comparison rule.  numpy and torch on the CPU only.

The reference (`reference`): np.fft.rfft along the line of the fp64 windowed field over N, the one-sided weight a_q (1 at q = 0 and
q = N/2, else 2), the planes (the C autospectra a_q |X_c|^2, then uv_co = a_q Re(X_0 conj X_1) and uv_quad = a_q Im(X_0 conj X_1)), a
TWO-PASS fluctuation (the time mean of the coefficients first, then the population moment of the differences) and two-pass mean /
population std over the members.  Fields are [T, S, B, C, H, W]; axis "x" transforms along W (lines = rows), "y" along H (lines =
columns); the timed steps are t_start .. T-1.

The rule (`compare`, the rule of tests/test_spectrum_gpu.py): every element of every output within max(1e-5 |ref| + 2e-6 P, 3 e32) of
the reference.  P: the largest line total of that output, the largest sum over q of |plane| over planes, lines, cases, steps and
members, taken, as that file's Etot is, on the member-level spectra the output is a mean or a population std of (a std over members
is formed from values of size P and inherits their rounding error, which is absolute in P, however small the std itself is).  e32:
the largest error against the reference of `mirror32`, a plain float32 torch restatement of the matrix DFT with the fp64-built
operand rounded to fp32 (CPU matmul) and of the Welford recurrences, per output.  Where it comes from: the fp32 matrix DFT of a line
is within about 1.5e-7 sum|a b| of fp64 (k-ordered fma chain, K <= 512), a plane is a product of two coefficients, so its error is
absolute in the line's power, some 1e-6 P at most; the relative arm covers the energetic modes, the e32 arm the outputs that are small
beside the power they are formed from (a std over members that nearly agree), where the restatement meets the same floor."""
import math

import numpy as np
import torch

MUTATIONS = ("nyquist2", "no_1_over_N", "window_rms", "ddof1", "quad_conj", "line_mean", "swap")
MEAN_KEYS = ("lspec_mean", "time_lspec_fluct_mean", "time_lspec_flow_mean")
STD_KEYS = ("lspec_std", "time_lspec_fluct_std", "time_lspec_flow_std")
KEYS = MEAN_KEYS + STD_KEYS + ("time_lspec_fluct_member",)
DERIVED = ("time_lspec_energy", "time_lspec_centroid", "time_lspec_coherence")


def fields(C):
    return tuple(("uu", "vv", "pp", "ss")[c] for c in range(C)) + ("uv_co", "uv_quad")


def hann(n, rms=True):
    w = 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n, dtype=np.float64) / n)
    return w / np.sqrt(np.mean(w * w)) if rms else w


def window(n, name, rms=True):
    return hann(n, rms) if name == "hann" else np.ones(n)


def lines(f, axis):
    """[..., H, W] -> [..., L, N]: the rows for axis "x", the columns for "y"."""
    return f if axis == "x" else np.swapaxes(f, -1, -2)


def weight(N, mutation=None):
    a = np.full(N // 2 + 1, 2.0)
    a[0] = 1.0
    a[-1] = 2.0 if mutation == "nyquist2" else 1.0
    return a


def planes(X, Y, a, mutation=None):
    """X, Y [..., C, L, NQ] complex -> [..., F, L, NQ]: a_q Re(X_c conj Y_c), then co and quad of (X_0, Y_1)."""
    auto = a * (X * np.conj(Y)).real
    cross = X[..., 0, :, :] * np.conj(Y[..., 1, :, :])
    if mutation == "quad_conj":
        cross = np.conj(X[..., 0, :, :]) * Y[..., 1, :, :]
    co, quad = a * cross.real, a * cross.imag
    if mutation == "swap":
        co, quad = quad, co
    return np.concatenate((auto, co[..., None, :, :], quad[..., None, :, :]), axis=-3)


def wavenumbers(N, d):
    return 2 * math.pi * np.arange(N // 2 + 1, dtype=np.float64) / (N * d)


def _stats(total, fluct, flow):
    """total [T, S, B, F, NQ], fluct / flow [S, B, F, L, NQ] -> the outputs, two-pass mean / population std over the members, and
    under "_P" the largest line total of every output's member-level spectra."""
    Pt, Pf, Pw = (float(np.abs(v).sum(-1).max()) for v in (total, fluct, flow))
    return {"_P": {"lspec_mean": Pt, "lspec_std": Pt, "time_lspec_fluct_mean": Pf, "time_lspec_fluct_std": Pf, "time_lspec_fluct_member": Pf,
                   "time_lspec_flow_mean": Pw, "time_lspec_flow_std": Pw},
            "lspec_mean": total.mean(1).transpose(1, 0, 2, 3), "lspec_std": total.std(1).transpose(1, 0, 2, 3),
            "time_lspec_fluct_mean": fluct.mean(0), "time_lspec_fluct_std": fluct.std(0),
            "time_lspec_flow_mean": flow.mean(0), "time_lspec_flow_std": flow.std(0),
            "time_lspec_fluct_member": fluct.transpose(1, 0, 2, 3, 4)}


def reference(f, axis="x", win="hann", t_start=0, mutation=None):
    """f [T, S, B, C, H, W] fp64 physical fields -> dict of the fp64 outputs (KEYS)."""
    z = lines(np.asarray(f, dtype=np.float64), axis)
    N = z.shape[-1]
    w = window(N, win, rms=mutation != "window_rms")
    a = weight(N, mutation)
    if mutation == "line_mean":
        z = z - z.mean(-1, keepdims=True)
    X = np.fft.rfft(w * z, axis=-1)
    if mutation != "no_1_over_N":
        X = X / N
    total = planes(X, X, a, mutation).mean(-2)                                  # the line average: [T, S, B, F, NQ]
    Xt = X[t_start:]
    Xbar = Xt.mean(0)
    D = Xt if mutation == "line_mean" else Xt - Xbar
    Tn = Xt.shape[0]
    fluct = planes(D, D, a, mutation).sum(0) / ((Tn - 1) if mutation == "ddof1" else Tn)
    return _stats(total, fluct, planes(Xbar, Xbar, a, mutation))


def reference_direct(f, axis="x", win="hann", t_start=0):
    """The second statement: the fluctuation is taken in physical space first (the field minus its time mean), every coefficient is
    the direct O(N^2) sum over the full circle of N modes, the two-sided products are folded by Hermitian symmetry (mode N - q onto
    q: its real part adds, its imaginary part subtracts)."""
    z = lines(np.asarray(f, dtype=np.float64), axis)
    N = z.shape[-1]
    n = np.arange(N)
    E = np.exp(-2j * math.pi * ((n[:, None] * n[None, :]) % N) / N)
    w = window(N, win)
    full = lambda v: (w * v) @ E / N                                            # noqa: E731  [..., L, N] -> [..., L, N modes]

    def fold(X, Y):
        two = planes(X, Y, np.ones(N))                                          # two-sided, weight 1
        nq = N // 2 + 1
        out = two[..., :nq].copy()
        mirror = two[..., N - 1:N // 2:-1]                                      # modes N-1 .. N/2+1 onto q = 1 .. N/2-1
        sign = np.ones(two.shape[-3])
        sign[-1] = -1.0                                                         # the quadrature plane is odd
        out[..., 1:N // 2] += sign[:, None, None] * mirror
        return out

    X = full(z)
    total = fold(X, X).mean(-2)
    zt = z[t_start:]
    D = full(zt - zt.mean(0))
    Xbar = full(zt.mean(0))
    return _stats(total, fold(D, D).mean(0), fold(Xbar, Xbar))


def parseval(f, axis="x", win="hann", t_start=0):
    """mean_n w[n]^2 var_t(yh_c[l, n]) [S, B, C, L]: what the autospectra of the fluctuation sum to over q."""
    z = lines(np.asarray(f, dtype=np.float64), axis)[t_start:]
    w = window(z.shape[-1], win)
    return (w * w * z.var(0)).mean(-1)


def derived(fluct, k, C):
    """The host-formed outputs in fp64 from the ensemble-mean fluctuation planes [B, F, L, NQ]: energy, centroid, coherence."""
    P = np.asarray(fluct, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        num, den = (P[:, :C, :, 1:] * k[1:]).sum(-1), P[:, :C, :, 1:].sum(-1)
        cen = np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)
        cden = P[:, 0] * P[:, 1]
        coh = np.where(cden != 0, (P[:, C] ** 2 + P[:, C + 1] ** 2) / np.where(cden != 0, cden, 1.0), np.nan)
    return {"time_lspec_energy": P.sum(-1), "time_lspec_centroid": cen, "time_lspec_coherence": coh}


def log_distance(ens, tgt, C):
    """[N, C, L]: the RMS over q = 1 .. NQ-1 of 10 log10(ens / tgt) of the autospectra, NaN where either is not positive."""
    a, b = np.asarray(ens, dtype=np.float64)[:, :C, :, 1:], np.asarray(tgt, dtype=np.float64)[:, :C, :, 1:]
    ok = ((a > 0) & (b > 0)).all(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 10 * np.log10(a / b)
        return np.where(ok, np.sqrt((r * r).mean(-1)), np.nan)


def operand64(N, win):
    """(re, im) [N, NQ] fp64 of (w[n] / N) exp(-2 pi i ((q n) mod N) / N): the statement the device operand is rounded from."""
    n, q = np.arange(N, dtype=np.int64), np.arange(N // 2 + 1, dtype=np.int64)
    ang = ((n[:, None] * q[None, :]) % N).astype(np.float64) * (-2 * math.pi / N)
    w = (window(N, win) / N)[:, None]
    return w * np.cos(ang), w * np.sin(ang)


def mirror32(f32, axis="x", win="hann", t_start=0):
    """The float32 restatement: f32 [T, S, B, C, H, W] float32 torch tensor (the physical field as the kernel forms it) -> dict of
    float64 numpy outputs.  X = z @ op by a CPU matmul, the members' running mean and co-moments by Welford over the timed steps, the
    step's statistics by a sequential Welford over the members, all in float32."""
    z = f32 if axis == "x" else f32.transpose(-1, -2)
    z = z.contiguous().float()
    T, S, B, C, L, N = z.shape
    cr, ci = operand64(N, win)
    opr, opi = torch.from_numpy(cr.astype(np.float32)), torch.from_numpy(ci.astype(np.float32))
    a = torch.from_numpy(weight(N).astype(np.float32))
    Xr, Xi = z @ opr, z @ opi                                                   # [T, S, B, C, L, NQ]

    def pl(ar, ai, br, bi):
        auto = ar * br + ai * bi
        co = ar[..., 0, :, :] * br[..., 1, :, :] + ai[..., 0, :, :] * bi[..., 1, :, :]
        quad = ai[..., 0, :, :] * br[..., 1, :, :] - ar[..., 0, :, :] * bi[..., 1, :, :]
        return torch.cat((auto, co.unsqueeze(-3), quad.unsqueeze(-3)), -3)

    def welford(v):                                                             # over dim 0, sequential
        m, q = torch.zeros_like(v[0]), torch.zeros_like(v[0])
        for i in range(v.shape[0]):
            d = v[i] - m
            m = m + d * torch.tensor(1.0 / (i + 1), dtype=torch.float32)
            q = q + d * (v[i] - m)
        return m, torch.sqrt(torch.clamp(q, min=0) * torch.tensor(1.0 / v.shape[0], dtype=torch.float32))

    total = a * pl(Xr, Xi, Xr, Xi).sum(-2) / torch.tensor(float(L), dtype=torch.float32)    # [T, S, B, F, NQ]
    tm, ts = welford(total.transpose(0, 1))                                     # over the members: [T, B, F, NQ]
    mr, mi = torch.zeros_like(Xr[0]), torch.zeros_like(Xi[0])
    M = torch.zeros((S, B, C + 2, L, N // 2 + 1), dtype=torch.float32)
    for j, t in enumerate(range(t_start, T)):
        rn = torch.tensor(1.0 / (j + 1), dtype=torch.float32)
        dor, doi = Xr[t] - mr, Xi[t] - mi
        mr, mi = mr + dor * rn, mi + doi * rn
        M = M + pl(dor, doi, Xr[t] - mr, Xi[t] - mi)
    fluct = a * M / torch.tensor(float(T - t_start), dtype=torch.float32)
    flow = a * pl(mr, mi, mr, mi)
    fm, fs = welford(fluct)
    wm, ws = welford(flow)
    out = {"lspec_mean": tm.transpose(0, 1), "lspec_std": ts.transpose(0, 1), "time_lspec_fluct_mean": fm, "time_lspec_fluct_std": fs,
           "time_lspec_flow_mean": wm, "time_lspec_flow_std": ws, "time_lspec_fluct_member": fluct.transpose(0, 1)}
    return {k: v.double().numpy() for k, v in out.items()}


def compare(got, ref, y32, what, keys=KEYS, report=print):
    """The rule of this module's docstring on the outputs `keys`; got: numpy / torch values, ref: the reference, y32: mirror32's
    outputs or None (then the e32 arm is absent).  Prints the achieved error beside the bound; -> list of the failures (strings)."""
    bad = []
    for name in keys:
        r = np.asarray(ref[name], dtype=np.float64)
        g = got[name]
        g = g.double().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g, dtype=np.float64)
        if g.shape != r.shape:
            bad.append("%s %s: shape %s, reference %s" % (what, name, g.shape, r.shape))
            continue
        P = ref["_P"][name]
        e32 = 0.0 if y32 is None else float(np.abs(np.asarray(y32[name]) - r).max())
        err = np.abs(g - r)
        bound = np.maximum(1e-5 * np.abs(r) + 2e-6 * P, 3 * e32)
        ok = np.isfinite(g) & (err <= bound)
        i = int(np.where(np.isfinite(err), err - bound, np.inf).argmax())
        report("%s %s: max err %.3e, P %.3e, e32 %.3e, worst element: err %.3e against bound %.3e" % (
            what, name, float(np.nanmax(err)) if err.size else 0.0, P, e32, float(err.ravel()[i]), float(bound.ravel()[i])))
        if not bool(ok.all()):
            bad.append("%s %s: %d of %d elements outside the bound, worst err %.3e against %.3e (P %.3e, e32 %.3e)" % (
                what, name, int((~ok).sum()), ok.size, float(err.ravel()[i]), float(bound.ravel()[i]), P, e32))
    return bad


def synthetic(T, S, B, C, Hh, Ww, seed, const_time=False):
    """[T, S, B, C, H, W] fp64: a mean flow that is neither periodic nor uniform (its power is about ten times the fluctuations')
    plus fluctuations with random phases and a power-law amplitude, rms 0.3; channel 1 holds a shifted, sign-flipped share of channel
    0's fluctuation, so that the co- and the quadrature spectrum are both far from 0.  const_time: every step repeats step 0."""
    rng = np.random.default_rng(seed)
    ky = np.fft.fftfreq(Hh) * Hh
    kx = np.fft.fftfreq(Ww) * Ww
    r = np.sqrt(ky[:, None] ** 2 + kx[None, :] ** 2)
    amp = np.where(r > 0, np.maximum(r, 1.0) ** (-4.0 / 3.0), 0.0)

    def noise():
        ph = rng.uniform(0, 2 * math.pi, (T, S, B, Hh, Ww))
        x = np.fft.ifft2(amp * np.exp(1j * ph)).real
        rms = np.sqrt((x ** 2).mean(axis=(-2, -1), keepdims=True))
        return 0.3 * x / np.where(rms > 0, rms, 1.0)

    yy = (np.arange(Hh)[:, None] + 0.5) / Hh
    xx = (np.arange(Ww)[None, :] + 0.5) / Ww
    mean = [1.0 + 0.5 * yy * (1.3 - yy) * 4 + 0.2 * xx, 0.1 - 0.3 * xx * yy, -0.5 + 0.6 * xx * xx - 0.2 * yy, 0.4 * yy - 0.1 * xx]
    f = np.empty((T, S, B, C, Hh, Ww))
    base = noise()
    for c in range(C):
        x = noise()
        if c == 0:
            x = base
        elif c == 1:
            x = 0.8 * x - 0.6 * np.roll(base, (1, 1), axis=(-2, -1))
        f[:, :, :, c] = mean[c] + x
    if const_time:
        f[:] = f[:1]
    return f
