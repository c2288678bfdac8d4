"""Ensemble temporal power spectra on the device (`-m gpu`): tmg_tspec_store / tmg_tspec_block / tmg_tspec_finalize through
tmg_ops.EnsembleTimeSpectrum and utils.modelPredTimeSpectra against an fp64 statement written here: numpy rfft of g (x - mean) on the
fp64 un-normalisation of the fp32 tensor, P_k = c_k |X_k|^2 / Tn^2, two-pass mean / population std over the members.

Bound on every element of every output: |got - ref| <= max(1e-5 |ref| + C_PRAW Praw, 3 e32).  Praw: the largest fp64
mean_n (g_n xh_n)^2 of any series of the case - the power INCLUDING the mean, because the subtraction A_k - xbar G_k makes the fp32
error absolute in it.  e32: the largest error against fp64 of a plain fp32 torch restatement of the same data flow (f32_psd: CPU
matmul of 16-step blocks with the fp64-built operand rounded to fp32, the fp32 sum for the mean, the same finalize), measured per case
and output (the yardstick rule of DESIGN section 2).  C_PRAW = 10 x the largest e32 / Praw that tests/test_tspec_cpu.py measures over
the case table below (CASES): measured 1.90e-8 Praw (case 7: Tn 5, no window; the Hann cases reach 1.87e-8), so C_PRAW = 1.9e-7.  The
pure-tone and Parseval inputs measure 1.96e-8 and 3.8e-8 Praw.  The margin is for the matrix pipe's summation order: one fmaf chain
over all steps started from the accumulator, where the restatement adds per-block sums.  Measured on an MI355X: the kernels' largest
error over CASES is 2.2e-8 Praw (case 2), between 0.8 and 1.4 times the restatement's per case."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LOG = SimpleNamespace(log=lambda *a, **k: None, warning=lambda *a, **k: None, error=lambda *a, **k: None)
KEYS = ("psd_mean", "psd_std")
C_PRAW = 1.9e-7
BLOCK = 16                       # steps per ring pass (csrc/tmg_tspec.hip)

MU = torch.tensor([0.3, -0.2, 0.5, 0.1])
SD = torch.tensor([1.7, 0.6, 2.5, 1.1])
U = torch.tensor([[1.3, 0.7, 1.69, 0.9], [0.8, 1.2, 0.64, 1.1]])


# ---- the fp64 statement and the fp32 yardstick ---------------------------------------------------------------------------------
def hann(n, periodic=True):
    w = 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n, dtype=np.float64) / (n if periodic else n - 1))
    return w / np.sqrt(np.mean(w * w))


def n_freq(Tn, nfreq):
    return min(nfreq, Tn // 2 + 1)


def ref_psd(x, nfreq, window, nyquist_c=1.0, remove_mean=True, periodic=True, shift=0):
    """x [Tn, S, B, C, H, W] fp64 -> P [S, B, NF, C, H, W] fp64: the issue's definition through numpy rfft.  The keyword arguments
    state WRONG definitions (test_tspec_cpu.py: the reference must tell them apart)."""
    Tn = x.shape[0]
    NF = n_freq(Tn, nfreq)
    g = hann(Tn, periodic) if window == "hann" else np.ones(Tn)
    g = np.roll(g, shift)                                                     # shift = 1: the window of n - 1
    d = g.reshape(-1, 1, 1, 1, 1, 1) * (x - (x.mean(0, keepdims=True) if remove_mean else 0.0))
    X = np.fft.rfft(d, axis=0)[:NF]
    ck = np.full(NF, 2.0)
    ck[0] = 1.0
    if Tn % 2 == 0 and NF > Tn // 2:
        ck[Tn // 2] = nyquist_c
    P = ck.reshape(-1, 1, 1, 1, 1, 1) * np.abs(X) ** 2 / float(Tn) ** 2
    return np.moveaxis(P, 0, 2)


def ref_stats(P):
    """P [S, B, NF, C, H, W] -> the two outputs (two-pass mean / population std over the members)."""
    return {"psd_mean": P.mean(0), "psd_std": P.std(0)}


def operand32(Tn, NF, window):
    """The constants of the blocked DFT as the issue states them, fp64 rounded once to fp32: tm [Tn, 2 NF + 1] (g cos, -g sin, ones),
    G [2, NF] (re, im of sum_n g_n exp(-2 pi i k n / Tn)), ck [NF] = c_k / Tn^2.  Also returns the fp64 originals."""
    g = hann(Tn) if window == "hann" else np.ones(Tn)
    n, k = np.arange(Tn, dtype=np.int64), np.arange(NF, dtype=np.int64)
    ang = ((n[:, None] * k[None, :]) % Tn).astype(np.float64) * (2 * math.pi / Tn)
    tm = np.concatenate([g[:, None] * np.cos(ang), -g[:, None] * np.sin(ang), np.ones((Tn, 1))], axis=1)
    G = np.stack([tm[:, :NF].sum(0), tm[:, NF:2 * NF].sum(0)])
    G[np.abs(G) < 1e-9 * Tn] = 0.0                                             # the sums that vanish analytically: no fp64 noise
    ck = np.full(NF, 2.0)
    ck[0] = 1.0
    if Tn % 2 == 0 and NF > Tn // 2:
        ck[Tn // 2] = 1.0
    ck = ck / float(Tn) ** 2
    f = lambda a: torch.from_numpy(a.astype(np.float32))                       # noqa: E731
    return (f(tm), f(G), f(ck)), (tm, G, ck)


def f32_psd(x32, nfreq, window):
    """The kernels' data flow as a plain fp32 torch restatement: x32 [Tn, S, B, C, H, W] fp32 (CPU) -> (psd_mean, psd_std) fp32
    [B, NF, C, H, W].  16-step blocks: acc (+)= tm[n0 : n0 + 16]^T ring; xbar from the fp32 sum row; Welford over the members."""
    Tn, S = x32.shape[:2]
    NF = n_freq(Tn, nfreq)
    (tm, G, ck), _ = operand32(Tn, NF, window)
    flat = x32.reshape(Tn, -1)
    acc = None
    for n0 in range(0, Tn, BLOCK):
        blk = tm[n0:n0 + BLOCK].t() @ flat[n0:n0 + BLOCK]
        acc = blk if acc is None else acc + blk
    acc = acc.reshape((2 * NF + 1,) + tuple(x32.shape[1:]))                    # [R, S, B, C, H, W]
    xbar = acc[2 * NF] * torch.tensor(1.0 / Tn, dtype=torch.float32)
    v = (1, NF, 1, 1, 1)
    mean = m2 = None
    for m in range(S):
        re = acc[:NF, m].transpose(0, 1) - xbar[m].unsqueeze(1) * G[0].view(v)  # [B, NF, C, H, W]
        im = acc[NF:2 * NF, m].transpose(0, 1) - xbar[m].unsqueeze(1) * G[1].view(v)
        P = ck.view(v) * (re * re + im * im)
        if m == 0:
            mean, m2 = P.clone(), torch.zeros_like(P)
        else:
            d = P - mean
            mean = mean + d * torch.tensor(1.0 / (m + 1), dtype=torch.float32)
            m2 = m2 + d * (P - mean)
    return {"psd_mean": mean, "psd_std": torch.sqrt(torch.clamp(m2, min=0) * torch.tensor(1.0 / S, dtype=torch.float32))}


def p_raw(x64, window):
    """The largest mean_n (g_n xh_n)^2 of any series."""
    g = hann(x64.shape[0]) if window == "hann" else np.ones(x64.shape[0])
    return float(((g.reshape(-1, 1, 1, 1, 1, 1) * x64) ** 2).mean(0).max())


def yardstick(x64, x32, nfreq, window, ref=None):
    """-> (ref outputs, {name: e32}, Praw): the fp64 statement, the fp32 restatement's largest error against it, the scale."""
    stated = ref_stats(ref_psd(x64, nfreq, window))
    y32 = f32_psd(x32, nfreq, window)
    e32 = {name: float(np.abs(y32[name].double().numpy() - stated[name]).max()) for name in KEYS}
    return (stated if ref is None else ref), e32, p_raw(x64, window)


def bound_of(r, e32, praw):
    return np.maximum(1e-5 * np.abs(r) + C_PRAW * praw, 3 * e32)


def check(got, x64, x32, nfreq, window, what, ref=None):
    """got: the outputs under test; x64 / x32: the un-normalised series [Tn, S, B, C, H, W] in fp64 and in fp32 as the kernel forms
    them; ref: expected outputs where they are not the fp64 statement of x64 (the analytic pure tone)."""
    ref, e32, praw = yardstick(x64, x32, nfreq, window, ref)
    for name in KEYS:
        r = ref[name]
        gv = got[name].double().cpu().numpy()
        assert gv.shape == r.shape, (name, gv.shape, r.shape)
        assert np.isfinite(gv).all(), "%s %s: non-finite" % (what, name)
        err = np.abs(gv - r)
        bound = bound_of(r, e32[name], praw)
        i = int(err.argmax())
        print("%s %s: max err %.3e (%.3e Praw), e32 %.3e Praw, bound there %.3e" % (what, name, float(err.max()), float(err.max()) / praw,
                                                                                    e32[name] / praw, float(bound.ravel()[i])))
        assert bool((err <= bound).all()), "%s %s: max err %.3e = %.3e Praw, e32 %.3e Praw" % (what, name, float(err.max()),
                                                                                              float(err.max()) / praw, e32[name] / praw)


# ---- synthetic series ---------------------------------------------------------------------------------------------------------------
def synthetic(Tn, S, B, Cc, Hh, Ww, seed, amp=0.3, noise=0.05):
    """[Tn, S, B, C, H, W] fp64: per member, case, channel and pixel a sinusoid of amplitude `amp` at a random non-integer frequency
    (in cycles per window) and phase plus white noise, on a mean of 1 in channel 0 and 0 elsewhere."""
    rng = np.random.default_rng(seed)
    shp = (S, B, Cc, Hh, Ww)
    f = rng.uniform(0.5, Tn / 2.0, shp)
    ph = rng.uniform(0, 2 * math.pi, shp)
    n = np.arange(Tn, dtype=np.float64).reshape(-1, 1, 1, 1, 1, 1)
    x = amp * np.cos(2 * math.pi * f * n / Tn + ph) + noise * rng.standard_normal((Tn,) + shp)
    x[:, :, :, 0] += 1.0
    return x


def normalised(f, u, dev=DEV):
    """The model-side tensor whose un-normalisation u[b, c] (sd y + mu) gives f: [Tn, S, B, C, H, W] fp32."""
    Cc = f.shape[3]
    y = torch.from_numpy(f)
    if u is not None:
        y = y / u.double().view(1, 1, u.shape[0], Cc, 1, 1)
    y = (y - MU[:Cc].double().view(1, 1, 1, Cc, 1, 1)) / SD[:Cc].double().view(1, 1, 1, Cc, 1, 1)
    return y.float().to(dev)


def fields(ys, u):
    """(fp64, fp32) un-normalised series of the fp32 tensor ys: the fp64 statement's input and the kernel's own fp32 form."""
    yc = ys.cpu()
    Cc = yc.shape[3]
    mu, sd = MU[:Cc].view(1, 1, 1, Cc, 1, 1), SD[:Cc].view(1, 1, 1, Cc, 1, 1)
    f64 = sd.double() * yc.double() + mu.double()
    f32 = sd * yc + mu
    if u is not None:
        f64 = f64 * u.double().view(1, 1, u.shape[0], Cc, 1, 1)
        f32 = f32 * u.view(1, 1, u.shape[0], Cc, 1, 1)
    return f64.numpy(), f32


def chunks(S, n):
    """n chunks of unequal size (as far as S allows) covering 0..S-1."""
    n = min(n, S)
    if n == 1:
        return [S]
    if n == 2:
        return [S - max(1, S // 3), max(1, S // 3)]
    return [1, S - 3, 2] if S >= 5 else [1, 1, S - 2]


def run(ys, u, nfreq, window, nchunks, padded=False, dt=1.0):
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = ys.shape
    ts = ops.EnsembleTimeSpectrum(S, B, Cc, Hh, Ww, Tn, DEV, MU[:Cc], SD[:Cc], u=None if u is None else u.to(DEV), nfreq=nfreq,
                                  window=window, dt=dt)
    sizes = chunks(S, nchunks)
    assert sum(sizes) == S and len(sizes) == min(nchunks, S)
    for t in range(Tn):
        m0 = 0
        for k in sizes:
            y = ys[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww).permute(0, 2, 3, 1)         # NHWC [k*B, H, W, C]
            if padded:                                                                  # a channel slice of a wider NHWC buffer
                wide = torch.full((k * B, Hh, Ww, Cc + 3), float("nan"), device=DEV)
                wide[..., 1:1 + Cc] = y
                y = wide[..., 1:1 + Cc]
            else:
                y = y.contiguous()
            ts.add(y.permute(0, 3, 1, 2), m0)
            m0 += k
    return ts.finalize()


# ---- 1. kernels against fp64 ----------------------------------------------------------------------------------------------------
# (Tn, nfreq, H, W, C, B, S, chunks, u given, window, channel-padded input)
#   Tn 5: a partial block only; 16: one exact block; 19: block + remainder; 35: two blocks + remainder
#   2 NF + 1 = 7 / 9 / 5 (< 16), 19 (NF 9: straddles a 16-row tile), 21, 37 (three row tiles); nfreq 32 / 10 capped at Tn // 2 + 1
#   Tn 16 with NF 9 keeps the Nyquist bin (c_k = 1)
CASES = [
    (5, 32, 5, 7, 3, 2, 3, 2, True, "hann", False),
    (16, 9, 12, 20, 2, 1, 5, 3, False, None, False),
    (19, 4, 16, 16, 4, 2, 1, 1, True, "hann", False),
    (35, 9, 5, 7, 3, 2, 5, 3, False, "hann", True),
    (35, 32, 12, 20, 3, 1, 3, 2, True, None, False),
    (16, 32, 5, 7, 4, 2, 3, 3, True, "hann", False),
    (19, 10, 12, 20, 2, 2, 5, 2, False, "hann", False),
    (5, 2, 16, 16, 3, 1, 1, 1, False, None, False),
]


def case_inputs(idx, dev=DEV):
    """-> (ys fp32 [Tn, S, B, C, H, W] on dev, u or None) of case idx."""
    Tn, nfreq, Hh, Ww, Cc, B, S, nchunks, u_given, window, padded = CASES[idx]
    u = U[:B, :Cc].contiguous() if u_given else None
    return normalised(synthetic(Tn, S, B, Cc, Hh, Ww, 300 + idx), u, dev), u


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_tspec_kernels_match_fp64(idx):
    Tn, nfreq, Hh, Ww, Cc, B, S, nchunks, u_given, window, padded = CASES[idx]
    ys, u = case_inputs(idx)
    got = run(ys, u, nfreq, window, nchunks, padded, dt=0.25)
    x64, x32 = fields(ys, u)
    check(got, x64, x32, nfreq, window, "case %d" % idx)
    NF = n_freq(Tn, nfreq)
    assert tuple(got["psd_mean"].shape) == tuple(got["psd_std"].shape) == (B, NF, Cc, Hh, Ww)
    assert got["psd_freq"].dtype == torch.float64 and got["psd_freq"].device.type == "cpu"
    np.testing.assert_allclose(got["psd_freq"].numpy(), np.arange(NF) / (Tn * 0.25), rtol=1e-15, atol=0)


# ---- 2. pure tone -----------------------------------------------------------------------------------------------------------------
TONE = (19, 3, 2, 3, 12, 20, 0.3)                      # Tn, S, B, C, H, W, a


def tone_inputs(dev=DEV):
    """x_n = 1 + a cos(2 pi k0 n / Tn + phi) with an integer k0 in 1 .. Tn // 2 and a phase per series -> (ys, u, analytic P)."""
    Tn, S, B, Cc, Hh, Ww, a = TONE
    rng = np.random.default_rng(11)
    shp = (S, B, Cc, Hh, Ww)
    k0 = rng.integers(1, Tn // 2 + 1, shp)
    ph = rng.uniform(0, 2 * math.pi, shp)
    n = np.arange(Tn, dtype=np.float64).reshape(-1, 1, 1, 1, 1, 1)
    x = 1.0 + a * np.cos(2 * math.pi * k0 * n / Tn + ph)
    P = np.zeros((S, B, Tn // 2 + 1, Cc, Hh, Ww))
    np.put_along_axis(P, np.expand_dims(k0, 2), a * a / 2, axis=2)
    u = U[:B, :Cc].contiguous()
    return normalised(x, u, dev), u, P


def test_pure_tone_lands_in_its_bin():
    Tn = TONE[0]
    ys, u, P = tone_inputs()
    got = run(ys, u, Tn // 2 + 1, None, 2)
    x64, x32 = fields(ys, u)
    check(got, x64, x32, Tn // 2 + 1, None, "tone", ref=ref_stats(P))


# ---- 3. Parseval ------------------------------------------------------------------------------------------------------------------
PARSEVAL = [(19, "hann"), (16, None)]


def parseval_inputs(Tn, dev=DEV):
    return normalised(synthetic(Tn, 1, 2, 3, 5, 7, 17), None, dev)


@pytest.mark.parametrize("Tn,window", PARSEVAL)
def test_bins_sum_to_the_fluctuation_power(Tn, window):
    ys = parseval_inputs(Tn)
    got = run(ys, None, Tn // 2 + 1, window, 1)
    x64, _ = fields(ys, None)
    g = (hann(Tn) if window == "hann" else np.ones(Tn)).reshape(-1, 1, 1, 1, 1, 1)
    power = ((g * (x64 - x64.mean(0, keepdims=True))) ** 2).mean(0)[0]         # [B, C, H, W]
    tot = got["psd_mean"].double().sum(1).cpu().numpy()
    np.testing.assert_allclose(tot, power, rtol=1e-5, atol=0)


# ---- 4. zero spread -----------------------------------------------------------------------------------------------------------------
def test_identical_members_have_zero_spread():
    Tn, S, B, Cc, Hh, Ww = 19, 5, 2, 3, 5, 7
    one = normalised(synthetic(Tn, 1, B, Cc, Hh, Ww, 8), None)
    ys = one.expand(Tn, S, B, Cc, Hh, Ww).contiguous()
    got = run(ys, None, 32, "hann", 3)
    assert not bool(torch.isnan(got["psd_std"]).any()) and not bool(torch.isnan(got["psd_mean"]).any())
    assert bool((got["psd_std"] == 0).all())
    assert float(got["psd_mean"].max()) > 0


# ---- 5. run-to-run determinism --------------------------------------------------------------------------------------------------
def test_two_objects_give_the_same_bits():
    Tn, S, B, Cc, Hh, Ww = 35, 5, 2, 3, 12, 20
    u = U[:B, :Cc].contiguous()
    ys = normalised(synthetic(Tn, S, B, Cc, Hh, Ww, 9), u)
    a = run(ys, u, 9, "hann", 3)
    a = {k: v.clone() for k, v in a.items()}
    b = run(ys, u, 9, "hann", 3)
    for name in KEYS + ("psd_freq",):
        assert torch.equal(a[name], b[name]), name


# ---- 6. end to end: modelPredTimeSpectra == modelPredStats on the shared keys, fp64 over modelPred's samples on the new ones ---------
def _model(seed, kw):
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    C.seed_all(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**kw)
    C.perturb_(m, 7, *C.perturb_scales(C.CFG_TINY3))
    return m.to(DEV).eval()


class _KeyPatch:
    """Deterministic latent keys: key(tag, t, m) for member m at step t; the folded runs' latent_nonces(k) calls and the serial
    run's latent_nonce calls are handed the keys in the order each run asks for them."""

    def __init__(self, monkeypatch, ops):
        self.fold, self.serial = [], []
        monkeypatch.setattr(ops, "latent_nonces", lambda device, k: self.fold.pop(0))
        monkeypatch.setattr(ops, "latent_nonce", lambda device: self.serial.pop(0))

    @staticmethod
    def key(tag, t, m):
        return torch.tensor([1000003 * t + 7919 * m + 104729 * tag + 17, -(65537 * m + 257 * t + 3 * tag + 5)], dtype=torch.int64)

    def queue_fold(self, tag, t, m0, k):
        self.fold.append(torch.stack([self.key(tag, t, m) for m in range(m0, m0 + k)]).to(DEV))

    def queue_serial(self, tag, t, m):
        self.serial.append(self.key(tag, t, m).to(DEV))


T_SERIES = 9                                           # steps of the synthetic simulation files


def _cylinder_case(tmp_path):
    from utils.dataLoader import DataLoaderAuto
    C.write_synthetic_cylinder_data(str(tmp_path), cases=(0, 47, 95, 96, 97), seed=98, T=T_SERIES, hw=(8, 8), up=4)
    kw = dict(in_features=3, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=4, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(21, kw)
    args = SimpleNamespace(exp_type='cylinder-array', ntrain=3, ntest=2, training_data_dir=str(tmp_path), testing_data_dir=str(tmp_path),
                           epoch_start=0, batch_size=2, test_batch_size=2, noise_std=0.0, seed=1)
    _, _, te = DataLoaderAuto.init_data_loaders(args, SimpleNamespace(module=model), LOG)
    return model, te


def _step_case(tmp_path):
    from utils.dataLoader import BackwardStepLoader
    C.write_synthetic_step_data(str(tmp_path), T=T_SERIES, hw=(8, 8))
    kw = dict(in_features=4, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=2, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(22, kw)
    ld = BackwardStepLoader(str(tmp_path), str(tmp_path), shuffle=False, device=torch.device(DEV))
    te = ld.createTestingLoader([0, 1], C.LOADER_U0, inUpscale=1, batch_size=2)
    with torch.no_grad():
        model.in_mu.copy_(torch.tensor([0.1, -0.3, 0.2])); model.in_std.copy_(torch.tensor([1.2, 0.8, 1.5]))
        model.out_mu.copy_(torch.tensor([0.4, -0.1, 0.25])); model.out_std.copy_(torch.tensor([1.6, 0.7, 2.2]))
    return model, te


@pytest.mark.parametrize("case,window,dt", [("cylinder", "hann", None), ("step", None, 0.05)])
def test_model_pred_time_spectra_end_to_end(monkeypatch, tmp_path, case, window, dt):
    import tmg_ops as ops
    from utils import utils
    model, te = (_cylinder_case if case == "cylinder" else _step_case)(tmp_path)
    steps = min(int(b[0].shape[1]) for b in te)                                # what the synthetic loader carries
    S, stride, t_start, max_rows, nfreq = 5, 2, 1, 4, 32
    tmax = steps - steps % stride
    nkeep = tmax // stride
    Tn = nkeep - t_start
    assert Tn >= 3, (steps, tmax, nkeep)
    batches = [int(b[0].shape[0]) for b in te]
    kp = _KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    for rep in range(2):                                                       # modelPredTimeSpectra, then modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
            assert per * B <= max_rows < S * B and len(range(0, S, per)) >= 2   # at least two chunks
    for bi, B in enumerate(batches):
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    kw = dict(samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    torch.manual_seed(77)
    got = utils.modelPredTimeSpectra(args, model, te, LOG, nfreq=nfreq, window=window, dt=dt, **kw)
    torch.manual_seed(77)
    plain = utils.modelPredStats(args, model, te, LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _inp = utils.modelPred(args, model, te, LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(plain) | set(KEYS) | {"psd_freq", "target_psd"}
    for name in plain:
        assert torch.equal(got[name], plain[name]), name

    NF = n_freq(Tn, nfreq)
    N = pred.shape[1]
    assert tuple(got["psd_mean"].shape) == tuple(got["target_psd"].shape) == (N, NF) + tuple(pred.shape[3:])
    step_dt = 1.0 if dt is None else stride * dt
    assert got["psd_freq"].dtype == torch.float64
    np.testing.assert_allclose(got["psd_freq"].numpy(), np.arange(NF) / (Tn * step_dt), rtol=1e-15, atol=0)
    # the ensemble: the fp64 statement over modelPred's samples [S, N, Tk, C, H, W] -> [Tn, S, N, C, H, W]
    x32 = pred[:, :, t_start:].permute(2, 0, 1, 3, 4, 5).contiguous()
    check(got, x32.double().numpy(), x32, nfreq, window, case)
    assert float(got["psd_std"].abs().max()) > 0                               # the members are distinct samples
    # the target: modelPred's target at steps j * stride, j = t_start .. Tk - 1, as a one-member ensemble
    t32 = tgt[:, [j * stride for j in range(t_start, nkeep)]].permute(1, 0, 2, 3, 4).unsqueeze(1).contiguous()   # [Tn, 1, N, C, H, W]
    tgot = {"psd_mean": got["target_psd"], "psd_std": torch.zeros_like(got["target_psd"])}
    check(tgot, t32.double().numpy(), t32, nfreq, window, case + " target")
