"""Ensemble kinetic-energy spectra on the device (`-m gpu`): tmg_spec_rows / tmg_spec_cols / tmg_spec_accum / tmg_spec_finalize
through tmg_ops.EnsembleSpectrum and utils.modelPredSpectra against fp64 statements written here (numpy fft2 of the fp64
un-normalised, windowed field, bincount over a shell map computed here, two-pass mean / std).

Bound on every element of every output: |got - ref| <= max(1e-5 |ref| + 2e-6 Etot, 3 e32).  Etot: the largest fp64 total energy
(sum over the shells) of any member-step of the case.  e32: the largest error against fp64 of a plain fp32 torch restatement of the
same matrix DFT (CPU matmul with the fp64-built operands rounded to fp32, index_add_ over the shell map), measured per case and
output (the yardstick rule of DESIGN section 2).  The floor: that restatement is within 2e-7 Etot at these shapes and 5.4e-7 Etot at
256 x 256; its relative error is <= 4e-7 on the energetic shells and reaches 1e-3 only on shells that hold 1e-10 of the total, so the
error is absolute in Etot; the floor leaves 10x over the measurement for the matrix pipe's different summation order."""
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
KEYS = ("spec_mean", "spec_std", "time_spec_mean", "time_spec_std")


# ---- the fp64 statement and the fp32 yardstick ---------------------------------------------------------------------------------
def _signed(n):
    m = np.arange(n, dtype=np.float64)
    return np.where(m <= n // 2, m, m - n)


def _bins(Hh, Ww, dx, dy):
    """(bins int64 [H, W], k [NK]) of the issue's shell definition; asserts that no r sits within 1e-6 of a shell edge."""
    Lx, Ly = Ww * dx, Hh * dy
    Lmax = max(Lx, Ly)
    r = np.sqrt((_signed(Hh)[:, None] * Lmax / Ly) ** 2 + (_signed(Ww)[None, :] * Lmax / Lx) ** 2)
    assert float(np.abs(r + 0.5 - np.round(r + 0.5)).min()) > 1e-6
    bins = np.floor(r + 0.5).astype(np.int64)
    return bins, np.arange(bins.max() + 1) * 2 * math.pi / Lmax


def _hann(n, dtype=np.float64):
    w = 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n, dtype=np.float64) / n)
    return (w / np.sqrt(np.mean(w * w))).astype(dtype)


def _stats(E, t_start):
    """E [T, S, B, NK] fp64 -> the four outputs (two-pass mean / population std)."""
    tm = E[t_start:].mean(0)                                                   # [S, B, NK]
    return {"spec_mean": E.mean(1).transpose(1, 0, 2), "spec_std": E.std(1).transpose(1, 0, 2),
            "time_spec_mean": tm.mean(0), "time_spec_std": tm.std(0)}


def _ref_E(f, grid, window):
    """f [T, S, B, 2, H, W] fp64 un-normalised velocity -> E [T, S, B, NK] fp64 (numpy fft2, bincount)."""
    Hh, Ww = f.shape[-2:]
    bins, _ = _bins(Hh, Ww, *grid)
    NK = int(bins.max()) + 1
    g = (_hann(Hh)[:, None] * _hann(Ww)[None, :]) if window == "hann" else np.ones((Hh, Ww))
    z = g * (f[..., 0, :, :] + 1j * f[..., 1, :, :])
    E2 = 0.5 * np.abs(np.fft.fft2(z)) ** 2 / float(Hh * Ww) ** 2
    flat = E2.reshape(-1, Hh * Ww)
    E = np.stack([np.bincount(bins.ravel(), weights=row, minlength=NK) for row in flat])
    return E.reshape(f.shape[:3] + (NK,))


def _operand32(n, window):
    """fp64-built (re, im) of T[x][m] = w[x] exp(-2 pi i ((x m) mod n) / n), rounded once to fp32."""
    i = np.arange(n, dtype=np.int64)
    ang = ((i[:, None] * i[None, :]) % n).astype(np.float64) * (-2 * math.pi / n)
    w = _hann(n) if window == "hann" else np.ones(n)
    return (torch.from_numpy((w[:, None] * np.cos(ang)).astype(np.float32)), torch.from_numpy((w[:, None] * np.sin(ang)).astype(np.float32)))


def _f32_E(f32, grid, window):
    """The same spectra as a plain fp32 torch restatement of the matrix DFT: f32 [T, S, B, 2, H, W] fp32 (CPU) -> E [T, S, B, NK] fp32."""
    Hh, Ww = f32.shape[-2:]
    bins, _ = _bins(Hh, Ww, *grid)
    NK = int(bins.max()) + 1
    wr, wi = _operand32(Ww, window)
    hr, hi = _operand32(Hh, window)
    u, v = f32[..., 0, :, :], f32[..., 1, :, :]
    yr, yi = u @ wr - v @ wi, u @ wi + v @ wr                                  # rows: Y = z T_W
    zr, zi = hr.T @ yr - hi.T @ yi, hr.T @ yi + hi.T @ yr                      # columns: Z = T_H^T Y
    E2 = (torch.tensor(0.5 / float(Hh * Ww) ** 2, dtype=torch.float32) * (zr * zr + zi * zi)).reshape(-1, Hh * Ww)
    E = torch.zeros(E2.shape[0], NK, dtype=torch.float32)
    E.index_add_(1, torch.from_numpy(bins.ravel()), E2)
    return E.reshape(tuple(f32.shape[:3]) + (NK,))


def _check(got, f64, f32, grid, window, t_start, what):
    """got: the outputs under test; f64 / f32: the un-normalised fields [T, S, B, 2, H, W] in fp64 and in fp32 as the kernel forms them."""
    E = _ref_E(f64, grid, window)
    ref = _stats(E, t_start)
    y32 = _stats(_f32_E(f32, grid, window).double().numpy(), t_start)
    Etot = float(E.sum(-1).max())
    for name in KEYS:
        r = ref[name]
        gv = got[name].double().cpu().numpy()
        assert gv.shape == r.shape, (name, gv.shape, r.shape)
        assert np.isfinite(gv).all(), "%s %s: non-finite" % (what, name)
        e32 = float(np.abs(y32[name] - r).max())
        err = np.abs(gv - r)
        bound = np.maximum(1e-5 * np.abs(r) + 2e-6 * Etot, 3 * e32)
        i = int(err.argmax())
        print("%s %s: max err %.3e (%.3e Etot), e32 %.3e Etot, bound there %.3e" % (what, name, float(err.max()), float(err.max()) / Etot,
                                                                                    e32 / Etot, float(bound.ravel()[i])))
        assert bool((err <= bound).all()), "%s %s: max err %.3e = %.3e Etot, e32 %.3e Etot" % (what, name, float(err.max()),
                                                                                              float(err.max()) / Etot, e32 / Etot)


# ---- synthetic fields -------------------------------------------------------------------------------------------------------------
def _synthetic(T, S, B, Hh, Ww, slope, seed):
    """[T, S, B, 3, H, W] fp64: u, v with random phases and amplitude ~ r^(-slope / 2 - 1 / 2) (E(k) ~ k^-slope), rms 0.3, plus a mean
    flow of 1 in u; the third channel is noise (ignored by the spectra)."""
    rng = np.random.default_rng(seed)
    r = np.sqrt(_signed(Hh)[:, None] ** 2 + _signed(Ww)[None, :] ** 2)
    amp = np.where(r > 0, np.maximum(r, 1.0) ** (-slope / 2 - 0.5), 0.0)
    f = np.empty((T, S, B, 3, Hh, Ww))
    for c in (0, 1):
        ph = rng.uniform(0, 2 * math.pi, (T, S, B, Hh, Ww))
        x = np.fft.ifft2(amp * np.exp(1j * ph)).real
        f[:, :, :, c] = 0.3 * x / np.sqrt((x ** 2).mean(axis=(-2, -1), keepdims=True))
    f[:, :, :, 0] += 1.0
    f[:, :, :, 2] = rng.standard_normal((T, S, B, Hh, Ww))
    return f


MU = torch.tensor([0.3, -0.2, 0.5])
SD = torch.tensor([1.7, 0.6, 2.5])


def _normalised(f, u):
    """The model-side tensor whose un-normalisation u[b, c] (sd y + mu) gives f: [T, S, B, 3, H, W] fp32 on the device."""
    y = torch.from_numpy(f)
    if u is not None:
        y = y / u.double().view(1, 1, *u.shape, 1, 1)
    y = (y - MU.double().view(1, 1, 1, 3, 1, 1)) / SD.double().view(1, 1, 1, 3, 1, 1)
    return y.float().to(DEV)


def _fields(ys, u):
    """(fp64, fp32) un-normalised velocity of the fp32 tensor ys: the fp64 statement and the kernel's own fp32 form."""
    yc = ys[:, :, :, :2].cpu()
    mu, sd = MU[:2].view(1, 1, 1, 2, 1, 1), SD[:2].view(1, 1, 1, 2, 1, 1)
    f64 = sd.double() * yc.double() + mu.double()
    f32 = sd * yc + mu
    if u is not None:
        f64 = f64 * u[:, :2].double().reshape(1, 1, -1, 2, 1, 1)
        f32 = f32 * u[:, :2].reshape(1, 1, -1, 2, 1, 1)
    return f64.numpy(), f32


def _chunks(S, n):
    """n chunks of unequal size (as far as S allows) covering 0..S-1."""
    n = min(n, S)
    if n == 1:
        return [S]
    if n == 2:
        return [S - max(1, S // 3), max(1, S // 3)]
    return [1, S - 3, 2] if S >= 5 else [1, 1, S - 2]


def _run(ys, u, grid, window, t_start, nchunks, padded=False):
    import tmg_ops as ops
    T, S, B, Cc, Hh, Ww = ys.shape
    sp = ops.EnsembleSpectrum(S, B, Hh, Ww, T, DEV, MU, SD, u=None if u is None else u.to(DEV), grid=grid, window=window)
    sizes = _chunks(S, nchunks)
    assert sum(sizes) == S and len(sizes) == min(nchunks, S)
    for t in range(T):
        m0 = 0
        for k in sizes:
            y = ys[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww).permute(0, 2, 3, 1)         # NHWC [k*B, H, W, C]
            if padded:                                                                  # a channel slice of a wider NHWC buffer
                wide = torch.full((k * B, Hh, Ww, Cc + 3), float("nan"), device=DEV)
                wide[..., 1:1 + Cc] = y
                y = wide[..., 1:1 + Cc]
            else:
                y = y.contiguous()
            sp.add(y.permute(0, 3, 1, 2), m0, time=t >= t_start)
            m0 += k
    return sp.finalize()


# ---- 1. kernels against fp64 ----------------------------------------------------------------------------------------------------
# (H, W, dx, dy, B, S, T, window, chunks, u given, t_start, channel-padded input, slope)
CASES = [
    (16, 16, 0.05, 0.05, 2, 5, 3, "hann", 3, True, 1, False, 5 / 3),
    (16, 16, 0.05, 0.05, 2, 5, 3, None, 2, False, 0, False, 4),
    (16, 32, 0.05, 0.07, 2, 4, 3, "hann", 2, False, 0, True, 4),
    (16, 32, 0.05, 0.07, 1, 5, 2, None, 3, True, 1, False, 5 / 3),
    (32, 16, 0.05, 0.07, 2, 3, 3, "hann", 1, True, 0, False, 5 / 3),
    (32, 16, 0.05, 0.07, 1, 3, 2, None, 3, False, 1, False, 4),
    (48, 80, 0.05, 0.07, 1, 2, 2, "hann", 2, False, 1, False, 4),
    (48, 80, 0.05, 0.07, 1, 2, 2, None, 1, True, 0, False, 5 / 3),
]


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_spectrum_kernels_match_fp64(idx):
    Hh, Ww, dx, dy, B, S, T, window, nchunks, u_given, t_start, padded, slope = CASES[idx]
    u = torch.tensor([[1.3, 0.7, 1.69], [0.8, 1.2, 0.64]])[:B] if u_given else None
    ys = _normalised(_synthetic(T, S, B, Hh, Ww, slope, 100 + idx), u)
    got = _run(ys, u, (dx, dy), window, t_start, nchunks, padded)
    f64, f32 = _fields(ys, u)
    _check(got, f64, f32, (dx, dy), window, t_start, "case %d" % idx)
    _, k = _bins(Hh, Ww, dx, dy)
    assert got["spec_k"].dtype == torch.float64 and got["spec_k"].device.type == "cpu"
    np.testing.assert_allclose(got["spec_k"].numpy(), k, rtol=1e-15, atol=0)
    assert tuple(got["spec_mean"].shape) == (B, T, k.size) and tuple(got["time_spec_std"].shape) == (B, k.size)


# ---- 2. Parseval ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hh,Ww", [(16, 32), (48, 80)])
def test_shells_sum_to_the_kinetic_energy(Hh, Ww):
    B, T = 2, 2
    ys = _normalised(_synthetic(T, 1, B, Hh, Ww, 5 / 3, 7), None)
    got = _run(ys, None, (0.05, 0.07), None, 0, 1)
    f64, _ = _fields(ys, None)
    ke = 0.5 * (f64 ** 2).sum(3).mean((-2, -1))[:, 0].T                        # [B, T]
    tot = got["spec_mean"].double().sum(-1).cpu().numpy()
    np.testing.assert_allclose(tot, ke, rtol=1e-5, atol=0)


# ---- 3. zero spread -----------------------------------------------------------------------------------------------------------------
def test_identical_members_have_zero_spread():
    T, S, B, Hh, Ww = 3, 4, 2, 32, 16
    one = _normalised(_synthetic(T, 1, B, Hh, Ww, 4, 8), None)
    ys = one.expand(T, S, B, 3, Hh, Ww).contiguous()
    got = _run(ys, None, (0.05, 0.07), "hann", 1, 3)
    for name in ("spec_std", "time_spec_std"):
        assert not bool(torch.isnan(got[name]).any()), name
        assert bool((got[name] == 0).all()), name
    assert float(got["spec_mean"].min()) > 0


# ---- 4. run-to-run determinism --------------------------------------------------------------------------------------------------
def test_two_objects_give_the_same_bits():
    T, S, B, Hh, Ww = 2, 5, 2, 48, 80
    u = torch.tensor([[1.3, 0.7, 1.69], [0.8, 1.2, 0.64]])
    ys = _normalised(_synthetic(T, S, B, Hh, Ww, 5 / 3, 9), u)
    a = _run(ys, u, (0.05, 0.07), "hann", 0, 3)
    a = {k: v.clone() for k, v in a.items()}
    b = _run(ys, u, (0.05, 0.07), "hann", 0, 3)
    for name in KEYS + ("spec_k",):
        assert torch.equal(a[name], b[name]), name


# ---- 5. end to end: modelPredSpectra == modelPredTurbulence on the shared keys, fp64 over modelPred's samples on the new ones ------
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


def _cylinder_case(tmp_path):
    from utils.dataLoader import DataLoaderAuto
    C.write_synthetic_cylinder_data(str(tmp_path), cases=(0, 47, 95, 96, 97), seed=98, hw=(8, 8), up=4)
    kw = dict(in_features=3, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=4, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(21, kw)
    args = SimpleNamespace(exp_type='cylinder-array', ntrain=3, ntest=2, training_data_dir=str(tmp_path), testing_data_dir=str(tmp_path),
                           epoch_start=0, batch_size=2, test_batch_size=2, noise_std=0.0, seed=1)
    _, _, te = DataLoaderAuto.init_data_loaders(args, SimpleNamespace(module=model), LOG)
    return model, te


def _step_case(tmp_path):
    from utils.dataLoader import BackwardStepLoader
    C.write_synthetic_step_data(str(tmp_path), hw=(8, 8))
    kw = dict(in_features=4, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=2, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(22, kw)
    ld = BackwardStepLoader(str(tmp_path), str(tmp_path), shuffle=False, device=torch.device(DEV))
    te = ld.createTestingLoader([0, 1], C.LOADER_U0, inUpscale=1, batch_size=2)
    with torch.no_grad():
        model.in_mu.copy_(torch.tensor([0.1, -0.3, 0.2])); model.in_std.copy_(torch.tensor([1.2, 0.8, 1.5]))
        model.out_mu.copy_(torch.tensor([0.4, -0.1, 0.25])); model.out_std.copy_(torch.tensor([1.6, 0.7, 2.2]))
    return model, te


@pytest.mark.parametrize("case,window", [("cylinder", "hann"), ("step", None)])
def test_model_pred_spectra_end_to_end(monkeypatch, tmp_path, case, window):
    import tmg_ops as ops
    from utils import utils
    model, te = (_cylinder_case if case == "cylinder" else _step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    nkeep = tmax // stride
    grid = (0.05, 0.07)
    batches = [int(b[0].shape[0]) for b in te]
    kp = _KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=grid[0], dy=grid[1])
    for rep in range(2):                                                       # modelPredSpectra, then modelPredTurbulence
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
    got = utils.modelPredSpectra(args, model, te, LOG, window=window, **kw)
    torch.manual_seed(77)
    plain = utils.modelPredTurbulence(args, model, te, LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _inp = utils.modelPred(args, model, te, LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(plain) | set(KEYS) | {"spec_k", "target_spec", "target_time_spec"}
    for name in plain:
        assert torch.equal(got[name], plain[name]), name

    Hh, Ww = pred.shape[-2:]
    assert (Hh, Ww) == ((32, 32) if case == "cylinder" else (16, 16))
    _, k = _bins(Hh, Ww, *grid)
    np.testing.assert_allclose(got["spec_k"].numpy(), k, rtol=1e-15, atol=0)
    # the ensemble's spectra: the fp64 statement over modelPred's samples [S, N, Tk, C, H, W] -> [Tk, S, N, 2, H, W]
    f32 = pred[:, :, :, :2].permute(2, 0, 1, 3, 4, 5).contiguous()
    _check(got, f32.double().numpy(), f32, grid, window, t_start, case)
    assert float(got["spec_std"].abs().max()) > 0                              # the members are distinct samples
    # the target's spectra: modelPred's target at steps j * stride, j = t_start .. Tk - 1, as a one-member ensemble
    t32 = tgt[:, [j * stride for j in range(t_start, nkeep)], :2].permute(1, 0, 2, 3, 4).unsqueeze(1).contiguous()   # [Tw, 1, N, 2, H, W]
    tgot = {"spec_mean": got["target_spec"], "time_spec_mean": got["target_time_spec"],
            "spec_std": torch.zeros_like(got["target_spec"]), "time_spec_std": torch.zeros_like(got["target_time_spec"])}
    _check(tgot, t32.double().numpy(), t32, grid, window, 0, case + " target")
