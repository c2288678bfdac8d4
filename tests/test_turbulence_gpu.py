"""Ensemble turbulence statistics on the device (`-m gpu`): tmg_ens_turb_accum / tmg_ens_turb_finalize through
tmg_ops.EnsembleStats(grid=(dx, dy)) and utils.modelPredTurbulence against fp64 torch statements written here (two-pass means,
unbiased=False, vorticity w = grad1x(v) - grad1y(u) through oracle.physics_oracle on the fp64 un-normalised field).

Bounds, element-wise over every element of every output: |got - ref| <= 4e-6 * scale + 1e-5 * |ref| with
  scale = ymax * (1 / dx + 1 / dy)   for the vorticity outputs (a 3x3 first-derivative stencil's weights sum to 1 in magnitude per
                                     axis, so ymax / dx + ymax / dy bounds the operands whose fp32 rounding enters w)
  scale = ymax * fl                  for <u'v'> and k (products of a fluctuation, itself a difference of values of size ymax, with a
                                     fluctuation of size fl)
where ymax is the largest |yh| and fl the largest fp64 time-RMS fluctuation of channels 0 and 1."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

import common as C
from oracle import physics_oracle as PO

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LOG = SimpleNamespace(log=lambda *a, **k: None, warning=lambda *a, **k: None, error=lambda *a, **k: None)
OLD_KEYS = ("mean", "std", "mag_mean", "mag_std", "time_mean_mean", "time_mean_std", "time_rms_mean", "time_rms_std")
VORT_KEYS = ("vort_mean", "vort_std", "time_vort_mean", "time_vort_std")
MOMENT_KEYS = ("time_uv_mean", "time_uv_std", "time_tke_mean", "time_tke_std")
DX, DY = 0.05, 0.08


@pytest.fixture(autouse=True)
def oracle_on_device(monkeypatch):
    """The oracle's first-derivative stencil moved to the GPU, so its fp64 convolutions run there."""
    monkeypatch.setattr(PO, "_G1", PO._G1.to(DEV))


def _chunks(S, n):
    """n chunks of unequal size (as far as S allows) covering 0..S-1."""
    n = min(n, S)
    if n == 1:
        return [S]
    if n == 2:
        a = max(1, (2 * S) // 3)
        return [a, S - a] if a < S else [S - 1, 1]
    a = max(1, S // 5)
    b = max(1, (S - a) // 2 + 1)
    if a + b >= S:
        a, b = 1, 1
    return [a, b, S - a - b]


def _vorticity(uv, dx, dy):
    """fp64 [..., 2, H, W] velocity -> [..., H, W] vorticity dv/dx - du/dy by the oracle's 3x3 stencils (zero padding)."""
    lead, (Hh, Ww) = uv.shape[:-3], uv.shape[-2:]
    f = uv.reshape(-1, 2, Hh, Ww)
    return (PO.grad1x(f[:, 1:2], dx) - PO.grad1y(f[:, 0:1], dy)).reshape(*lead, Hh, Ww)


def _time_moments(U, V, vort):
    """[T, ..] series of u, v, vorticity -> (<u'v'>, k, time-mean vorticity, largest RMS fluctuation), two-pass."""
    du, dv = U - U.mean(0), V - V.mean(0)
    uu, vv = (du * du).mean(0), (dv * dv).mean(0)
    return (du * dv).mean(0), 0.5 * (uu + vv), vort.mean(0), float(torch.sqrt(torch.maximum(uu.max(), vv.max())))


def _unnorm(ys, u, mu, sd):
    yh = ys.double() * sd.double().view(1, 1, 1, -1, 1, 1) + mu.double().view(1, 1, 1, -1, 1, 1)
    if u is not None:
        yh = yh * u.double().view(1, 1, *u.shape, 1, 1)
    return yh


def _ref_turb(ys, u, mu, sd, t_start, dx, dy):
    """fp64 statement: ys [T, S, B, C, H, W] raw model outputs -> the turbulence outputs of EnsembleStats, ymax and fl."""
    yh = _unnorm(ys, u, mu, sd)
    vort = torch.stack([_vorticity(yh[t, :, :, :2], dx, dy) for t in range(yh.shape[0])])     # [T, S, B, H, W]
    ref = {"vort_mean": vort.mean(1).permute(1, 0, 2, 3), "vort_std": vort.std(1, unbiased=False).permute(1, 0, 2, 3)}
    uv, tke, tv, fl = _time_moments(yh[t_start:, :, :, 0], yh[t_start:, :, :, 1], vort[t_start:])   # [S, B, H, W]
    for name, q in (("uv", uv), ("tke", tke), ("vort", tv)):
        ref["time_%s_mean" % name] = q.mean(0)
        ref["time_%s_std" % name] = q.std(0, unbiased=False)
    return ref, float(yh.abs().max()), fl


def _run_stats(ys, u, mu, sd, t_start, nchunks, padded, grid):
    import tmg_ops as ops
    T, S, B, Cc, Hh, Ww = ys.shape
    st = ops.EnsembleStats(S, B, Cc, Hh, Ww, T, DEV, mu, sd, u=u, grid=grid)
    sizes = _chunks(S, nchunks)
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
            st.add(y.permute(0, 3, 1, 2), m0, time=t >= t_start)
            m0 += k
    return st.finalize()


def _scales(ymax, fl, dx, dy):
    s = {k: ymax * (1.0 / dx + 1.0 / dy) for k in VORT_KEYS}
    s.update({k: ymax * fl for k in MOMENT_KEYS})
    return s


def _check(got, ref, scales, what):
    assert set(ref) == set(VORT_KEYS) | set(MOMENT_KEYS)
    for name, r in ref.items():
        gv = got[name].double().to(r.device)
        assert gv.shape == r.shape, (name, gv.shape, r.shape)
        assert bool(torch.isfinite(gv).all()), "%s %s: non-finite" % (what, name)
        err = (gv - r).abs()
        bound = 4e-6 * scales[name] + 1e-5 * r.abs()
        i = int((err - bound).argmax())
        print("%s %s: max err %.3e, worst element err %.3e bound %.3e" % (what, name, float(err.max()), float(err.flatten()[i]),
                                                                          float(bound.flatten()[i])))
        assert bool((err <= bound).all()), "%s %s: err %.3e, bound at that element %.3e" % (
            what, name, float(err.flatten()[i]), float(bound.flatten()[i]))


# the sweep of the ensemble statistics tests plus a field whose sides are multiples of no tile or wave size
SWEEP = [(S, B, Cc, hw) for S in (1, 2, 7, 33) for B in (1, 3) for Cc in (3, 4) for hw in ((5, 7), (256, 256))]
SWEEP += [(33, 1, 4, (66, 130)), (7, 3, 3, (66, 130)), (2, 3, 4, (66, 130)), (1, 1, 3, (66, 130))]
T_SWEEP = 12


def _features(idx):
    """(u given, t_start, channel-padded input, chunk count) of sweep entry idx, mixed so that every field size and member count
    >= 3 meets each value of each feature."""
    hw, c, b = idx % 2, (idx // 2) % 2, (idx // 4) % 2
    return (hw ^ c) == 0, c ^ b, (hw ^ b) == 1, 1 + (idx + idx // 8) % 3


def _sweep_case(idx):
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    g = torch.Generator(device=DEV).manual_seed(2000 + idx)
    ys = torch.randn(T_SWEEP, S, B, Cc, Hh, Ww, device=DEV, generator=g) * 0.8 + 0.1
    mu = torch.tensor([0.3, -0.2, 0.5, 1.0][:Cc], device=DEV)
    sd = torch.tensor([1.7, 0.6, 2.5, 0.9][:Cc], device=DEV)
    u_given, t_start, padded, nchunks = _features(idx)
    u = (0.5 + torch.rand(B, Cc, device=DEV, generator=g)) if u_given else None
    return ys, u, mu, sd, t_start, nchunks, padded


# ---- 1. sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(SWEEP)))
def test_turbulence_kernels_match_fp64(idx):
    """Every member count, case count, channel count and field size; 12 steps; the features rotate over the sweep: members fed in
    1 / 2 / 3 chunks of unequal size, u given or absent, a channel-padded NHWC input with NaN in the padding, t_start = 0 or 1;
    dx != dy."""
    ys, u, mu, sd, t_start, nchunks, padded = _sweep_case(idx)
    got = _run_stats(ys, u, mu, sd, t_start, nchunks, padded, (DX, DY))
    ref, ymax, fl = _ref_turb(ys, u, mu, sd, t_start, DX, DY)
    _check(got, ref, _scales(ymax, fl, DX, DY), "sweep %s" % (SWEEP[idx],))


# ---- 2. the existing outputs do not depend on grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [13, 26, 33])
def test_existing_outputs_are_bitwise_unchanged_by_grid(idx):
    ys, u, mu, sd, t_start, nchunks, padded = _sweep_case(idx)
    plain = _run_stats(ys, u, mu, sd, t_start, nchunks, padded, None)
    turb = _run_stats(ys, u, mu, sd, t_start, nchunks, padded, (DX, DY))
    assert set(plain) == set(OLD_KEYS)
    assert set(turb) == set(OLD_KEYS) | set(VORT_KEYS) | set(MOMENT_KEYS)
    for name in OLD_KEYS:
        assert torch.equal(plain[name], turb[name]), name


# ---- 3. analytic fields -----------------------------------------------------------------------------------------------------------
def test_solid_body_rotation_has_vorticity_2w0():
    """u = -W0 y, v = W0 x times a per-step factor, every member the same: vort_mean = 2 W0 factor on the interior, no spread."""
    S, B, Cc, Hh, Ww, T, W0 = 7, 2, 3, 40, 72, 5, 0.75
    x = (torch.arange(Ww, device=DEV, dtype=torch.float64) * DX).view(1, Ww).expand(Hh, Ww)
    yy = (torch.arange(Hh, device=DEV, dtype=torch.float64) * DY).view(Hh, 1).expand(Hh, Ww)
    factor = torch.tensor([1.0, 0.5, -1.25, 2.0, 0.3], device=DEV, dtype=torch.float64)
    field = torch.zeros(T, 1, 1, Cc, Hh, Ww, device=DEV, dtype=torch.float64)
    field[:, 0, 0, 0] = -W0 * yy * factor.view(T, 1, 1)
    field[:, 0, 0, 1] = W0 * x * factor.view(T, 1, 1)
    ys = field.float().expand(T, S, B, Cc, Hh, Ww).contiguous()
    one, zero = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    got = _run_stats(ys, None, zero, one, 0, 3, False, (DX, DY))
    ymax = float(ys.abs().max())
    inner = got["vort_mean"][:, :, 1:-1, 1:-1].double()
    ref = (2 * W0 * factor).view(1, T, 1, 1).expand_as(inner)
    err = (inner - ref).abs()
    bound = 4e-6 * ymax * (1 / DX + 1 / DY) + 1e-5 * ref.abs()
    print("rotation: max err %.3e, smallest bound %.3e" % (float(err.max()), float(bound.min())))
    assert bool((err <= bound).all()), "max err %.3e" % float(err.max())
    for name in ("vort_std", "time_vort_std", "time_uv_std", "time_tke_std"):
        assert not bool(torch.isnan(got[name]).any()), name
        assert bool((got[name] == 0).all()), name


def test_constant_in_time_members_have_zero_moments():
    S, B, Cc, Hh, Ww, T = 7, 3, 3, 16, 20, 6
    g = torch.Generator(device=DEV).manual_seed(3)
    one = torch.randn(1, S, B, Cc, Hh, Ww, device=DEV, generator=g) * 3.0
    ys = one.expand(T, S, B, Cc, Hh, Ww).contiguous()
    got = _run_stats(ys, torch.full((B, Cc), 1.3, device=DEV), torch.zeros(Cc, device=DEV) + 0.1, torch.ones(Cc, device=DEV) * 1.1, 1, 2,
                     False, (DX, DY))
    for name in MOMENT_KEYS:
        assert not bool(torch.isnan(got[name]).any()), name
        assert bool((got[name] == 0).all()), name
    assert float(got["vort_std"].abs().max()) > 0                              # the members differ from each other


def test_identical_members_have_zero_spread():
    S, B, Cc, Hh, Ww, T = 7, 3, 4, 16, 20, 5
    g = torch.Generator(device=DEV).manual_seed(5)
    one = torch.randn(T, 1, B, Cc, Hh, Ww, device=DEV, generator=g) * 3.0
    ys = one.expand(T, S, B, Cc, Hh, Ww).contiguous()
    got = _run_stats(ys, torch.full((B, Cc), 1.3, device=DEV), torch.zeros(Cc, device=DEV) + 0.1, torch.ones(Cc, device=DEV) * 1.1, 0, 3,
                     True, (DX, DY))
    for name, v in got.items():
        assert not bool(torch.isnan(v).any()), name
        if name.endswith("_std"):
            assert bool((v == 0).all()), name
    assert float(got["time_tke_mean"].abs().max()) > 0 and float(got["time_uv_mean"].abs().max()) > 0


# ---- 4. large offset --------------------------------------------------------------------------------------------------------------
def test_large_offset_field_stays_in_bound():
    """1e3 + 1e-2 N(0, 1): the bound on <u'v'> and k (about 1e-4) is as large as the values, so the field averages of time_tke_mean and
    time_uv_std must also be within 10 % of fp64 (a naive fp32 E[uv] - E[u] E[v] returns noise of order 1e-1 here)."""
    S, B, Cc, Hh, Ww, T = 33, 3, 4, 64, 64, 4
    g = torch.Generator(device=DEV).manual_seed(4)
    ys = 1e3 + 1e-2 * torch.randn(T, S, B, Cc, Hh, Ww, device=DEV, generator=g)
    one, zero = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    got = _run_stats(ys, None, zero, one, 1, 3, True, (DX, DY))
    ref, ymax, fl = _ref_turb(ys, None, zero, one, 1, DX, DY)
    _check(got, ref, _scales(ymax, fl, DX, DY), "offset field")
    for name in ("time_tke_mean", "time_uv_std"):
        a, r = float(got[name].double().mean()), float(ref[name].mean())
        print("offset field %s: field average %.6e, fp64 %.6e" % (name, a, r))
        assert abs(a - r) <= 0.1 * abs(r), (name, a, r)


# ---- 6. run to run ----------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    ys, u, mu, sd, t_start, nchunks, padded = _sweep_case(27)
    a = _run_stats(ys, u, mu, sd, t_start, nchunks, padded, (DX, DY))
    a = {k: v.clone() for k, v in a.items()}
    b = _run_stats(ys, u, mu, sd, t_start, nchunks, padded, (DX, DY))
    assert set(a) == set(b)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ---- 5. end to end: modelPredTurbulence == modelPredStats on the shared keys, fp64 over modelPred's samples on the new ones -------
def _model(cfg, seed=12345, kw=None):
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    C.seed_all(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**(kw or C.build_kwargs(cfg)))
    C.perturb_(m, 7, *C.perturb_scales(cfg))
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
    model = _model(C.CFG_TINY3, seed=21, kw=kw)
    args = SimpleNamespace(exp_type='cylinder-array', ntrain=3, ntest=2, training_data_dir=str(tmp_path), testing_data_dir=str(tmp_path),
                           epoch_start=0, batch_size=2, test_batch_size=2, noise_std=0.0, seed=1)
    _, _, te = DataLoaderAuto.init_data_loaders(args, SimpleNamespace(module=model), LOG)
    return model, te


def _step_case(tmp_path):
    from utils.dataLoader import BackwardStepLoader
    C.write_synthetic_step_data(str(tmp_path), hw=(8, 8))
    kw = dict(in_features=4, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=2, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(C.CFG_TINY3, seed=22, kw=kw)
    ld = BackwardStepLoader(str(tmp_path), str(tmp_path), shuffle=False, device=torch.device(DEV))
    te = ld.createTestingLoader([0, 1], C.LOADER_U0, inUpscale=1, batch_size=2)
    with torch.no_grad():
        model.in_mu.copy_(torch.tensor([0.1, -0.3, 0.2])); model.in_std.copy_(torch.tensor([1.2, 0.8, 1.5]))
        model.out_mu.copy_(torch.tensor([0.4, -0.1, 0.25])); model.out_std.copy_(torch.tensor([1.6, 0.7, 2.2]))
    return model, te


@pytest.mark.parametrize("stride,t_start", [(1, 0), (1, 2), (2, 0), (2, 2)])
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_turbulence_end_to_end(monkeypatch, tmp_path, case, stride, t_start):
    import tmg_ops as ops
    from utils import utils
    model, te = (_cylinder_case if case == "cylinder" else _step_case)(tmp_path)
    S, tmax, max_rows = 5, 6, 4
    nkeep = tmax // stride
    batches = [int(b[0].shape[0]) for b in te]
    kp = _KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=DX, dy=DY)
    for rep in range(2):                                                       # modelPredTurbulence, then modelPredStats
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
    got = utils.modelPredTurbulence(args, model, te, LOG, **kw)
    torch.manual_seed(77)
    plain = utils.modelPredStats(args, model, te, LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _inp = utils.modelPred(args, model, te, LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    target_keys = {"target_time_mean", "target_time_rms", "target_time_uv", "target_time_tke", "target_time_vort"}
    assert set(plain) == set(OLD_KEYS) | {"target", "input"}
    assert set(got) == set(plain) | set(VORT_KEYS) | set(MOMENT_KEYS) | target_keys
    for name in plain:
        assert torch.equal(got[name], plain[name]), name

    # the new keys: the fp64 statement over modelPred's samples
    p = pred.double().to(DEV)                                                  # [S, N, Tk, C, H, W], un-normalised and scaled
    ymax = float(p.abs().max())
    vort = _vorticity(p[:, :, :, :2], DX, DY)                                  # [S, N, Tk, H, W]
    tU, tV, tW = (q.permute(2, 0, 1, 3, 4)[t_start:] for q in (p[:, :, :, 0], p[:, :, :, 1], vort))
    uv, tke, tv, fl = _time_moments(tU, tV, tW)
    ref = {"vort_mean": vort.mean(0), "vort_std": vort.std(0, unbiased=False)}
    for name, q in (("uv", uv), ("tke", tke), ("vort", tv)):
        ref["time_%s_mean" % name] = q.mean(0)
        ref["time_%s_std" % name] = q.std(0, unbiased=False)
    _check(got, ref, _scales(ymax, fl, DX, DY), "%s stride %d t_start %d" % (case, stride, t_start))
    assert float(got["vort_std"].abs().max()) > 0                              # the members are distinct samples

    # the target's statistics: the fp64 statement over modelPred's target at steps j * stride, j = t_start .. Tk - 1
    tw = tgt.double().to(DEV)[:, [j * stride for j in range(t_start, nkeep)]].permute(1, 0, 2, 3, 4)   # [Tw, N, C, H, W]
    tmean = tw.mean(0)
    trms = torch.sqrt(((tw - tmean) ** 2).mean(0))
    tvort = _vorticity(tw[:, :, :2], DX, DY)
    uv, tke, tv, fl = _time_moments(tw[:, :, 0], tw[:, :, 1], tvort)
    tymax = float(tw.abs().max())
    for name, r, scale in (("target_time_mean", tmean, tymax), ("target_time_rms", trms, tymax), ("target_time_uv", uv, tymax * fl),
                           ("target_time_tke", tke, tymax * fl), ("target_time_vort", tv, tymax * (1 / DX + 1 / DY))):
        gv = got[name].double().to(DEV)
        assert gv.shape == r.shape, (name, gv.shape, r.shape)
        err = (gv - r).abs()
        bound = 4e-6 * scale + 1e-5 * r.abs()
        print("%s %s: max err %.3e, smallest bound %.3e" % (case, name, float(err.max()), float(bound.min())))
        assert bool((err <= bound).all()), "%s: max err %.3e" % (name, float(err.max()))
