"""Ensemble line spectra on the device (`-m gpu`): tmg_ens_lspec_chunk / tmg_ens_lspec_step / tmg_ens_lspec_finalize through
tmg_ops.EnsembleLineSpectra and utils.modelPredLineSpectra against the fp64 reference of tests/lspec_cases.py (np.fft.rfft, two-pass
fluctuation, two-pass mean / std over the members).

Bound on every element of every output (lspec_cases.compare): |got - ref| <= max(1e-5 |ref| + 2e-6 P, 3 e32), P the largest line
total of the output's member-level spectra, e32 the error of the plain float32 torch restatement of the matrix DFT and the Welford
recurrences (lspec_cases.mirror32), computed here on the CPU from the field as the kernel forms it.  The achieved error is printed
beside the bound.  The bitwise properties are asserted with torch.equal.

Observed on an MI355X (LAB_NOTES.md): 20 passed in 4 s, the longest 0.9 s (end to end on the cylinder loader); the largest error
9.9e-7 P (time_lspec_fluct_member, 33 lines of 272 points), the largest share of the bound reached by any element 0.20."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import lspec_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

LOG = SimpleNamespace(log=lambda *a, **k: None, warning=lambda *a, **k: None, error=lambda *a, **k: None)
MU = torch.tensor([0.3, -0.2, 0.5, 0.1])
SD = torch.tensor([1.7, 0.6, 2.5, 0.9])
U = torch.tensor([[1.3, 0.7, 1.69, 1.1], [0.8, 1.2, 0.64, 0.9]])
GRID = (0.05, 0.07)
DEVICE_KEYS = K.KEYS


def _normalised(f, u):
    """The model-side tensor whose un-normalisation u[b, c] (sd y + mu) gives f: [T, S, B, C, H, W] fp32 on the device."""
    Cc = f.shape[3]
    y = torch.from_numpy(f)
    if u is not None:
        y = y / u.double().view(1, 1, *u.shape, 1, 1)
    y = (y - MU[:Cc].double().view(1, 1, 1, Cc, 1, 1)) / SD[:Cc].double().view(1, 1, 1, Cc, 1, 1)
    return y.float().to(DEV)


def _fields(ys, u):
    """(fp64, fp32) physical fields of the fp32 tensor ys: the fp64 statement's input and the kernel's own fp32 form."""
    yc = ys.cpu()
    Cc = yc.shape[3]
    mu, sd = MU[:Cc].view(1, 1, 1, Cc, 1, 1), SD[:Cc].view(1, 1, 1, Cc, 1, 1)
    f64 = sd.double() * yc.double() + mu.double()
    f32 = sd * yc + mu
    if u is not None:
        f64 = f64 * u.double().reshape(1, 1, -1, Cc, 1, 1)
        f32 = f32 * u.reshape(1, 1, -1, Cc, 1, 1)
    return f64.numpy(), f32


def _sizes(S, how):
    """The chunk sizes of one step: one member per chunk, all at once, or unevenly."""
    if how == "one":
        return [1] * S
    if how == "all" or S == 1:
        return [S]
    return [1, S - 1] if S < 5 else [1, S - 3, 2]


def _make(ys, u, axis, win, per_member=True):
    import tmg_ops as ops
    T, S, B, Cc, Hh, Ww = ys.shape
    return ops.EnsembleLineSpectra(S, B, Cc, Hh, Ww, T, DEV, MU[:Cc], SD[:Cc], u=None if u is None else u.to(DEV), grid=GRID, axis=axis,
                                   window=win, per_member=per_member)


def _feed(acc, ys, how, t_start, padded=False):
    T, S, B, Cc, Hh, Ww = ys.shape
    for t in range(T):
        m0 = 0
        for k in _sizes(S, how):
            y = ys[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww).permute(0, 2, 3, 1)         # NHWC [k*B, H, W, C]
            if padded:                                                                  # a channel slice of a wider NHWC buffer
                wide = torch.full((k * B, Hh, Ww, Cc + 3), float("nan"), device=DEV)
                wide[..., 2:2 + Cc] = y
                y = wide[..., 2:2 + Cc]
            else:
                y = y.contiguous()
            acc.add(y.permute(0, 3, 1, 2), m0, time=t >= t_start)
            m0 += k
    return acc.finalize()


def _run(ys, u, axis, win, how, t_start, padded=False):
    return _feed(_make(ys, u, axis, win), ys, how, t_start, padded)


def _shape(axis, L, N):
    return (L, N) if axis == "x" else (N, L)


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for name, v in a.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, b[name]) or bool((torch.isnan(v) == torch.isnan(b[name])).all() and
                                                   torch.equal(torch.nan_to_num(v), torch.nan_to_num(b[name]))), "%s: %s" % (what, name)
        else:
            assert v == b[name], "%s: %s" % (what, name)


# ---- 1. kernels against fp64 ----------------------------------------------------------------------------------------------------
# (axis, L, N, B, C, S, timed steps T (after one untimed step), window, chunking, u given, channel-padded input)
CASES = [
    ("x", 1, 16, 2, 2, 1, 3, "hann", "all", True, False),           # one mode tile with 7 padded columns, a single masked line tile
    ("x", 16, 48, 1, 3, 2, 6, None, "one", False, True),            # 2 mode tiles: fewer than the waves
    ("y", 17, 80, 2, 4, 5, 3, "hann", "uneven", True, False),       # columns; a second line tile that holds one line
    ("x", 33, 272, 1, 3, 2, 3, "hann", "all", False, False),        # 9 mode tiles: three rounds of the four waves
    ("y", 33, 16, 1, 3, 5, 6, None, "one", True, True),
    ("y", 16, 272, 2, 2, 1, 1, "hann", "all", False, True),
    ("x", 17, 48, 2, 4, 5, 1, None, "uneven", False, False),
    ("y", 1, 80, 1, 3, 2, 3, None, "uneven", True, False),
]


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_lspec_kernels_match_fp64(idx):
    import tmg_ops as ops
    axis, L, N, B, Cc, S, Tn, win, how, u_given, padded = CASES[idx]
    Hh, Ww = _shape(axis, L, N)
    T, t_start = Tn + 1, 1
    u = U[:B, :Cc].contiguous() if u_given else None
    ys = _normalised(K.synthetic(T, S, B, Cc, Hh, Ww, 300 + idx), u)
    got = _run(ys, u, axis, win, how, t_start, padded)
    f64, f32 = _fields(ys, u)
    ref = K.reference(f64, axis, win, t_start)
    y32 = K.mirror32(f32, axis, win, t_start)
    bad = K.compare(got, ref, y32, "case %d" % idx)
    assert not bad, "\n".join(bad)
    nq = N // 2 + 1
    assert tuple(got["lspec_mean"].shape) == (B, T, Cc + 2, nq) and tuple(got["time_lspec_fluct_member"].shape) == (B, S, Cc + 2, L, nq)
    assert got["lspec_k"].dtype == torch.float64 and got["lspec_k"].device.type == "cpu"
    np.testing.assert_allclose(got["lspec_k"].numpy(), K.wavenumbers(N, GRID[0] if axis == "x" else GRID[1]), rtol=1e-15, atol=0)
    assert got["lspec_fields"] == K.fields(Cc) == ops.lspec_fields(Cc)
    want = K.derived(got["time_lspec_fluct_mean"].double().cpu().numpy(), got["lspec_k"].numpy(), Cc)
    for name in K.DERIVED:
        g = got[name]
        assert g.dtype == torch.float64 and g.device.type == "cpu"
        np.testing.assert_allclose(g.numpy(), want[name], rtol=2.0 ** -24, atol=2.0 ** -40, equal_nan=True)
    if Tn == 1:                                                                          # one timed step: no fluctuation at all
        for name in ("time_lspec_fluct_mean", "time_lspec_fluct_std", "time_lspec_fluct_member"):
            assert bool((got[name] == 0).all()), name


# ---- 2. bitwise: chunking, objects, runs, garbage in every buffer -----------------------------------------------------------------------
@pytest.mark.parametrize("axis,L,N,Cc", [("x", 17, 48, 3), ("y", 33, 80, 4)])
def test_every_chunking_object_and_run_gives_the_same_bits(monkeypatch, axis, L, N, Cc):
    import tmg_ops as ops
    T, S, B = 4, 5, 2
    Hh, Ww = _shape(axis, L, N)
    u = U[:B, :Cc].contiguous()
    ys = _normalised(K.synthetic(T, S, B, Cc, Hh, Ww, 41), u)
    base = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in _run(ys, u, axis, "hann", "all", 1).items()}
    assert float(base["lspec_std"].abs().max()) > 0 and float(base["time_lspec_fluct_std"].abs().max()) > 0
    for how in ("one", "uneven", "all"):                                                 # "all" again: a second object, a second run
        _same_bits(base, _run(ys, u, axis, "hann", how, 1), how)
    _same_bits(base, _run(ys, u, axis, "hann", "uneven", 1, padded=True), "channel slice")
    # state, partials and outputs pre-filled with NaN: every element is written before it is read
    nan = float("nan")
    acc = _make(ys, u, axis, "hann")
    for t in (acc.mean_state, acc.comom_state, acc.step_state, acc.out["lspec_mean"], acc.out["lspec_std"]):
        t.fill_(nan)
    acc._part = torch.full((S * acc.plan["part_floats"],), nan, device=DEV)
    monkeypatch.setattr(ops, "empty", lambda shape, device: torch.full(tuple(shape), nan, device=device, dtype=torch.float32))
    _same_bits(base, _feed(acc, ys, "uneven", 1), "NaN pre-fill")


@pytest.mark.parametrize("L,N,win", [(17, 48, "hann"), (16, 272, None)])
def test_columns_equal_rows_of_the_transposed_field_bit_for_bit(L, N, win):
    T, S, B, Cc = 3, 2, 2, 3
    f = K.synthetic(T, S, B, Cc, N, L, 42)                                               # [.., H = N, W = L]: axis "y" has L lines of N
    u = U[:B, :Cc].contiguous()
    a = _run(_normalised(f, u), u, "y", win, "uneven", 1)
    b = _run(_normalised(np.ascontiguousarray(np.swapaxes(f, -1, -2)), u), u, "x", win, "uneven", 1)
    for name in DEVICE_KEYS + ("time_lspec_energy", "time_lspec_coherence"):
        assert torch.equal(a[name], b[name]) or (name in K.DERIVED and torch.equal(torch.nan_to_num(a[name]), torch.nan_to_num(b[name]))), name
    # the wavenumbers, and the centroid with them, differ by the cell size: d = dy against d = dx
    assert not torch.equal(a["lspec_k"], b["lspec_k"])
    np.testing.assert_allclose(a["lspec_k"].numpy() * GRID[1], b["lspec_k"].numpy() * GRID[0], rtol=1e-15, atol=0)
    np.testing.assert_allclose(a["time_lspec_centroid"].numpy() * GRID[1], b["time_lspec_centroid"].numpy() * GRID[0], rtol=1e-13, atol=0)


# ---- 3. exact zeros ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["x", "y"])
def test_a_field_constant_in_time_has_no_fluctuation_at_all(axis):
    T, S, B, Cc, L, N = 5, 2, 2, 3, 17, 48
    Hh, Ww = _shape(axis, L, N)
    ys = _normalised(K.synthetic(T, S, B, Cc, Hh, Ww, 43, const_time=True), None)
    got = _run(ys, None, axis, "hann", "one", 1)
    for name in ("time_lspec_fluct_mean", "time_lspec_fluct_std", "time_lspec_fluct_member"):
        assert bool((got[name] == 0).all()), name
    assert float(got["time_lspec_flow_mean"][:, :Cc].min()) >= 0 and float(got["time_lspec_flow_mean"].abs().max()) > 0


def test_one_timed_step_has_no_fluctuation_at_all():
    T, S, B, Cc, L, N = 3, 2, 1, 3, 16, 16
    ys = _normalised(K.synthetic(T, S, B, Cc, L, N, 44), None)
    got = _run(ys, None, "x", None, "all", T - 1)                                        # the last step alone is timed
    for name in ("time_lspec_fluct_mean", "time_lspec_fluct_std", "time_lspec_fluct_member"):
        assert bool((got[name] == 0).all()), name
    e = got["time_lspec_energy"]
    assert bool((e == 0).all()) and bool(torch.isnan(got["time_lspec_centroid"]).all())


def test_identical_members_have_zero_spread():
    T, S, B, Cc, L, N = 4, 4, 2, 3, 17, 80
    one = _normalised(K.synthetic(T, 1, B, Cc, L, N, 45), None)
    ys = one.expand(T, S, B, Cc, L, N).contiguous()
    got = _run(ys, None, "x", "hann", "uneven", 1)
    for name in K.STD_KEYS:
        assert not bool(torch.isnan(got[name]).any()) and bool((got[name] == 0).all()), name
    assert float(got["time_lspec_fluct_mean"][:, :Cc].max()) > 0
    for m in range(1, S):
        assert torch.equal(got["time_lspec_fluct_member"][:, m], got["time_lspec_fluct_member"][:, 0])


# ---- 4. Parseval against the ensemble statistics ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,L,N", [("x", 17, 48), ("y", 16, 80)])
def test_autospectra_sum_to_the_squared_time_rms_of_ensemble_stats(axis, L, N):
    import tmg_ops as ops
    T, B, Cc = 6, 2, 3
    Hh, Ww = _shape(axis, L, N)
    u = U[:B, :Cc].contiguous()
    ys = _normalised(K.synthetic(T, 1, B, Cc, Hh, Ww, 46), u)
    got = _run(ys, u, axis, None, "all", 1)
    st = ops.EnsembleStats(1, B, Cc, Hh, Ww, T, DEV, MU[:Cc].to(DEV), SD[:Cc].to(DEV), u=u.to(DEV))
    for t in range(T):
        st.add(ys[t, 0].contiguous(memory_format=torch.channels_last), 0, time=t >= 1)
    rms = st.finalize()["time_rms_mean"].double().cpu()                                  # [B, C, H, W]
    ref = (rms ** 2).mean(-1 if axis == "x" else -2).numpy()                             # [B, C, L]
    tot = got["time_lspec_energy"][:, :Cc].numpy()
    # e32: the float32 restatement's line totals against the fp64 reference's
    f64, f32 = _fields(ys, u)
    e64 = K.reference(f64, axis, None, 1)["time_lspec_fluct_mean"][:, :Cc].sum(-1)
    e32 = float(np.abs(K.mirror32(f32, axis, None, 1)["time_lspec_fluct_mean"][:, :Cc].sum(-1) - e64).max())
    P = float(ref.max())
    err = np.abs(tot - ref)
    bound = np.maximum(1e-5 * np.abs(ref) + 2e-6 * P, 3 * e32)
    print("Parseval %s: max err %.3e, bound there %.3e, P %.3e, e32 %.3e" % (axis, float(err.max()), float(bound.ravel()[int(err.argmax())]),
                                                                             P, e32))
    assert bool((err <= bound).all())


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("case,axis,win", [("cylinder", "x", "hann"), ("step", "y", None)])
def test_model_pred_line_spectra_end_to_end(monkeypatch, tmp_path, case, axis, win):
    import tmg_ops as ops
    from utils import utils
    model, te = (_cylinder_case if case == "cylinder" else _step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    nkeep = tmax // stride
    batches = [int(b[0].shape[0]) for b in te]
    kp = _KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=GRID[0], dy=GRID[1])
    for rep in range(2):                                                       # modelPredLineSpectra, then modelPredTurbulence
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
    got = utils.modelPredLineSpectra(args, model, te, LOG, axis=axis, window=win, per_member=True, **kw)
    torch.manual_seed(77)
    plain = utils.modelPredTurbulence(args, model, te, LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _inp = utils.modelPred(args, model, te, LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    new = set(K.KEYS) | set(K.DERIVED) | {"lspec_k", "lspec_fields", "target_lspec", "target_time_lspec_fluct", "target_time_lspec_flow",
                                          "lspec_log_distance"}
    assert set(got) == set(plain) | new
    for name in plain:
        assert torch.equal(got[name], plain[name]), name

    Hh, Ww = pred.shape[-2:]
    assert (Hh, Ww) == ((32, 32) if case == "cylinder" else (16, 16))
    N = Ww if axis == "x" else Hh
    np.testing.assert_allclose(got["lspec_k"].numpy(), K.wavenumbers(N, GRID[0] if axis == "x" else GRID[1]), rtol=1e-15, atol=0)
    assert got["lspec_fields"] == K.fields(3)
    # the ensemble's spectra: the reference over modelPred's samples [S, N, Tk, C, H, W] -> [Tk, S, N, C, H, W]
    f32 = pred.permute(2, 0, 1, 3, 4, 5).contiguous()
    ref = K.reference(f32.double().numpy(), axis, win, t_start)
    bad = K.compare(got, ref, K.mirror32(f32, axis, win, t_start), case)
    assert not bad, "\n".join(bad)
    assert float(got["lspec_std"].abs().max()) > 0                              # the members are distinct samples
    # the target's spectra: modelPred's target at steps j * stride, j = t_start .. Tk - 1, as a one-member ensemble
    t32 = tgt[:, [j * stride for j in range(t_start, nkeep)]].permute(1, 0, 2, 3, 4).unsqueeze(1).contiguous()   # [Tw, 1, N, C, H, W]
    tref = K.reference(t32.double().numpy(), axis, win, 0)
    tgot = {"lspec_mean": got["target_lspec"], "time_lspec_fluct_mean": got["target_time_lspec_fluct"],
            "time_lspec_flow_mean": got["target_time_lspec_flow"]}
    bad = K.compare(tgot, tref, K.mirror32(t32, axis, win, 0), case + " target", keys=K.MEAN_KEYS)
    assert not bad, "\n".join(bad)
    d = K.log_distance(got["time_lspec_fluct_mean"].numpy(), got["target_time_lspec_fluct"].numpy(), 3)
    assert got["lspec_log_distance"].dtype == torch.float64 and tuple(got["lspec_log_distance"].shape) == d.shape == (len(pred[0]), 3, Ww if axis == "y" else Hh)
    np.testing.assert_allclose(got["lspec_log_distance"].numpy(), d, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert bool(np.isfinite(d).any())
