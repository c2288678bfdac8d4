"""Ensemble POD projection on the device (`-m gpu`): tmg_ens_pod_project through tmg_ops.EnsembleModes against the references of
tests/modes_cases.py (explicitly formed d, direct einsum, never the kernel's slicing), and utils.modelPredModes against the same
reference over modelPred's samples.  The definitions, the rounding count cnt = L + P + 6 and the bounds are in tests/modes_cases.py;
L and P come from tmg_hip.ens_pod_plan for the case.

Integer mode: x and m integers in -8..8, psi in -2..2, a = 1: every product and partial sum is exact in fp32, so the raw sums must
EQUAL the int64 reference.  Every case runs with the workspace and the raw outputs pre-filled with NaN.

Worst share of the bound reached on an MI355X (the tests print it; LAB_NOTES.md): 0.0026 integer, 0.0075 real data, 0.0055
self-consistency, 0.0092 end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import modes_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
NAN = float("nan")


def run_modes(xs, tgt, m, psi, channels, sizes, padded, t_start, sd=None, u=None, members=None):
    """Feed EnsembleModes as utils.modelPredModes does, in chunks of `sizes` members per step; padded: y and target are channel slices
    of wider NaN-filled NHWC buffers.  Every buffer the kernels write is pre-filled with NaN.  members: feed only the first `members`
    of xs, as an ensemble of that size.  -> dict of numpy arrays (with the raw sums), and the plan."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    S = S if members is None else members
    xd = torch.from_numpy(xs).to(DEV)
    td = torch.from_numpy(tgt).to(DEV)

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), NAN, device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    en = ops.EnsembleModes(S, B, Cc, Hh, Ww, Tn, DEV, torch.ones(Cc) if sd is None else sd, u=u, channels=channels,
                           mean=torch.from_numpy(m), basis=torch.from_numpy(psi))
    for v in (en.ws, en.coef_raw, en.en_raw, en.tcoef_raw, en.ten_raw):
        if v is not None:
            v.fill_(NAN)
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
        assert m0 == S
    got = {k: v.cpu().numpy() for k, v in en.finalize().items()}
    got.update(coef_raw=en.coef_raw.cpu().numpy(), en_raw=en.en_raw.cpu().numpy(), tcoef_raw=en.tcoef_raw.cpu().numpy(),
               ten_raw=en.ten_raw.cpu().numpy())
    for k in K.STEP_KEYS + ("coef_raw", "en_raw", "tcoef_raw", "ten_raw"):
        assert not np.isnan(got[k]).any(), "%s holds NaN" % k
    return got, en.plan


# ---- integer mode: equality on every edge of the plan ----------------------------------------------------------------------------------
def _integer_case(case, idx, steps=K.T):
    S, B, Cc, chs, hw, Kk, t_start, kind, padded = case
    t_start = min(t_start, steps - 1)
    xs, tgt, m, psi = K.int_inputs(S, B, Cc, chs, hw, Kk, 5000 + idx, steps)
    got, plan = run_modes(xs, tgt, m, psi, chs, K.chunk_sizes(S, kind), padded, t_start)
    a = K.scales(None, None, B, Cc, chs)
    ref = K.reference(xs, tgt, a, m, psi, chs, integer=True)
    what = "integer %s" % (case,)
    K.shapes(got, S, B, steps, Kk)
    K.check_integer(got, ref, hw, what)
    worst = K.check_bound(got, ref, plan, hw, what)
    K.check_derived(got, t_start, what)
    print("%s: plan P=%d SL=%d L=%d; worst share of the bound %.4f" % (what, plan["P"], plan["SL"], plan["L"], worst))
    return plan


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE)))
def test_integer_data_gives_the_integer_reference_bit_for_bit(idx):
    _integer_case(K.INT_TABLE[idx], idx)


def test_integer_data_with_two_chunks_per_wave():
    plan = _integer_case(K.LONG_CASE, 100, steps=1)
    assert plan["SL"] == 512 and plan["P"] == 17


def test_integer_data_at_the_largest_member_count():
    plan = _integer_case(K.MAX_CASE, 101, steps=2)
    assert plan["P"] == 1


# ---- real data inside the counted bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_real_data_stays_in_the_rounding_bound(idx):
    S, B, Cc, chs, hw, Kk, kind, with_u = K.REAL_TABLE[idx]
    xs, tgt, m, psi, sd, u = K.real_inputs(S, B, Cc, chs, hw, Kk, kind, with_u, 6000 + idx)
    t_start = idx % 2
    got, plan = run_modes(xs, tgt, m, psi, chs, K.chunk_sizes(S, idx % 3), idx % 2 == 0, t_start, sd=torch.from_numpy(sd),
                          u=None if u is None else torch.from_numpy(u))
    a = K.scales(sd, u, B, Cc, chs)
    ref = K.reference(xs, tgt, a, m, psi, chs)
    what = "%s %s" % (kind, K.REAL_TABLE[idx][:6])
    K.shapes(got, S, B, xs.shape[0], Kk)
    worst = K.check_bound(got, ref, plan, hw, what)
    K.check_derived(got, t_start, what)
    print("%s: cnt = %d + %d + %d; worst share of the bound %.4f" % (what, plan["L"], plan["P"], K.C_ROUND, worst))


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 3])
def test_outputs_are_bitwise_the_same_for_every_feed_run_and_ensemble_size(idx):
    S, B, Cc, chs, hw, Kk, kind, with_u = K.REAL_TABLE[idx]
    xs, tgt, m, psi, sd, u = K.real_inputs(S, B, Cc, chs, hw, Kk, kind, with_u, 6000 + idx)
    kw = dict(sd=torch.from_numpy(sd), u=None if u is None else torch.from_numpy(u))
    outs = [run_modes(xs, tgt, m, psi, chs, K.chunk_sizes(S, ck), padded, 1, **kw)[0]
            for ck, padded in ((0, False), (1, True), (2, False), (2, False))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name
    # the same members inside a smaller ensemble, and (the first of them) inside this larger one: a member's rows need no other member
    small = S // 2 + 1
    part = run_modes(xs, tgt, m, psi, chs, K.chunk_sizes(small, 1), False, 1, members=small, **kw)[0]
    for name in ("coef", "fluct_energy", "coef_raw", "en_raw", "time_mode_energy", "time_mode_mean", "time_coef_cov", "time_captured_frac",
                 "time_resid_energy"):
        assert np.array_equal(part[name], outs[0][name][:, :small]), name
    for name in ("target_coef", "target_fluct_energy", "target_time_mode_energy", "target_time_coef_cov"):
        assert np.array_equal(part[name], outs[0][name]), name


# ---- self-consistency: the target's own coefficients -----------------------------------------------------------------------------------
def test_the_target_reproduces_its_own_coefficients():
    import tmg_ops as ops
    B, Tn, Cc, hw, chs, Kk, S = 3, 6, 3, (17, 31), (0, 1), 4, 2
    series = K.wave_series(B, Tn, Cc, hw, 77).float()
    sd = torch.tensor(K.SD[:Cc])
    u = 0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(5))
    a64 = u.double() * sd.double().view(1, Cc)
    m, psi, lam, lam_total, tc = ops.pod_basis(series, a64, chs, Kk)
    tgt = series.permute(1, 0, 2, 3, 4).contiguous().numpy()
    xs = np.ascontiguousarray(np.broadcast_to(tgt[:, None], (Tn, S) + tgt.shape[1:]))        # the members: the target itself
    m32, psi32 = m.numpy().astype(F32), psi.numpy().astype(F32)
    got, plan = run_modes(xs, tgt, m32, psi32, chs, [S], False, 0, sd=sd, u=u)
    # against the fp64 basis' own coefficients sqrt(Tn lam_k) v_k[j]: the counted bound about the fp32 tables, plus what rounding the
    # tables to fp32 moves: |d| u |psi| for psi, a u |m| |psi| for m, and u |d| |psi| for a (rounded once from fp64)
    a = K.scales(sd.numpy(), u.numpy(), B, Cc, chs)
    ref = K.reference(xs, tgt, a, m32, psi32, chs)
    n = float(hw[0] * hw[1])
    am = np.einsum("bc,bchw,bkchw->bk", a, np.abs(m32).astype(np.float64), np.abs(psi32).astype(np.float64))[:, None]
    slack = K.U24 * (2.0 * ref["abs_tcoef"] + am) / n
    want = {"coef_raw": ref["coef_raw"], "abs_coef": ref["abs_coef"], "en_raw": ref["en_raw"], "ten_raw": ref["ten_raw"],
            "tcoef_raw": tc.numpy() * n, "abs_tcoef": ref["abs_tcoef"]}
    worst = K.check_bound(got, want, plan, hw, "self-consistency",
                          extra={"coef": 0.0, "fluct_energy": 0.0, "target_coef": slack, "target_fluct_energy": 0.0})
    assert np.array_equal(got["coef"][:, 0], got["target_coef"]) and np.array_equal(got["coef"][:, 1], got["target_coef"])
    frac = (lam.sum(1) / lam_total).numpy()
    assert np.abs(got["target_time_captured_frac"].astype(np.float64) - frac).max() <= 1e-5 * np.abs(frac).min()
    assert np.abs(got["target_time_mode_energy"].astype(np.float64) - lam.numpy()).max() <= 1e-5 * float(lam.max())
    assert np.abs(got["mode_energy_ratio_mean"] - 1.0).max() == 0.0 and not got["mode_energy_ratio_std"].any()
    print("self-consistency: cnt = %d + %d + %d; worst share of the bound %.4f" % (plan["L"], plan["P"], K.C_ROUND, worst))


# ---- end to end: modelPredModes against the reference over modelPred's samples ---------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_modes_matches_the_reference_over_model_pred(monkeypatch, tmp_path, case):
    """The reference forms d = p - pod_mean from modelPred's un-normalised samples p and the returned physical mean.  modelPred
    un-normalises in fp32 (product, sum, product: an error of at most u (3 |p| + |u0 mu|)); the kernel's mean plane and the returned
    pod_mean are each rounded to fp32 once (u |pod_mean - u0 mu| and u |pod_mean|), and its scale a once (u |d|).  So the reference's
    d is uncertain by e = u (3 |p| + 2 |u0 mu| + 2 |pod_mean| + |d|), which adds sum e |psi| / HW to a coefficient's bound and
    sum (2 |d| e + e^2) / HW to the energy's."""
    import tmg_hip
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows, Kk, chs = 5, 5, 1, 1, 4, 3, (0, 1)
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    for _ in range(2):                                                        # two folded runs: modelPredModes, modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    for bi, B in enumerate(batches):
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    torch.manual_seed(77)
    got = utils.modelPredModes(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows, modes=Kk,
                               channels=chs)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    new = set(K.STEP_KEYS + K.DERIVED_KEYS) | {"pod_energy", "pod_energy_frac", "pod_modes", "pod_mean"}
    assert set(got) == set(stats) | new
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Hh, Ww = y.shape[0], y.shape[3], y.shape[4]
    Cg = len(chs)
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    K.shapes(g, S, N, Tk, Kk)
    assert g["pod_modes"].shape == (N, Kk, Cg, Hh, Ww) and g["pod_mean"].shape == (N, Cg, Hh, Ww) and g["pod_energy"].shape == (N, Kk)
    # the basis is the target's own: its mean, orthonormal modes, and energies that are the target's mode energies
    ych = y[:, t_start:, list(chs)]
    assert np.abs(g["pod_mean"] - ych.mean(1)).max() <= K.U24 * np.abs(ych).max()
    pm = g["pod_modes"].astype(np.float64).reshape(N, Kk, -1)
    assert np.abs(pm @ pm.transpose(0, 2, 1) / (Hh * Ww) - np.eye(Kk)).max() <= 1e-5
    assert np.all(np.diff(g["pod_energy"], axis=1) <= 0) and np.all(g["pod_energy_frac"].sum(1) <= 1 + 1e-12)
    xs = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5))
    ys = np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))
    ones = np.ones((N, Cg))
    mean, psi = g["pod_mean"].astype(np.float64), g["pod_modes"].astype(np.float64)
    ref = K.reference(xs, ys, ones, mean, psi, chs)
    plans = [tmg_hip.ens_pod_plan(S, B, Cg, Hh * Ww, Kk) for B in batches]
    plan = {"L": max(q["L"] for q in plans), "P": max(q["P"] for q in plans)}
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, list(chs)]                        # [N, Cg]
    umu = np.abs(uc * mu[list(chs)].reshape(1, Cg)).reshape(N, Cg, 1, 1)
    n = float(Hh * Ww)

    def slack(rows, member):
        """rows [T, (S,) N, Cg, H, W] physical -> the added bounds (coefficient, energy), shaped as the outputs."""
        d = np.abs(rows - mean)
        e = K.U24 * (3 * np.abs(rows) + 2 * umu + 2 * np.abs(mean) + d)
        q = 2 * d * e + e * e
        if member:
            return np.einsum("tsbchw,bkchw->bstk", e, np.abs(psi)) / n, np.einsum("tsbchw->bst", q) / n
        return np.einsum("tbchw,bkchw->btk", e, np.abs(psi)) / n, np.einsum("tbchw->bt", q) / n

    ec, ee = slack(xs[:, :, :, list(chs)], True)
    tc, te_ = slack(ys[:, :, list(chs)], False)
    extra = {"coef": ec, "fluct_energy": ee, "target_coef": tc, "target_fluct_energy": te_}
    worst = K.check_bound(g, ref, plan, (Hh, Ww), case, extra=extra)
    K.check_derived(g, t_start, case, lam=g["pod_energy"])                      # the wrapper hands the accumulator pod_basis' energies
    # the target through the kernel against the basis' own energies
    assert np.abs(g["target_time_mode_energy"] - g["pod_energy"]).max() <= 1e-4 * g["pod_energy"].max()
    print("%s: cnt = %d + %d + %d; worst share of the bound %.4f" % (case, plan["L"], plan["P"], K.C_ROUND, worst))
