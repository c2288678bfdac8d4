"""Ensemble phase averages on the device (`-m gpu`): tmg_ens_phase_label and tmg_ens_phase_accum through tmg_ops.EnsemblePhase against
the references of tests/phase_cases.py (a float32 numpy mirror of the labelling; the raw sums grouped by label with boolean masks and
summed directly, never through the kernel's tiling), and utils.modelPredPhase against the same references over modelPred's samples.
The definitions, the counts C_ROUND_LIN = 3 / C_ROUND_PROD = 6 and the bound (n + C_ROUND) u sum |term| are in tests/phase_cases.py.

The kernel tests drive EnsemblePhase with an EnsembleModes whose add() writes prescribed raw coefficient sums instead of projecting,
so that the label of every row is chosen by the test; the rows, the accumulation and every host formula are the product's.  Integer
mode: x and m integers in -8..8, a = 1, at most 2^7 rows per sector: every term and partial sum is exact in fp32, so the accumulators
must EQUAL the int64 reference.  The tests print the worst share of the bound they reach.

Worst share of the bound reached on an MI355X (LAB_NOTES.md): 0.67 real data (sectors of one to a few rows, where the bound is
(1 + 3) u against an error of up to 2 u), 0.55 through the projection, 0.47 end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import modes_cases as K
import phase_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
NAN = float("nan")


def _fixed_modes(S, B, Cc, Hh, Ww, steps, craw, tcraw):
    """An EnsembleModes of the feed whose add() writes the prescribed raw sums craw [B, S, T, K] / tcraw [B, T, K] of the chunk."""
    import tmg_ops as ops

    class Fixed(ops.EnsembleModes):
        def __init__(self):
            ops.EnsembleFeed.__init__(self, S, B, Cc, Hh, Ww, steps)
            self.K = craw.shape[-1]
            self.src, self.tsrc = torch.from_numpy(craw).to(DEV), torch.from_numpy(tcraw).to(DEV)
            self.coef_raw = torch.full((B, S, steps, self.K), NAN, device=DEV)
            self.tcoef_raw = torch.full((B, steps, self.K), NAN, device=DEV)

        def add(self, y, m0, target, time=True):
            yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
            t = self._step
            self.coef_raw[:, m0:m0 + k, t] = self.src[:, m0:m0 + k, t]
            if last:
                self.tcoef_raw[:, t] = self.tsrc[:, t]
            self.close_chunk(m0, k, time, last)

        def finalize(self):
            self.finalize_guard()
            n = float(Hh * Ww)
            return {"coef": (self.coef_raw.double() / n).float(), "target_coef": (self.tcoef_raw.double() / n).float()}

    return Fixed()


def nhwc(v, Cc, padded):
    """[rows, C, H, W] -> an API-shaped view whose channels-last form is dense, or a channel slice of a wider NaN-filled buffer."""
    v = v.permute(0, 2, 3, 1)
    if not padded:
        return v.contiguous().permute(0, 3, 1, 2)
    wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), NAN, device=v.device)
    wide[..., 1:1 + Cc] = v
    return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)


def feed(en, xs, tgt, sizes, padded, timed):
    """Feed the accumulator as utils.modelPredPhase does -> the accumulators' clones after every step [(acc, tacc)]."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    xd, td = torch.from_numpy(xs).to(DEV), torch.from_numpy(tgt).to(DEV)
    snaps = []
    for t in range(Tn):
        target = nhwc(td[t], Cc, padded)
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww), Cc, padded), m0, target, time=t in timed)
            m0 += k
        assert m0 == S
        snaps.append((en.acc.cpu().numpy().copy(), en.tacc.cpu().numpy().copy()))
    return snaps


def run_phase(xs, tgt, m, craw, tcraw, NB, sizes, padded, timed, min_amp=0.25, sd=None, u=None, lam=None, pair=(0, 1)):
    """EnsemblePhase over prescribed coefficients -> (dict of numpy arrays: the outputs, the raw accumulators acc / tacc, the snapshots,
    g), the accumulator."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    lam = np.ones((B, 2)) if lam is None else lam
    fm = _fixed_modes(S, B, Cc, Hh, Ww, Tn, craw, tcraw)
    en = ops.EnsemblePhase(S, B, Cc, Hh, Ww, Tn, DEV, torch.ones(Cc) if sd is None else sd, u=u, modes=fm, pair=pair, bins=NB,
                           min_amp=min_amp, mean=torch.from_numpy(m), lam=torch.from_numpy(lam))
    en.label.fill_(-7)
    en.tlabel.fill_(-7)
    snaps = feed(en, xs, tgt, sizes, padded, timed)
    got = {k: v.cpu().numpy() for k, v in en.finalize().items()}
    got.update(acc=en.acc.cpu().numpy(), tacc=en.tacc.cpu().numpy(), snaps=snaps, g=en.g.cpu().numpy())
    return got, en


def check_labels(got, craw, tcraw, lam, hw, NB, min_amp, pair, what):
    """The labels equal the float32 mirror bit for bit -> (labels, target labels) of the mirror."""
    g = P.gains(lam, hw[0] * hw[1])
    assert np.array_equal(got["g"], g), what
    tab = P.table(NB, min_amp)
    lab = P.label_mirror(craw[..., pair[0]], craw[..., pair[1]], g[:, None, None, 0], g[:, None, None, 1], tab, NB)
    tlab = P.label_mirror(tcraw[..., pair[0]], tcraw[..., pair[1]], g[:, None, 0], g[:, None, 1], tab, NB)
    assert got["phase_bin"].dtype == np.int32 and np.array_equal(got["phase_bin"], lab), "%s: labels differ from the mirror" % what
    assert got["target_phase_bin"].dtype == np.int32 and np.array_equal(got["target_phase_bin"], tlab), "%s: target labels" % what
    return lab, tlab


# ---- 1: the labels -----------------------------------------------------------------------------------------------------------------------
EDGE_POINTS = [(1, 0), (2, 2), (0, 3), (-1, 1), (-5, 0), (-3, -3), (0, -2), (4, -4), (0, 0), (1, 1), (3, 1), (1, 3), (-2, 1), (7, -1)]


@pytest.mark.parametrize("idx", range(len(P.LABEL_TABLE)))
def test_labels_equal_the_float32_mirror_bit_for_bit(idx):
    NB, B, S = P.LABEL_TABLE[idx]
    Tn, Cc, hw, Kk, pair = 3, 2, (2, 2), 3, (2, 0)
    HW = hw[0] * hw[1]
    min_amp = 0.25 if idx % 2 == 0 else 0.0
    rng = np.random.RandomState(40 + idx)
    craw = (rng.randn(B, S, Tn, Kk) * HW * 10.0 ** rng.uniform(-2, 1, size=(B, S, Tn, 1))).astype(F32)   # gated and kept rows
    tcraw = (rng.randn(B, Tn, Kk) * HW).astype(F32)
    pts = np.array(EDGE_POINTS + [(0.25, 0.25), (0.25, -0.25)], dtype=np.float64) * HW          # g = 1 / 4 exactly: x, y are the points
    flat = craw.reshape(-1, Kk)
    npts = min(len(pts), len(flat))
    flat[:npts, pair[0]], flat[:npts, pair[1]] = pts[:npts, 0], pts[:npts, 1]
    craw = flat.reshape(B, S, Tn, Kk)
    tcraw[0, :, pair[0]], tcraw[0, :, pair[1]] = pts[[1, 8, 14], 0], pts[[1, 8, 14], 1]
    xs, tgt, m = P.int_inputs(S, B, Cc, hw, 41, Tn)
    got, en = run_phase(xs, tgt, m, craw, tcraw, NB, P.chunk_sizes(S, idx % 3), False, range(Tn), min_amp=min_amp, pair=pair)
    lab, tlab = check_labels(got, craw, tcraw, np.ones((B, 2)), hw, NB, min_amp, pair, "labels %s" % (P.LABEL_TABLE[idx],))
    away = P.label_atan2(craw[..., pair[0]], craw[..., pair[1]], NB)
    th = np.mod(np.arctan2(craw[..., pair[1]].astype(np.float64), craw[..., pair[0]].astype(np.float64)), 2 * np.pi) / (2 * np.pi / NB)
    clear = (lab >= 0) & (np.abs(th - np.round(th)) > 1e-3)
    assert np.array_equal(lab[clear], away[clear])
    if S * B * Tn >= 20:
        assert (lab < 0).any() == (min_amp > 0) and len(np.unique(lab[lab >= 0])) >= NB // 2
    print("labels %s: %d rows, %d skipped, %d on the listed edge points" % (P.LABEL_TABLE[idx], lab.size, int((lab < 0).sum()), npts))


# ---- 2: integer data -------------------------------------------------------------------------------------------------------------------
def _integer_case(case, idx, steps=P.T):
    S, B, Cc, hw, NB, kind, padded, pattern = case
    HW = hw[0] * hw[1]
    timed = range(1, steps)
    xs, tgt, m = P.int_inputs(S, B, Cc, hw, 7000 + idx, steps)
    want = P.pattern_labels(pattern, S, B, NB, steps)
    craw = P.coefs_for(want, NB, HW, 7100 + idx)
    twant = (want[:, 0] + 1) % NB if pattern != "skip" else np.where(want[:, 0] < 0, -1, (want[:, 0] + 1) % NB)
    tcraw = P.coefs_for(twant, NB, HW, 7200 + idx)
    got, en = run_phase(xs, tgt, m, craw, tcraw, NB, P.chunk_sizes(S, kind), padded, timed)
    what = "integer %s" % (case,)
    lab, tlab = check_labels(got, craw, tcraw, np.ones((B, 2)), hw, NB, 0.25, (0, 1), what)
    assert np.array_equal(lab, want) and np.array_equal(tlab, twant), what
    assert en.plan["vec"] == (HW % 4 == 0) and en.plan["tile"] == (1024 if HW % 4 == 0 else 256)
    a = P.scales(None, None, B, Cc)
    ref = P.reference(xs, lab, timed, a, m, NB, integer=True)
    tref = P.reference(tgt[:, None], tlab[:, None], timed, a, m, NB, integer=True)
    P.check_integer(got["acc"], ref, what)
    P.check_integer(got["tacc"], tref, what + " target")
    # untimed steps are labelled, not accumulated; a step whose rows are all skipped leaves the accumulators as they were
    assert not got["snaps"][0][0].any() and not got["snaps"][0][1].any(), what
    assert (got["phase_bin"][:, :, 0] >= 0).all() or pattern == "skip"
    for t in range(1, steps):
        if (lab[:, :, t] < 0).all():
            assert np.array_equal(got["snaps"][t][0], got["snaps"][t - 1][0]), "%s: step %d is wholly skipped" % (what, t)
        if (tlab[:, t] < 0).all():
            assert np.array_equal(got["snaps"][t][1], got["snaps"][t - 1][1]), what
    empty = ref["n"] == 0
    assert not got["acc"][empty].any()                                        # a sector that never gets a row stays zero
    der = P.derive(got, got["acc"], got["tacc"], Cc, hw, a[:, :, None, None] * m.astype(np.float64), np.ones((B, 2)), (0, 1), timed)
    P.check_derived(got, der, what)
    assert np.isnan(got["phase_mean"][empty]).all() and not np.isnan(got["phase_mean"][~empty]).any()
    return got, ref


@pytest.mark.parametrize("idx", range(len(P.INT_TABLE)))
def test_integer_data_gives_the_integer_reference_bit_for_bit(idx):
    got, ref = _integer_case(P.INT_TABLE[idx], idx)
    pattern = P.INT_TABLE[idx][7]
    if pattern == "never":
        assert (ref["n"][:, -1] == 0).all() and (ref["n"][:, :-1] > 0).any()
    if pattern == "skip":
        assert (got["phase_bin"][:, :, 2] == -1).all() and got["phase_skipped"].min() >= P.INT_TABLE[idx][0]


def test_integer_data_at_the_largest_member_count():
    got, ref = _integer_case(P.MAX_CASE, 100, steps=3)
    assert got["phase_bin"].shape[1] == 1024 and ref["n"].max() <= 2 ** 7 and ref["n"].min() > 0


# ---- 3, 4: real data inside the counted bound; reproducibility ---------------------------------------------------------------------------
def _real_case(idx, kind=None, padded=None):
    S, B, Cc, hw, NB, kind0, padded0, with_u = P.REAL_TABLE[idx]
    kind, padded = kind0 if kind is None else kind, padded0 if padded is None else padded
    HW = hw[0] * hw[1]
    xs, tgt, m, sd, u = P.real_inputs(S, B, Cc, hw, with_u, 8000 + idx)
    rng = np.random.RandomState(8100 + idx)
    lam = rng.uniform(0.5, 3.0, size=(B, 2))
    amp = HW * np.sqrt(lam)
    craw = (rng.randn(B, S, P.T, 2) * amp[:, None, None, :] * rng.choice([0.05, 1.0, 1.0, 1.0], size=(B, S, P.T, 1))).astype(F32)
    tcraw = (rng.randn(B, P.T, 2) * amp[:, None, :]).astype(F32)
    timed = range(idx % 2, P.T)
    got, en = run_phase(xs, tgt, m, craw, tcraw, NB, P.chunk_sizes(S, kind), padded, timed, sd=torch.from_numpy(sd),
                        u=None if u is None else torch.from_numpy(u), lam=lam, pair=(1, 0))
    return got, (xs, tgt, m, sd, u, lam, craw, tcraw, timed)


@pytest.mark.parametrize("idx", range(len(P.REAL_TABLE)))
def test_real_data_stays_in_the_rounding_bound(idx):
    S, B, Cc, hw, NB = P.REAL_TABLE[idx][:5]
    got, (xs, tgt, m, sd, u, lam, craw, tcraw, timed) = _real_case(idx)
    what = "real %s" % (P.REAL_TABLE[idx],)
    lab, tlab = check_labels(got, craw, tcraw, lam, hw, NB, 0.25, (1, 0), what)
    assert (lab < 0).any() and (lab >= 0).any()
    a = P.scales(sd, u, B, Cc)
    ref = P.reference(xs, lab, timed, a, m, NB)
    tref = P.reference(tgt[:, None], tlab[:, None], timed, a, m, NB)
    worst = max(P.check_bound(got["acc"], ref, Cc, what), P.check_bound(got["tacc"], tref, Cc, what + " target"))
    der = P.derive(got, got["acc"], got["tacc"], Cc, hw, a[:, :, None, None] * m.astype(np.float64), lam, (1, 0), timed)
    P.check_derived(got, der, what)
    print("%s: up to %d rows per sector; worst share of the bound %.4f" % (what, int(ref["n"].max()), worst))


@pytest.mark.parametrize("idx", [0, 3])
def test_outputs_are_bitwise_the_same_for_every_chunking_and_run(idx):
    outs = [_real_case(idx, kind, padded)[0] for kind, padded in ((0, False), (1, True), (2, False), (2, False))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            if name == "snaps":
                assert all(np.array_equal(x, y) for s0, s1 in zip(v, o[name]) for x, y in zip(s0, s1))
            else:
                assert np.array_equal(v, o[name], equal_nan=True), name


# ---- 5: through EnsembleModes and EnsemblePhase, a synthetic rotating pair ---------------------------------------------------------------
def _rotating(S, B, Tn, Cc, hw, seed, noise):
    """mean + A (cos phi_t psi_1 + sin phi_t psi_2) / a + noise, psi from pod_basis of a wave series; the members are phase-shifted
    copies with their own noise, member 1 and the target without noise -> the tables and the series."""
    import tmg_ops as ops
    rng = np.random.RandomState(seed)
    chs, A, omega = (0, 1), 1.3, 2 * np.pi / 7.3
    sd = torch.tensor(K.SD[:Cc])
    u = 0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(seed))
    a64 = (u.double() * sd.double().view(1, Cc)).numpy()
    _, psi, _, _, _ = ops.pod_basis(K.wave_series(B, 12, Cc, hw, seed), torch.from_numpy(a64), chs, 2)
    psi = psi.numpy()                                                        # [B, 2, 2, H, W], <psi_k, psi_l> = delta_kl
    mean = 0.3 * rng.randn(B, Cc, *hw)
    third = 0.5 * rng.randn(B, 1, *hw)                                       # the third channel follows the cycle too

    def series(shift, eps):
        phi = 0.4 + omega * np.arange(Tn) + shift
        c, s = np.cos(phi).reshape(Tn, 1, 1, 1, 1), np.sin(phi).reshape(Tn, 1, 1, 1, 1)
        x = np.broadcast_to(mean[None], (Tn,) + mean.shape).copy()
        x[:, :, :2] += A * (c * psi[None, :, 0] + s * psi[None, :, 1]) / a64[None, :, :2, None, None]
        x[:, :, 2:3] += c * third[None]
        return x + eps * rng.randn(*x.shape)

    tgt = series(0.0, 0.0)
    xs = np.stack([series(0.9 * s_, 0.0 if s_ == 1 else noise) for s_ in range(S)], 1)
    return (xs.astype(F32), tgt.astype(F32), mean, psi, sd, u, a64, np.full((B, 2), A * A / 2), omega)


def _run_rotating(xs, tgt, mean, psi, sd, u, lam, NB, sizes, timed):
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    em = ops.EnsembleModes(S, B, Cc, Hh, Ww, Tn, DEV, sd, u=u, channels=(0, 1), mean=torch.from_numpy(mean[:, :2]), basis=torch.from_numpy(psi))
    en = ops.EnsemblePhase(S, B, Cc, Hh, Ww, Tn, DEV, sd, u=u, modes=em, pair=(0, 1), bins=NB, mean=torch.from_numpy(mean),
                           lam=torch.from_numpy(lam))
    feed(en, xs, tgt, sizes, False, timed)
    got = {k: v.cpu().numpy() for k, v in en.finalize().items()}
    got.update(acc=en.acc.cpu().numpy(), tacc=en.tacc.cpu().numpy(), g=en.g.cpu().numpy(), craw=em.coef_raw.cpu().numpy(),
               tcraw=em.tcoef_raw.cpu().numpy())
    return got, em


def test_a_synthetic_rotating_pair_through_the_projection():
    import tmg_hip
    S, B, Tn, Cc, hw, NB = 5, 2, 16, 3, (12, 20), 8
    xs, tgt, mean, psi, sd, u, a64, lam, omega = _rotating(S, B, Tn, Cc, hw, 91, 0.05)
    timed = range(1, Tn)
    got, em = _run_rotating(xs, tgt, mean, psi, sd, u, lam, NB, P.chunk_sizes(S, 1), timed)
    what = "rotating pair"
    assert set(got) >= set(P.NEW_KEYS) | set(K.STEP_KEYS) | set(K.DERIVED_KEYS)
    lab, tlab = check_labels(got, got["craw"], got["tcraw"], lam, hw, NB, 0.25, (0, 1), what)
    assert (lab >= 0).all() and len(np.unique(tlab)) == NB                    # the cycle visits every sector, nothing is gated
    a = P.scales(sd.numpy(), u.numpy(), B, Cc)
    m32 = mean.astype(F32)
    ref, tref = P.reference(xs, lab, timed, a, m32, NB), P.reference(tgt[:, None], tlab[:, None], timed, a, m32, NB)
    worst = max(P.check_bound(got["acc"], ref, Cc, what), P.check_bound(got["tacc"], tref, Cc, what + " target"))
    der = P.derive(got, got["acc"], got["tacc"], Cc, hw, a[:, :, None, None] * m32.astype(np.float64), lam, (0, 1), timed)
    P.check_derived(got, der, what)
    # the constructed rate.  A normalised coefficient is off by at most dc = (cnt + 4) u sum a (|x| + |m|) |psi| / (HW sqrt(lam)): the
    # projection's counted roundings (tests/modes_cases.py) and one rounding each of x, m, psi and a to fp32; on the circle of radius
    # sqrt(2) a point that moves by at most sqrt(2) dc turns by at most asin(dc) <= 2 dc, and the mean increment is (last - first) / (T - 1)
    plan = tmg_hip.ens_pod_plan(S, B, 2, hw[0] * hw[1], 2)
    cnt = K.count(plan) + 4
    mag = np.abs(xs[:, :, :, :2]).astype(np.float64) + np.abs(m32[None, None, :, :2])
    dc = cnt * P.U24 * np.einsum("bc,tsbchw,bkchw->tsbk", a[:, :2], mag, np.abs(psi)).max() / (hw[0] * hw[1] * np.sqrt(lam.min()))
    tol = 2 * (2 * dc) / (len(timed) - 1) + P.U24 * omega
    assert abs(got["phase_speed"][:, 1] - omega).max() <= tol and abs(got["target_phase_speed"] - omega).max() <= tol, (tol, got["phase_speed"])
    assert abs(got["phase_speed"] - omega).max() <= 0.05                       # the noisy members turn at the same rate
    # organised motion dominates, and the members' coherent pattern is the target's shifted by less than a sector's worth of noise
    assert (got["target_coh_tke_frac"] > 0.9).all() and (got["coh_tke_frac"] > 0.5).all()
    print("%s: worst share of the bound %.4f; speed off by %.3g (tolerance %.3g)" % (what, worst, abs(got["phase_speed"][:, 1] - omega).max(), tol))


def test_the_target_fed_as_the_only_member_reproduces_the_target():
    B, Tn, Cc, hw, NB = 2, 16, 3, (12, 20), 8
    xs, tgt, mean, psi, sd, u, a64, lam, omega = _rotating(1, B, Tn, Cc, hw, 92, 0.0)
    xs = np.ascontiguousarray(tgt[:, None])
    got, _ = _run_rotating(xs, tgt, mean, psi, sd, u, lam, NB, [1], range(Tn))
    assert np.array_equal(got["phase_bin"][:, 0], got["target_phase_bin"]) and np.array_equal(got["acc"], got["tacc"])
    for key in P.FIELD_KEYS:
        assert np.array_equal(got[key], got["target_" + key], equal_nan=True), key
    assert not np.isnan(got["phase_mean"]).any()
    assert (got["coh_corr"] == 1.0).all() and not got["phase_mean_rmse"].any()
    assert np.array_equal(got["phase_speed"][:, 0], got["target_phase_speed"])


# ---- 6: end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_phase_matches_the_reference_over_model_pred(monkeypatch, tmp_path, case):
    """Same seed: modelPredPhase returns modelPredModes' keys with equal values plus exactly the new keys.  The reference forms
    d = p - mean from modelPred's un-normalised samples p and the target's physical time mean, groups the rows by the RETURNED labels
    and sums directly.  As in test_modes_gpu, modelPred un-normalises in fp32 (an error of at most u (3 |p| + |u0 mu|)), the kernel's
    mean plane and the physical mean are each rounded once and the scale a once, so the reference's d is uncertain by
    e = u (3 |p| + 2 |u0 mu| + 2 |mean| + |d|).  With D = sum d / n, a phase mean may differ by
      bm = ((n + 3) u sum |d| + sum e) / n + u |phase_mean|                          (the counted bound, e, the output's rounding)
    and the second moments by bq = ((n + 6) u sum |d d'| + sum (|d| e' + |d'| e + e e')) / n, so that
      phase_var, phase_uv:  bq + (|D| bm' + |D'| bm + bm bm') + u |ref|."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows, Kk, chs, NB, min_amp = 5, 5, 1, 1, 4, 3, (0, 1), 4, 0.0
    thr = 2 * min_amp * min_amp                                              # (the tiny models' members stay near the target's mean: no gate)
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    for _ in range(2):                                                        # two folded runs: modelPredPhase, modelPredModes
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    for bi, B in enumerate(batches):
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    kw = dict(samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows, modes=Kk, channels=chs)
    torch.manual_seed(77)
    got = utils.modelPredPhase(args, model, te, E.LOG, pair=(0, 1), bins=NB, min_amp=min_amp, **kw)
    torch.manual_seed(77)
    modes = utils.modelPredModes(args, model, te, E.LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(modes) | set(P.NEW_KEYS)
    for name, v in modes.items():
        assert torch.equal(got[name], v), name
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    timed = range(t_start, Tk)
    assert g["phase_bin"].shape == (N, S, Tk) and g["target_phase_bin"].shape == (N, Tk) and g["phase_edges"].shape == (NB + 1,)
    assert np.array_equal(g["phase_edges"], 2 * np.pi * np.arange(NB + 1) / NB)
    # the labels: the sector of the returned coefficients' angle, wherever that is clear of an edge and of the gate
    lam = g["pod_energy"][:, :2]
    for lab, coef in ((g["phase_bin"], g["coef"].astype(np.float64)), (g["target_phase_bin"], g["target_coef"].astype(np.float64))):
        sl = np.sqrt(lam).reshape((N,) + (1,) * (coef.ndim - 2) + (2,))
        x, yy = coef[..., 0] / sl[..., 0], coef[..., 1] / sl[..., 1]
        r2, th = x * x + yy * yy, np.mod(np.arctan2(yy, x), 2 * np.pi) / (2 * np.pi / NB)
        clear = (np.abs(th - np.round(th)) > 1e-4) & (np.abs(r2 - thr) > 1e-5)
        assert clear.mean() > 0.9
        assert np.array_equal(lab[clear], np.where(r2 < thr, -1, P.label_atan2(x, yy, NB))[clear])
    # the fields against modelPred's samples grouped by the returned labels
    mean = y[:, t_start:].mean(1)                                            # [N, C, H, W], physical
    xs = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5))                 # [Tk, S, N, C, H, W]
    ys = np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))[:, None]           # [Tk, 1, N, C, H, W]
    ones = np.ones((N, Cc))
    uc = np.stack([u0, u0, u0 ** 2], 1)                                      # [N, C]
    umu = np.abs(uc * mu[:Cc].reshape(1, Cc)).reshape(N, Cc, 1, 1)
    worst = 0.0
    for pre, rows, lab in (("", xs, g["phase_bin"]), ("target_", ys, g["target_phase_bin"][:, None])):
        ref = P.reference(rows, lab, timed, ones, mean, NB)
        d = np.abs(rows - mean[None, None])
        e = P.U24 * (3 * np.abs(rows) + 2 * umu[None, None] + 2 * np.abs(mean)[None, None] + d)
        e_ref = P.reference(e + mean[None, None], lab, timed, ones, mean, NB)           # sums of e over the same rows (linear planes)
        HW = Hh * Ww
        dd, ee = d.reshape(d.shape[:4] + (HW,)), e.reshape(e.shape[:4] + (HW,))
        n = ref["n"].astype(np.float64)[:, :, None, None]
        has = ref["n"] > 0
        assert np.array_equal(ref["n"], g[pre + "phase_count"]) and has.any()
        nn = np.where(n > 0, n, 1.0)
        D = ref["raw"][:, :, :Cc] / nn
        se = e_ref["raw"][:, :, :Cc]
        bm = ((n + P.C_ROUND_LIN) * P.U24 * ref["abs"][:, :, :Cc] + se) / nn
        f = P.fields(ref["n"], ref["raw"], Cc)
        pm = (mean.reshape(N, 1, Cc, HW) + f["dev"])
        bm_out = bm + P.U24 * np.abs(np.where(has[:, :, None, None], pm, 0.0))
        # sum (|d| e' + |d'| e + e e') per product plane, by the same masks
        on = np.zeros(len(rows), dtype=bool)
        on[list(timed)] = True
        sq = np.zeros((N, NB, Cc + 1, HW))
        for b in range(N):
            for k in range(NB):
                mask = (lab[b].T == k) & on[:, None]
                db, eb = dd[:, :, b][mask], ee[:, :, b][mask]                # [rows, C, HW]
                sq[b, k, :Cc] = (2 * db * eb + eb * eb).sum(0)
                sq[b, k, Cc] = (db[:, 0] * eb[:, 1] + db[:, 1] * eb[:, 0] + eb[:, 0] * eb[:, 1]).sum(0)
        bq = ((n + P.C_ROUND_PROD) * P.U24 * ref["abs"][:, :, Cc:] + sq) / nn
        aD = np.abs(D)
        bvar = bq[:, :, :Cc] + 2 * aD * bm + bm * bm
        buv = bq[:, :, Cc] + aD[:, :, 0] * bm[:, :, 1] + aD[:, :, 1] * bm[:, :, 0] + bm[:, :, 0] * bm[:, :, 1]
        for name, r, bnd in (("phase_mean", pm, bm_out), ("phase_var", f["var"], bvar), ("phase_uv", f["uv"], buv)):
            gv = g[pre + name].astype(np.float64).reshape(r.shape)
            fin = np.isfinite(r)
            assert np.array_equal(np.isfinite(gv), fin), pre + name
            bnd = bnd + P.U24 * np.abs(np.where(fin, r, 0.0)) + 2.0 ** -40
            err = np.abs(gv - r)[fin]
            share = float((err / bnd[fin]).max())
            assert share <= 1.0, "%s%s: worst error is %.3g of its bound" % (pre, name, share)
            worst = max(worst, share)
    # the aggregates are the formulas of tests/phase_cases.py applied to the RETURNED phase fields and counts, which are rounded to fp32:
    # M_k is off by u |M_k|, so coh_k by 2 u max |M| and, with |coh_k| <= 2 max |M|, its square by 8 u max |M|^2, doubled for the output's
    # own rounding and the second order; a weighted mean of the phase_var_k by u max |var| twice; the fraction of two sums of terms
    # that are each u-accurate by 4 u, doubled
    for pre in ("", "target_"):
        n = g[pre + "phase_count"].astype(np.float64)
        assert (g[pre + "phase_skipped"] + n.sum(1) == (S if pre == "" else 1) * len(timed)).all()
        w = (n / n.sum(1, keepdims=True))[:, :, None, None, None]
        M = np.where(np.isfinite(g[pre + "phase_mean"]), g[pre + "phase_mean"], 0.0).astype(np.float64)
        V = np.where(np.isfinite(g[pre + "phase_var"]), g[pre + "phase_var"], 0.0).astype(np.float64)
        coh = M - (w * M).sum(1, keepdims=True)
        assert np.abs((w * coh * coh).sum(1) - g[pre + "coh_var"]).max() <= 16 * P.U24 * np.abs(M).max() ** 2
        assert np.abs((w * V).sum(1) - g[pre + "incoh_var"]).max() <= 4 * P.U24 * np.abs(V).max()
        cv, iv = g[pre + "coh_var"].astype(np.float64)[:, :2].sum((1, 2, 3)), g[pre + "incoh_var"].astype(np.float64)[:, :2].sum((1, 2, 3))
        assert np.abs(cv / (cv + iv) - g[pre + "coh_tke_frac"]).max() <= 8 * P.U24
    assert np.isfinite(g["phase_speed"]).all() and (np.abs(g["phase_speed"]) <= np.pi).all()
    print("%s: worst share of the bound %.4f" % (case, worst))
