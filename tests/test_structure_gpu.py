"""Ensemble structure functions and variogram score on the device (`-m gpu`): tmg_ens_score_store / tmg_ens_sfun_step through
tmg_ops.EnsembleStructure against the fp64 / int64 reference of tests/structure_cases.py (direct slicing of the field), and
utils.modelPredStructure against the same reference over modelPred's samples.  The definitions, the rounding counts
cnt = Lc + P + k_q (k_2, k_3, k_4 = 4, 6, 8), the variogram's bound and the physical outputs' bounds are in tests/structure_cases.py; Lc
and P come from tmg_hip.ens_sfun_plan for the case.

Integer mode, a = 1: `small` (integers in -3..3) makes every moment sum exact in fp32, `binary` (values in {0, 1}) also the variogram
sum when S is a power of two: mom, vsum, tmom and tvar must EQUAL the int64 reference after every step.  Every case runs with xs, the
workspace, mom, vsum, tmom and tvar pre-filled with NaN.

Worst share of a bound reached on an MI355X (the tests print it; LAB_NOTES.md): 0.076 integer, 0.284 real data (the raw sums alone:
0.284), 0.057 end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import structure_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32


def run_structure(xs, tgt, lags, sizes, padded, t_start, sd=None, u=None, weights=None, grid=(1.0, 1.0)):
    """Feed EnsembleStructure as utils.modelPredStructure does, in chunks of `sizes` members per step; padded: y and target are channel
    slices of wider NaN-filled NHWC buffers.  Every buffer the kernels write is pre-filled with NaN.  -> dict of numpy arrays: the
    outputs, the raw buffers mom / vsum, their planes read right after their step (mom_steps, vsum_steps) and tmom / tvar after
    every step (tmom_steps, tvar_steps); and the launch plan."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    xd = torch.from_numpy(xs).to(DEV)
    td = torch.from_numpy(tgt).to(DEV)

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), float("nan"), device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    en = ops.EnsembleStructure(S, B, Cc, Hh, Ww, Tn, DEV, torch.ones(Cc) if sd is None else sd, u=u, lags=lags, weights=weights, grid=grid)
    for v in (en.xs, en.ws, en.mom, en.vsum, en.tmom, en.tvar):
        v.fill_(float("nan"))
    keep = {k: [] for k in ("mom_steps", "vsum_steps", "tmom_steps", "tvar_steps")}
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
        assert bool(torch.isnan(en.mom[t + 1:]).all()) and bool(torch.isnan(en.vsum[t + 1:]).all())       # a step writes its own plane
        for name, v in (("mom_steps", en.mom[t]), ("vsum_steps", en.vsum[t]), ("tmom_steps", en.tmom), ("tvar_steps", en.tvar)):
            keep[name].append(v.cpu().numpy().copy())
    got = {k: v.cpu().numpy() for k, v in en.finalize().items()}
    for k, v in got.items():
        assert not np.isnan(v).any(), "%s holds NaN" % k
    got.update({k: np.stack(v) for k, v in keep.items()})
    got["mom"], got["vsum"] = en.mom.cpu().numpy(), en.vsum.cpu().numpy()
    assert np.array_equal(got["mom"], got["mom_steps"]) and np.array_equal(got["vsum"], got["vsum_steps"])   # no later step touched them
    return got, en.plan


def expected_shapes(got, S, B, Tn, Cc, L):
    for k in K.SF_KEYS:
        assert got[k].shape == (B, Tn, Cc, L, S + 1) and got["time_" + k].shape == (B, Cc, L, S + 1), k
    for k in ("sf2_mean", "sf2_std", "vario_lag"):
        assert got[k].shape == (B, Tn, Cc, L), k
    assert got["vario_score"].shape == (B, Tn, Cc) and got["time_vario_lag"].shape == (B, Cc, L) and got["time_vario_score"].shape == (B, Cc)
    assert got["time_skew"].shape == got["time_flat"].shape == (B, Cc, L, S + 1)
    assert got["lags"].shape == (L, 2) and got["lags"].dtype == np.int64 and got["lag_dist"].shape == (L,) and got["lag_dist"].dtype == np.float64


# ---- integer mode: equality on every edge of the launch plan ---------------------------------------------------------------------------
def _integer_case(case, idx):
    mode, S, B, Cc, hw, t_start, kind, padded = case
    steps = 2 if case is K.LONG_CASE else K.T
    t_start = min(t_start, steps - 1)
    lags = K.LAGS[hw]
    xs, tgt = K.int_inputs(mode, S, B, Cc, hw, 7000 + idx, steps)
    got, plan = run_structure(xs, tgt, lags, K.chunk_sizes(S, kind), padded, t_start)
    a, w, N = K.scales(None, None, B, Cc), [1.0] * len(lags), K.pair_counts(lags, hw)
    ref = K.reference(xs, tgt, lags, integer=True)
    what = "integer %s" % (case,)
    expected_shapes(got, S, B, steps, Cc, len(lags))
    assert np.array_equal(got["lags"], np.array(lags)) and np.array_equal(got["lag_dist"], [float(np.hypot(dx, dy)) for dx, dy in lags])
    vex = K.check_integer(got, ref, mode, S, t_start, what)
    phys = K.derive(ref["mom"], ref["vsum"], a, w, N, t_start, S)
    worst, cnt = K.check(got, ref, phys, K.bounds(ref, phys, plan, a, w, N, t_start, S), t_start, what)
    print("%s: plan P=%d SL=%d Lc=%d; variogram compared for equality: %s; worst share of a bound %.4f" % (what, plan["P"], plan["SL"], plan["Lc"], vex, worst))
    return plan, vex


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE)))
def test_integer_data_gives_the_integer_reference_bit_for_bit(idx):
    mode, S = K.INT_TABLE[idx][:2]
    _, vex = _integer_case(K.INT_TABLE[idx], idx)
    assert vex == (mode == "binary" and S & (S - 1) == 0)                     # binary and a power of two of members: the variogram too


def test_integer_data_with_three_pixels_per_thread():
    plan, vex = _integer_case(K.LONG_CASE, len(K.INT_TABLE))
    assert plan["SL"] == 768 and plan["P"] == 44 and vex


# ---- Gaussian, smooth and biased members with a real normalisation ---------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_real_data_stays_in_the_rounding_bounds(idx):
    S, B, Cc, hw, kind, with_u = K.REAL_TABLE[idx]
    lags = K.LAGS[hw]
    xs, tgt = K.real_inputs(S, B, Cc, hw, kind, 8000 + idx)
    sd = torch.tensor(K.SD[:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))) if with_u else None
    t_start = idx % 2
    wts = K.weights_of(len(lags))
    got, plan = run_structure(xs, tgt, lags, K.chunk_sizes(S, idx % 3), idx % 2 == 0, t_start, sd=sd, u=u, weights=wts, grid=K.GRID)
    a, N = K.scales(sd.numpy(), None if u is None else u.numpy(), B, Cc), K.pair_counts(lags, hw)
    ref = K.reference(xs, tgt, lags)
    phys = K.derive(ref["mom"], ref["vsum"], a, wts, N, t_start, S)
    bnd = K.bounds(ref, phys, plan, a, wts, N, t_start, S)
    what = "%s %s" % (kind, K.REAL_TABLE[idx][:4])
    expected_shapes(got, S, B, K.T, Cc, len(lags))
    assert np.array_equal(got["lag_dist"], [float(np.hypot(dx * K.GRID[0], dy * K.GRID[1])) for dx, dy in lags])
    worst, cnt = K.check(got, ref, phys, bnd, t_start, what)
    raw = max(float((np.abs(got[n].astype(np.float64) - ref[n]) / np.maximum(bnd[n], 1e-300)).max()) for n in K.RAW_KEYS)
    print("%s: Lc = %d, P = %d; worst share of a bound %.4f (raw sums %.4f); %d skewness / flatness entries compared"
          % (what, plan["Lc"], plan["P"], worst, raw, cnt))
    assert cnt == B * Cc * len(lags) * (S + 1)                                # every entry of the table qualifies


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,Cc,hw", [(5, 3, 3, (16, 33)), (17, 1, 4, (16, 17)), (7, 3, 2, (50, 58))])
def test_outputs_are_bitwise_the_same_for_every_feed_and_run(S, B, Cc, hw):
    xs, tgt = K.real_inputs(S, B, Cc, hw, "gauss", 43)
    sd = torch.tensor(K.SD[:Cc])
    u = 0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(3))
    outs = [run_structure(xs, tgt, K.LAGS[hw], K.chunk_sizes(S, kind), padded, 1, sd=sd, u=u)[0]
            for kind, padded in ((0, False), (1, True), (2, False), (2, False))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name


def test_a_target_equal_to_every_member_scores_zero_and_shares_their_moments():
    S, B, Cc, hw = 5, 3, 3, (16, 17)
    xs, tgt = K.real_inputs(S, B, Cc, hw, "gauss", 44)
    same = np.ascontiguousarray(np.broadcast_to(tgt[:, None], xs.shape))
    got, _ = run_structure(same, tgt, K.LAGS[hw], K.chunk_sizes(S, 1), True, 0, sd=torch.tensor(K.SD[:Cc]))
    assert np.array_equal(got["mom"][..., :S], np.broadcast_to(got["mom"][..., S:], got["mom"][..., :S].shape))   # the same bits in every row
    assert np.array_equal(got["sf2"][..., 0], got["sf2"][..., S])
    # sf2_std is formed in fp64 from S equal numbers: their mean is off by at most S 2^-53 of them, and so is every deviation
    assert bool((got["sf2_std"] <= 2.0 ** -50 * got["sf2_mean"]).all())
    # sbar = (S s) fl(1 / S) is s up to S + 1 roundings: the score is a few u^2 of sum |D|, never a visible number
    assert float(got["vario_score"].max()) <= ((S + 4) * K.U24) ** 2 * 4 * float(np.abs(tgt).max()) * 2.5 * len(K.LAGS[hw]) * 3


def test_shuffling_the_members_per_pixel_moves_the_structure_functions_and_the_variogram_score():
    """The discriminating case: every member its own smooth field (a double cumulative sum), the target another one.  Permuting the
    members independently at every pixel leaves every pixel's set of member values, hence every per-pixel score's input, unchanged;
    the increments of a 'member' become differences between different fields."""
    S, B, Cc, hw = 16, 1, 3, (16, 33)
    lags = ((1, 0), (0, 1), (2, 2))
    g = torch.Generator().manual_seed(45)
    fld = lambda *s: (0.05 * torch.randn(*s, *hw, generator=g)).cumsum(-2).cumsum(-1)     # noqa: E731
    xs, tgt = fld(K.T, S, B, Cc).numpy().astype(F32), fld(K.T, B, Cc).numpy().astype(F32)
    perm = torch.rand(K.T, S, B, Cc, *hw, generator=g).argsort(1).numpy()
    shuf = np.take_along_axis(xs, perm, 1)
    assert np.array_equal(np.sort(xs, 1), np.sort(shuf, 1)) and not np.array_equal(xs, shuf)     # the per-pixel inputs are the same
    sd = torch.tensor(K.SD[:Cc])
    a, w, N = K.scales(sd.numpy(), None, B, Cc), [1.0] * len(lags), K.pair_counts(lags, hw)
    res = []
    for data in (xs, shuf):
        got, plan = run_structure(data, tgt, lags, [S], False, 0, sd=sd)
        ref = K.reference(data, tgt, lags)
        phys = K.derive(ref["mom"], ref["vsum"], a, w, N, 0, S)
        bnd = K.bounds(ref, phys, plan, a, w, N, 0, S)
        K.check(got, ref, phys, bnd, 0, "shuffle test")
        res.append((got, bnd))
    (g0, b0), (g1, b1) = res
    for name in ("vario_score", "sf2_mean"):
        moved = np.abs(g1[name].astype(np.float64) - g0[name]) - (b0[name] + b1[name])
        assert bool((moved > 0).all()), name
    assert bool((g1["sf2_mean"][..., 0] > 4 * g0["sf2_mean"][..., 0]).all())  # lag (1, 0): shuffling a smooth ensemble raises sf2
    assert bool((g1["sf2"][..., 0, :S] > g0["sf2"][..., 0, :S].max(-1, keepdims=True)).all())
    assert np.array_equal(g1["sf2"][..., S], g0["sf2"][..., S])               # the target's own row does not know the members
    print("shuffled / smooth: sf2_mean at lag (1, 0) x%.1f, vario_score x%.2f" % (float((g1["sf2_mean"][..., 0] / g0["sf2_mean"][..., 0]).min()),
                                                                                 float((g1["vario_score"] / g0["vario_score"]).mean())))


# ---- end to end: modelPredStructure against the reference over modelPred's samples --------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_structure_matches_the_reference_over_model_pred(monkeypatch, tmp_path, case):
    """modelPred un-normalises every member and the target in fp32, xh = fl(u fl(fl(sd x) + mu)): three roundings, together at most
    3 u a (|x| + |mu| / sd).  The normalised members recovered from its samples in fp64 are therefore known to eps_x = 3 u (max |x|
    + |mu| / sd) and every increment to eps = 2 eps_x, which the reference takes as its own uncertainty (structure_cases.reference)."""
    import tmg_hip
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    lags = ((1, 0), (0, 1), (3, -2), (8, 0), (0, 8))
    wts = K.weights_of(len(lags))
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=K.GRID[0], dy=K.GRID[1])
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    for _ in range(2):                                                        # two folded runs: modelPredStructure, modelPredStats
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
    got = utils.modelPredStructure(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows,
                                   lags=lags, weights=wts)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    new = set(K.STEP_KEYS + K.TIME_KEYS) | {"lags", "lag_dist"}
    assert set(got) == set(stats) | new
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N_, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    xs, ys = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5)), np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]                              # [N, C]
    nrm = lambda v: (v / uc.reshape(N_, Cc, 1, 1) - mu[:Cc].reshape(1, Cc, 1, 1)) / sd[:Cc].reshape(1, Cc, 1, 1)   # noqa: E731
    xn, yn = nrm(xs), nrm(ys)
    eps = 2 * 3 * K.U24 * (max(float(np.abs(xn).max()), float(np.abs(yn).max())) + np.abs(mu[:Cc]) / sd[:Cc]).reshape(1, 1, Cc, 1, 1, 1)
    ref = K.reference(xn, yn, lags, eps=eps)
    a = uc * sd[:Cc].reshape(1, Cc)
    cnt_n = K.pair_counts(lags, (Hh, Ww))
    plans = [tmg_hip.ens_sfun_plan(S, B, Cc, Hh, Ww, lags) for B in batches]
    plan = {"Lc": max(q["Lc"] for q in plans), "P": max(q["P"] for q in plans)}
    phys = K.derive(ref["mom"], ref["vsum"], a, wts, cnt_n, t_start, S)
    bnd = K.bounds(ref, phys, plan, a, wts, cnt_n, t_start, S)
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    expected_shapes(g, S, N_, Tk, Cc, len(lags))
    assert np.array_equal(g["lags"], np.array(lags))
    assert np.array_equal(g["lag_dist"], [float(np.hypot(dx * K.GRID[0], dy * K.GRID[1])) for dx, dy in lags])
    worst, n_cmp = 0.0, int(bnd["qualifies"].sum())
    for name in K.STEP_KEYS + K.TIME_KEYS:
        assert g[name].dtype == F32, name
        err = np.abs(g[name].astype(np.float64) - phys[name])
        share = np.where(err > 0, err / np.maximum(bnd[name], 1e-300), 0.0)
        if name in ("time_skew", "time_flat"):
            share = np.where(bnd["qualifies"], share, 0.0)
        assert float(share.max()) <= 1.0, "%s %s: worst error is %.3g of its bound" % (case, name, float(share.max()))
        worst = max(worst, float(share.max()))
    assert n_cmp == bnd["qualifies"].size                                    # every skewness / flatness entry was compared
    print("%s: Lc = %d, P = %d; worst share of a bound %.4f; %d skewness / flatness entries compared" % (case, plan["Lc"], plan["P"], worst, n_cmp))
