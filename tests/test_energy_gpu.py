"""Ensemble energy score and member distances on the device (`-m gpu`): tmg_ens_score_store / tmg_ens_gram_step / tmg_ens_gram_traj
through tmg_ops.EnsembleEnergy against the fp64 reference of tests/energy_cases.py (direct differences, never a Gram matrix), and
utils.modelPredEnergy against the same reference over modelPred's samples.  The definitions, the rounding count cnt = L + P + 10 and
the bounds are in tests/energy_cases.py; L and P come from tmg_hip.ens_gram_plan for the case.

Integer mode: small integer data whose pixel sums over the members are divisible by S, a = 1: every product and partial sum is
exact in fp32, so the mean plane, d2 and traj_dist2 must EQUAL the integer reference.  Every case runs with xs, the mean plane, the
workspace, traj_dist2 and the outputs pre-filled with NaN.

Worst share of the bound reached on an MI355X (the tests print it; LAB_NOTES.md): 0.0036 integer, 0.017 real data, 0.0064 end to end."""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import energy_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32


def run_energy(xs, tgt, sizes, padded, t_start, sd=None, u=None, groups=None):
    """Feed EnsembleEnergy as utils.modelPredEnergy does, in chunks of `sizes` members per step; padded: y and target are channel slices
    of wider NaN-filled NHWC buffers.  Every buffer the kernels write is pre-filled with NaN.  -> dict of numpy arrays, with the mean
    plane r [T, B, C, HW] and traj_dist2 after every step (traj_steps [T, B, Gn, R, R]), and the launch plan."""
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

    en = ops.EnsembleEnergy(S, B, Cc, Hh, Ww, Tn, DEV, torch.ones(Cc) if sd is None else sd, u=u, groups=groups)
    for v in (en.xs, en.r, en.ws, en.traj, en.outf):
        v.fill_(float("nan"))
    en.outi.fill_(-1)
    rs, steps = [], []
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
        rs.append(en.r.cpu().numpy().copy())
        steps.append(en.traj.cpu().numpy().copy())
    got = {k: v.cpu().numpy() for k, v in en.finalize().items()}
    for k, v in got.items():
        assert not np.isnan(v).any(), "%s holds NaN" % k
    got["r"], got["traj_steps"] = np.stack(rs), np.stack(steps)
    return got, en.plan


def expected_shapes(got, S, B, Tn, Gn):
    for k in K.STEP_KEYS + ("medoid", "nearest"):
        assert got[k].shape == (B, Tn, Gn), k
    for k in K.TRAJ_KEYS + ("time_energy_score", "time_energy_score_fair", "traj_medoid", "traj_nearest"):
        assert got[k].shape == (B, Gn), k
    assert got["traj_dist2"].shape == (B, Gn, S + 1, S + 1)


# ---- integer mode: equality on every edge of the launch plan ---------------------------------------------------------------------------
def _integer_case(case, idx, steps=K.T):
    S, B, Cc, hw, groups, t_start, kind, padded = case
    t_start = min(t_start, steps - 1)
    xs, tgt, k = K.int_inputs(S, B, Cc, hw, 5000 + idx, steps)
    got, plan = run_energy(xs, tgt, K.chunk_sizes(S, kind), padded, t_start, groups=groups)
    a, _ = K.scales(None, None, B, Cc)
    ref = K.reference(xs, tgt, a, groups, t_start, integer=True)
    what = "integer %s" % (case,)
    expected_shapes(got, S, B, steps, len(groups))
    K.check_integer(got, ref, k, t_start, what)
    bnd = K.bounds(xs, tgt, got["r"], a, groups, plan, ref, t_start)
    worst = K.check(got, ref, bnd, S, t_start, what)
    print("%s: plan P=%d L=%d pairs=%d; the scores' worst share of their bound %.4f" % (what, plan["P"], plan["L"], len(plan["pairs"]), worst))
    return plan


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE)))
def test_integer_data_gives_the_integer_reference_bit_for_bit(idx):
    _integer_case(K.INT_TABLE[idx], idx)


def test_integer_data_with_two_chunks_per_wave():
    plan = _integer_case(K.LONG_CASE, 100, steps=1)
    assert plan["SL"] == 512 and plan["P"] == 6 and len(plan["pairs"]) == 6


def test_integer_data_at_the_largest_member_count():
    plan = _integer_case(K.MAX_CASE, 101, steps=2)
    assert plan["NT"] == 17 and len(plan["pairs"]) == 153


# ---- Gaussian, biased and nearly equal members with a real normalisation ---------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_real_data_stays_in_the_rounding_bound(idx):
    S, B, Cc, hw, groups, kind, with_u = K.REAL_TABLE[idx]
    xs, tgt = K.real_inputs(S, B, Cc, hw, kind, 6000 + idx)
    sd = torch.tensor(K.SD[:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))) if with_u else None
    t_start = idx % 2
    got, plan = run_energy(xs, tgt, K.chunk_sizes(S, idx % 3), idx % 2 == 0, t_start, sd=sd, u=u, groups=groups)
    a, _ = K.scales(sd.numpy(), None if u is None else u.numpy(), B, Cc)
    ref = K.reference(xs, tgt, a, groups, t_start)
    bnd = K.bounds(xs, tgt, got["r"], a, groups, plan, ref, t_start)
    what = "%s %s" % (kind, K.REAL_TABLE[idx][:4])
    # the mean plane is the sequential fp32 sum times fl(1 / S): S roundings on a sum of at most sum |x|
    x64 = xs.astype(np.float64)
    rerr = np.abs(got["r"].astype(np.float64).reshape(x64[:, 0].shape) - x64.mean(1))
    assert bool((rerr <= (S + 1) * K.U24 * np.abs(x64).sum(1) / S).all()), "%s mean plane" % what
    worst = K.check(got, ref, bnd, S, t_start, what)
    print("%s: cnt = %d + %d + %d; worst share of the bound %.4f" % (what, plan["L"], plan["P"], K.C_ROUND, worst))


# ---- the bits of the commit before the Gram engine moved to csrc/tmg_symgram.h ----------------------------------------------------------
# The code promises the same bits for the same inputs and has no float atomics, so the outputs of these cases are pinned by their
# SHA-256 (tests/golden/symgram_bits.json, written by tests/golden/make_symgram_golden.py on an MI355X from the commit before).  Rows of
# REAL_TABLE run as the test above runs them, and the 70-member case of the feed test as row 8: between them the one-tile instance,
# NT = 1 with four tiles, the off-diagonal instance, P = 1 and P > 1, float4 and scalar loads and HW that is no multiple of 16
# (tests/test_symgram_cpu.py asserts that coverage from the recorded plans).
BITS = os.path.join(C.GOLDEN, "symgram_bits.json")
BITS_ROWS = [K.REAL_TABLE[i] + (i,) for i in (0, 2, 3, 4, 5, 7)] + [(70, 3, 2, K.HWS[65], K.G2, "gauss", True, 8)]


def bits_name(row):
    return "S%d_B%d_C%d_hw%d_%s" % (row[0], row[1], row[2], row[3][0] * row[3][1], row[5])


def energy_bits(S, B, Cc, hw, groups, kind, with_u, idx):
    """-> (name -> SHA-256 of every output array: the scores of outf, the argmins of outi, traj_dist2 after every step and the mean
    plane; what the plan says of the engine's branches)."""
    xs, tgt = K.real_inputs(S, B, Cc, hw, kind, 6000 + idx)
    sd = torch.tensor(K.SD[:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))) if with_u else None
    got, plan = run_energy(xs, tgt, K.chunk_sizes(S, idx % 3), idx % 2 == 0, idx % 2, sd=sd, u=u, groups=groups)
    HW = hw[0] * hw[1]
    return ({k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(got.items())},
            {"part": plan["part"], "NT": plan["NT"], "P": plan["P"], "vec": HW % 4 == 0, "HW": HW, "Cg": 1})


@pytest.mark.parametrize("row", BITS_ROWS, ids=bits_name)
def test_real_data_gives_the_bits_of_the_commit_before_the_shared_engine(row):
    gold = json.load(open(BITS))["gram"][bits_name(row)]
    sha, plan = energy_bits(*row)
    assert plan == gold["plan"]
    assert set(sha) == set(gold["sha256"])
    assert sha == gold["sha256"], [k for k in sha if sha[k] != gold["sha256"][k]]


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
def test_one_member_scores_its_distance_to_the_target():
    S, B, Cc, hw = 1, 3, 3, K.HWS[272]
    xs, tgt = K.real_inputs(S, B, Cc, hw, "gauss", 41)
    got, _ = run_energy(xs, tgt, [1], False, 0, sd=torch.tensor(K.SD[:Cc]), groups=K.G3)
    assert np.array_equal(got["energy_score"], got["energy_score_fair"]) and np.array_equal(got["energy_score"], got["nearest_dist"])
    assert np.array_equal(got["energy_score"], got["target_dist_mean"]) and not got["pair_dist_mean"].any()
    assert not got["medoid"].any() and not got["nearest"].any()
    assert np.array_equal(got["traj_energy_score"], np.sqrt(got["traj_dist2"][:, :, 0, 1]))


@pytest.mark.parametrize("S,hw", [(9, K.HWS[272]), (70, K.HWS[65])])
def test_equal_members_have_no_spread_and_an_equal_target_is_the_nearest(S, hw):
    B, Cc = 3, 3
    xs, tgt = K.real_inputs(S, B, Cc, hw, "biased", 42 + S)
    same = np.ascontiguousarray(np.broadcast_to(xs[:, :1], xs.shape))
    got, _ = run_energy(same, tgt, K.chunk_sizes(S, 1), True, 0, sd=torch.tensor(K.SD[:Cc]), groups=K.G3)
    assert not got["pair_dist_mean"].any() and not got["traj_dist2"][:, :, :S, :S].any()        # 0.0 exactly
    assert np.array_equal(got["energy_score"], got["target_dist_mean"]) and not got["medoid"].any() and not got["nearest"].any()
    twin = xs.copy()
    lo, hi = S // 3, S - 2                                                   # (S = 70: two different macro-tiles)
    twin[:, lo] = tgt
    twin[:, hi] = tgt
    got, _ = run_energy(twin, tgt, K.chunk_sizes(S, 2), False, 0, sd=torch.tensor(K.SD[:Cc]), groups=K.G3)
    assert bool((got["nearest"] == lo).all()) and not got["nearest_dist"].any() and bool((got["traj_nearest"] == lo).all())
    assert not got["traj_dist2"][:, :, lo, hi].any() and not got["traj_dist2"][:, :, lo, S].any()


@pytest.mark.parametrize("S,B,Cc,hw", [(7, 3, 3, K.HWS[272]), (33, 1, 4, K.HWS[528]), (70, 3, 2, K.HWS[65])])
def test_outputs_are_bitwise_the_same_for_every_feed_and_run(S, B, Cc, hw):
    xs, tgt = K.real_inputs(S, B, Cc, hw, "gauss", 43)
    sd = torch.tensor(K.SD[:Cc])
    u = 0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(3))
    outs = [run_energy(xs, tgt, K.chunk_sizes(S, kind), padded, 1, sd=sd, u=u)[0]
            for kind, padded in ((0, False), (1, True), (2, False), (2, False))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name


# ---- end to end: modelPredEnergy against the reference over modelPred's samples -----------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_energy_matches_the_reference_over_model_pred(monkeypatch, tmp_path, case):
    """modelPred un-normalises every member and the target in fp32 (product, sum, product: 3 roundings, each <= u |xh|), so the
    reference distance itself is uncertain by the norm of those errors, <= 3 u (|xh_m|_g + |xh_n|_g), which is added to every
    distance's bound; the mean plane is the fp64 mean of the recovered normalised members, known to (S + 1) u max |x|."""
    import tmg_hip
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    groups = ((0, 1), (2,))
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    for _ in range(2):                                                        # two folded runs: modelPredEnergy, modelPredStats
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
    got = utils.modelPredEnergy(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows, groups=groups)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    new = set(K.STEP_KEYS + K.TRAJ_KEYS) | {"medoid", "nearest", "traj_medoid", "traj_nearest", "traj_dist2", "time_energy_score",
                                            "time_energy_score_fair", "energy_groups"}
    assert set(got) == set(stats) | new and got["energy_groups"] == groups
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    xs, ys = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5)), np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))
    ones = np.ones((N, Cc))
    ref = K.reference(xs, ys, ones, groups, t_start)
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]                              # [N, C]
    nrm = lambda v: (v / uc.reshape(N, Cc, 1, 1) - mu[:Cc].reshape(1, Cc, 1, 1)) / sd[:Cc].reshape(1, Cc, 1, 1)   # noqa: E731
    xn, yn = nrm(xs), nrm(ys)
    plans = [tmg_hip.ens_gram_plan(S, B, Cc, Hh * Ww) for B in batches]
    plan = {"L": max(q["L"] for q in plans), "P": max(q["P"] for q in plans)}
    rows = K.rows_of(xs, ys).numpy()                                         # [Tk, N, C, R, HW]
    norms = np.stack([np.sqrt(sum((rows[:, :, c] ** 2).sum(-1) for c in g)) for g in groups], 2)          # [Tk, N, Gn, R]
    extra = 3 * K.U24 * (norms[..., :, None] + norms[..., None, :])
    bnd = K.bounds(xn, yn, xn.mean(1).reshape(Tk, N, Cc, -1), uc * sd[:Cc].reshape(1, Cc), groups, plan, ref, t_start,
                   r_slack=(S + 1) * K.U24 * float(np.abs(xn).max()), extra_dist=extra)
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    expected_shapes(g, S, N, Tk, len(groups))
    worst = K.check(g, ref, bnd, S, t_start, case, d2=False)
    print("%s: cnt = %d + %d + %d; worst share of the bound %.4f" % (case, plan["L"], plan["P"], K.C_ROUND, worst))
