"""Ensemble event verification on the device (`-m gpu`): tmg_ens_event_count / tmg_ens_event_step through tmg_ops.EnsembleEvents
against the int64 / fp64 reference of tests/event_cases.py (direct comparison, shifted slices, bincount; other formulas for the
derived scores), and utils.modelPredEvents against the same reference over modelPred's samples.

Every integer output (rel_count, rel_hit, fss_raw, the four per-pixel sums after every step, the time counts) must EQUAL the reference,
on integer data (thresholds ON a value, so strictness shows) and on real data (float32 comparisons have no rounding).  Every float32
output lies within 2^-24 |ref| + 2^-40 of it, with NaNs where the reference has them.  Every case runs with cnt, the tables, the raw
sums and the per-pixel sums pre-filled with garbage.

Worst share of the float tolerance reached on an MI355X (the tests print it; LAB_NOTES.md): 0.994 on integer data, 0.970 on real data,
0.963 end to end.  The tolerance is one float32 rounding to nearest, which reaches 2^-24 |ref| just above a power of two, so shares
close to 1 are what a correctly rounded output gives."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import event_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
GARBAGE = -1077952577                                                         # 0xBFBFBFBF as int32


def run_events(xs, tgt, events, scales, sizes, padded, t_start, mu=None, sd=None, u=None):
    """Feed EnsembleEvents as utils.modelPredEvents does, in chunks of `sizes` members per step; padded: y and target are channel
    slices of wider NaN-filled NHWC buffers.  Every buffer the kernels write is pre-filled with garbage.  -> dict of numpy arrays: the
    outputs, and tsum_steps [T, 4, B, K, H, W]: the per-pixel sums read after every step (zeros before the first timed step)."""
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

    en = ops.EnsembleEvents(S, B, Cc, Hh, Ww, Tn, DEV, torch.zeros(Cc) if mu is None else mu, torch.ones(Cc) if sd is None else sd, u=u,
                            events=events, scales=scales)
    for v in (en.cnt, en.tsum, en.rel, en.fss_raw):
        v.fill_(GARBAGE)
    steps = []
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
        assert bool((en.rel[:, :, t + 1:] == GARBAGE).all()) and bool((en.fss_raw[:, t + 1:] == GARBAGE).all())   # a step writes its own planes
        if t < t_start:
            assert bool((en.tsum == GARBAGE).all())                           # an untimed step leaves the per-pixel sums alone
        steps.append(en.tsum.cpu().numpy().astype(np.int64).reshape(4, B, len(events), Hh, Ww) if t >= t_start
                     else np.zeros((4, B, len(events), Hh, Ww), np.int64))
    rel_before, raw_before = en.rel.cpu().numpy().copy(), en.fss_raw.cpu().numpy().copy()
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in en.finalize().items()}
    assert np.array_equal(en.rel.cpu().numpy(), rel_before) and np.array_equal(en.fss_raw.cpu().numpy(), raw_before)
    got["tsum_steps"] = np.stack(steps)
    return got, en.plan


def check_all(got, ref, S, B, Tn, Kn, scales, hw, what):
    NS = len(scales)
    assert set(got) == set(K.ALL_KEYS) | {"tsum_steps"}
    assert got["rel_count"].shape == (B, Tn, Kn, S + 1) and got["fss_raw"].shape == (B, Tn, Kn, NS, 3) and got["fss"].shape == (B, Tn, Kn, NS)
    assert got["time_roc_hit_rate"].shape == (B, Kn, S + 2) and got["time_brier_map"].shape == (B, Kn) + tuple(hw)
    K.check_integers(got, ref, what)
    assert np.array_equal(got["tsum_steps"], ref["tsum_steps"]), "%s: the per-pixel sums after every step" % what
    K.check_identities(got, S, scales, hw, what)
    return K.check_floats(got, ref, what)


# ---- integer data: equality on every branch of the launch plan ---------------------------------------------------------------------------
def _integer_case(case, idx):
    S, B, Cc, hw, t_start, kind, padded, Kn, scales = case
    xs, tgt, events, t_start = K.int_case_inputs(case, idx)
    got, plan = run_events(xs, tgt, events, scales, K.SC.chunk_sizes(S, kind), padded, t_start)
    worst = check_all(got, K.int_reference(idx), S, B, xs.shape[0], Kn, scales, hw, "integer %s" % (case,))
    print("integer %s: %d x %d tiles, halo %d, lds %d B; worst share of the float tolerance %.3f"
          % (case, plan["NTY"], plan["NTX"], plan["halo"], plan["lds"], worst))
    return plan


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE)))
def test_integer_data_gives_the_integer_reference_bit_for_bit(idx):
    _integer_case(K.INT_TABLE[idx], idx)


def test_integer_data_on_six_by_six_tiles():
    plan = _integer_case(K.LONG_CASE, len(K.INT_TABLE))
    assert plan["NTY"] == 6 and plan["NTX"] == 6 and plan["halo"] == 16


# ---- Gaussian, smooth and biased members with a real normalisation ---------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_real_data_gives_the_reference_and_the_quantile_class_counts(idx):
    import tmg_ops as ops
    S, B, Cc, hw, kind, with_u, events, scales = K.REAL_TABLE[idx]
    xs, tgt, u = K.real_case_inputs(idx)
    mu, sd = torch.tensor(K.MU[:Cc]), torch.tensor(K.SD[:Cc])
    t_start = idx % 2
    sizes = K.SC.chunk_sizes(S, idx % 3)
    got, plan = run_events(xs, tgt, events, scales, sizes, idx % 2 == 0, t_start, mu=mu, sd=sd, u=u)
    worst = check_all(got, K.real_reference(idx), S, B, K.T, len(events), scales, hw, "%s %s" % (kind, K.REAL_TABLE[idx][:4]))
    # the same events through EnsembleQuantiles: its member counts over the timed steps, bit for bit
    qt = ops.EnsembleQuantiles(S, B, Cc, hw[0], hw[1], K.T, DEV, mu, sd, u=u, levels=(0.5,), exceed=events)
    xd = torch.from_numpy(xs).to(DEV)
    for t in range(K.T):
        m0 = 0
        for k in sizes:
            qt.add(xd[t, m0:m0 + k].reshape(k * B, Cc, *hw).contiguous(memory_format=torch.channels_last), m0, time=t >= t_start)
            m0 += k
    assert np.array_equal(qt.finalize()["time_exceed_count"].cpu().numpy(), got["time_event_count"])
    print("%s %s: worst share of the float tolerance %.3f" % (kind, K.REAL_TABLE[idx][:4], worst))


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 3, 7])
def test_outputs_are_bitwise_the_same_for_every_feed_and_run(idx):
    S, B, Cc, hw, kind, with_u, events, scales = K.REAL_TABLE[idx]
    xs, tgt, u = K.real_case_inputs(idx)
    mu, sd = torch.tensor(K.MU[:Cc]), torch.tensor(K.SD[:Cc])
    outs = [run_events(xs, tgt, events, scales, K.SC.chunk_sizes(S, kd), padded, 1, mu=mu, sd=sd, u=u)[0]
            for kd, padded in ((0, False), (1, True), (2, False), (2, False))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name


def test_a_perfect_ensemble_scores_zero_brier_and_full_skill():
    """Every member equal to the target: n = S o, so brier = 0, roc_area = 1 and fss = 1 at every width."""
    S, B, Cc, hw = 5, 3, 3, (16, 33)
    _, tgt = K.SC.real_inputs(S, B, Cc, hw, "gauss", 61)
    xs = np.ascontiguousarray(np.broadcast_to(tgt[:, None], (K.T, S) + tgt.shape[1:]))
    got, _ = run_events(xs, tgt, ((0, 0.3, ">"), (1, 0.3, "<")), K.DEFAULT_SCALES, [2, 3], True, 0)
    assert not got["brier"].any() and not got["time_brier_map"].any() and not got["brier_rel"].any()
    assert bool((got["roc_area"] == 1).all()) and bool((got["fss"] == 1).all()) and bool((got["time_fss"] == 1).all())
    assert np.array_equal(got["time_event_count"], S * got["time_obs_count"])
    assert float(np.abs(got["brier_res"].astype(np.float64) - got["brier_unc"]).max()) <= 2.0 ** -23      # resolution = uncertainty


def test_a_shifted_ensemble_is_punished_per_pixel_and_forgiven_at_scale():
    """The double-penalty case the fractions skill score was made for: the members are the target shifted by two pixels along W.  The
    Brier score sees misses and false alarms; fss rises with every width and ends above the uniform value."""
    S, B, Cc, hw = 4, 1, 2, (48, 64)
    g = torch.Generator().manual_seed(62)
    base = torch.randn(K.T, B, Cc, hw[0], hw[1] + 2, generator=g).cumsum(-1).cumsum(-2)
    tgt = base[..., 2:].contiguous().numpy().astype(F32)
    xs = np.ascontiguousarray(np.broadcast_to(base[..., :-2].numpy().astype(F32)[:, None], (K.T, S) + tgt.shape[1:]))
    events, scales = ((0, 0.0, "<"),), (1, 3, 5, 9, 17, 33)
    got, _ = run_events(xs, tgt, events, scales, [S], False, 0)
    ref = K.reference(xs, tgt, K.thresholds(events, B, Cc), events, scales, 0)
    check_all(got, ref, S, B, K.T, 1, scales, hw, "shifted")
    f = got["time_fss"][0, 0]
    assert float(got["time_brier"][0, 0]) > 0 and bool((np.diff(f) > 0).all()) and f[0] < f[-1]
    assert f[-1] > float(got["time_fss_uniform"][0, 0])
    print("shifted by 2 pixels: time_brier %.4f, time_fss %s against uniform %.4f" % (float(got["time_brier"][0, 0]), np.round(f, 4).tolist(),
                                                                                      float(got["time_fss_uniform"][0, 0])))


def test_feeding_errors_are_the_quantile_class_errors():
    import tmg_ops as ops
    en = ops.EnsembleEvents(3, 2, 3, 4, 5, 2, DEV, torch.zeros(3), torch.ones(3))
    y = torch.zeros(2, 3, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="target shape None"):
        en.add(y, 0, None)
    with pytest.raises(ValueError, match="whole members"):
        en.add(y[:1], 0, y)
    with pytest.raises(ValueError, match="fed in order"):
        en.add(y, 1, y)
    with pytest.raises(RuntimeError, match="0 of 2 steps"):
        en.finalize()
    for _ in range(2):
        for m in range(3):
            en.add(y, m, y, time=False)
    with pytest.raises(RuntimeError, match="no time statistics"):
        en.finalize()


# ---- end to end: modelPredEvents against the reference over modelPred's samples ------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_events_matches_the_reference_over_model_pred(monkeypatch, tmp_path, case):
    """modelPred un-normalises every member and the target in fp32, xh = fl(u fl(fl(sd x) + mu)): three roundings, together at most
    3 u a (|x| + |mu| / sd), so a physical value within 4 u * scale of the event's value may fall on either side of it.  Those pixels
    are counted (`near`); the per-pixel counts may differ from the reference by at most their number at the pixel, the tables by at
    most twice their number per plane, and when there is none (the usual case) every output is held to the reference as in the
    tests above."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    scales = (1, 3, 9, 33)
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    tall = torch.cat([b[1].cpu() for b in te]).double().numpy()                    # the normalised target series [N, T, C, H, W]
    umed = float(np.median(u0.reshape(-1, 1, 1, 1) * (sd[0] * tall[:, :, 0] + mu[0])))        # the target's median ux
    pmed = float(np.median(u0.reshape(-1, 1, 1, 1) ** 2 * (sd[2] * tall[:, :, 2] + mu[2])))   # and median pressure
    events = ((0, umed, "<"), (2, pmed, ">"))
    for _ in range(2):                                                        # two folded runs: modelPredEvents, modelPredStats
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
    got = utils.modelPredEvents(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows,
                                events=events, scales=scales)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(stats) | set(K.ALL_KEYS) | {"events"}
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    assert got["events"] == events and np.array_equal(got["event_scales"].numpy(), scales)
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    xs, ys = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5)), np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]                              # [N, C]
    xn = (p / uc.reshape(1, N, 1, Cc, 1, 1) - mu[:Cc].reshape(1, 1, 1, Cc, 1, 1)) / sd[:Cc].reshape(1, 1, 1, Cc, 1, 1)
    scale = uc.reshape(N, 1, Cc, 1, 1) * (sd[:Cc].reshape(1, 1, Cc, 1, 1) * np.maximum(np.abs(xn).max(0), np.abs(tall[:, ::stride][:, :Tk]))
                                          + np.abs(mu[:Cc]).reshape(1, 1, Cc, 1, 1))            # [N, Tk, C, H, W]
    # the reference on the physical values against the physical thresholds: thr[b, k] = value, every case the same
    thr = np.array([[v for _, v, _ in events]] * N)
    ref = K.reference(xs, ys, thr, events, scales, t_start)
    near_n = np.stack([(np.abs(p[:, :, :, ch] - v) <= 4 * K.U24 * scale[None, :, :, ch]).sum(0) for ch, v, _ in events], 2)   # [N, Tk, K, H, W]
    near_o = np.stack([np.abs(y[:, :, ch] - v) <= 4 * K.U24 * scale[:, :, ch] for ch, v, _ in events], 2).astype(np.int64)
    near_total = int(near_n.sum() + near_o.sum())
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    assert bool((np.abs(g["time_event_count"] - ref["time_event_count"]) <= near_n[:, t_start:].sum(1)).all()), "%s time_event_count" % case
    assert bool((np.abs(g["time_obs_count"] - ref["time_obs_count"]) <= near_o[:, t_start:].sum(1)).all()), "%s time_obs_count" % case
    plane = (near_n + near_o).sum((-2, -1))                                  # [N, Tk, K]
    for key in ("rel_count", "rel_hit"):
        assert g[key].dtype == np.int64 and bool((np.abs(g[key] - ref[key]).sum(-1) <= 2 * plane).all()), "%s %s" % (case, key)
    K.check_identities(g, S, scales, (Hh, Ww), case)
    print("%s: comparisons within the rounding of their threshold: %d of %d" % (case, near_total, near_n.size * (S + 1)))
    assert near_total <= 1e-3 * near_n.size
    if near_total == 0:
        K.check_integers(g, ref, case)
        worst = K.check_floats(g, ref, case)
        print("%s: every output held to the reference; worst share of the float tolerance %.3f" % (case, worst))
