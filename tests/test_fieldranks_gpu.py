"""Ensemble field ranks on the device (`-m gpu`): tmg_ens_score_store / tmg_ens_frank_step through tmg_ops.EnsembleFieldRanks against
the int64 numpy reference of tests/fieldrank_cases.py, and utils.modelPredFieldRanks against the same reference on the chunks and
targets that reach the accumulator.

Every device quantity is an integer sum of comparisons of fp32 values, so there is no rounding and no tolerance: pre_raw,
outside_count and time_outside_count must EQUAL the reference, and so must every host output formed from them (the histograms are
fp64 sums of 1 / (equal + 1) added step by step, in the same order on both sides).  That the comparison is sensitive is
tests/test_fieldranks_cpu.py, which runs without a GPU on the inputs of this file."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import fieldrank_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)


def run_ranks(xs, tgt, t_start, sizes, padded, groups):
    """Feed EnsembleFieldRanks as utils.modelPredFieldRanks does, in chunks of `sizes` members per step; padded: y and target are
    channel slices of wider NaN-filled NHWC buffers.  The device buffers are pre-filled with garbage.  -> dict of numpy arrays."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    xd, td = torch.from_numpy(xs).to(DEV), torch.from_numpy(tgt).to(DEV)

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), float("nan"), device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    q = ops.EnsembleFieldRanks(S, B, Cc, Hh, Ww, Tn, DEV, groups=groups)
    q.xs.fill_(float("nan"))
    for buf in (q.ws, q.tout):
        buf.fill_(-77)
    q.pre_raw.fill_(-7777)
    q.outside.fill_(-7777)
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            q.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
    out = q.finalize()
    assert all(v.device.type == "cpu" for v in out.values())
    return {k: v.numpy() for k, v in out.items()}


def same(a, b, what):
    assert set(a) == set(b), what
    for k, v in a.items():
        assert v.dtype == b[k].dtype and np.array_equal(v, b[k]), "%s: %s" % (what, k)


@pytest.mark.parametrize("idx", range(len(K.SWEEP)))
def test_outputs_equal_the_int64_reference(idx):
    """Every member count, case count, channel count and field of the sweep, on continuous and on tie-heavy integer data; the features
    rotate: t_start 0 or 2, chunks of one member / three members / the whole ensemble, y and target contiguous or NaN-surrounded
    channel slices."""
    S, B, Cc, (Hh, Ww) = K.SWEEP[idx]
    t_start, padded, kind = K.features(idx)
    groups = K.GROUPS[Cc]
    for ties in (False, True):
        xs, tgt = K.inputs(idx, ties)
        what = "sweep %s ties=%s" % (K.SWEEP[idx], ties)
        got = run_ranks(xs, tgt, t_start, K.chunk_sizes(S, (kind + ties) % 3), padded != ties, groups)
        ref = K.reference(xs, tgt, t_start, groups)
        assert got["pre_raw"].shape == (B, K.T, Cc, S + 1, 2) and got["time_outside_count"].shape == (B, Cc, Hh, Ww)
        K.assert_equal(got, ref, what)
        Tn = K.T - t_start
        for kind_ in ("avg", "depth"):
            assert float(np.abs(got[kind_ + "_rank_hist"].sum(-1) - Tn).max()) <= Tn * 2.0 ** -50, what


def test_a_target_that_copies_a_member_and_all_rows_equal():
    S, B, Cc, Hh, Ww = 7, 3, 3, 16, 17
    idx = K.SWEEP.index((S, B, Cc, (Hh, Ww)))
    groups = K.GROUPS[Cc]
    xs, _ = K.inputs(idx)
    tgt = xs[:, 4].copy()                                                     # bitwise the member 4
    got = run_ranks(xs, tgt, 1, K.chunk_sizes(S, 1), True, groups)
    K.assert_equal(got, K.reference(xs, tgt, 1, groups), "copied member")
    assert np.array_equal(got["pre_raw"][:, :, :, 4], got["pre_raw"][:, :, :, S])
    assert (got["avg_rank_equal"] >= 1).all() and (got["depth_rank_equal"] >= 1).all()
    allsame = np.ascontiguousarray(np.broadcast_to(tgt[:, None], xs.shape))
    got = run_ranks(allsame, tgt, 0, K.chunk_sizes(S, 0), False, groups)
    K.assert_equal(got, K.reference(allsame, tgt, 0, groups), "all rows equal")
    HW = Hh * Ww
    assert (got["pre_raw"][..., 0] == S * HW).all() and (got["pre_raw"][..., 1] == K.choose2(S) * HW).all()
    assert not got["outside_count"].any() and (got["avg_rank_equal"] == S).all()
    h = np.zeros(S + 1)
    for _ in range(K.T):
        h += 1.0 / (S + 1)
    assert np.array_equal(got["avg_rank_hist"], np.broadcast_to(h, got["avg_rank_hist"].shape))
    high = (xs.max(1) + 1).astype(K.F32)                                      # a target above every member everywhere
    got = run_ranks(xs, high, 0, K.chunk_sizes(S, 2), False, groups)
    assert (got["avg_rank_below"] == S).all() and (got["depth_prerank"][..., S] == 0).all() and (got["outside_count"] == HW).all()


def test_the_largest_member_count():
    idx = len(K.SWEEP) - 1
    S, B, Cc, (Hh, Ww) = K.SWEEP[idx]
    assert S == 1024
    xs, tgt = K.inputs(idx, True)
    got = run_ranks(xs, tgt, 1, K.chunk_sizes(S, 2), False, K.GROUPS[Cc])
    K.assert_equal(got, K.reference(xs, tgt, 1, K.GROUPS[Cc]), "1024 members, ties")
    same_rows = np.zeros_like(xs)                                             # the largest A and D a pixel can hold, on every pixel
    got = run_ranks(same_rows, np.zeros_like(tgt), 0, [S], False, K.GROUPS[Cc])
    assert (got["pre_raw"][..., 1] == 523776 * Hh * Ww).all() and (got["pre_raw"][..., 0] == 1024 * Hh * Ww).all()


@pytest.mark.parametrize("S,B,Cc,hw", [(7, 3, 3, (16, 17)), (33, 3, 4, (5, 7)), (17, 1, 2, (3, 300)), (9, 2, 3, (16, 16)), (9, 2, 3, (1, 257))])
def test_outputs_are_bitwise_the_same_for_every_feed_and_run(S, B, Cc, hw):
    """HW = 256 fills one block exactly; HW = 257 leaves one pixel to a second block whose other 255 lanes are past the field."""
    xs, tgt = K.make_inputs(S, B, Cc, hw[0], hw[1], 600 + S, ties=S == 9)
    groups = K.GROUPS[Cc]
    outs = [run_ranks(xs, tgt, 1, K.chunk_sizes(S, kind), padded, groups)
            for kind, padded in ((0, False), (1, True), (2, False), (2, False), (1, False))]
    K.assert_equal(outs[0], K.reference(xs, tgt, 1, groups), "feeds")
    for o in outs[1:]:
        same(outs[0], o, "feeds %s" % ((S, B, Cc, hw),))


def test_time_outside_count_covers_the_timed_steps_only():
    S, B, Cc, Hh, Ww = 6, 3, 3, 16, 17
    idx = K.SWEEP.index((S, B, Cc, (Hh, Ww)))
    xs, tgt = K.inputs(idx)
    groups = K.GROUPS[Cc]
    late = run_ranks(xs, tgt, 2, K.chunk_sizes(S, 1), False, groups)
    _, _, O = K.pixel_terms(xs, tgt)
    assert np.array_equal(late["time_outside_count"], O[2:].sum(0)) and O[:2].any()
    full = run_ranks(xs, tgt, 0, K.chunk_sizes(S, 1), False, groups)
    assert np.array_equal(full["time_outside_count"], O.sum(0))
    same({k: late[k] for k in ("pre_raw", "outside_count", "avg_prerank", "depth_prerank", "depth_median")},
         {k: full[k] for k in ("pre_raw", "outside_count", "avg_prerank", "depth_prerank", "depth_median")}, "per-step outputs")
    assert np.array_equal(late["traj_depth_prerank"], full["depth_prerank"][:, 2:].sum(1))


def test_feeding_errors_come_before_any_launch():
    import tmg_ops as ops
    q = ops.EnsembleFieldRanks(3, 2, 3, 5, 7, 2, DEV)
    y = torch.zeros(2, 3, 5, 7, device=DEV)
    with pytest.raises(ValueError):
        q.add(y, 0, None)
    with pytest.raises(ValueError):
        q.add(y, 1, y)
    with pytest.raises(ValueError):
        q.add(y[:, :2], 0, y)
    with pytest.raises(RuntimeError):
        q.finalize()


# ---- end to end: modelPredFieldRanks == the reference on the chunks that reach the accumulator -----------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_fieldranks_equals_the_reference_on_its_own_chunks(monkeypatch, tmp_path, case):
    """The reference is computed from clones of the chunks and targets that reach EnsembleFieldRanks.add, not from modelPred's fp32
    un-normalised samples: un-normalising can merge two distinct values into a tie."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    groups = ((0, 1), (2,))
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    for _ in range(2):                                                        # two folded runs: modelPredFieldRanks, modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    seen = []                                                                 # per accumulator: [(y, m0, target, time), ..]
    add = ops.EnsembleFieldRanks.add

    def recording(self, y, m0, target, time=True):
        if not seen or seen[-1][0] is not self:
            seen.append((self, []))
        seen[-1][1].append((y.detach().clone().cpu(), int(m0), target.detach().clone().cpu(), bool(time)))
        return add(self, y, m0, target, time=time)

    monkeypatch.setattr(ops.EnsembleFieldRanks, "add", recording)
    torch.manual_seed(77)
    got = utils.modelPredFieldRanks(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows,
                                    groups=groups)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold and len(seen) == len(batches)
    new = set(K.DEVICE_KEYS) | set(K.FLOAT_KEYS) | {"fieldrank_groups", "depth_median", "traj_depth_median"} \
        | {p + k + s for p in ("", "traj_") for k in ("avg", "depth") for s in ("_prerank", "_rank_below", "_rank_equal")}
    assert set(got) == set(stats) | new and got["fieldrank_groups"] == groups
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    case0 = 0
    Tk = tmax // stride
    for (acc, calls), B in zip(seen, batches):
        Cc, Hh, Ww = calls[0][2].shape[1:]
        xs = np.zeros((Tk, S, B, Cc, Hh, Ww), dtype=K.F32)
        tgt = np.zeros((Tk, B, Cc, Hh, Ww), dtype=K.F32)
        step, timed = 0, []
        for y, m0, target, time in calls:
            k = y.shape[0] // B
            xs[step, m0:m0 + k] = y.numpy().reshape(k, B, Cc, Hh, Ww)
            if m0 + k == S:
                tgt[step] = target.numpy()
                timed.append(time)
                step += 1
        assert step == Tk and timed == [t >= t_start for t in range(Tk)]
        ref = K.reference(xs, tgt, t_start, groups)
        part = {k: got[k][case0:case0 + B].numpy() for k in ref}
        K.assert_equal(part, ref, "%s cases %d..%d" % (case, case0, case0 + B - 1))
        case0 += B
    assert case0 == got["pre_raw"].shape[0]
    N, HW = case0, got["time_outside_count"].shape[-1] * got["time_outside_count"].shape[-2]
    assert tuple(got["avg_rank_hist"].shape) == (N, len(groups), S + 1) and tuple(got["outside_frac"].shape) == (N, Tk, 3)
    print("%s: outside_frac mean %.3f (calibrated: %.3f), avg-rank histogram %s" % (
        case, float(got["outside_frac"].mean()), 2.0 / (S + 1), got["avg_rank_hist"].sum(0).tolist()))
    assert HW > 0
