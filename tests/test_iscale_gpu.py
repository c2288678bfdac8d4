"""Intensity-scale verification on the device (`-m gpu`): tmg_ens_iscale_chunk / tmg_ens_iscale_step through
tmg_ops.EnsembleIntensityScale against the int64 reference of tests/iscale_cases.py (zero-pad, reshape, sum, square, sum; held
against explicit Haar components on the CPU), and utils.modelPredIntensityScale against the same reference over modelPred's samples.

Everything the device forms is an integer: the three raw tables must EQUAL the reference bit for bit, on integer data (thresholds ON
a value, so strictness shows), on smooth real fields and with NaN and infinities planted, with one event every pixel is in and one no
pixel is in; they are bitwise the same for every chunking and for two runs.  The shapes sit on every edge of the 64 x 64 tile and of
the 4 x 4 patch.  Every case runs with the count and the three tables pre-filled with garbage: the step's first chunk writes the count
and zeroes the tables.  The float32 outputs lie within 2^-24 |ref| + 2^-40 of the fp64 restatement of tmg_ops.iscale_outputs, and the
Brier components sum to EnsembleEvents' brier of the same data."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import iscale_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
GARBAGE = -1077952577                                                         # 0xBFBFBFBF as int32
TIME_RAW = tuple("time_" + k for k in K.RAW_KEYS)
TIME_FLOAT = tuple("time_" + k for k in K.FLOAT_KEYS)


def _nhwc(v, Cc, padded):
    """API-shaped [n, C, H, W] whose channels-last view is dense, or a channel slice at offset 1 of 4-channel NaN-filled storage."""
    v = v.permute(0, 2, 3, 1)
    if not padded:
        return v.contiguous().permute(0, 3, 1, 2)
    wide = torch.full(tuple(v.shape[:3]) + (4,), float("nan"), device=v.device)
    wide[..., 1:1 + Cc] = v
    return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)


def run_iscale(xs, tgt, events, L, sizes, padded, with_events=False):
    """Feed EnsembleIntensityScale as utils.modelPredIntensityScale does, in chunks of `sizes` members per step, the steps timed as
    K.TIMED.  Every buffer the kernels write is pre-filled with garbage.  -> dict of numpy arrays, the plan and, with_events,
    EnsembleEvents' outputs of the same feed."""
    import tmg_ops as ops
    Tk, S, B, Cc, Hh, Ww = xs.shape
    xd = torch.from_numpy(np.array(xs)).to(DEV)                              # (a copy: the cached inputs are read-only)
    td = torch.from_numpy(np.array(tgt)).to(DEV)
    assert not padded or Cc <= 3
    acc = ops.EnsembleIntensityScale(S, B, Cc, Hh, Ww, Tk, DEV, torch.zeros(Cc), torch.ones(Cc), events=events, levels=L)
    acc.cnt.fill_(GARBAGE)
    for v in (acc.member, acc.target, acc.ens):
        v.fill_(GARBAGE * 4294967296 + 12345)
    evs = ops.EnsembleEvents(S, B, Cc, Hh, Ww, Tk, DEV, torch.zeros(Cc), torch.ones(Cc), events=events, scales=(1,)) if with_events else None
    for t in range(Tk):
        target = _nhwc(td[t], Cc, padded)
        m0 = 0
        for k in sizes:
            y = _nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww), Cc, padded)
            acc.add(y, m0, target, time=K.TIMED[t])
            if evs is not None:
                evs.add(y, m0, target, time=K.TIMED[t])
            m0 += k
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in acc.finalize().items()}
    if evs is None:
        return out, acc.plan
    return out, acc.plan, {k: v.cpu().numpy() for k, v in evs.finalize().items()}


def check_all(got, ref, case, what):
    S, B, Cc, hw, Kn, L, kind, _ = case
    assert set(got) == set(K.ALL_KEYS)
    want = K.full_reference(ref, S, hw[0] * hw[1])
    bad = K.mismatches(got, want, K.RAW_KEYS + TIME_RAW + ("iscale_blocks",))
    assert not bad, "%s: %s differ from the integer reference" % (what, bad)
    K.check_identities(got, S, hw[0] * hw[1])
    return K.check_floats(got, want, K.FLOAT_KEYS + TIME_FLOAT, what)


# ---- every case of the table, in three chunkings and twice ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_raw_tables_equal_the_reference_bit_for_bit_for_every_chunking(idx):
    case = K.TABLE[idx]
    S, B, Cc, hw, Kn, L, kind, padded = case
    xs, tgt = K.inputs(idx)
    events = K.events_for(Cc, Kn)
    ref = K.case_reference(idx)
    outs = []
    for kd in (0, 1, 2, 2):
        got, plan = run_iscale(xs, tgt, events, L, K.chunk_sizes(S, kd), padded)
        assert plan["grid"] == (-(-hw[0] // 64) * -(-hw[1] // 64), Kn, B)
        worst = check_all(got, ref, case, "%s chunks %s" % (case, K.chunk_sizes(S, kd)))
        outs.append(got)
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name
    print("%s: %d blocks; worst share of the float tolerance %.3f" % (case, plan["blocks"], worst))


@pytest.mark.parametrize("case", K.GROUP_CASES)
def test_member_groups_of_four_and_eight_give_the_same_tables(case):
    """One chunk of S members runs as groups of 4 + 1 and of 8 + 1 members per tile, which add to the count atomically; one member
    per chunk runs one group per tile, which writes it.  Both equal the reference."""
    S, B, Cc, hw, Kn, L, kind, padded = case
    xs, tgt = K.make_inputs(case, 71)
    events = K.events_for(Cc, Kn)
    ref = K.reference(xs, tgt, K.thresholds(events, B), events, L)
    assert K.group(K.planes(case), S) in (4, 8) and S % K.group(K.planes(case), S) == 1
    outs = []
    for kd in (0, 1):
        got, plan = run_iscale(xs, tgt, events, L, K.chunk_sizes(S, kd), padded)
        assert plan["group"] == K.group(K.planes(case), S)
        check_all(got, ref, case, "%s chunks %s" % (case, K.chunk_sizes(S, kd)))
        outs.append(got)
    for name, v in outs[0].items():
        assert np.array_equal(v, outs[1][name], equal_nan=True), name


def test_the_chunkings_the_cases_run():
    assert K.chunk_sizes(5, 0) == [5] and K.chunk_sizes(5, 1) == [1] * 5 and K.chunk_sizes(5, 2) == [2, 3]
    assert {c[0] for c in K.TABLE} == {1, 2, 5} and {c[4] for c in K.TABLE} == {1, 4} and {c[1] for c in K.TABLE} == {2}
    assert {(c[3], c[5]) for c in K.TABLE} == {(hw, L) for hw in ((1, 1), (3, 130), (64, 64), (65, 63), (70, 70)) for L in (1, 3, 6)}
    assert len(K.TIMED) == 3 and sum(K.TIMED) == 2


def test_nan_and_infinities_are_in_no_event_they_compare_false_to():
    case = K.NONFINITE_CASE
    S, B, Cc, hw, Kn, L, kind, padded = case
    xs, tgt = K.make_inputs(case, 41)
    K.plant_nonfinite(xs, tgt, 42)
    assert np.isnan(xs).any() and np.isnan(tgt).any() and np.isinf(xs).any() and np.isinf(tgt).any()
    events = K.events_for(Cc, Kn)
    thr = K.thresholds(events, B)
    ref = K.reference(xs, tgt, thr, events, L)
    assert K.mismatches(K.reference(xs, tgt, thr, events, L, "nan_in_event"), ref, K.RAW_KEYS)
    for kd in (0, 2):
        got, _ = run_iscale(xs, tgt, events, L, K.chunk_sizes(S, kd), padded)
        check_all(got, ref, case, "non-finite, chunks %s" % K.chunk_sizes(S, kd))
    xs[:], tgt[:] = np.nan, np.nan                                            # none in: zero tables, every ratio 0 / 0
    got, _ = run_iscale(xs, tgt, events, L, [S], padded)
    check_all(got, K.reference(xs, tgt, thr, events, L), case, "all NaN")
    assert not got["iscale_member_raw"].any() and not got["iscale_ens_raw"].any() and np.isnan(got["iscale_skill"]).all()


@pytest.mark.parametrize("idx", [7, 11, 14])
def test_the_brier_components_sum_to_ensemble_events_brier(idx):
    case = K.TABLE[idx]
    S, B, Cc, hw, Kn, L, kind, padded = case
    xs, tgt = K.inputs(idx)
    got, _, ev = run_iscale(xs, tgt, K.events_for(Cc, Kn), L, K.chunk_sizes(S, 2), padded, with_events=True)
    import tmg_ops as ops
    for pre in ("", "time_"):
        # against the fp64 score of EnsembleEvents' tables: each non-negative component is rounded to float32 once, so the errors sum
        # to at most 2^-24 of their sum; against its float32 output, which is rounded once more, twice that
        exact = ops.event_table_scores(torch.from_numpy(ev[pre + "rel_count"]), torch.from_numpy(ev[pre + "rel_hit"]), S)["brier"].numpy()
        total = got[pre + "iscale_brier"].astype(np.float64).sum(-1)
        assert bool((np.abs(total - exact) <= K.U24 * np.abs(exact) + K.TOL_ABS).all()), pre
        assert bool((np.abs(total - ev[pre + "brier"]) <= 2 * K.U24 * np.abs(exact) + K.TOL_ABS).all()), pre
    j = np.arange(S + 1)
    assert np.array_equal((ev["rel_count"] * j * j).sum(-1), got["iscale_ens_raw"][..., 0, 0])       # sum n^2 is AN[0], exactly
    assert np.array_equal((ev["rel_hit"] * j).sum(-1), got["iscale_ens_raw"][..., 0, 1])             # sum n o is XN[0]
    assert np.array_equal(ev["rel_hit"].sum(-1), got["iscale_target_raw"][..., 0])


def test_return_codes_come_before_any_launch():
    import tmg_hip as H
    S, B, Cc, Hh, Ww, Kn, L = 3, 2, 3, 5, 7, 2, 2
    cnt = torch.full((B, Kn, Hh * Ww), GARBAGE, device=DEV, dtype=torch.int32)
    i64 = dict(device=DEV, dtype=torch.int64)
    member, tt, ens = torch.full((B, Kn, S, L + 1, 2), 77, **i64), torch.full((B, Kn, L + 1), 77, **i64), torch.full((B, Kn, L + 1, 2), 77, **i64)
    thr = torch.zeros(B, Kn, device=DEV)
    y = torch.zeros(2 * B, Hh, Ww, Cc, device=DEV)
    tg = torch.zeros(B, Hh, Ww, Cc, device=DEV)
    ev = ((0, 0), (2, 1))
    chunk = lambda **kw: H.ens_iscale_chunk(**dict(dict(y=y, target=tg, thr=thr, ev=ev, cnt=cnt, member=member, target_tab=tt, ens=ens, S=S,  # noqa: E731
                                                        k=2, m0=0, code=True), **kw))
    step = lambda **kw: H.ens_iscale_step(**dict(dict(cnt=cnt, target=tg, thr=thr, ev=ev, ens=ens, S=S, code=True), **kw))  # noqa: E731
    assert chunk(m0=2) == -1 and chunk(m0=-1) == -1 and chunk(k=1, m0=3, y=y[:B]) == -1
    assert chunk(ev=((3, 0), (2, 1))) == -1 and chunk(ev=((0, 2), (2, 1))) == -1 and step(ev=((3, 0), (2, 1))) == -1
    big = torch.full((B, Kn, 1025, L + 1, 2), 77, **i64)
    assert chunk(S=1025, member=big) == -2 and step(S=1025) == -2
    deep = [torch.full(s, 77, **i64) for s in ((B, Kn, S, 8, 2), (B, Kn, 8), (B, Kn, 8, 2))]
    assert chunk(member=deep[0], target_tab=deep[1], ens=deep[2]) == -1 and step(ens=deep[2]) == -1      # L = 7
    # a null pointer: -3, straight through the C entries (the wrappers cannot pass one)
    import ctypes
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)                           # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    lib, evf, yd, nul = H.lib(), i64s(0, 0, 2, 1), i64s(Cc, 0), ctypes.c_void_p(0)
    cd, sd = i64s(2, B, Hh, Ww, Cc, S, 0, Kn, L), i64s(S, B, Hh, Ww, Cc, Kn, L)
    assert lib.tmg_ens_iscale_chunk(vp(y), yd, vp(tg), yd, vp(thr), evf, vp(cnt), vp(member), vp(tt), nul, cd, nul) == -3
    assert lib.tmg_ens_iscale_chunk(vp(y), yd, vp(tg), yd, vp(thr), evf, nul, vp(member), vp(tt), vp(ens), cd, nul) == -3
    assert lib.tmg_ens_iscale_chunk(vp(y), None, vp(tg), yd, vp(thr), evf, vp(cnt), vp(member), vp(tt), vp(ens), cd, nul) == -3
    assert lib.tmg_ens_iscale_step(vp(cnt), vp(tg), yd, vp(thr), evf, nul, sd, nul) == -3
    assert lib.tmg_ens_iscale_step(vp(cnt), vp(tg), yd, vp(thr), None, vp(ens), sd, nul) == -3
    with pytest.raises(RuntimeError):
        chunk(m0=2, code=False)
    with pytest.raises(RuntimeError, match="member is a contiguous"):
        chunk(member=member[:, :, :2])
    with pytest.raises(RuntimeError, match="cnt is a contiguous"):
        step(cnt=cnt[:1])
    torch.cuda.synchronize()
    assert bool((cnt == GARBAGE).all()) and all(bool((v == 77).all()) for v in (member, tt, ens, big) + tuple(deep))   # nothing was launched


def test_feeding_errors_are_the_class_errors():
    import tmg_ops as ops
    acc = ops.EnsembleIntensityScale(3, 2, 3, 4, 5, 2, DEV, torch.zeros(3), torch.ones(3))
    assert acc.L == 2
    y = torch.zeros(2, 3, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="target shape None"):
        acc.add(y, 0, None)
    with pytest.raises(ValueError, match="whole members"):
        acc.add(y[:1], 0, y)
    with pytest.raises(ValueError, match="fed in order"):
        acc.add(y, 1, y)
    with pytest.raises(RuntimeError, match="0 of 2 steps"):
        acc.finalize()
    for _ in range(2):
        for m in range(3):
            acc.add(y, m, y)
    out = acc.finalize()
    assert not bool(out["iscale_member_raw"].any()) and bool(torch.isnan(out["iscale_skill"]).all())   # zeros are not below zero
    with pytest.raises(ValueError, match="fed in order"):
        acc.add(y, 0, y)


# ---- end to end: modelPredIntensityScale against the reference over modelPred's samples -------------------------------------------------
def test_model_pred_intensity_scale_matches_the_reference_over_model_pred(monkeypatch, tmp_path):
    """The keys shared with modelPredStats are identical, and the raw tables equal the reference fed with modelPred's roll-outs.
    modelPred un-normalises in fp32 (three roundings, tests/test_events_gpu.py), so a physical value within 4 u * scale of an event's
    value may fall on either side of it: those comparisons are counted, and when there is none (the usual case) every output is held
    to the reference bit for bit; otherwise the level-0 sums may differ by at most their number."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = E._cylinder_case(tmp_path)
    S, tmax, stride, t_start, max_rows, L = 5, 6, 2, 1, 4, 3
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    tall = torch.cat([b[1].cpu() for b in te]).double().numpy()                    # the normalised target series [N, T, C, H, W]
    umed = float(np.median(u0.reshape(-1, 1, 1, 1) * (sd[0] * tall[:, :, 0] + mu[0])))
    pmed = float(np.median(u0.reshape(-1, 1, 1, 1) ** 2 * (sd[2] * tall[:, :, 2] + mu[2])))
    events = ((0, umed, "<"), (2, pmed, ">"))
    for _ in range(2):                                                        # two folded runs: intensity scales, stats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    for bi, B in enumerate(batches):
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    kw = dict(samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    torch.manual_seed(77)
    got = utils.modelPredIntensityScale(args, model, te, E.LOG, events=events, levels=L, **kw)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(stats) | set(K.ALL_KEYS) | {"events"}
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    assert got["events"] == events and got["iscale_blocks"].tolist() == [2, 4, 8, 0]
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    xs = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5))
    ys = np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]
    xn = (p / uc.reshape(1, N, 1, Cc, 1, 1) - mu[:Cc].reshape(1, 1, 1, Cc, 1, 1)) / sd[:Cc].reshape(1, 1, 1, Cc, 1, 1)
    scale = uc.reshape(N, 1, Cc, 1, 1) * (sd[:Cc].reshape(1, 1, Cc, 1, 1) * np.maximum(np.abs(xn).max(0), np.abs(tall[:, ::stride][:, :Tk]))
                                          + np.abs(mu[:Cc]).reshape(1, 1, Cc, 1, 1))            # [N, Tk, C, H, W]
    thr = np.array([[v for _, v, _ in events]] * N)
    ref = K.reference(xs, ys, thr, events, L)
    near_n = np.stack([(np.abs(p[:, :, :, ch] - v) <= 4 * K.U24 * scale[None, :, :, ch]).sum(0) for ch, v, _ in events], 2)   # [N, Tk, K, H, W]
    near_o = np.stack([np.abs(y[:, :, ch] - v) <= 4 * K.U24 * scale[:, :, ch] for ch, v, _ in events], 2).astype(np.int64)
    near_total = int(near_n.sum() + near_o.sum())
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    near = (near_n + S * near_o).sum((-2, -1))                               # [N, Tk, K]: the comparisons that may fall either way
    assert bool((np.abs(g["iscale_member_raw"][..., 0, 0] - ref["iscale_member_raw"][..., 0, 0]).sum(-1) <= near).all())
    assert bool((np.abs(g["iscale_target_raw"][..., 0] - ref["iscale_target_raw"][..., 0]) <= near).all())
    K.check_identities(g, S, Hh * Ww)
    print("comparisons within the rounding of their threshold: %d of %d" % (near_total, near_n.size * (S + 1)))
    assert near_total <= 1e-3 * near_n.size
    if near_total == 0:
        timed = tuple(j >= t_start for j in range(Tk))
        want = K.full_reference(ref, S, Hh * Ww, timed)
        assert not K.mismatches(g, want, K.RAW_KEYS + TIME_RAW)
        worst = K.check_floats(g, want, K.FLOAT_KEYS + TIME_FLOAT, "cylinder")
        print("every output held to the reference; worst share of the float tolerance %.3f" % worst)
