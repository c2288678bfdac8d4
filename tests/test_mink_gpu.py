"""Excursion-set morphology on the device (`-m gpu`): tmg_ens_mink_chunk through tmg_ops.EnsembleMorphology against the int64 reference
of tests/mink_cases.py (J direct compares, slices, `&`, sums; held against pieces and holes by flood fill on the CPU), and
utils.modelPredMorphology against the same reference over modelPred's samples.

Everything the device forms is an integer: mink_raw must EQUAL the reference bit for bit, on integer data (thresholds ON a value, so
strictness shows), on smooth real fields and with NaN and infinities planted, with a ladder every pixel is above and one no pixel is
above, with equal neighbours in the ladder and with a decreasing one; it is bitwise the same for every chunking and for two runs.
The shapes sit on every edge of the tile the plan reports, with a full quad, a diagonal pair and a pair across each tile edge planted
at every tile corner.  Every case runs with the tables pre-filled with garbage: the step's first chunk zeroes them.  The float32
outputs lie within 2^-24 |ref| + 2^-40 of the fp64 restatement of tmg_ops.mink_outputs."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import mink_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
GARBAGE = -1077952577 * 4294967296 + 12345
TIME_INT = tuple("time_" + k for k in K.INT_KEYS)
FLOATS = K.FLOAT_KEYS + tuple("time_" + k for k in K.FLOAT_KEYS)


def _nhwc(v, Cc, padded):
    """API-shaped [n, C, H, W] whose channels-last view is dense, or a channel slice at offset 1 of 4-channel NaN-filled storage."""
    v = v.permute(0, 2, 3, 1)
    if not padded:
        return v.contiguous().permute(0, 3, 1, 2)
    wide = torch.full(tuple(v.shape[:3]) + (4,), float("nan"), device=v.device)
    wide[..., 1:1 + Cc] = v
    return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)


def run_mink(case, xs, tgt, sizes):
    """Feed EnsembleMorphology as utils.modelPredMorphology does, in chunks of `sizes` members per step, the steps timed as K.TIMED.
    The tables are pre-filled with garbage.  -> dict of numpy arrays and the plan."""
    import tmg_ops as ops
    S, B, Cc, hw, F, J, kind, padded = case
    Tk = xs.shape[0]
    xd = torch.from_numpy(np.array(xs)).to(DEV)                              # (a copy: the cached inputs are read-only)
    td = torch.from_numpy(np.array(tgt)).to(DEV)
    assert not padded or Cc <= 3
    acc = ops.EnsembleMorphology(S, B, Cc, hw[0], hw[1], Tk, DEV, torch.zeros(Cc), torch.ones(Cc), fields=K.fields_for(Cc, F),
                                 thresholds=K.ladder(kind, F, J), grid=K.GRID)
    raw = torch.from_numpy(np.array(K.raw_ladder(case))).to(DEV)
    if kind == "decr":
        acc.thr.copy_(raw)                                                    # the class takes ascending ladders only: the device any
    assert torch.equal(acc.thr, raw)                                         # out_mu = 0, out_std = 1, u = 1: the float32 rounding
    acc.table.fill_(GARBAGE)
    for t in range(Tk):
        target = _nhwc(td[t], Cc, padded)
        m0 = 0
        for k in sizes:
            acc.add(_nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, hw[0], hw[1]), Cc, padded), m0, target, time=K.TIMED[t])
            m0 += k
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in acc.finalize().items()}, acc.plan


def check_all(got, ref, case, what):
    S, B, Cc, hw, F, J, kind, _ = case
    assert set(got) == set(K.ALL_KEYS)
    want = K.full_reference(ref, S, hw[0], hw[1], K.GRID, K.levels_of(case))
    bad = K.mismatches(got, want, ("mink_raw", "time_mink_raw", "mink_levels") + K.INT_KEYS + TIME_INT)
    assert not bad, "%s: %s differ from the integer reference" % (what, bad)
    return K.check_floats(got, want, FLOATS, what)


# ---- every case of the table, in three chunkings and twice ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_raw_counts_equal_the_reference_bit_for_bit_for_every_chunking(idx):
    case = K.TABLE[idx]
    S, B, Cc, hw, F, J, kind, padded = case
    xs, tgt = K.inputs(idx)
    ref = K.case_reference(idx)
    outs = []
    for kd in (0, 1, 2, 2):
        got, plan = run_mink(case, xs, tgt, K.chunk_sizes(S, kd))
        assert (plan["tile_h"], plan["tile_w"]) == K.TILE and plan["group"] == K.group(K.planes(case), S)
        worst = check_all(got, ref, case, "%s chunks %s" % (case, K.chunk_sizes(S, kd)))
        outs.append(got)
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name
    print("%s: %d blocks; worst share of the float tolerance %.3f" % (case, plan["blocks"], worst))


def test_the_field_sizes_sit_on_the_edges_of_the_plans_tile():
    import tmg_hip as H
    p = H.ens_mink_plan(2, 1, 70, 69, 1, 1)
    th, tw = p["tile_h"], p["tile_w"]
    assert {(th, tw), (th + 1, tw - 1), (th + 6, tw + 6)} <= {c[3] for c in K.TABLE} and (th, tw) == K.TILE
    assert (p["tiles_x"], p["tiles_y"]) == (2, 2)


@pytest.mark.parametrize("case", K.GROUP_CASES)
def test_member_groups_of_two_and_four_give_the_same_tables(case):
    """One chunk of 5 members runs as groups of 4 + 1 (2 + 2 + 1) members per block; one member per chunk runs one member per block."""
    S = case[0]
    xs, tgt = K.make_inputs(case, 71)
    ref = K.reference(xs, tgt, K.raw_ladder(case), K.fields_for(case[2], case[4]))
    outs = []
    for kd in (0, 1, 2):
        got, plan = run_mink(case, xs, tgt, K.chunk_sizes(S, kd))
        assert plan["group"] == K.group(K.planes(case), S)
        check_all(got, ref, case, "%s chunks %s" % (case, K.chunk_sizes(S, kd)))
        outs.append(got)
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name


def test_nan_is_in_no_set_and_plus_infinity_in_every_one():
    import tmg_ops as ops
    S, B, Cc, Hh, Ww, J = 2, 1, 2, 3, 5, 4
    case = (S, B, Cc, (Hh, Ww), 1, J, "smooth", False)
    xs = np.full((1, S, B, Cc, Hh, Ww), np.nan, np.float32)
    tgt = np.full((1, B, Cc, Hh, Ww), np.inf, np.float32)
    xs[0, 1] = -np.inf
    acc = ops.EnsembleMorphology(S, B, Cc, Hh, Ww, 1, DEV, torch.zeros(Cc), torch.ones(Cc), fields=(1,), thresholds=K.ladder("smooth", 1, J))
    acc.table.fill_(GARBAGE)
    acc.add(torch.from_numpy(xs[0].reshape(S * B, Cc, Hh, Ww)).to(DEV).contiguous(memory_format=torch.channels_last), 0,
            torch.from_numpy(tgt[0]).to(DEV).contiguous(memory_format=torch.channels_last))
    raw = acc.finalize()["mink_raw"].cpu().numpy()
    assert not raw[:, :, :, :S].any()                                         # NaN and -Inf: rank 0
    assert bool((raw[0, 0, 0, S] == np.array([Hh * Ww, Hh * (Ww - 1), (Hh - 1) * Ww, (Hh - 1) * (Ww - 1), 0])).all())   # +Inf: rank J
    assert np.array_equal(raw, K.reference(xs, tgt, K.raw_ladder(case), (1,)))


def test_return_codes_come_before_any_launch():
    import tmg_hip as H
    S, B, Cc, Hh, Ww, F, J = 3, 2, 3, 5, 7, 2, 3
    i64 = dict(device=DEV, dtype=torch.int64)
    table = torch.full((B, F, S + 1, J, 5), 77, **i64)
    thr = torch.zeros(B, F, J, device=DEV)
    y = torch.zeros(2 * B, Hh, Ww, Cc, device=DEV)
    tg = torch.zeros(B, Hh, Ww, Cc, device=DEV)
    chunk = lambda **kw: H.ens_mink_chunk(**dict(dict(y=y, target=tg, thr=thr, fields=(0, 2), table=table, S=S, k=2, m0=0, code=True), **kw))  # noqa: E731
    assert chunk(m0=2) == -1 and chunk(m0=-1) == -1 and chunk(k=1, m0=3, y=y[:B]) == -1
    assert chunk(fields=(0, 3)) == -1 and chunk(fields=(2, 2)) == -1 and chunk(fields=(-1, 0)) == -1
    big = torch.full((B, F, 1026, J, 5), 77, **i64)
    assert chunk(S=1025, table=big) == -2
    deep = torch.full((B, F, S + 1, 33, 5), 77, **i64)
    assert chunk(table=deep, thr=torch.zeros(B, F, 33, device=DEV)) == -1    # J = 33
    wide = torch.full((B, 5, S + 1, J, 5), 77, **i64)
    assert chunk(table=wide, thr=torch.zeros(B, 5, J, device=DEV), fields=(0, 1, 2, 0, 1)) == -1   # F = 5
    # a null pointer: -3, straight through the C entry (the wrapper cannot pass one)
    import ctypes
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)                           # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    lib, ff, yd, nul = H.lib(), i64s(0, 2), i64s(Cc, 0), ctypes.c_void_p(0)
    cd = i64s(2, B, Hh, Ww, Cc, S, 0, F, J)
    assert lib.tmg_ens_mink_chunk(vp(y), yd, vp(tg), yd, vp(thr), ff, nul, cd, nul) == -3
    assert lib.tmg_ens_mink_chunk(vp(y), yd, nul, yd, vp(thr), ff, vp(table), cd, nul) == -3
    assert lib.tmg_ens_mink_chunk(vp(y), None, vp(tg), yd, vp(thr), ff, vp(table), cd, nul) == -3
    assert lib.tmg_ens_mink_chunk(vp(y), yd, vp(tg), yd, vp(thr), None, vp(table), cd, nul) == -3
    with pytest.raises(RuntimeError):
        chunk(m0=2, code=False)
    with pytest.raises(RuntimeError, match="table is a contiguous"):
        chunk(table=table[:, :, :2])
    with pytest.raises(RuntimeError, match="thr is a contiguous"):
        chunk(thr=thr[:1])
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in (table, big, deep, wide))      # nothing was launched
    assert chunk() == 0 and chunk(m0=2, k=1, y=y[:B]) == 0                   # and the good calls are taken
    torch.cuda.synchronize()
    assert not bool(table.any())                                              # zeros are not above zero


def test_feeding_errors_are_the_class_errors():
    import tmg_ops as ops
    acc = ops.EnsembleMorphology(3, 2, 3, 4, 5, 2, DEV, torch.zeros(3), torch.ones(3))
    assert (acc.F, acc.J, acc.fields) == (1, 1, (0,))
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
    assert not bool(out["mink_raw"].any()) and bool((out["mink_equal"] == 3).all())      # zeros are not above zero
    assert out["mink_raw"].is_cuda and out["mink_raw"].dtype == torch.int64 and tuple(out["mink_raw"].shape) == (2, 2, 1, 4, 1, 5)
    with pytest.raises(ValueError, match="fed in order"):
        acc.add(y, 0, y)


# ---- end to end: modelPredMorphology against the reference over modelPred's samples -------------------------------------------------------
def test_model_pred_morphology_matches_the_reference_over_model_pred(monkeypatch, tmp_path):
    """The keys shared with modelPredStats are identical, and the raw counts equal the reference fed with modelPred's roll-outs.
    modelPred un-normalises in fp32 (three roundings, tests/test_events_gpu.py), so a physical value within 4 u * scale of a level may
    fall on either side of it: those comparisons are counted, and when there is none (the usual case) every output is held to the
    reference bit for bit; in every case N, (Nh, Nv) and (Nq, Nd) of a level differ by at most 1, 2 and 4 times their number.  The default ladder is the target's mean +- 2 std."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = E._cylinder_case(tmp_path)
    S, tmax, stride, t_start, max_rows, J = 5, 6, 2, 1, 4, 3
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=K.GRID[0], dy=K.GRID[1])
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    tall = torch.cat([b[1].cpu() for b in te]).double().numpy()                    # the normalised target series [N, T, C, H, W]
    fields = (2, 0)
    phys = [u0.reshape(-1, 1, 1, 1) ** (2 if ch == 2 else 1) * (sd[ch] * tall[:, :, ch] + mu[ch]) for ch in fields]
    thresholds = tuple(tuple(float(v) for v in np.quantile(p, (0.25, 0.5, 0.75))) for p in phys)
    for _ in range(3):                                                        # three folded runs: morphology, stats, default ladder
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
    got = utils.modelPredMorphology(args, model, te, E.LOG, fields=fields, thresholds=thresholds, **kw)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, **kw)
    torch.manual_seed(77)
    auto = utils.modelPredMorphology(args, model, te, E.LOG, fields=fields, levels=5, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    for res in (got, auto):
        assert set(res) == set(stats) | set(K.ALL_KEYS) | {"fields"} and res["fields"] == fields
        for name, v in stats.items():
            assert torch.equal(res[name], v), name
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    timed = tuple(j >= t_start for j in range(Tk))
    # the default ladder: 5 levels on the mean +- 2 population std of the target over the timed steps
    yt = y[:, [j for j in range(Tk) if timed[j]]][:, :, list(fields)].transpose(0, 2, 1, 3, 4).reshape(N, len(fields), -1)
    want_lv = yt.mean(-1, keepdims=True) + yt.std(-1, keepdims=True) * np.linspace(-2.0, 2.0, 5)
    lv_auto = auto["mink_levels"].numpy()
    assert lv_auto.shape == (N, len(fields), 5) and lv_auto.dtype == np.float64
    assert bool((np.abs(lv_auto - want_lv) <= 1e-12 * np.abs(want_lv).max()).all())
    assert np.array_equal(got["mink_levels"].numpy(), np.broadcast_to(np.array(thresholds), (N, len(fields), J)))
    xs = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5)).astype(np.float64)
    ys = np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]
    xn = (p / uc.reshape(1, N, 1, Cc, 1, 1) - mu[:Cc].reshape(1, 1, 1, Cc, 1, 1)) / sd[:Cc].reshape(1, 1, 1, Cc, 1, 1)
    scale = uc.reshape(N, 1, Cc, 1, 1) * (sd[:Cc].reshape(1, 1, Cc, 1, 1) * np.maximum(np.abs(xn).max(0), np.abs(tall[:, ::stride][:, :Tk]))
                                          + np.abs(mu[:Cc]).reshape(1, 1, Cc, 1, 1))            # [N, Tk, C, H, W]
    for res, name in ((got, "given"), (auto, "default")):
        lv = res["mink_levels"].numpy()                                      # [N, F, J] physical, fp64
        ref = np.zeros(tuple(res["mink_raw"].shape), np.int64)
        near = np.zeros(ref.shape[:-1], np.int64)                            # per (case, step, field, row, level): comparisons that may fall either way
        for b in range(N):
            for t in range(Tk):
                for f, ch in enumerate(fields):
                    for m in range(S + 1):
                        x = ys[t, b, ch] if m == S else xs[t, m, b, ch]
                        ref[b, t, f, m] = _counts64(x, lv[b, f])
                        near[b, t, f, m] = [(np.abs(x - v) <= 4 * K.U24 * scale[b, t, ch]).sum() for v in lv[b, f]]
        g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in res.items()}
        # a pixel lies in 1 count of N, in 2 horizontal and 2 vertical pairs and in 4 quads: the five counts of a level move by at
        # most that often the pixels within the rounding of that level (the ladders ascend: only they can change sides)
        assert g["mink_raw"].dtype == np.int64
        for q, per_pixel in enumerate((1, 2, 2, 4, 4)):
            assert bool((np.abs(g["mink_raw"][..., q] - ref[..., q]) <= per_pixel * near).all()), (name, q)
        print("%s ladder: comparisons within the rounding of their level: %d of %d" % (name, int(near.sum()), near.size * Hh * Ww))
        assert near.sum() <= 1e-3 * near.size * Hh * Ww
        if not near.any():
            want = K.full_reference(ref, S, Hh, Ww, K.GRID, lv, timed)
            assert not K.mismatches(g, want, ("mink_raw", "time_mink_raw") + K.INT_KEYS + TIME_INT), name
            worst = K.check_floats(g, want, FLOATS, "cylinder, %s ladder" % name)
            print("every output held to the reference; worst share of the float tolerance %.3f" % worst)


def _counts64(x, lv):
    """K.counts on fp64 physical values against an fp64 physical ladder (u out_std > 0 keeps the order)."""
    J = len(lv)
    rank = sum((x > v).astype(np.int64) for v in lv)
    out = np.zeros((J, 5), np.int64)
    for j in range(J):
        m = rank > j
        a, b, c, d = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
        out[j] = (m.sum(), (m[:, :-1] & m[:, 1:]).sum(), (m[:-1] & m[1:]).sum(), (a & b & c & d).sum(),
                  ((a & d & ~b & ~c) | (b & c & ~a & ~d)).sum())
    return out
