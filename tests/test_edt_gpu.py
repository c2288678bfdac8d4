"""Distance-map verification on the device (`-m gpu`): tmg_ens_edt_chunk / tmg_ens_edt_step through tmg_ops.EnsembleDistance against the
int64 reference of tests/edt_cases.py (row distances by broadcasting, the minimum over the rows, math.isqrt, bincount; held against the
all-pairs minimum and scipy's transform on the CPU), and utils.modelPredDistance against the same reference over modelPred's samples.

Everything the device forms is an integer: dist_pair_raw, dist_hist_raw, the time maps and the target's distance map must EQUAL the
reference bit for bit, on integer data (thresholds ON a value, so strictness shows), on smooth fields, a checkerboard, a single set
pixel in a corner (the search with no early exit), far blobs, a pixel exactly the cutoff away, empty and full sets, NaN and infinities
planted, and a set pixel on each side of every 64-column word edge and 64-row band edge; it is bitwise the same for every chunking
and for two runs.  Every case runs with the scratch words, the set sizes, the step tables, the member sum and the target's map
pre-filled with garbage: the step's first chunk presets or overwrites them.  The float32 outputs lie within 2^-24 |ref| + 2^-40 of the
fp64 restatement of tmg_ops.dist_outputs."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import edt_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
GARBAGE = -1077952577 * 4294967296 + 12345
GARBAGE32 = -1077952577


def _nhwc(v, Cc, padded):
    """API-shaped [n, C, H, W] whose channels-last view is dense, or a channel slice at offset 1 of 4-channel NaN-filled storage."""
    v = v.permute(0, 2, 3, 1)
    if not padded:
        return v.contiguous().permute(0, 3, 1, 2)
    wide = torch.full(tuple(v.shape[:3]) + (4,), float("nan"), device=v.device)
    wide[..., 1:1 + Cc] = v
    return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)


def run_edt(case, xs, tgt, sizes):
    """Feed EnsembleDistance as utils.modelPredDistance does, in chunks of `sizes` members per step, the steps timed as K.TIMED.
    Every buffer the step's first chunk must preset is pre-filled with garbage.  -> dict of numpy arrays (with the target's map of
    the last step as d2_target) and the plan."""
    import tmg_ops as ops
    S, B, Cc, hw, Kk, c, kind, padded = case
    Tk = xs.shape[0]
    xd = torch.from_numpy(np.array(xs)).to(DEV)                              # (a copy: the cached inputs are read-only)
    td = torch.from_numpy(np.array(tgt)).to(DEV)
    assert not padded or Cc <= 3
    acc = ops.EnsembleDistance(S, B, Cc, hw[0], hw[1], Tk, DEV, torch.zeros(Cc), torch.ones(Cc), events=K.events_for(Cc, Kk), cutoff=c,
                               quantiles=K.QUANTILES)
    assert torch.equal(acc.thr.cpu(), torch.from_numpy(K.thresholds(case)))  # out_mu = 0, out_std = 1, u = 1: the values themselves
    for buf in (acc.scratch, acc.pair, acc.hist):
        buf.fill_(GARBAGE)
    for buf in (acc.count, acc.dmap, acc.msum):
        buf.fill_(GARBAGE32)
    for t in range(Tk):
        target = _nhwc(td[t], Cc, padded)
        m0 = 0
        for k in sizes:
            acc.add(_nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, hw[0], hw[1]), Cc, padded), m0, target, time=K.TIMED[t])
            m0 += k
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in acc.finalize().items()}
    out["d2_target"] = acc.dmap.cpu().numpy().reshape(B, Kk, hw[0], hw[1])
    return out, acc.plan


def check_all(got, ref, case, what):
    S, B, Cc, hw, Kk, c, kind, _ = case
    assert set(got) == set(K.ALL_KEYS) | {"d2_target"}
    want = K.full_reference(ref, S, hw[0], hw[1], c, K.QUANTILES)
    bad = K.mismatches(got, want, K.INT_KEYS + K.META_KEYS)
    assert not bad, "%s: %s differ from the integer reference" % (what, bad)
    assert got["d2_target"].dtype == np.int32 and np.array_equal(got["d2_target"], ref["d2_target"][:, -1]), what
    for k in K.INT_KEYS:
        assert got[k].dtype == np.int64, k
    return K.check_floats(got, want, K.ALL_FLOAT_KEYS, what)


# ---- every case of the table, in three chunkings and twice ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_raw_tables_and_maps_equal_the_reference_bit_for_bit_for_every_chunking(idx):
    case = K.TABLE[idx]
    S, B, Cc, hw, Kk, c, kind, padded = case
    xs, tgt = K.inputs(idx)
    ref = K.case_reference(idx)
    outs = []
    for kd in (0, 1, 2, 2):
        got, plan = run_edt(case, xs, tgt, K.chunk_sizes(S, kd))
        assert (plan["band"], plan["tile_w"]) == K.TILE
        worst = check_all(got, ref, case, "%s chunks %s" % (case, K.chunk_sizes(S, kd)))
        outs.append(got)
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name
    print("%s: %d blocks; worst share of the float tolerance %.3f" % (case, plan["blocks"], worst))


def test_the_field_sizes_sit_on_the_edges_of_the_plans_strip_and_band():
    import tmg_hip as H
    p = H.ens_edt_plan(2, 1, 70, 70, 1, 5)
    th, tw = p["band"], p["tile_w"]
    assert (th, tw) == K.TILE and (p["strips"], p["bands"]) == (2, 2)
    sizes = {c[3] for c in K.TABLE}
    assert {(th, tw), (th + 1, tw - 1), (th + 6, tw + 6), (3, 2 * tw + 2), (2, 4 * tw + 44), (3 * th + 8, tw + 6), (2 * th + 2, 2 * tw + 2)} <= sizes
    assert H.ens_edt_plan(5, 1, 200, 70, 1, 255)["bands"] == 4 and H.ens_edt_plan(5, 1, 2, 300, 1, 255)["strips"] == 5


def test_nan_is_in_no_event_and_an_infinity_only_on_its_side():
    import tmg_ops as ops
    S, B, Cc, Hh, Ww, c = 3, 1, 2, 3, 70, 5
    ev = ((1, 0.0, ">"), (0, 0.0, "<"))
    xs = np.full((1, S, B, Cc, Hh, Ww), np.nan, np.float32)                    # member 0: NaN, in no event
    xs[0, 1] = np.inf                                                         # member 1: in the ">" event everywhere, never in "<"
    xs[0, 2] = -np.inf
    tgt = np.full((1, B, Cc, Hh, Ww), 1.0, np.float32)
    tgt[0, 0, :, 1, 65] = np.nan
    acc = ops.EnsembleDistance(S, B, Cc, Hh, Ww, 1, DEV, torch.zeros(Cc), torch.ones(Cc), events=ev, cutoff=c)
    for buf in (acc.scratch, acc.pair, acc.hist):
        buf.fill_(GARBAGE)
    for buf in (acc.count, acc.dmap, acc.msum):
        buf.fill_(GARBAGE32)
    acc.add(torch.from_numpy(xs[0].reshape(S * B, Cc, Hh, Ww)).to(DEV).contiguous(memory_format=torch.channels_last), 0,
            torch.from_numpy(tgt[0]).to(DEV).contiguous(memory_format=torch.channels_last))
    out = acc.finalize()
    pair = out["dist_pair_raw"].cpu().numpy()
    HW = Hh * Ww
    assert pair[0, 0, :, :, 0].tolist() == [[0, HW, 0], [0, 0, HW]] and pair[0, 0, :, 0, 1].tolist() == [HW - 1, 0]
    ref = K.reference(xs, tgt, np.zeros((B, 2), np.float32), ev, c)
    assert np.array_equal(pair, ref["pair"]) and np.array_equal(out["dist_hist_raw"].cpu().numpy(), ref["hist"])
    assert np.array_equal(out["time_dist_member_sum"].cpu().numpy(), ref["w_members"][:, 0])
    assert np.array_equal(acc.dmap.cpu().numpy().reshape(B, 2, Hh, Ww), ref["d2_target"][:, 0])


def test_return_codes_come_before_any_launch():
    import tmg_hip as H
    S, B, Cc, Hh, Ww, Kk, c = 3, 2, 3, 5, 7, 2, 5
    i64, i32 = dict(device=DEV, dtype=torch.int64), dict(device=DEV, dtype=torch.int32)
    bufs = dict(scratch=torch.full((S + 1, B, Kk, Hh, 1), 77, **i64), count=torch.full((B, Kk, S + 1), 77, **i32),
                dmap=torch.full((B, Kk, Hh * Ww), 77, **i32), msum=torch.full((B, Kk, Hh * Ww), 77, **i32),
                pair=torch.full((B, Kk, S, 11), 77, **i64), hist=torch.full((B, Kk, S, 2, c + 1), 77, **i64))
    thr = torch.zeros(B, Kk, device=DEV)
    y = torch.zeros(2 * B, Hh, Ww, Cc, device=DEV)
    tg = torch.zeros(B, Hh, Ww, Cc, device=DEV)
    ev = ((0, 0), (2, 1))
    chunk = lambda **kw: H.ens_edt_chunk(**dict(dict(y=y, target=tg, thr=thr, ev=ev, S=S, k=2, m0=0, code=True, **bufs), **kw))  # noqa: E731
    assert chunk(m0=2) == -1 and chunk(m0=-1) == -1 and chunk(k=1, m0=3, y=y[:B]) == -1
    assert chunk(ev=((0, 0), (3, 1))) == -1 and chunk(ev=((0, 2), (1, 1))) == -1 and chunk(ev=((-1, 0), (1, 1))) == -1
    wide = torch.full((B, Kk, S, 2, 257), 77, **i64)
    assert chunk(hist=wide) == -1                                             # c = 256
    tmem, ttgt = torch.full((B, Kk, Hh * Ww), 77, **i64), torch.full((B, Kk, Hh * Ww), 77, **i64)
    assert H.ens_edt_step(bufs["msum"], bufs["dmap"], tmem, ttgt, Hh, Ww, 0, code=True) == -1
    assert H.ens_edt_step(bufs["msum"], bufs["dmap"], tmem, ttgt, Hh, Ww, 256, code=True) == -1
    # a null pointer: -3, straight through the C entry (the wrapper cannot pass one)
    i64s = lambda *v: (ctypes.c_int64 * len(v))(*v)                           # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    lib, evs, yd, nul = H.lib(), i64s(0, 0, 2, 1), i64s(Cc, 0), ctypes.c_void_p(0)
    cd = i64s(2, B, Hh, Ww, Cc, S, 0, Kk, c)
    six = [vp(bufs[n]) for n in ("scratch", "count", "dmap", "msum", "pair", "hist")]
    for i in range(6):
        assert lib.tmg_ens_edt_chunk(vp(y), yd, vp(tg), yd, vp(thr), evs, *[nul if j == i else b for j, b in enumerate(six)], cd, nul) == -3
    assert lib.tmg_ens_edt_chunk(vp(y), yd, nul, yd, vp(thr), evs, *six, cd, nul) == -3
    assert lib.tmg_ens_edt_chunk(vp(y), None, vp(tg), yd, vp(thr), evs, *six, cd, nul) == -3
    assert lib.tmg_ens_edt_step(vp(bufs["msum"]), vp(bufs["dmap"]), nul, vp(ttgt), i64s(B, Hh, Ww, Kk, c), nul) == -3
    with pytest.raises(RuntimeError):
        chunk(m0=2, code=False)
    with pytest.raises(RuntimeError, match="pair is a contiguous"):
        chunk(pair=bufs["pair"][:, :, :2])
    with pytest.raises(RuntimeError, match="scratch is a contiguous"):
        chunk(scratch=bufs["scratch"][:S])
    with pytest.raises(RuntimeError, match="thr is a contiguous"):
        chunk(thr=thr[:1])
    with pytest.raises(RuntimeError, match="tmem is a contiguous"):
        H.ens_edt_step(bufs["msum"], bufs["dmap"], tmem[:1], ttgt, Hh, Ww, c)
    torch.cuda.synchronize()
    assert all(bool((v == 77).all()) for v in list(bufs.values()) + [wide, tmem, ttgt])      # nothing was launched
    assert chunk() == 0 and chunk(m0=2, k=1, y=y[:B]) == 0                    # and the good calls are taken
    assert H.ens_edt_step(bufs["msum"], bufs["dmap"], tmem, ttgt, Hh, Ww, c, code=True) == 0
    torch.cuda.synchronize()
    # zeros are not below zero, nor above: every set is empty, every distance INF, every w the cutoff
    HW = Hh * Ww
    want = [0, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1]
    assert bufs["pair"].cpu().reshape(-1, 11).tolist() == [want] * (B * Kk * S) and not bool(bufs["hist"].any())
    assert bool((bufs["dmap"] == K.INF).all()) and bool((bufs["msum"] == S * 256 * c).all()) and not bool(bufs["count"].any())
    assert bool((tmem == 77 + S * 256 * c).all()) and bool((ttgt == 77 + 256 * c).all()) and HW == 35


def test_feeding_errors_are_the_class_errors():
    import tmg_ops as ops
    acc = ops.EnsembleDistance(3, 2, 3, 4, 5, 2, DEV, torch.zeros(3), torch.ones(3))
    assert (acc.K, acc.cutoff, acc.quantiles, acc.events) == (1, 1, (0.5, 0.75, 0.9), [(0, 0.0, "<")])
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
    assert out["dist_pair_raw"].is_cuda and out["dist_pair_raw"].dtype == torch.int64 and tuple(out["dist_pair_raw"].shape) == (2, 2, 1, 3, 11)
    assert tuple(out["dist_hist_raw"].shape) == (2, 2, 1, 3, 2, 2) and tuple(out["time_dist_mean_map"].shape) == (2, 1, 4, 5)
    assert bool((out["dist_hausdorff"] == 0).all()) and bool(torch.isnan(out["dist_med"]).all())     # zeros are not below zero: all empty
    assert bool((out["time_dist_member_sum"] == 2 * 3 * 256).all()) and bool((out["time_dist_bias_map"] == 0).all())
    assert int(out["dist_cutoff"]) == 1 and out["dist_quantiles"].tolist() == [0.5, 0.75, 0.9]
    with pytest.raises(ValueError, match="fed in order"):
        acc.add(y, 0, y)


# ---- end to end: modelPredDistance against the reference over modelPred's samples -------------------------------------------------------
def test_model_pred_distance_matches_the_reference_over_model_pred(monkeypatch, tmp_path):
    """The keys shared with modelPredStats are identical, the raw tables equal the reference fed with modelPred's roll-outs, and the
    set sizes agree with modelPredEvents' reliability table (it keeps no per-member counts: the sum over the members of nA is the sum
    over j of j rel_count[j], and nO the sum of rel_hit).  modelPred un-normalises in fp32 (three roundings,
    tests/test_events_gpu.py), so a physical value within 4 u * scale of an event's value may fall on either side of it: those
    comparisons are counted, and when there is none (the usual case) every output is held to the reference bit for bit; otherwise
    the set sizes may differ by at most their number."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = E._cylinder_case(tmp_path)
    S, tmax, stride, t_start, max_rows, c = 5, 6, 2, 1, 4, 7
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    tall = torch.cat([b[1].cpu() for b in te]).double().numpy()                    # the normalised target series [N, T, C, H, W]
    ulow = float(np.quantile(u0.reshape(-1, 1, 1, 1) * (sd[0] * tall[:, :, 0] + mu[0]), 0.2))
    phigh = float(np.quantile(u0.reshape(-1, 1, 1, 1) ** 2 * (sd[2] * tall[:, :, 2] + mu[2]), 0.9))
    events = ((0, ulow, "<"), (2, phigh, ">"))
    for _ in range(3):                                                        # three folded runs: distances, stats, events
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
    got = utils.modelPredDistance(args, model, te, E.LOG, events=events, cutoff=c, quantiles=K.QUANTILES, **kw)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, **kw)
    torch.manual_seed(77)
    evs = utils.modelPredEvents(args, model, te, E.LOG, events=events, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(stats) | set(K.ALL_KEYS) | {"events"}
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    assert got["events"] == events and int(got["dist_cutoff"]) == c and got["dist_quantiles"].tolist() == list(K.QUANTILES)
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    j = np.arange(S + 1)
    assert np.array_equal(g["dist_pair_raw"][..., 0].sum(-1), (evs["rel_count"].numpy() * j).sum(-1))
    assert np.array_equal(g["dist_pair_raw"][..., 1], np.broadcast_to(evs["rel_hit"].numpy().sum(-1)[..., None], g["dist_pair_raw"].shape[:-1]))
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
    ref = K.reference(xs, ys, thr, events, c)
    near_n = np.stack([(np.abs(p[:, :, :, ch] - v) <= 4 * K.U24 * scale[None, :, :, ch]).sum(0) for ch, v, _ in events], 2)   # [N, Tk, K, H, W]
    near_o = np.stack([np.abs(y[:, :, ch] - v) <= 4 * K.U24 * scale[:, :, ch] for ch, v, _ in events], 2).astype(np.int64)
    near_total = int(near_n.sum() + near_o.sum())
    near = (near_n + S * near_o).sum((-2, -1))                               # [N, Tk, K]: the comparisons that may fall either way
    assert bool((np.abs(g["dist_pair_raw"][..., 0] - ref["pair"][..., 0]).sum(-1) <= near).all())
    assert bool((np.abs(g["dist_pair_raw"][..., 0, 1] - ref["pair"][..., 0, 1]) <= near).all())
    assert (ref["pair"][..., 0] > 0).any() and (ref["pair"][..., 1] > 0).any()                    # the events happen
    print("comparisons within the rounding of their threshold: %d of %d" % (near_total, near_n.size * (S + 1)))
    assert near_total <= 1e-3 * near_n.size
    if near_total == 0:
        timed = tuple(jj >= t_start for jj in range(Tk))
        want = K.full_reference(ref, S, Hh, Ww, c, K.QUANTILES, timed)
        assert not K.mismatches(g, want, K.INT_KEYS)
        worst = K.check_floats(g, want, K.ALL_FLOAT_KEYS, "cylinder")
        print("every output held to the reference; worst share of the float tolerance %.3f" % worst)
