"""Ensemble event durations on the device (`-m gpu`): tmg_ens_spell_step / tmg_ens_spell_finalize through tmg_ops.EnsembleSpells
against the int64 reference of tests/spell_cases.py (run-length encoding by np.diff, held against a second statement on the CPU), and
utils.modelPredSpells against the same reference over modelPred's samples.

Everything the device forms is an integer: the four tables and the seven maps must EQUAL the reference bit for bit, on integer data
(thresholds ON a value, so strictness shows), on AR(1) data (run lengths vary) and with NaN and infinities planted; they are bitwise
the same for every chunking and for two runs.  Every case runs with the state, the tables and the maps pre-filled with garbage: step 0
writes the state without reading it, the first step call zeroes the tables, the first chunk writes the maps.  The float32 outputs lie
within 2^-24 |ref| + 2^-40 of the fp64 restatement of tmg_ops.spell_outputs."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import spell_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
GARBAGE = -1077952577                                                         # 0xBFBFBFBF as int32
INT_KEYS = K.TABLE_KEYS + K.MAP_KEYS + K.INT_HOST_KEYS
FLOAT_KEYS = K.FLOAT_HOST_KEYS + K.FLOAT_MAP_KEYS


def run_spells(xs, tgt, events, L, sizes, padded):
    """Feed EnsembleSpells as utils.modelPredSpells does, in chunks of `sizes` members per step; padded: y and target are channel
    slices at offset 1 of 4-channel NaN-filled NHWC buffers.  Every buffer the kernels write is pre-filled with garbage.  -> dict of
    numpy arrays and the plan."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    xd = torch.from_numpy(np.array(xs)).to(DEV)                              # (a copy: the cached inputs are read-only)
    td = torch.from_numpy(np.array(tgt)).to(DEV)

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (4,), float("nan"), device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    assert not padded or Cc <= 3
    sp = ops.EnsembleSpells(S, B, Cc, Hh, Ww, Tn, DEV, torch.zeros(Cc), torch.ones(Cc), events=events, max_len=L)
    sp.state = torch.empty_like(sp.state)
    for v in (sp.state, sp.maps):
        v.fill_(GARBAGE)
    sp.table.fill_(GARBAGE * 4294967296 + 12345)
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            sp.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target)
            m0 += k
    out = sp.finalize()
    assert sp.finalize() is out                                               # finalize counts the open runs once
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}, sp.plan


def check_all(got, ref, case, what):
    S, B, Cc, hw, Kn, Tn, L, kind, _ = case
    assert set(got) == set(K.ALL_KEYS)
    want = dict(ref)
    want.update(K.host_reference(ref, S, ref))
    bad = K.mismatches(got, want, INT_KEYS)
    assert not bad, "%s: %s differ from the integer reference" % (what, bad)
    K.check_identities(got, Tn, hw[0] * hw[1])
    assert np.array_equal(got["spell_bins"], np.arange(1, L + 1)) and got["spell_bins"].dtype == np.int64
    return K.check_floats(got, want, FLOAT_KEYS, what)


# ---- every case of the table, in three chunkings and twice ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_tables_and_maps_equal_the_reference_bit_for_bit_for_every_chunking(idx):
    case = K.TABLE[idx]
    S, B, Cc, hw, Kn, Tn, L, kind, padded = case
    xs, tgt = K.inputs(idx)
    events = K.events_for(Cc, Kn)
    ref = K.case_reference(idx)
    outs = []
    for kd in (0, 1, 2, 2):
        got, plan = run_spells(xs, tgt, events, L, K.chunk_sizes(S, kd), padded)
        assert plan["group"] == K.group(Kn, L)
        worst = check_all(got, ref, case, "%s chunks %s" % (case, K.chunk_sizes(S, kd)))
        outs.append(got)
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True), name
    print("%s: group %d, lds %d B, %d blocks; worst share of the float tolerance %.3f"
          % (case, plan["group"], plan["lds_bytes"], plan["blocks"], worst))


def test_a_window_of_300_steps_keeps_its_run_lengths():
    """A state word narrower than 15 bits of length would wrap: the always-in pixel gives one both-run of 300 steps."""
    case = K.LONG_CASE
    S, B, Cc, hw, Kn, Tn, L, kind, padded = case
    assert (S, B, Kn, hw[0] * hw[1], Tn) == (1, 1, 1, 35, 300)
    xs, tgt = K.make_inputs(case, 31)
    events = K.events_for(Cc, Kn)
    got, _ = run_spells(xs, tgt, events, L, [1], padded)
    check_all(got, K.reference(xs, tgt, K.thresholds(events, B), events, L), case, "long window")
    for key in ("time_longest_max", "time_longest_sum", "target_longest", "time_in_count", "target_in_count"):
        assert int(got[key].reshape(-1)[0]) == 300, key
    assert int(got["time_spell_count"].reshape(-1)[0]) == 1 and int(got["target_longest"].reshape(-1)[1]) == 0
    # pixel 0 of the member is the only spell that covers the window (the AR(1) pixels change sign within 300 steps)
    assert got["spell_cens"][0, 0, 0, 1, 2] == 1 and got["spell_cens_len"][0, 0, 0, 1, 2] == 300
    assert got["spell_cens"][0, 0, 1, 1, 2] == 1 and got["spell_cens_len"][0, 0, 1, 1, 2] == 300


def test_nan_and_infinities_are_in_no_event_they_compare_false_to():
    case = K.NONFINITE_CASE
    S, B, Cc, hw, Kn, Tn, L, kind, padded = case
    xs, tgt = K.make_inputs(case, 41)
    K.plant_nonfinite(xs, tgt, 42)
    assert np.isnan(xs).any() and np.isnan(tgt).any() and np.isinf(xs).any() and np.isinf(tgt).any()
    events = K.events_for(Cc, Kn)
    ref = K.reference(xs, tgt, K.thresholds(events, B), events, L)
    assert K.mismatches(K.reference(xs, tgt, K.thresholds(events, B), events, L, "nan_in_event"), ref, K.TABLE_KEYS)
    for kd in (0, 2):
        got, _ = run_spells(xs, tgt, events, L, K.chunk_sizes(S, kd), padded)
        check_all(got, ref, case, "non-finite, chunks %s" % K.chunk_sizes(S, kd))


def test_return_codes_come_before_any_launch():
    import tmg_hip as H
    S, B, Cc, Hh, Ww, Kn, L, Tn = 3, 2, 3, 5, 7, 2, 4, 5
    i32 = dict(device=DEV, dtype=torch.int32)
    state = torch.full((S + 1, B, Kn, Hh * Ww), GARBAGE, **i32)
    table = torch.full((B, Kn, S + 1, 2, L + 7), 77, device=DEV, dtype=torch.int64)
    maps = torch.full((7, B, Kn, Hh * Ww), GARBAGE, **i32)
    thr = torch.zeros(B, Kn, device=DEV)
    y = torch.zeros(2 * B, Hh, Ww, Cc, device=DEV)
    ev = ((0, 0), (2, 1))
    step = lambda **kw: H.ens_spell_step(**dict(dict(y=y, thr=thr, ev=ev, state=state, table=table, maps=maps, S=S, k=2, row0=0, Tn=Tn, t=0,  # noqa: E731
                                                     code=True), **kw))
    assert step(t=Tn) == -1 and step(t=-1) == -1 and step(row0=2) == -1 and step(row0=S) == -1 and step(Tn=1) == -1
    assert step(ev=((3, 0), (2, 1))) == -1 and step(ev=((0, 2), (2, 1))) == -1
    assert step(Tn=32768) == -2
    assert H.ens_spell_finalize(state, table, maps, 1, code=True) == -1 and H.ens_spell_finalize(state, table, maps, 32768, code=True) == -2
    with pytest.raises(RuntimeError):
        step(Tn=1, code=False)
    with pytest.raises(RuntimeError, match="state is a contiguous"):
        step(state=state[:S])
    torch.cuda.synchronize()
    assert bool((state == GARBAGE).all()) and bool((table == 77).all()) and bool((maps == GARBAGE).all())   # nothing was launched


def test_feeding_errors_are_the_windowed_class_errors():
    import tmg_ops as ops
    sp = ops.EnsembleSpells(3, 2, 3, 4, 5, 2, DEV, torch.zeros(3), torch.ones(3))
    y = torch.zeros(2, 3, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="target shape None"):
        sp.add(y, 0, None)
    with pytest.raises(ValueError, match="whole members"):
        sp.add(y[:1], 0, y)
    with pytest.raises(ValueError, match="fed in order"):
        sp.add(y, 1, y)
    with pytest.raises(RuntimeError, match="0 of 2 steps"):
        sp.finalize()
    for _ in range(2):
        for m in range(3):
            sp.add(y, m, y)
    out = sp.finalize()
    assert int(out["spell_cens"][..., 0, 2].sum()) == 2 * 4 * 20              # zeros are not below zero: one gap per row and pixel
    with pytest.raises(ValueError, match="fed in order"):
        sp.add(y, 0, y)


# ---- end to end: modelPredSpells against the reference over modelPred's samples ---------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_spells_matches_the_reference_over_model_pred(monkeypatch, tmp_path, case):
    """The keys shared with modelPredStats are identical, time_in_count is modelPredEvents' time_event_count, and the tables and maps
    equal the reference fed with modelPred's roll-outs.  modelPred un-normalises in fp32 (three roundings, tests/test_events_gpu.py),
    so a physical value within 4 u * scale of an event's value may fall on either side of it: those comparisons are counted, the
    per-pixel count may differ by at most their number at the pixel, and when there is none (the usual case) every output is held
    to the reference bit for bit."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows, L = 5, 6, 2, 0, 4, 2
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
    for _ in range(3):                                                        # three folded runs: spells, events, stats
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
    got = utils.modelPredSpells(args, model, te, E.LOG, events=events, max_len=L, **kw)
    torch.manual_seed(77)
    evs = utils.modelPredEvents(args, model, te, E.LOG, events=events, scales=(1,), **kw)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(stats) | set(K.ALL_KEYS) | {"events"}
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    assert got["events"] == events and np.array_equal(got["spell_bins"].numpy(), np.arange(1, L + 1))
    assert torch.equal(got["time_in_count"], evs["time_event_count"])
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    xs = np.ascontiguousarray(p.transpose(2, 0, 1, 3, 4, 5))[t_start:]
    ys = np.ascontiguousarray(y.transpose(1, 0, 2, 3, 4))[t_start:]
    Tn = xs.shape[0]
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]
    xn = (p / uc.reshape(1, N, 1, Cc, 1, 1) - mu[:Cc].reshape(1, 1, 1, Cc, 1, 1)) / sd[:Cc].reshape(1, 1, 1, Cc, 1, 1)
    scale = uc.reshape(N, 1, Cc, 1, 1) * (sd[:Cc].reshape(1, 1, Cc, 1, 1) * np.maximum(np.abs(xn).max(0), np.abs(tall[:, ::stride][:, :Tk]))
                                          + np.abs(mu[:Cc]).reshape(1, 1, Cc, 1, 1))            # [N, Tk, C, H, W]
    thr = np.array([[v for _, v, _ in events]] * N)
    ref = K.reference(xs, ys, thr, events, L)
    near_n = np.stack([(np.abs(p[:, :, :, ch] - v) <= 4 * K.U24 * scale[None, :, :, ch]).sum(0) for ch, v, _ in events], 2)   # [N, Tk, K, H, W]
    near_o = np.stack([np.abs(y[:, :, ch] - v) <= 4 * K.U24 * scale[:, :, ch] for ch, v, _ in events], 2).astype(np.int64)
    near_total = int(near_n[:, t_start:].sum() + near_o[:, t_start:].sum())
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    assert bool((np.abs(g["time_in_count"] - ref["time_in_count"]) <= near_n[:, t_start:].sum(1)).all()), "%s time_in_count" % case
    assert bool((np.abs(g["target_in_count"] - ref["target_in_count"]) <= near_o[:, t_start:].sum(1)).all()), "%s target_in_count" % case
    K.check_identities(g, Tn, Hh * Ww)
    print("%s: comparisons within the rounding of their threshold: %d of %d" % (case, near_total, near_n.size * (S + 1)))
    assert near_total <= 1e-3 * near_n.size
    if near_total == 0:
        want = dict(ref)
        want.update(K.host_reference(ref, S, ref))
        assert not K.mismatches(g, want, INT_KEYS)
        worst = K.check_floats(g, want, FLOAT_KEYS, case)
        print("%s: every output held to the reference; worst share of the float tolerance %.3f" % (case, worst))
