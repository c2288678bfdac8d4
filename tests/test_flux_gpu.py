"""Ensemble energy flux on the device (`-m gpu`): tmg_ens_flux_accum and tmg_ens_flux_terms through tmg_ops.EnsembleFlux against the
references of tests/flux_cases.py (a float32 numpy mirror of the state; an int64 reference on integer data; the fp64 direct sums;
the fp64 reference by direct definition with the full physical velocity; the fp64 host restatement of the finalize formulas on the
device's own state), two known answers, and utils.modelPredFlux against the definition over modelPred's samples.  The definitions,
the counts c_Q = 4 w + 1, c_A = 6 w + 6, c_P = c_A + 3, C_FIN = 24 and the bounds are in tests/flux_cases.py.  The tests print the worst
share of the bound they reach.

Worst share of the bound reached on an MI355X: raw against the fp64 direct sums 0.19; the fields against the host restatement 0.998
(the output's rounding to fp32), against the definition 0.80; the known answers 0.11 (pure strain) and 0.14 (diagonal ramp); end to
end 0.72."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import flux_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
NAN = float("nan")


def nhwc(v, padded):
    """[rows, 3, H, W] -> an API-shaped view whose channels-last form is dense, or a channel slice of a wider NaN-filled buffer."""
    v = v.permute(0, 2, 3, 1)
    if not padded:
        return v.contiguous().permute(0, 3, 1, 2)
    wide = torch.full(tuple(v.shape[:3]) + (6,), NAN, device=v.device)
    wide[..., 1:4] = v
    return wide[..., 1:4].permute(0, 3, 1, 2)


def feed(en, xs, sizes, padded, timed):
    """Feed the accumulator as utils.modelPredFlux does (row S of xs is the target) -> the state's clone after every step."""
    steps, R, B = xs.shape[:3]
    S, (Hh, Ww) = R - 1, xs.shape[-2:]
    xd = torch.from_numpy(xs).to(DEV)
    snaps = []
    for t in range(steps):
        target = nhwc(xd[t, S], padded)
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, 3, Hh, Ww), padded), m0, target, time=t in timed)
            m0 += k
        assert m0 == S
        snaps.append(en.raw.cpu().numpy().copy())
    return snaps


def run(xs, sd, mu, u, grid, widths, sizes, padded, timed, per_member=True, prefill=NAN):
    """EnsembleFlux over the rows xs [steps, S + 1, B, 3, H, W] -> dict of numpy arrays: the outputs, raw, the snapshots."""
    import tmg_ops as ops
    steps, R, B = xs.shape[:3]
    Hh, Ww = xs.shape[-2:]
    en = ops.EnsembleFlux(R - 1, B, 3, Hh, Ww, steps, DEV, torch.zeros(3) if mu is None else torch.from_numpy(mu),
                          torch.ones(3) if sd is None else torch.from_numpy(sd), u=None if u is None else torch.from_numpy(u), grid=grid,
                          widths=widths, per_member=per_member)
    if prefill is not None:
        en.raw.fill_(prefill)                                                # the first timed step stores: nothing of this survives at a valid pixel
    snaps = feed(en, xs, sizes, padded, timed)
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in en.finalize().items()}
    got.update(raw=en.raw.cpu().numpy(), snaps=snaps, a=en.a.cpu().numpy(), kk=en.kk.cpu().numpy(), k64=en.k64.cpu().numpy())
    return got


@functools.lru_cache(maxsize=None)
def _real(i, ci):
    """Case i of the table under its ci-th chunking, once."""
    S, B, hw, widths, padded, T = K.CASES[i]
    xs, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
    return run(xs, sd, mu, u, K.GRID, widths, K.CHUNKINGS[S][ci], padded, range(1, T + 1))


@functools.lru_cache(maxsize=None)
def _ref(i):
    return K.case_refs(i)


ALL_RUNS = [(i, ci) for i, c in enumerate(K.CASES) for ci in range(len(K.CHUNKINGS[c[0]]))]


# ---- 1: integer data -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.CASES)))
def test_integer_data_gives_the_int64_sums_bit_for_bit(i):
    S, B, hw, widths, padded, T = K.CASES[i]
    for planes, amp, ws, Tn, keep in (("Q", 2, widths, min(T, 3), [4, 5, 6]),
                                      ("AB", 1, tuple(w for w in (3, 5) if w <= min(hw) - 2), T, [0, 1, 3, 4, 5, 6])):
        xs = K.int_inputs(S, B, hw, Tn, 300 + i, amp)
        timed = range(1, Tn + 1)
        ref = K.int_reference(xs, ws, timed, planes)
        for sizes in K.CHUNKINGS[S]:
            got = run(xs, None, None, None, K.GRID_INT, ws, sizes, padded, timed)
            raw = got["raw"][:, :, :, keep]
            assert np.isnan(got["snaps"][0]).all()                           # the untimed step launched nothing
            for l, w in enumerate(ws):                                       # written exactly at the valid pixels
                assert np.array_equal(np.isfinite(raw[:, :, l]), np.broadcast_to(K.valid_mask(w, hw).reshape(-1), raw[:, :, l].shape)), (i, w)
            assert raw.dtype == F32 and np.array_equal(np.where(np.isfinite(raw), raw, 0), ref[:, :, :, keep].astype(F32)), \
                "case %d %s chunks %s: raw is not the integer sums" % (i, planes, sizes)


# ---- 2, 3: real data against the mirror and against the bound --------------------------------------------------------------------------
@pytest.mark.parametrize("i,ci", ALL_RUNS)
def test_real_data_equals_the_float32_mirror_after_every_step(i, ci):
    got, r = _real(i, ci), _ref(i)
    assert np.array_equal(got["a"], r["a"]) and np.array_equal(got["k64"], r["k64"]) and np.array_equal(got["kk"], r["k64"].astype(F32))
    for t, (snap, mir) in enumerate(zip(got["snaps"], r["snaps"])):
        if mir is None:
            assert np.isnan(snap).all()
        else:
            assert snap.dtype == F32 and np.array_equal(snap, mir, equal_nan=True), \
                "case %d chunking %d: raw differs from the mirror after step %d" % (i, ci, t)


def test_real_data_stays_inside_the_counted_bound_of_the_fp64_sums():
    worst = max(K.check_raw(_real(i, 0)["raw"], _ref(i)["ref"], "case %d" % i) for i in range(len(K.CASES)))
    print("raw against the fp64 direct sums: worst share of the bound %.4f" % worst)


# ---- 4: the published fields -------------------------------------------------------------------------------------------------------------
def test_fields_match_the_host_restatement_of_the_device_raw_and_the_definition():
    worst = worst_def = 0.0
    for i, (S, B, hw, widths, padded, T) in enumerate(K.CASES):
        got, r = _real(i, 0), _ref(i)
        rows = K.restate(got["raw"], T, widths, r["k64"], hw)
        bnd, mags = K.same_raw_bounds(got["raw"], T, widths, r["k64"], hw)
        worst = max(worst, K.check_fields(got, rows, bnd, mags, S, widths, hw, "case %d" % i))
        worst_def = max(worst_def, K.check_against_definition(r, got, r["rows"], "case %d definition" % i))
        for l, w in enumerate(widths):                                       # the NaN pattern is exactly the invalid region of each width
            m = K.valid_mask(w, hw)
            assert np.isnan(got["flux_mean"][:, l][:, ~m]).all() and np.isfinite(got["flux_mean"][:, l][:, m]).all()
        assert list(got["flux_widths"]) == list(widths) and np.array_equal(got["flux_lengths"], np.outer(widths, K.GRID))
    print("fields: worst share of the bound against the host restatement %.4f, against the definition %.4f" % (worst, worst_def))


# ---- 5: determinism --------------------------------------------------------------------------------------------------------------------
def test_outputs_are_bitwise_the_same_for_every_chunking_run_and_prefill():
    for i, (S, B, hw, widths, padded, T) in enumerate(K.CASES):
        base = _real(i, 0)
        others = [_real(i, ci) for ci in range(1, len(K.CHUNKINGS[S]))]
        xs, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
        others.append(run(xs, sd, mu, u, K.GRID, widths, K.CHUNKINGS[S][-1], padded, range(1, T + 1), prefill=None))   # a second run, raw as allocated
        others.append(run(xs, sd, mu, u, K.GRID, widths, K.CHUNKINGS[S][0], padded, range(1, T + 1), prefill=7.5))
        valid = np.isfinite(base["raw"])
        for o in others:
            for key in K.FIELD_KEYS + ("member_flux",):
                assert np.array_equal(base[key], o[key], equal_nan=True), (i, key)
            assert np.array_equal(base["raw"][valid], o["raw"][valid]), i
        assert (others[-1]["raw"][~valid] == 7.5).all()                       # invalid pixels are never written


def test_per_member_toggle_leaves_every_other_output_unchanged():
    i = 3
    S, B, hw, widths, padded, T = K.CASES[i]
    xs, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
    off = run(xs, sd, mu, u, K.GRID, widths, K.CHUNKINGS[S][0], padded, range(1, T + 1), per_member=False)
    on = _real(i, 0)
    assert "member_flux" not in off and on["member_flux"].shape == (B, S, len(widths)) + hw
    for key in K.FIELD_KEYS + ("raw",):
        assert np.array_equal(off[key], on[key], equal_nan=True), key


def test_the_target_fed_as_the_only_member_reproduces_the_target():
    S, B, hw, widths, padded, T = K.CASES[3]
    xs, sd, mu, u = K.real_inputs(S, B, hw, T, 103)
    xs = np.ascontiguousarray(xs[:, [S, S]])                                 # one member: the target itself
    got = run(xs, sd, mu, u, K.GRID, widths, (1,), padded, range(1, T + 1))
    assert np.array_equal(got["raw"][0], got["raw"][1], equal_nan=True)
    for mean, std, tgt in (("flux_mean", "flux_std", "target_flux"), ("flux_tstd_mean", None, "target_flux_tstd"),
                           ("backscatter_mean", "backscatter_std", "target_backscatter"), ("sgs_mean", "sgs_std", "target_sgs")):
        assert np.array_equal(got[mean], got[tgt], equal_nan=True), mean
        assert std is None or not np.nan_to_num(got[std]).any(), std
    assert np.array_equal(got["member_flux"][:, 0], got["target_flux"], equal_nan=True)
    assert np.array_equal(got["flux_curve"][:, 0], got["flux_curve"][:, 1]) and np.array_equal(got["sgs_energy_curve"][:, 0], got["sgs_energy_curve"][:, 1])


# ---- 6: known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["strain", "ramp"])
def test_known_answers_on_the_device(which):
    xs, want = K.kat_strain() if which == "strain" else K.kat_ramp()
    a, sd, mu, u = K.kat_tables()
    S = xs.shape[1] - 1
    timed = range(1, K.KAT_T + 1)
    k64 = K.factors(K.KAT_WIDTHS, K.KAT_GRID)
    got = run(xs, sd, mu, u, K.KAT_GRID, K.KAT_WIDTHS, (S,) if which == "strain" else (1,) * S, which == "ramp", timed)
    assert np.array_equal(got["raw"], K.mirror(xs, a, K.KAT_WIDTHS, k64.astype(F32), timed)[-1], equal_nan=True)
    ref = K.direct(xs, a, K.KAT_WIDTHS, k64, timed, k=K.KAT_K)
    bnd = K.definition_bounds(ref, ref, want, K.KAT_T, K.KAT_WIDTHS, k64, K.KAT_HW)
    dev = {"flux": np.concatenate([np.moveaxis(got["member_flux"], 1, 0), got["target_flux"][None]]).astype(np.float64)}
    share = K.check_known(dev, {"flux": want["flux"]}, bnd, K.KAT_WIDTHS, K.KAT_HW, which + " on the device", keys=("flux",))
    # the members' amplitudes differ, so the published means are checked through the per-row restatement of the device's own state;
    # the target's fields are row S's
    tgt = {"flux": got["target_flux"], "tstd": got["target_flux_tstd"], "back": got["target_backscatter"], "sgs": got["target_sgs"]}
    share = max(share, K.check_known({k: v[None].astype(np.float64) for k, v in tgt.items()}, {k: v[-1:] for k, v in want.items()},
                                     {k: v[-1:] for k, v in bnd.items()}, K.KAT_WIDTHS, K.KAT_HW, which + " target on the device"))
    print("%s: worst share of the bound %.5f" % (which, share))


# ---- 7: the largest member count -------------------------------------------------------------------------------------------------------
def test_largest_member_count():
    S, B, hw, widths, padded, T = K.MAX_CASE
    xs = K.int_inputs(S, B, hw, T, 399, 1)
    timed = range(1, T + 1)
    ref = K.int_reference(xs, widths, timed, "AB").astype(F32)
    keep = [0, 1, 3, 4, 5, 6]
    one = run(xs, None, None, None, K.GRID_INT, widths, (1024,), padded, timed, per_member=False)
    many = run(xs, None, None, None, K.GRID_INT, widths, (64,) * 16, padded, timed, per_member=False)
    for got in (one, many):
        raw = got["raw"][:, :, :, keep]
        assert np.array_equal(np.where(np.isfinite(raw), raw, 0), ref[:, :, :, keep])
    for key in K.FIELD_KEYS:
        assert np.array_equal(one[key], many[key], equal_nan=True), key
    k64 = K.factors(widths, K.GRID_INT)
    rows = K.restate(one["raw"], T, widths, k64, hw)
    bnd, mags = K.same_raw_bounds(one["raw"], T, widths, k64, hw)
    K.check_fields(one, rows, bnd, mags, S, widths, hw, "1024 members")


# ---- 8: end to end ---------------------------------------------------------------------------------------------------------------------
def test_model_pred_flux_matches_the_definition_over_model_pred(monkeypatch, tmp_path):
    """Same seed: modelPredFlux returns modelPredStats' keys with equal values plus exactly the new keys.  The reference is the
    definition on modelPred's un-normalised samples p (a = 1, nothing left out: the physical velocity with u0 out_mu inside).
    modelPred un-normalises in fp32 (an error of at most u (3 |p| + |u0 mu|)), the kernel's f = a y carries the rounding of a and
    its own product (2 u (|p| + |u0 mu|)): both are within k = 1 extra rounding of the magnitude 4 |p| + 2 |u0 mu|, which stands for
    |f| in the bounds.  max_rows = 4 splits the 5 members of a batch of 2 into chunks of 2, 2, 1."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = E._cylinder_case(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 5, 1, 1, 4
    grid = (0.5, 0.25)
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=grid[0], dy=grid[1])
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    for _ in range(2):                                                        # two folded runs: modelPredFlux, modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            assert (S + per - 1) // per >= 2
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    for bi, B in enumerate(batches):
        for mm in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, mm)
    kw = dict(samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    torch.manual_seed(77)
    got = utils.modelPredFlux(args, model, te, E.LOG, per_member=True, **kw)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(stats) | set(K.NEW_KEYS)
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Hh, Ww = y.shape[0], y.shape[3], y.shape[4]
    widths = tuple(w for w in K.DEFAULT_WIDTHS if w <= min(Hh, Ww) - 2)
    assert list(g["flux_widths"]) == list(widths) and np.array_equal(g["flux_lengths"], np.outer(widths, grid))
    timed = range(t_start, Tk)
    T = len(timed)
    rows = np.concatenate([p.transpose(2, 0, 1, 3, 4, 5), y.transpose(1, 0, 2, 3, 4)[:, None]], axis=1)   # [Tk, S + 1, N, 3, H, W]
    one, zero = np.ones((N, 2), F32), np.zeros((N, 2))
    k64 = K.factors(widths, grid)
    umu = np.abs(u0[:, None] * mu[None, :2])                                  # [N, 2]
    absf = tuple(4 * np.abs(rows[list(timed)][:, :, :, c]) + 2 * umu[None, None, :, c, None, None] for c in (0, 1))
    ref = K.direct(rows, one, widths, k64, timed, k=1, absf=absf)
    want = K.definition(rows, one, zero, widths, grid, timed)
    bnd = K.definition_bounds(ref, ref, want, T, widths, k64, (Hh, Ww))
    mags = K.field_mags(ref, T, widths, k64, (Hh, Ww))
    assert g["flux_mean"].shape == (N, len(widths), Hh, Ww) and g["member_flux"].shape == (N, S, len(widths), Hh, Ww)
    assert g["sgs_std"].shape == (N, len(widths), 3, Hh, Ww) and g["flux_curve"].shape == (N, S + 1, len(widths))
    share = K.check_fields(g, want, bnd, mags, S, widths, (Hh, Ww), "end to end")
    assert np.nanmax(np.abs(g["member_flux"])) > 0
    print("end to end: worst share of the bound %.4f" % share)
