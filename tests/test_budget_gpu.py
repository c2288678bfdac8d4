"""Ensemble TKE budget on the device (`-m gpu`): tmg_ens_budget_accum and tmg_ens_budget_terms through tmg_ops.EnsembleBudget against
the references of tests/budget_cases.py (a float32 numpy mirror of the raw state; an int64 reference on integer data; the fp64
reference by direct definition; the fp64 host restatement of the shift formulas on the device's own raw state), two known answers,
and utils.modelPredBudget against the definition over modelPred's samples.  The definitions, the counts C_LIN = 3, C_PROD = 6,
C_TRIPLE = 9, C_GRAD = 13, C_TERM = 48 and the bounds are in tests/budget_cases.py.  The tests print the worst share of the bound
they reach.

Worst share of the bound reached on an MI355X (LAB_NOTES.md): raw against the fp64 direct sums 0.74; the terms against the host
restatement 0.997 (the output's rounding to fp32); the known answers 0.0007 (mean shear) and 0.0014 (wave); end to end 0.0016."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import budget_cases as K

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
    """Feed the accumulator as utils.modelPredBudget does (row S of xs is the target) -> the state's clone after every step."""
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


def run(xs, m, sd, mu, u, fl, sizes, padded, timed, per_member=True, prefill=NAN):
    """EnsembleBudget over the rows xs [steps, S + 1, B, 3, H, W] -> dict of numpy arrays: the outputs, raw, the snapshots."""
    import tmg_ops as ops
    steps, R, B = xs.shape[:3]
    Hh, Ww = xs.shape[-2:]
    en = ops.EnsembleBudget(R - 1, B, 3, Hh, Ww, steps, DEV, torch.zeros(3) if mu is None else torch.from_numpy(mu),
                            torch.ones(3) if sd is None else torch.from_numpy(sd), u=None if u is None else torch.from_numpy(u),
                            grid=fl[:2], nu=fl[2], rho=fl[3], mean=None if m is None else torch.from_numpy(m), per_member=per_member)
    if prefill is not None:
        en.raw.fill_(prefill)                                                # the first timed step stores: nothing of this survives
    snaps = feed(en, xs, sizes, padded, timed)
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in en.finalize().items()}
    got.update(raw=en.raw.cpu().numpy(), snaps=snaps, a=en.a.cpu().numpy(), M=en.M.cpu().numpy())
    return got


@functools.lru_cache(maxsize=None)
def _real(i, ci):
    """Case i of the table under its ci-th chunking, once."""
    S, B, hw, padded, T = K.CASES[i]
    xs, m, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
    sizes = K.CHUNKINGS[S][ci]
    return run(xs, m, sd, mu, u, K.fl_of(i), sizes, padded, range(1, T + 1))


@functools.lru_cache(maxsize=None)
def _real_ref(i):
    S, B, hw, padded, T = K.CASES[i]
    xs, m, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
    a = K.scales(sd, u, B)
    M = K.phys_mean(a, m, u, mu)
    return dict(a=a, M=M, mirror=K.mirror(xs, a, m, range(1, T + 1)), ref=K.definition(xs, a, m, range(1, T + 1), M, K.fl_of(i)))


ALL_RUNS = [(i, ci) for i, c in enumerate(K.CASES) for ci in range(len(K.CHUNKINGS[c[0]]))]


# ---- 1: integer data -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(K.CASES)))
def test_integer_data_gives_the_int64_sums_bit_for_bit(i):
    S, B, hw, padded, T = K.CASES[i]
    xs, m = K.int_inputs(S, B, hw, T, 300 + i)
    timed = range(1, T + 1)
    ref = K.int_reference(xs, m, timed)
    for sizes in K.CHUNKINGS[S]:
        got = run(xs, m, None, None, None, K.fl_of(i), sizes, padded, timed)
        assert got["raw"].dtype == F32 and np.array_equal(got["raw"], ref.astype(F32)), "case %d chunks %s: raw is not the integer sums" % (i, sizes)
        assert np.isnan(got["snaps"][0]).all()                               # the untimed step launched nothing


# ---- 2, 3: real data against the mirror and against the bound --------------------------------------------------------------------------
@pytest.mark.parametrize("i,ci", ALL_RUNS)
def test_real_data_equals_the_float32_mirror_after_every_step(i, ci):
    got, r = _real(i, ci), _real_ref(i)
    assert np.array_equal(got["a"], r["a"]) and np.array_equal(got["M"].reshape(r["M"].shape), r["M"])
    for t, (snap, mir) in enumerate(zip(got["snaps"], r["mirror"])):
        if mir is None:
            assert np.isnan(snap).all()
        else:
            assert snap.dtype == F32 and np.array_equal(snap, mir), "case %d chunking %d: raw differs from the mirror after step %d" % (i, ci, t)


def test_real_data_stays_inside_the_counted_bound_of_the_fp64_sums():
    worst = max(K.check_raw(_real(i, 0)["raw"], _real_ref(i)["ref"], "case %d" % i) for i in range(len(K.CASES)))
    print("raw against the fp64 direct sums: worst share of the bound %.4f" % worst)


# ---- 4: the terms ----------------------------------------------------------------------------------------------------------------------
def test_terms_match_the_host_restatement_of_the_device_raw():
    worst = 0.0
    for i, (S, B, hw, padded, T) in enumerate(K.CASES):
        got, r, fl = _real(i, 0), _real_ref(i), K.fl_of(i)
        rows = K.restate(got["raw"], T, r["M"], fl, hw)
        mags = K.restate(got["raw"], T, r["M"], fl, hw, mag=True)
        what = "case %d" % i
        worst = max(worst, K.check_fields(got, rows, mags, S, what))
        # against the definition as well, inside the wider bound that carries the roundings of raw
        dmag = K.restate(r["ref"]["mags"], T, r["M"], fl, hw, mag=True)
        K.check_fields(got, (r["ref"]["terms"], r["ref"]["stress"]), dmag, S, what + " definition", rel=K.rel_definition(T))
        mb = got["member_budget"].astype(np.float64)                          # [B, S, 7, H, W]
        mg = np.moveaxis(mags[0][:-1], 0, 1)
        inner = (slice(None),) * 2 + (slice(1, -1), slice(1, -1))
        six = mb[:, :, :6].sum(2)
        tol = K.U24 * (np.abs(mb[:, :, 6]) + np.abs(mb[:, :, :6]).sum(2)) + K.C_TERM * K.E53 * mg[:, :, 6]
        assert (np.abs(mb[:, :, 6] - six)[inner] <= tol[inner]).all(), what + ": resid is not the sum of the six"
        # the mean and the population std over the members of the published member terms: every member value was rounded once
        # (u |x|), the mean and the std move by at most the largest such change, their own rounding adds u |.|, Welford's roundings
        # are carried as in check_fields
        big = np.abs(mb).max(1)
        c64 = (K.C_TERM + 4 * S) * K.E53
        mmax = mags[0][:-1].max(0)
        tol = K.U24 * (big + np.abs(mb.mean(1))) + c64 * mmax
        assert (np.abs(got["budget_mean"] - mb.mean(1))[inner] <= tol[inner]).all(), what + ": budget_mean"
        tol = K.U24 * (big + mb.std(1)) + c64 * mmax + np.sqrt(2.0 * c64) * mmax
        assert (np.abs(got["budget_std"] - mb.std(1))[inner] <= tol[inner]).all(), what + ": budget_std"
    print("terms against the host restatement: worst share of the bound %.4f" % worst)


def test_per_member_toggle_leaves_every_other_output_unchanged():
    i = 3
    S, B, hw, padded, T = K.CASES[i]
    xs, m, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
    off = run(xs, m, sd, mu, u, K.fl_of(i), K.CHUNKINGS[S][0], padded, range(1, T + 1), per_member=False)
    on = _real(i, 0)
    assert "member_budget" not in off and off["budget_terms"] == K.TERMS == on["budget_terms"]
    for key in K.FIELD_KEYS + ("raw",):
        assert np.array_equal(off[key], on[key], equal_nan=True), key


# ---- 5: determinism --------------------------------------------------------------------------------------------------------------------
def test_outputs_are_bitwise_the_same_for_every_chunking_run_and_prefill():
    for i, (S, B, hw, padded, T) in enumerate(K.CASES):
        base = _real(i, 0)
        others = [_real(i, ci) for ci in range(1, len(K.CHUNKINGS[S]))]
        xs, m, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
        others.append(run(xs, m, sd, mu, u, K.fl_of(i), K.CHUNKINGS[S][-1], padded, range(1, T + 1), prefill=None))   # a second run, raw as allocated
        others.append(run(xs, m, sd, mu, u, K.fl_of(i), K.CHUNKINGS[S][0], padded, range(1, T + 1), prefill=7.5))
        for o in others:
            for key in K.FIELD_KEYS + ("member_budget", "raw"):
                assert np.array_equal(base[key], o[key], equal_nan=True), (i, key)


# ---- 6: the target as a member ---------------------------------------------------------------------------------------------------------
def test_the_target_fed_as_the_only_member_reproduces_the_target():
    S, B, hw, padded, T = K.CASES[2]
    xs, m, sd, mu, u = K.real_inputs(S, B, hw, T, 102)
    xs = np.ascontiguousarray(xs[:, [S, S]])                                 # one member: the target itself
    got = run(xs, m, sd, mu, u, K.FL, (1,), padded, range(1, T + 1))
    assert np.array_equal(got["raw"][0], got["raw"][1])
    assert np.array_equal(got["budget_mean"], got["target_budget"], equal_nan=True)
    assert np.array_equal(got["stress_mean"], got["target_stress"]) and not got["stress_std"].any()
    assert not got["budget_std"][:, :, 1:-1, 1:-1].any() and np.isnan(got["budget_std"][:, :, 0]).all()
    assert np.array_equal(got["member_budget"][:, 0], got["target_budget"], equal_nan=True)


# ---- 7: known answers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["shear", "wave"])
def test_known_answers_on_the_device(which):
    xs, m, want = K.kat_shear() if which == "shear" else K.kat_wave()
    a, sd, mu, u = K.kat_tables()
    S = xs.shape[1] - 1
    timed = range(1, K.KAT_T + 1)
    got = run(xs, m, sd, mu, u, K.KAT_FL, (S,) if which == "shear" else (1,) * S, which == "wave", timed)
    assert np.array_equal(got["raw"], K.mirror(xs, a, m, timed)[-1])
    M = K.phys_mean(a, m, u, mu)
    ref = K.definition(xs, a, m, timed, M, K.KAT_FL, pad=K.kat_pad(xs, m, a))
    magt, _ = K.restate(ref["mags"], K.KAT_T, M, K.KAT_FL, K.KAT_HW, mag=True)
    dev = np.concatenate([np.moveaxis(got["member_budget"], 1, 0), got["target_budget"][None]]).astype(np.float64)   # [R, B, 7, H, W]
    share = K.check_known(dev, want, magt, K.KAT_T, which + " on the device", rel_extra=K.U24)   # (+ the output's rounding)
    print("%s: worst share of the bound %.5f" % (which, share))


# ---- 8: the largest member count -------------------------------------------------------------------------------------------------------
def test_largest_member_count():
    S, B, hw, padded, T = K.MAX_CASE
    xs, m = K.int_inputs(S, B, hw, T, 399)
    timed = range(1, T + 1)
    ref = K.int_reference(xs, m, timed).astype(F32)
    one = run(xs, m, None, None, None, K.FL, (1024,), padded, timed, per_member=False)
    many = run(xs, m, None, None, None, K.FL, (64,) * 16, padded, timed, per_member=False)
    assert np.array_equal(one["raw"], ref) and np.array_equal(many["raw"], ref)
    for key in K.FIELD_KEYS:
        assert np.array_equal(one[key], many[key], equal_nan=True), key
    M = K.phys_mean(np.ones((B, 3), F32), m, None, np.zeros(3, F32))
    rows = K.restate(one["raw"], T, M, K.FL, hw)
    mags = K.restate(one["raw"], T, M, K.FL, hw, mag=True)
    K.check_fields(one, rows, mags, S, "1024 members")


# ---- 9: end to end ---------------------------------------------------------------------------------------------------------------------
def test_model_pred_budget_matches_the_definition_over_model_pred(monkeypatch, tmp_path):
    """Same seed: modelPredBudget returns modelPredStats' keys with equal values plus exactly the new keys.  The reference is the
    definition on modelPred's un-normalised samples p with a = 1 about the target's physical time mean.  modelPred un-normalises in
    fp32 (an error of at most u (3 |p| + |u0 mu|)), the kernel's mean plane and the scale a are each rounded once, so the reference's
    d is uncertain by u (3 |p| + 2 |u0 mu| + 2 |mean| + |d|): the pad of the magnitudes; the mean velocity's magnitude carries
    |u0 mu| as well.  max_rows = 4 splits the 5 members of a batch of 2 into chunks of 2, 2, 1."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = E._cylinder_case(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 5, 1, 1, 4
    fl = (0.5, 0.25, 0.01, 1.3)
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=fl[0], dy=fl[1], nu=fl[2])
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    for _ in range(2):                                                        # two folded runs: modelPredBudget, modelPredStats
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
    got = utils.modelPredBudget(args, model, te, E.LOG, rho=fl[3], per_member=True, **kw)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, **kw)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    assert set(got) == set(stats) | set(K.NEW_KEYS) and got["budget_terms"] == K.TERMS
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Hh, Ww = y.shape[0], y.shape[3], y.shape[4]
    timed = range(t_start, Tk)
    T = len(timed)
    mean = y[:, t_start:].mean(1)                                            # [N, 3, H, W], physical
    rows = np.concatenate([p.transpose(2, 0, 1, 3, 4, 5), y.transpose(1, 0, 2, 3, 4)[:, None]], axis=1)   # [Tk, S + 1, N, 3, H, W]
    uc = np.stack([u0, u0, u0 ** 2], 1)
    umu = np.abs(uc * mu[:3].reshape(1, 3)).reshape(N, 3, 1, 1)
    d = np.abs(rows - mean[None, None])
    pad = (3 * np.abs(rows) + 2 * umu[None, None] + 2 * np.abs(mean)[None, None] + d)[list(timed)]
    ref = K.definition(rows, np.ones((N, 3)), mean, timed, mean[:, :2], fl, pad=pad)
    Mmag = np.abs(mean[:, :2]) + umu[:, :2]
    mags = K.restate(ref["mags"], T, Mmag, fl, (Hh, Ww), mag=True)
    assert g["budget_mean"].shape == (N, 7, Hh, Ww) and g["member_budget"].shape == (N, S, 7, Hh, Ww) and g["stress_std"].shape == (N, 3, Hh, Ww)
    share = K.check_fields(g, (ref["terms"], ref["stress"]), mags, S, "end to end", rel=K.rel_definition(T))
    assert np.abs(g["member_budget"][:, :, 1, 1:-1, 1:-1]).max() > 0
    print("end to end: worst share of the bound %.4f" % share)
