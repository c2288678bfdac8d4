"""Ensemble spectral skill on the device (`-m gpu`): tmg_ens_xspec_prep / tmg_spec_rows / tmg_ens_xspec_cols / tmg_ens_xspec_accum
through tmg_ops.EnsembleSpectralSkill and utils.modelPredSpectralSkill against the fp64 statements of tests/xspec_cases.py.

Raw sums: |got - ref| <= max(1e-5 |ref| + 2e-6 Etot, 3 e32), the rule of tests/test_spectrum_gpu.py::_check (e32: the error of a
plain fp32 restatement of the same matrix DFT on that output, Etot: the largest total of P_T).  Derived outputs: recomputed from the
device's own raw sums with the fp64 formulas of xspec_cases, to 2^-40 + 2^-50 |ref|: the host does only fp64 work.  A member equal
to the target reproduces its bits, and every output is bitwise the same for every chunking, for two objects and for two runs."""
import numpy as np
import pytest
import torch

import common as C  # noqa: F401  (puts the package on the path)
import xspec_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sizes(S, k):
    """Chunks of k members, the last one smaller."""
    return [min(k, S - m0) for m0 in range(0, S, k)]


def _feed(sk, ym, yt, t_start, sizes, padded=False):
    """ym [T, S, B, 3, H, W], yt [T, B, 3, H, W]: fp32 device tensors -> the finalized outputs."""
    T, S, B, Cc, Hh, Ww = ym.shape

    def view(a):                                                               # [n, C, H, W] -> API-shaped view of an NHWC buffer
        n = a.shape[0]
        if not padded:
            return a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        wide = torch.full((n, Hh, Ww, 4), float("nan"), device=a.device)        # a channel slice with pixel stride 4
        wide[..., :Cc] = a.permute(0, 2, 3, 1)
        return wide[..., :Cc].permute(0, 3, 1, 2)
    for t in range(T):
        m0 = 0
        tgt = view(yt[t])
        for k in sizes:
            sk.add(view(ym[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, tgt, time=t >= t_start)
            m0 += k
    return sk.finalize()


def _run(c, sizes, mu=K.MU, ym=None):
    import tmg_ops as ops
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # noqa: E731
    sk = ops.EnsembleSpectralSkill(c["S"], c["B"], 3, c["H"], c["W"], c["T"], DEV, torch.from_numpy(mu), torch.from_numpy(K.SD),
                                   u=dev(c["u"]), grid=c["grid"], window=c["window"], center=dev(c["cen"]), level=0.5)
    out = _feed(sk, dev(c["ym"] if ym is None else ym), dev(c["yt"]), c["t_start"], sizes, c["padded"])
    return {key: v.cpu().numpy().copy() for key, v in out.items()}


_REF = {}


def _reference(idx):
    """(fp64 raw reference, fp32 yardstick, the case) of CASES[idx], computed once and left unchanged."""
    if idx not in _REF:
        c = K.make_case(idx)
        fm64, fm32 = K.fields(c["ym"], c["u"])
        ft64, ft32 = K.fields(c["yt"], c["u"])
        _REF[idx] = (K.reference(fm64, ft64, c["cen"], c["grid"], c["window"], c["t_start"]),
                     K.f32_raw(fm32, ft32, c["cen"], c["grid"], c["window"], c["t_start"]), c)
    return _REF[idx]


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for key in a:
        assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key], equal_nan=True), "%s: %s" % (what, key)


# ---- 1. raw sums against fp64, derived outputs against the host formulas -------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.CASES)))
def test_raw_sums_match_fp64_and_the_host_does_fp64(idx):
    ref, y32, c = _reference(idx)
    S, B, T = c["S"], c["B"], c["T"]
    sizes = _sizes(S, 1 + idx % S) if idx % 3 else ([1, S - 3, 2] if S >= 5 else _sizes(S, S))
    got = _run(c, sizes)
    assert set(got) == set(K.RAW_KEYS) | set(K.DERIVED_KEYS)
    bad = K.mismatches(got, ref, y32, report=print)
    assert not bad, (K.CASES[idx], bad)
    k = K.bins(c["H"], c["W"], *c["grid"])[1]
    assert got["xs_k"].dtype == np.float64 and np.allclose(got["xs_k"], k, rtol=1e-15, atol=0)
    for key in K.RAW_KEYS:
        assert got[key].dtype == np.float32
    assert got["xs_sum"].shape == (B, T, 3, k.size) and got["xs_time_member"].shape == (B, S, 3, k.size)
    want = K.derived({key: got[key] for key in K.RAW_KEYS}, S, got["xs_k"], 0.5, T - c["t_start"])
    assert not K.derived_mismatches(got, want), K.derived_mismatches(got, want)
    assert got["spec_corr"].shape == (B, T, k.size) and got["cutoff_k"].shape == (B, S + 1)


# ---- 2. a member equal to the target, and its negative ---------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,S", [(4, 2), (2, 3), (0, 1)])
def test_a_member_equal_to_the_target_gives_its_bits(idx, S):
    _, _, c = _reference(idx)
    c = dict(c, S=S)
    ym = np.ascontiguousarray(np.broadcast_to(c["yt"][:, None], (c["T"], S) + c["yt"].shape[1:]))
    got = _run(c, _sizes(S, 2), ym=ym)
    PT, tT = got["xs_target_power"], got["xs_time_target"]
    assert (PT > 0).all()
    for m in range(S):                                                         # per member: X == P == P_T bit for bit, D == 0.0
        P, X, D = got["xs_time_member"][:, m, 0], got["xs_time_member"][:, m, 1], got["xs_time_member"][:, m, 2]
        assert np.array_equal(P, tT) and np.array_equal(X, tT) and (D == 0.0).all()
    assert (got["time_member_corr"] == 1.0).all()
    assert np.array_equal(got["xs_sum"][:, :, 0], got["xs_sum"][:, :, 1]) and (got["xs_sum"][:, :, 2] == 0.0).all()
    if S in (1, 2):                                                            # sums and means of 1 or 2 equal values are exact
        assert np.array_equal(got["xs_sum"][:, :, 0], np.float32(S) * PT)
        assert np.array_equal(got["xs_mean_field"][:, :, 0], PT) and np.array_equal(got["xs_mean_field"][:, :, 1], PT)
        assert (got["xs_mean_field"][:, :, 2] == 0.0).all()
        assert (got["spec_corr"] == 1.0).all() and (got["mean_field_corr"] == 1.0).all()
        assert (got["err_spec"] == 0.0).all() and (got["power_ratio"] == 1.0).all()


def test_a_member_equal_to_minus_the_target_gives_minus_its_power():
    _, _, c = _reference(5)                                                    # centre None; out_mu = 0 makes -y the field -f
    c = dict(c, S=2)
    mu0 = np.zeros(3, dtype=np.float32)
    ym = np.ascontiguousarray(np.broadcast_to(-c["yt"][:, None], (c["T"], 2) + c["yt"].shape[1:]))
    got = _run(c, [1, 1], mu=mu0, ym=ym)
    tm = got["xs_time_member"]
    for m in range(2):
        assert np.array_equal(tm[:, m, 0], got["xs_time_target"]) and np.array_equal(tm[:, m, 1], -tm[:, m, 0])
    assert np.array_equal(got["xs_sum"][:, :, 1], -got["xs_sum"][:, :, 0])
    assert (got["time_member_corr"] == -1.0).all()
    assert np.allclose(got["time_rel_err"], 4.0, rtol=1e-5)                    # |-Z - Z|^2 = 4 |Z|^2


# ---- 3. reproducibility ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [2, 8])
def test_every_chunking_two_objects_and_two_runs_give_the_same_bits(idx):
    _, _, c = _reference(idx)
    S = c["S"]
    assert S == 5
    first = _run(c, _sizes(S, S))
    for k in range(1, S):                                                      # chunks of every size from 1 to S
        _same_bits(_run(c, _sizes(S, k)), first, "chunks of %d" % k)
    _same_bits(_run(c, [1, 2, 2]), first, "uneven chunks")
    _same_bits(_run(c, _sizes(S, S)), first, "a second object")


# ---- 4. the known cut-off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [3, 5, 8])
def test_cutoff_falls_in_the_interval_of_the_reference(idx):
    ref, _, c = _reference(idx)
    S, Tn = c["S"], c["T"] - c["t_start"]
    got = _run(c, _sizes(S, 2))
    k = got["xs_k"]
    want = K.derived(ref, S, k, 0.5, Tn)
    corr = np.concatenate((want["time_member_corr"], want["time_mean_field_corr"][:, None]), axis=1)
    seen = 0
    for n in range(c["B"]):
        for m in range(S + 1):
            prev, s = K.cutoff_shell(corr[n, m], 0.5)
            cut = got["cutoff_k"][n, m]
            if s is None:
                assert np.isinf(cut)
                continue
            if abs(corr[n, m, s] - 0.5) < 0.05 or (prev is not None and abs(corr[n, m, prev] - 0.5) < 0.05):
                continue                                                       # too close to the level to pin the shell
            assert (k[s] if prev is None else k[prev]) <= cut <= k[s], (n, m, prev, s, cut)
            if m < S and c["window"] is None:
                assert s == c["k0"]                                            # the band-copied member: the step sits at k0
            seen += 1
    assert seen >= S


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------
def test_model_pred_spectral_skill_end_to_end(monkeypatch, tmp_path):
    import test_spectrum_gpu as TS
    import tmg_ops as ops
    from types import SimpleNamespace
    from utils import utils
    model, te = TS._cylinder_case(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    nkeep = tmax // stride
    grid = (0.05, 0.07)
    batches = [int(b[0].shape[0]) for b in te]
    kp = TS._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=grid[0], dy=grid[1])
    for rep in range(2):                                                       # modelPredSpectralSkill, then modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
            assert len(range(0, S, per)) >= 2                                  # at least two chunks
    kw = dict(samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    torch.manual_seed(77)
    got = utils.modelPredSpectralSkill(args, model, te, TS.LOG, **kw)
    torch.manual_seed(77)
    plain = utils.modelPredStats(args, model, te, TS.LOG, **kw)
    assert not kp.fold
    assert set(got) == set(plain) | set(K.RAW_KEYS) | set(K.DERIVED_KEYS)
    for name in plain:
        assert torch.equal(got[name], plain[name]), name
    tgt = got["target"]                                                        # [N, T, 3, H, W] physical
    N, Hh, Ww = tgt.shape[0], tgt.shape[-2], tgt.shape[-1]
    k = K.bins(Hh, Ww, *grid)[1]
    NK = k.size
    shapes = {"xs_target_power": (N, nkeep, NK), "xs_sum": (N, nkeep, 3, NK), "xs_mean_field": (N, nkeep, 3, NK),
              "xs_time_member": (N, S, 3, NK), "xs_time_target": (N, NK), "xs_time_mean_field": (N, 3, NK), "spec_corr": (N, nkeep, NK),
              "time_spread_skill": (N, NK), "time_member_corr": (N, S, NK), "cutoff_k": (N, S + 1), "cutoff_k_mean": (N,), "xs_k": (NK,)}
    for name, shp in shapes.items():
        assert tuple(got[name].shape) == shp and got[name].device.type == "cpu", name
    for name in K.RAW_KEYS:
        assert got[name].dtype == torch.float32 and bool(torch.isfinite(got[name]).all()), name
    assert bool(torch.isfinite(got["spec_corr"]).all()) and float(got["spec_corr"].abs().max()) <= 1 + 1e-6
    assert float(got["xs_sum"][:, :, 2].min()) > 0                             # the members are distinct samples
    np.testing.assert_allclose(got["xs_k"].numpy(), k, rtol=1e-15, atol=0)
    # the target's power: the fp64 statement on the returned target, centred on its time mean over the kept steps from t_start on
    t32 = tgt[:, [j * stride for j in range(nkeep)], :2].permute(1, 0, 2, 3, 4).contiguous().numpy()          # [Tk, N, 2, H, W]
    t64 = t32.astype(np.float64)
    cen = K.centre(t64, t_start)
    ref = K.reference(t64[:, None], t64, cen, grid, "hann", t_start)
    y32 = K.f32_raw(t32[:, None], t32, cen, grid, "hann", t_start)
    raw = {name: got[name].numpy() for name in K.RAW_KEYS}
    bad = K.mismatches(raw, ref, y32, report=print, keys=("xs_target_power", "xs_time_target"))
    assert not bad, bad
    want = K.derived(raw, S, k, 0.5, nkeep - t_start)
    assert not K.derived_mismatches({name: got[name].numpy() for name in K.DERIVED_KEYS}, want)
