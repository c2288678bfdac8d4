"""CPU-side checks of the ensemble two-point space-time correlations: the kernel entries are declared in their own header, listed apart
and exported; the signatures and defaults of the three Python layers; the launch plan and the codes the entries return before any
launch; every argument error without a GPU; the float32 mirror of the state against the int64 reference and, through the fp64
restatement, against the reference by direct definition inside the propagated bounds of tests/corr_cases.py; the host functions
corr_probe_stats, corr_lengths and corr_shift on known answers; and the sensitivity of the measure: every deliberate mistake in the
reference exceeds the bound."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import corr_cases as K

NAMES = ["tmg_ens_corr_plan", "tmg_ens_corr_probe", "tmg_ens_corr_accum", "tmg_ens_corr_finalize"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_corr.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.CORR_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert "tmg_ens_corr" not in main and "tmglow_hip_corr" not in main
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.GRAM_EXPORTS,
                      tmg_hip.SFUN_EXPORTS, tmg_hip.EVENT_EXPORTS, tmg_hip.PDF_EXPORTS, tmg_hip.POD_EXPORTS, tmg_hip.PHASE_EXPORTS,
                      tmg_hip.SPOD_EXPORTS, tmg_hip.LAYOUT_EXPORTS, tmg_hip.BUDGET_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert len(tmg_hip.RET_I64) == 4
    assert "tmg_corr.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_corr.hip"))
    assert "tmg_corr.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_corr.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"for f in [^;]*\btmg_corr\b[^;]*;", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_corr.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)                                       # (the header comment says "no atomics")
    assert not re.search(r"atomic|\basm\b|__shared__|hipMemset", code)
    assert src.count("#pragma clang fp contract(off)") >= 3


def test_signatures_and_defaults():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredCorrelation).parameters
    assert list(sig) == old + ["probes", "pairs", "lags", "per_member", "dt"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, None, ((0, 0), (1, 1)), (0, 1, 2, 4), False, None]
    init = inspect.signature(tmg_ops.EnsembleCorrelation.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid", "probes", "pairs",
                          "lags", "mean", "per_member", "step_dt"]
    assert [init[n].default for n in list(init)[10:]] == [None, (1.0, 1.0), None, ((0, 0), (1, 1)), (0, 1, 2, 4), None, False, 1.0]
    add = inspect.signature(tmg_ops.EnsembleCorrelation.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleCorrelation, tmg_ops.EnsembleFeed)
    assert (tmg_ops.CORR_MAX_PROBES, tmg_ops.CORR_MAX_PAIRS, tmg_ops.CORR_MAX_LAGS, tmg_ops.CORR_MAX_LAG) == (8, 4, 8, 64)
    assert list(inspect.signature(tmg_ops.corr_args).parameters) == ["probes", "pairs", "lags", "C", "Hh", "Ww"]
    assert list(inspect.signature(tmg_ops.corr_probe_stats).parameters) == ["series", "pairs", "lags", "T"]
    assert list(inspect.signature(tmg_ops.corr_lengths).parameters) == ["line", "pos", "step"]
    assert list(inspect.signature(tmg_ops.corr_shift).parameters) == ["line", "pos"]
    assert list(inspect.signature(tmg_hip.ens_corr_plan).parameters) == ["S", "B", "Hh", "Ww", "P", "Q", "L", "J"]
    assert list(inspect.signature(tmg_hip.ens_corr_probe).parameters)[:4] == ["y", "a", "m", "series"]
    assert list(inspect.signature(tmg_hip.ens_corr_accum).parameters)[:5] == ["y", "a", "m", "series", "raw"]
    assert list(inspect.signature(tmg_hip.ens_corr_finalize).parameters)[:3] == ["raw", "pm", "pv"]
    assert tmg_ops.corr_args(None, None, None, 3, 64, 128) == (((32, 32), (32, 64), (32, 96)), ((0, 0), (1, 1)), (0, 1, 2, 4))
    for doc in (utils.modelPredCorrelation.__doc__, tmg_ops.EnsembleCorrelation.__doc__):
        for word in ("NPL * 4", "40 planes", "Not supported", "off the pixel grid", "pixel-box", "negative lags", "exchange ci and cj",
                     "more than 8 probes", "lag over 64", "full two-point tensor", "non-finite"):
            assert word in doc, word


def test_plan_covers_the_pixels_once_names_the_path_and_packs_the_planes():
    import tmg_hip
    shapes = [c[2] for c in K.CASES] + [K.MAX_CASE[2], (1, 1), (3, 1024), (256, 256), (64, 257), (1025, 3), (4, 256), (3, 1 << 20)]
    for Hh, Ww in shapes:
        for S, B in ((1, 1), (1024, 3)):
            for P, Q, L, J in ((1, 1, 1, 1), (3, 2, 4, 2), (6, 4, 5, 3), (8, 4, 8, 3)):
                if (S + 1) * B * (P * Q * L + 2 * J * L) * Hh * Ww >= 1 << 40:
                    continue
                q = tmg_hip.ens_corr_plan(S, B, Hh, Ww, P, Q, L, J)
                HW = Hh * Ww
                assert q["vec"] == (Ww % 4 == 0) and q["tile"] == (1024 if q["vec"] else 256) and q["ws"] == 0
                assert q["grid"] == (q["tiles"], B)
                assert q["tiles"] * q["tile"] >= HW and (q["tiles"] - 1) * q["tile"] < HW   # every pixel in exactly one block
                # X, F and G are disjoint and dense: [0, PQL), [PQL, PQL + JL), [PQL + JL, NPL)
                assert (q["offX"], q["offF"], q["offG"], q["planes"]) == (0, P * Q * L, P * Q * L + J * L, P * Q * L + 2 * J * L)
                assert q == dict(tmg_hip.ens_corr_plan(1, B, Hh, Ww, P, Q, L, J))           # not a function of S
    assert tmg_hip.ens_corr_plan(4, 4, 256, 256, 3, 2, 4, 2)["planes"] == 40 == K.planes(3, ((0, 0), (1, 1)), 4)   # the defaults
    paths = {(tmg_hip.ens_corr_plan(c[0], c[1], *c[2], 6, 4, 5, 3)["vec"], tmg_hip.ens_corr_plan(c[0], c[1], *c[2], 6, 4, 5, 3)["tiles"] > 1)
             for c in K.CASES}
    assert paths == {(True, True), (True, False), (False, True), (False, False)}


def test_entries_return_their_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                    # noqa: E731
    plan = (c_i64 * 8)()
    ok = (4, 2, 5, 7, 3, 2, 4, 2)
    assert lib.tmg_ens_corr_plan(i64(*ok), plan) == 0 and list(plan) == [256, 1, 0, 40, 0, 24, 32, 0]
    for pos, v in ((0, 0), (1, 0), (2, 0), (3, -1), (4, 0), (5, 0), (6, 0), (7, 0), (7, 3), (7, 4)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_corr_plan(i64(*d), plan) == -1, (pos, v)
    for pos, v in ((0, 1025), (1, 65536), (2, 1 << 31), (3, (1 << 31) - 1), (4, 9), (5, 5), (6, 9)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_corr_plan(i64(*d), plan) == -2, (pos, v)
    assert lib.tmg_ens_corr_plan(i64(*ok), None) == -3 and lib.tmg_ens_corr_plan(None, plan) == -3
    # the launches: a non-null dummy pointer is never dereferenced by a call that returns a code
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(probes=((2, 1), (2, 3), (2, 3)), pairs=((0, 0), (1, 1)), lags=(0, 1, 2, 4))

    def cfg(**kw):
        c = dict(good)
        c.update(kw)
        return tmg_hip.ens_corr_cfg(c["probes"], c["pairs"], c["lags"])

    feed_dims = (2, 4, 2, 5, 7, 0, 0, 6)                                     # {k, S, B, H, W, row0, t, steps}

    def probe(dims=feed_dims, td=(3, 0), ptr=p, c=None):
        return lib.tmg_ens_corr_probe(ptr, i64(*td) if td else None, p, p, p, cfg() if c is None else c, i64(*dims), None)

    def accum(dims=feed_dims, td=(3, 0), ptr=p, c=None):
        return lib.tmg_ens_corr_accum(ptr, i64(*td) if td else None, p, p, p, p, cfg() if c is None else c, i64(*dims), None)

    def fin(dims=(4, 2, 5, 7, 3), ptr=p, c=None):
        return lib.tmg_ens_corr_finalize(ptr, p, p, p, p, p, p, p, p, None, p, p, cfg() if c is None else c, i64(*dims), None)

    bad_cfg = [cfg(probes=((5, 0),)), cfg(probes=((0, 7),)), cfg(probes=((-1, 0),)), cfg(pairs=((3, 0),)), cfg(pairs=((0, -1),)),
               cfg(lags=(1, 2)), cfg(lags=(0, 2, 2)), cfg(lags=(0, 3, 1)), i64(0, 1, 1), i64(1, 0, 1), i64(1, 1, 0)]
    big_cfg = [cfg(probes=((0, 0),) * 9), cfg(pairs=((0, 0),) * 5), cfg(lags=tuple(range(9))), cfg(lags=(0, 65))]
    for call in (probe, accum):
        for pos, v in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, -1), (5, 4), (6, -1), (6, 6), (7, 0)):
            d = list(feed_dims)
            d[pos] = v
            assert call(dims=tuple(d)) == -1, (call.__name__, pos, v)
        assert call(td=(2, 0)) == -1 and call(td=(5, 3)) == -1 and call(td=(3, -1)) == -1
        for c in bad_cfg:
            assert call(c=c) == -1, list(c)
        for c in big_cfg:
            assert call(c=c) == -2, list(c)
        assert call(dims=(2, 1025, 2, 5, 7, 0, 0, 6)) == -2 and call(dims=(2, 4, 65536, 5, 7, 0, 0, 6)) == -2 and call(td=(1 << 31, 0)) == -2
        assert call(dims=(2, 4, 2, 5, 7, 0, 0, 1 << 30)) == -2                # the series block beyond the index range
        assert call(ptr=None) == -3 and call(td=None) == -3
    assert lib.tmg_ens_corr_probe(p, i64(3, 0), p, p, p, None, i64(*feed_dims), None) == -3
    assert lib.tmg_ens_corr_accum(p, i64(3, 0), p, p, p, p, cfg(), None, None) == -3
    assert lib.tmg_ens_corr_accum(p, i64(3, 0), p, p, p, None, cfg(), i64(*feed_dims), None) == -3
    assert fin(dims=(0, 2, 5, 7, 3)) == -1 and fin(dims=(4, 2, 0, 7, 3)) == -1 and fin(dims=(4, 2, 5, 7, 0)) == -1
    for c in bad_cfg:
        assert fin(c=c) == -1, list(c)
    for c in big_cfg:
        assert fin(c=c) == -2, list(c)
    assert fin(dims=(1025, 2, 5, 7, 3)) == -2 and fin(dims=(4, 2, 5, 7, 1 << 31)) == -2
    assert fin(ptr=None) == -3 and lib.tmg_ens_corr_finalize(p, p, p, p, p, p, p, p, p, None, p, p, None, i64(4, 2, 5, 7, 3), None) == -3


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_corr_args_names_every_error():
    import tmg_ops as ops
    assert ops.corr_args([(0, 0), [4, 6], (0, 0)], [(2, 1)], [0, 64], 3, 5, 7) == (((0, 0), (4, 6), (0, 0)), ((2, 1),), (0, 64))
    bad = [dict(C=2), dict(C=4), dict(probes=((5, 0),)), dict(probes=((0, 7),)), dict(probes=((-1, 0),)), dict(probes=((0, 0),) * 9),
           dict(probes=()), dict(probes=((0.5, 1),)), dict(probes=((0, 1, 2),)), dict(probes=3), dict(probes=((True, 0),)),
           dict(pairs=((0, 0),) * 5), dict(pairs=()), dict(pairs=((3, 0),)), dict(pairs=((0, 3),)), dict(pairs=((-1, 0),)), dict(pairs=((0, -1),)),
           dict(pairs=((0,),)), dict(lags=tuple(range(9))), dict(lags=()), dict(lags=(1, 2)), dict(lags=(0, 2, 2)), dict(lags=(0, 3, 1)),
           dict(lags=(0, 65)), dict(lags=(0, 1.5)), dict(lags=(-1, 0)), dict(lags=4)]
    for kw in bad:
        full = dict(probes=((2, 3),), pairs=((0, 0),), lags=(0, 1), C=3, Hh=5, Ww=7)
        full.update(kw)
        with pytest.raises(ValueError):
            ops.corr_args(**full)


def test_constructor_validates_before_it_touches_a_device():
    import tmg_ops as ops
    ok = dict(members=3, B=2, C=3, Hh=5, Ww=7, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3), grid=(0.5, 0.25))
    bad = [dict(members=0), dict(members=1025), dict(C=2), dict(steps=0), dict(B=0), dict(grid=(0.0, 1.0)), dict(grid=(1.0,)),
           dict(step_dt=0.0), dict(step_dt=float("nan")), dict(probes=((5, 0),)), dict(pairs=((0, 3),)), dict(lags=(0, 65)),
           dict(out_std=torch.tensor([1.0, 0.0, 1.0])), dict(out_std=torch.ones(2)), dict(out_mu=torch.tensor([0.0, float("nan"), 0.0])),
           dict(u=torch.zeros(2, 3)), dict(mean=torch.zeros(2, 3, 5, 6)), dict(mean=torch.full((2, 3, 5, 7), float("nan")))]
    for kw in bad:
        full = dict(ok)
        full.update(kw)
        with pytest.raises(ValueError):
            ops.EnsembleCorrelation(**full)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.EnsembleCorrelation(**dict(ok, device="cpu"))


def test_model_pred_correlation_validates_its_arguments_first():
    from types import SimpleNamespace
    from utils import utils
    args = SimpleNamespace(dx=1.0, dy=1.0)
    for kw in (dict(lags=(1, 2)), dict(lags=(0, 65)), dict(pairs=((0, 3),)), dict(probes=((-1, 0),)), dict(probes=((0, 0),) * 9), dict(dt=0.0),
               dict(dt=float("inf"))):
        with pytest.raises(ValueError):
            utils.modelPredCorrelation(args, None, None, None, **kw)


# ---- the mirror against the references ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_cases():
    """Every case of the table once: inputs, tables, the mirror's snapshots and the definition's reference."""
    out = []
    for i, (S, B, hw, padded, T) in enumerate(K.CASES):
        steps = K.FRONT[i] + T
        xs, m, sd, mu, u = K.real_inputs(S, B, hw, steps, 100 + i)
        a = K.scales(sd, u, B)
        timed, probes, lags = range(K.FRONT[i], steps), K.probes_of(hw), K.lags_of(T)
        d = K.fluct(xs, a, m, timed)
        out.append(dict(S=S, B=B, hw=hw, T=T, d=d, probes=probes, lags=lags, snaps=K.mirror(xs, a, m, timed, probes, K.PAIRS, lags),
                        ref=K.definition(d, probes, K.PAIRS, lags)))
    return out


def test_real_cases_keep_their_variances_away_from_zero(real_cases):
    """Nothing needs excluding: on every case and lag pv * vf of the definition stays above 1e-3 of its median, and every bound is
    finite."""
    for i, c in enumerate(real_cases):
        assert c["T"] >= 5
        for l, tau in enumerate(c["lags"]):
            v = c["ref"]["pvvf"][:, :, :, :, l]
            if c["T"] - tau < 2:
                assert np.isnan(v).all() and np.isnan(c["ref"]["rho"][:, :, :, :, l]).all()
                continue
            assert np.isfinite(v).all() and v.min() > 1e-3 * np.median(v), (i, tau, v.min(), np.median(v))
            assert np.isfinite(c["ref"]["brho"][:, :, :, :, l]).all() and np.isfinite(c["ref"]["bcov"][:, :, :, :, l]).all()
            assert np.abs(c["ref"]["rho"][:, :, :, :, l]).max() <= 1.0 + 1e-12


def test_mirror_agrees_with_the_definition_inside_the_propagated_bounds(real_cases):
    worst = 0.0
    for i, c in enumerate(real_cases):
        series, raw = c["snaps"][-1]
        for f in range(K.FRONT[i]):                                          # the untimed steps write nothing
            assert np.isnan(c["snaps"][f][0]).all() and np.isnan(c["snaps"][f][1]).all()
        assert raw.dtype == K.F32 and series.dtype == K.F32
        L = len(c["lags"])
        dead = [pl for pl in range(raw.shape[2]) if c["lags"][pl % L] >= c["T"]]
        live = [pl for pl in range(raw.shape[2]) if c["lags"][pl % L] < c["T"]]
        assert dead and np.isnan(raw[:, :, dead]).all() and np.isfinite(raw[:, :, live]).all()
        assert np.isfinite(series[:, :, :c["T"]]).all() and np.isnan(series[:, :, c["T"]:]).all()
        rows = K.restate(raw, series, c["T"], c["hw"], c["probes"], K.PAIRS, c["lags"])
        got = {k: v.astype(K.F32) for k, v in K.outputs_from_rows(*rows).items()}
        worst = max(worst, K.check_definition(got, c["ref"], c["S"], "case %d" % i))
        # rho is 1 at the probe for lag 0 and ci == cj, inside the bound
        for p, (h, w) in enumerate(c["probes"]):
            for q, (ci, cj) in enumerate(K.PAIRS):
                if ci == cj:
                    assert (np.abs(rows[1][:, :, p, q, 0, h, w] - 1.0) <= c["ref"]["brho"][:, :, p, q, 0, h, w]).all()
        # the duplicate probe's planes are the same bits
        pa, pb = K.DUPLICATE
        QL = len(K.PAIRS) * L
        assert np.array_equal(raw[:, :, pa * QL:(pa + 1) * QL], raw[:, :, pb * QL:(pb + 1) * QL], equal_nan=True)
    print("mirror against the definition: worst share of the bound %.4f" % worst)


def test_mirror_of_integer_data_is_exact():
    for i, (S, B, hw, padded, T) in enumerate(K.CASES + [(5,) + K.MAX_CASE[1:]]):   # (the member limit's shape with five members)
        steps = 1 + T
        xs, m = K.int_inputs(S, B, hw, steps, 300 + i)
        probes, lags = K.probes_of(hw), K.lags_of(T)
        ref, written = K.int_reference(xs, m, range(1, steps), probes, K.PAIRS, lags)
        series, raw = K.mirror(xs, np.ones((B, 3), K.F32), m, range(1, steps), probes, K.PAIRS, lags)[-1]
        assert np.array_equal(raw[:, :, written].astype(np.float64), ref[:, :, written]) and np.isnan(raw[:, :, ~written]).all()
        assert (~written).sum() == (len(probes) * len(K.PAIRS) + 6) * sum(1 for tau in lags if tau >= T)


def test_probe_stats_of_the_package_equal_the_reference():
    import tmg_ops as ops
    g = np.random.default_rng(5)
    series = g.normal(size=(3, 2, 7, 4, 3)).astype(K.F32)
    lags = (0, 1, 5, 6, 7, 9)
    pm, pv = ops.corr_probe_stats(series, K.PAIRS, lags, 7)
    rm, rv = K.probe_stats(series, K.PAIRS, lags, 7)
    assert pm.dtype == torch.float64 and tuple(pm.shape) == (3, 2, 4, 4, 6)
    for got, ref in ((pm.numpy(), rm), (pv.numpy(), rv)):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref[..., 4:]).all() and np.isfinite(ref[..., :4]).all()
        assert np.allclose(got[..., :4], ref[..., :4], rtol=1e-13, atol=1e-15)
    assert np.allclose(rm[:, :, 1, 2, 1], series[:, :, :6, 1, 0].astype(np.float64).mean(2), rtol=1e-13)
    assert np.allclose(rv[:, :, 1, 2, 1], series[:, :, :6, 1, 0].astype(np.float64).var(2), rtol=1e-13)
    assert (rv[..., 3] == 0).all()                                           # n = 1: one sample has no variance


# ---- the host functions --------------------------------------------------------------------------------------------------------------------
def test_corr_lengths_of_a_triangle_and_of_a_line_cut_by_the_edge():
    import tmg_ops as ops
    for k, pos, step in ((4, 10, 0.5), (1, 3, 2.0), (7, 8, 0.25)):
        i = np.arange(24) - pos
        tri = np.maximum(0.0, 1.0 - np.abs(i) / k)
        got = ops.corr_lengths(tri, pos, step)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2,)
        assert np.allclose(got.numpy(), step * k / 2.0, rtol=1e-14), (k, got)
    # cut by the field edge: the sum stops at the last pixel
    line = np.array([0.25, 0.5, 1.0, 0.75, 0.5])
    assert ops.corr_lengths(line, 2, 2.0).tolist() == [2.0 * (0.5 + 0.75 + 0.5), 2.0 * (0.5 + 0.5 + 0.25)]
    assert ops.corr_lengths(line, 0, 1.0).tolist() == [0.125 + 0.5 + 1.0 + 0.75 + 0.5, 0.125]
    assert ops.corr_lengths(line, 4, 1.0).tolist() == [0.25, 0.25 + 0.75 + 1.0 + 0.5 + 0.25]
    # a zero crossing, a NaN and what lies behind them are left out; batched lines
    lines = np.array([[0.1, 0.9, 1.0, 0.5, -0.1, 0.7], [0.4, np.nan, 1.0, 0.5, 0.0, 0.7], [np.nan] * 6])
    got = ops.corr_lengths(lines, 2, 1.0).numpy()
    assert got[0].tolist() == [1.0, 1.5] and got[1].tolist() == [1.0, 0.5] and np.isnan(got[2]).all()


def test_corr_shift_of_a_sampled_parabola_and_of_an_edge_peak():
    import tmg_ops as ops
    x = np.arange(12, dtype=np.float64)
    for peak, pos in ((5.25, 3), (6.5 - 1e-9, 6), (2.0, 0), (8.75, 11)):
        got = float(ops.corr_shift(1.0 - 0.03 * (x - peak) ** 2, pos))
        assert abs(got - (peak - pos)) < 1e-12, (peak, pos, got)
    # a peak on the edge is not refined; nor is one beside a NaN
    assert float(ops.corr_shift(np.array([1.0, 0.5, 0.2, 0.1]), 2)) == -2.0
    assert float(ops.corr_shift(np.array([0.1, 0.2, 0.5, 1.0]), 1)) == 2.0
    assert float(ops.corr_shift(np.array([0.1, np.nan, 0.9, 0.5]), 0)) == 2.0
    got = ops.corr_shift(np.array([[np.nan] * 5, [0.0, 0.5, 1.0, 0.5, 0.0], [np.nan, 0.2, 0.1, np.nan, np.nan]]), 2)
    assert got.dtype == torch.float64 and bool(torch.isnan(got[0])) and got[1] == 0.0 and got[2] == -1.0


# ---- the sensitivity of the measure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", ["lag", "n", "window", "swap"])
def test_a_mistake_in_the_reference_exceeds_the_bound(real_cases, mut):
    caught = 0
    for i, c in enumerate(real_cases):
        bad = K.definition(c["d"], c["probes"], K.PAIRS, c["lags"], mut=mut)
        bad.update(bcov=c["ref"]["bcov"], brho=c["ref"]["brho"])
        series, raw = c["snaps"][-1]
        rows = K.restate(raw, series, c["T"], c["hw"], c["probes"], K.PAIRS, c["lags"])
        got = {k: v.astype(K.F32) for k, v in K.outputs_from_rows(*rows).items()}
        try:
            K.check_definition(got, bad, c["S"], "case %d" % i)
        except AssertionError:
            caught += 1
    assert caught == len(real_cases), "the bound lets %s through on %d cases" % (mut, len(real_cases) - caught)
