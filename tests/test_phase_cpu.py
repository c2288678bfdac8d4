"""CPU-side checks of the ensemble phase averages: the kernel entries are declared in their own header, listed apart and exported; the
signatures of the three Python layers; the launch plan covers every pixel once, names its load path and returns its codes before any
launch; the float32 mirror of the labelling against fp64 atan2 binning and on the edges; the derived formulas against a brute-force
fp64 computation; every argument error without a GPU; and the case tables of tests/phase_cases.py reach both load paths and every
sector count."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import phase_cases as P

NAMES = ["tmg_ens_phase_plan", "tmg_ens_phase_label", "tmg_ens_phase_accum"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_phase.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.PHASE_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert len(re.findall(r'^#include "tmglow_hip_phase\.h"$', main, re.M)) == 1 and main.count("tmglow_hip_phase.h") == 1
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.GRAM_EXPORTS,
                      tmg_hip.SFUN_EXPORTS, tmg_hip.EVENT_EXPORTS, tmg_hip.PDF_EXPORTS, tmg_hip.POD_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert name not in main and hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_phase.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_phase.hip"))
    assert "tmg_phase.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_phase.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_phase\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredPhase).parameters
    assert list(sig) == old + ["modes", "channels", "pair", "bins", "min_amp"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, 8, (0, 1), (0, 1), 8, 0.25]
    init = inspect.signature(tmg_ops.EnsemblePhase.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_std", "u", "modes", "pair", "bins", "min_amp",
                          "mean", "lam"]
    assert [init[n].default for n in list(init)[9:]] == [None, None, (0, 1), 8, 0.25, None, None]
    add = inspect.signature(tmg_ops.EnsemblePhase.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsemblePhase, tmg_ops.EnsembleFeed) and not issubclass(tmg_ops.EnsemblePhase, tmg_ops.EnsembleModes)
    assert list(inspect.signature(tmg_hip.ens_phase_plan).parameters) == ["S", "B", "C", "HW", "NB"]
    assert list(inspect.signature(tmg_hip.ens_phase_label).parameters)[:2] == ["coef", "cstrides"]
    assert list(inspect.signature(tmg_hip.ens_phase_accum).parameters)[:2] == ["y", "lab"]
    # EnsembleModes and modelPredModes are as they were
    assert list(inspect.signature(tmg_ops.EnsembleModes.__init__).parameters)[-3:] == ["channels", "mean", "basis"]
    assert list(inspect.signature(utils.modelPredModes).parameters) == old + ["modes", "channels"]


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def test_plan_covers_the_pixels_once_and_names_the_load_path():
    import tmg_hip
    cases = [(c[0], c[1], c[2], c[3], c[4]) for c in P.INT_TABLE + [P.MAX_CASE] + P.REAL_TABLE]
    cases += [(S, B, Cc, (1, HW), NB) for HW in (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 1028, 4096, 65536, (1 << 20) + 4) for Cc in (2, 4)
              for S, B, NB in ((1, 1, 4), (1024, 3, 32))]
    for S, B, Cc, hw, NB in cases:
        HW = hw[0] * hw[1]
        q = tmg_hip.ens_phase_plan(S, B, Cc, HW, NB)
        assert q["vec"] == (HW % 4 == 0) and q["tile"] == (1024 if q["vec"] else 256) and q["ws"] == 0
        assert q["grid"] == (q["tiles"], NB, B)
        assert q["tiles"] * q["tile"] >= HW and (q["tiles"] - 1) * q["tile"] < HW            # every pixel in exactly one tile
        assert q == tmg_hip.ens_phase_plan(1, B, Cc, HW, NB)                                  # not a function of the rows


def test_entries_return_their_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                    # noqa: E731
    plan = (c_i64 * 6)()
    ok = (4, 2, 3, 100, 8)
    assert lib.tmg_ens_phase_plan(i64(*ok), plan) == 0
    for pos, v in ((0, 0), (1, 0), (2, 1), (2, 5), (3, 0), (4, 0), (4, 2), (4, 6), (4, 12), (4, 24)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_phase_plan(i64(*d), plan) == -1, (pos, v)
    for pos, v in ((0, 1025), (1, 65536), (3, (1 << 31) - 1024), (4, 64), (4, 36)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_phase_plan(i64(*d), plan) == -2, (pos, v)
    assert lib.tmg_ens_phase_plan(i64(*ok), None) == -3 and lib.tmg_ens_phase_plan(None, plan) == -3
    # the launches: a non-null dummy pointer is never dereferenced by a call that returns a code
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    tab = (ctypes.c_float * 8)(0.125, 1.0, 0, 0, 0, 0, 0, 0)
    label = lambda dims=(4, 2, 8), cd=(36, 9), pair=(0, 1), tab=tab, ld=(12, 3), ptr=p: lib.tmg_ens_phase_label(   # noqa: E731
        ptr, i64(*cd), i64(*pair), p, tab, p, i64(*ld), i64(*dims), None)
    assert label(dims=(0, 2, 8)) == -1 and label(dims=(4, 0, 8)) == -1 and label(dims=(4, 2, 6)) == -1
    assert label(cd=(-1, 9)) == -1 and label(ld=(12, -3)) == -1 and label(pair=(1, 1)) == -1 and label(pair=(-1, 0)) == -1
    assert label(tab=(ctypes.c_float * 8)(-1.0, 1.0)) == -1 and label(tab=(ctypes.c_float * 8)(float("nan"), 1.0)) == -1
    assert label(tab=(ctypes.c_float * 8)(0.125, 0.0)) == -1                                   # NB = 8 needs one positive tangent
    assert label(dims=(4, 2, 16), tab=(ctypes.c_float * 8)(0.0, 0.5, 0.4, 2.0)) == -1          # not increasing
    assert label(dims=(1025, 2, 8)) == -2 and label(dims=(4, 65536, 8)) == -2 and label(dims=(4, 2, 64)) == -2
    assert label(pair=(0, 1 << 31)) == -2
    assert label(ptr=None) == -3 and label(tab=None) == -3
    accum = lambda dims=(4, 2, 100, 3, 8), td=(3, 0), ld=(12, 3), ptr=p: lib.tmg_ens_phase_accum(   # noqa: E731
        ptr, i64(*td), p, i64(*ld), p, p, p, i64(*dims), None)
    assert accum(dims=(0, 2, 100, 3, 8)) == -1 and accum(dims=(4, 2, 100, 5, 8)) == -1 and accum(dims=(4, 2, 100, 1, 8)) == -1
    assert accum(dims=(4, 2, 0, 3, 8)) == -1 and accum(dims=(4, 2, 100, 3, 12)) == -1
    assert accum(td=(2, 0)) == -1 and accum(td=(5, 3)) == -1 and accum(td=(3, -1)) == -1 and accum(ld=(-12, 3)) == -1
    assert accum(dims=(1025, 2, 100, 3, 8)) == -2 and accum(dims=(4, 2, 100, 3, 64)) == -2 and accum(td=(1 << 31, 0)) == -2
    assert accum(ptr=None) == -3


# ---- the labelling mirror --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NB", P.BINS)
def test_label_mirror_equals_fp64_atan2_binning_away_from_the_edges(NB):
    w = 2 * np.pi / NB
    k = np.arange(NB, dtype=np.float64)
    th = np.concatenate([(k + 0.5) * w, (k + 0.25) * w, (k + 0.75) * w])
    want = np.concatenate([k, k, k]).astype(np.int32)
    tab = P.table(NB, 0.0)
    for r in (1e-3, 1e-2, 1e-1, 1.0, 10.0, 1e2, 1e3):                        # six decades
        x, y = (r * np.cos(th)).astype(P.F32), (r * np.sin(th)).astype(P.F32)
        got = P.label_mirror(x, y, P.F32(1), P.F32(1), tab, NB)
        assert np.array_equal(got, want), (NB, r)
        assert np.array_equal(P.label_atan2(x, y, NB), want), (NB, r)
        g = P.F32(0.37)                                                      # through a gain
        assert np.array_equal(P.label_mirror(x / g, y / g, g, g, tab, NB), want), (NB, r)


def test_label_mirror_edge_convention_and_gate():
    # a point exactly on an edge belongs to the higher sector; NB = 8: the edges are the axes and the diagonals
    pts = [(1, 0), (2, 2), (0, 3), (-1, 1), (-5, 0), (-3, -3), (0, -2), (4, -4)]
    for NB, step in ((8, 1), (4, 2)):
        tab = P.table(NB, 0.0)
        assert float(tab[0]) == 0.0 and (NB == 4 or float(tab[1]) == 1.0)    # tan(pi / 4) rounds to 1 exactly
        x, y = np.array([p[0] for p in pts], dtype=P.F32), np.array([p[1] for p in pts], dtype=P.F32)
        got = P.label_mirror(x, y, P.F32(1), P.F32(1), tab, NB)
        want = [(i // step) for i in range(8)] if NB == 4 else list(range(8))
        assert got.tolist() == want, (NB, got.tolist())
        # (0, 0) with min_amp = 0 passes the gate and is sector 0; -0.0 is 0
        z = P.label_mirror(np.array([0.0, -0.0], dtype=P.F32), np.array([0.0, 0.0], dtype=P.F32), P.F32(1), P.F32(1), tab, NB)
        assert z.tolist() == [0, 0]
    # the gate: r^2 == thr exactly is kept, one unit in the last place under it is skipped
    tab = P.table(8, 0.25)
    assert float(tab[0]) == 0.125
    x = np.array([0.25, 0.25, np.nextafter(P.F32(0.25), P.F32(0)), 0.0], dtype=P.F32)
    y = np.array([0.25, -0.25, 0.25, 0.0], dtype=P.F32)
    assert P.label_mirror(x, y, P.F32(1), P.F32(1), tab, 8).tolist() == [1, 7, -1, -1]
    # the product tables of tmg_ops are the mirror's
    import tmg_ops as ops
    for NB in P.BINS:
        for amp in (0.0, 0.25, 1.3):
            assert np.array_equal(np.array(ops.phase_table(NB, amp), dtype=P.F32), P.table(NB, amp)), (NB, amp)
            assert all(float(P.F32(v)) == v for v in ops.phase_table(NB, amp))


def test_patterns_produce_the_labels_they_promise():
    for S, B, Cc, hw, NB, kind, padded, pattern in P.INT_TABLE + [P.MAX_CASE]:
        HW = hw[0] * hw[1]
        lab = P.pattern_labels(pattern, S, B, NB)
        craw = P.coefs_for(lab, NB, HW, 11)
        g = P.gains(np.ones((B, 2)), HW)
        got = P.label_mirror(craw[..., 0], craw[..., 1], g[:, None, None, 0], g[:, None, None, 1], P.table(NB, 0.25), NB)
        assert np.array_equal(got, lab), (S, B, NB, pattern)
        used = set(np.unique(lab[:, :, 1:]).tolist())
        if pattern == "one":
            assert used == {NB - 1}
        if pattern == "never":
            assert NB - 1 not in used and -1 not in used
        if pattern == "skip":
            assert (lab[:, :, 2] == -1).all() and (S < 5 or ((lab[:, :, 3] == -1).any() and (lab[:, :, 3] >= 0).any()))
        mc, _ = P.counts(lab, range(1, P.T), NB)
        assert mc.sum(1).max() <= 2 ** 7


# ---- the derived formulas against brute force ------------------------------------------------------------------------------------------
def _brute_case(seed=3, B=2, NB=8, Cc=3, HW=6, rows=40, empty=(2, 5)):
    rng = np.random.RandomState(seed)
    d = rng.randn(B, rows, Cc, HW) + 0.5 * rng.randn(B, 1, Cc, HW)
    lab = rng.randint(0, NB, size=(B, rows))
    for e in empty:
        lab[lab == e] = (e + 1) % NB
    lab[1, :3] = -1
    d = d + 0.7 * np.cos(lab[:, :, None, None] + np.arange(HW))              # a coherent part
    n = np.stack([(lab == k).sum(1) for k in range(NB)], -1)
    raw = np.zeros((B, NB, 2 * Cc + 1, HW))
    for b in range(B):
        for k in range(NB):
            r = d[b][lab[b] == k]
            raw[b, k] = np.concatenate([r.sum(0), (r * r).sum(0), (r[:, 0] * r[:, 1]).sum(0)[None]], 0)
    return d, lab, n, raw


def test_derived_formulas_match_brute_force_and_the_law_of_total_variance():
    d, lab, n, raw = _brute_case()
    B, NB, Cc, HW = n.shape[0], n.shape[1], d.shape[2], d.shape[3]
    f = P.fields(n, raw, Cc)
    for b in range(B):
        kept = d[b][lab[b] >= 0]
        for k in range(NB):
            r = d[b][lab[b] == k]
            if len(r) == 0:
                assert np.isnan(f["dev"][b, k]).all() and np.isnan(f["var"][b, k]).all() and np.isnan(f["uv"][b, k]).all()
                assert np.isnan(f["coh"][b, k]).all()
                continue
            assert np.allclose(f["dev"][b, k], r.mean(0), rtol=1e-12, atol=1e-14)
            assert np.allclose(f["var"][b, k], r.var(0), rtol=1e-10, atol=1e-13)
            assert np.allclose(f["uv"][b, k], ((r[:, 0] - r[:, 0].mean(0)) * (r[:, 1] - r[:, 1].mean(0))).mean(0), rtol=1e-10, atol=1e-13)
            assert np.allclose(f["coh"][b, k], r.mean(0) - kept.mean(0), rtol=1e-10, atol=1e-13)
        # the law of total variance: coherent + incoherent = the variance of the labelled rows about their own mean
        tot = kept.var(0)
        assert np.abs(f["coh_var"][b] + f["incoh_var"][b] - tot).max() <= 1e-12 * np.abs(tot).max()
        cov = ((kept[:, 0] - kept[:, 0].mean(0)) * (kept[:, 1] - kept[:, 1].mean(0))).mean(0)
        assert np.abs(f["coh_uv"][b] + f["incoh_uv"][b] - cov).max() <= 1e-12 * np.abs(tot).max()
        assert 0 < f["coh_tke_frac"][b] < 1
        assert abs(f["coh_tke_frac"][b] - f["coh_var"][b, :2].sum() / tot[:2].sum()) <= 1e-12
    for key in ("coh_var", "incoh_var", "coh_uv", "incoh_uv", "coh_tke_frac"):
        assert np.isfinite(f[key]).all()                                     # empty sectors are left out, not spread
    # a case without any labelled row is NaN throughout
    f0 = P.fields(np.zeros((1, NB)), np.zeros((1, NB, 2 * Cc + 1, HW)), Cc)
    assert all(np.isnan(v).all() for v in f0.values())


def test_the_product_forms_the_fields_by_the_same_formulas():
    import tmg_ops as ops
    d, lab, n, raw = _brute_case(seed=9, empty=(0,))
    n[1], raw[1] = 0, 0                                                      # and a case without a row
    Cc = d.shape[2]
    want = P.fields(n, raw, Cc)
    got = ops._phase_fields(torch.from_numpy(n).double(), torch.from_numpy(raw), Cc)
    assert set(got) == set(want)
    for key, r in want.items():
        g = got[key].numpy()
        fin = np.isfinite(r)
        assert g.shape == r.shape and np.array_equal(np.isfinite(g), fin), key
        assert np.abs(g[fin] - r[fin]).max() <= 1e-13 * max(1.0, np.abs(r[fin]).max()), key


def test_speed_wraps_to_the_half_open_interval():
    lam = np.array([[4.0, 0.25]])
    for rate in (0.3, -0.3, 3.0, -3.0):
        th = 0.2 + rate * np.arange(7)
        coef = np.stack([2.0 * np.cos(th), 0.5 * np.sin(th), np.zeros(7)], -1)[None, None]       # [B, S, T, K], pair (0, 1)
        got = P.speed(coef, lam, (0, 1), range(7))
        assert got.shape == (1, 1) and abs(got[0, 0] - rate) <= 1e-12, rate
        two = P.speed(coef, lam, (0, 1), [0, 2, 4, 6])                      # every other step: twice the rate, wrapped
        want = 2 * rate - 2 * np.pi * np.ceil((2 * rate - np.pi) / (2 * np.pi))
        assert abs(two[0, 0] - want) <= 1e-12, rate
    # an increment of exactly pi stays +pi: (1, 0) -> (-1, 0) -> (1, 0)
    flip = np.array([[1.0, 0.0], [-1.0, 0.0], [1.0, 0.0]])[None, None]
    assert P.speed(flip, np.ones((1, 2)), (0, 1), range(3))[0, 0] == np.pi
    assert np.isnan(P.speed(np.zeros((1, 2, 5, 2)), lam, (0, 1), [3])).all()


# ---- every ValueError ------------------------------------------------------------------------------------------------------------------
def test_phase_args_errors():
    import tmg_ops as ops
    assert ops.phase_args([1, 0], 16, 0, 2) == ((1, 0), 16, 0.0)
    for kw, msg in ((dict(pair=(0, 0)), "different"), (dict(pair=(0,)), "two mode"), (dict(pair=(0, -1)), "two mode"), (dict(pair=3), "two modes"),
                    (dict(pair=(0, 1.0)), "two mode"), (dict(pair=(0, 8)), "modes >= 9"), (dict(bins=6), "bins"), (dict(bins=64), "bins"),
                    (dict(bins=8.0), "bins"), (dict(min_amp=-0.1), "min_amp"), (dict(min_amp=float("nan")), "min_amp"),
                    (dict(min_amp=float("inf")), "min_amp")):
        with pytest.raises(ValueError, match=msg):
            ops.phase_args(**{**dict(pair=(0, 1), bins=8, min_amp=0.25, K=8), **kw})


def test_wrapper_errors_come_before_the_model():
    from utils import utils
    for kw, msg in ((dict(modes=1), "modes >= 2"), (dict(pair=(2, 2)), "different"), (dict(bins=12), "bins"), (dict(min_amp=-1), "min_amp"),
                    (dict(pair=(0, 3), modes=3), "modes >= 4"), (dict(channels=(0, 0)), "distinct")):
        with pytest.raises(ValueError, match=msg):
            utils.modelPredPhase(None, None, None, None, **kw)


def test_constructor_errors_come_before_the_device():
    import tmg_ops as ops
    B, Cc, Hh, Ww = 2, 3, 4, 5
    mean, lam = torch.zeros(B, Cc, Hh, Ww), torch.ones(B, 2)
    base = dict(members=4, B=B, C=Cc, Hh=Hh, Ww=Ww, steps=3, device="cpu", out_std=torch.ones(Cc), mean=mean, lam=lam)

    class Ready(ops.EnsembleModes):                                          # an EnsembleModes without a device: the feed's fields only
        def __init__(self, S=4, K=3, steps=3):
            ops.EnsembleFeed.__init__(self, S, B, Cc, Hh, Ww, steps)
            self.K = K

    mk = lambda **kw: ops.EnsemblePhase(**{**base, "modes": Ready(), **kw})  # noqa: E731
    for kw, msg in ((dict(C=5), "2 <= C <= 4"), (dict(members=0), "members"), (dict(out_std=torch.tensor([1.0, 0.0, 1.0])), "strictly positive"),
                    (dict(u=-torch.ones(B, Cc)), "strictly positive"), (dict(steps=0), "steps, B, H, W >= 1"),
                    (dict(modes=None), "a ready EnsembleModes"), (dict(modes=Ready(S=5)), "another feed"), (dict(modes=Ready(steps=4)), "another feed"),
                    (dict(pair=(0, 3)), "modes >= 4"), (dict(pair=(1, 1)), "different"), (dict(bins=5), "bins"), (dict(min_amp=-1.0), "min_amp"),
                    (dict(mean=None), "need the tables"), (dict(lam=None), "need the tables"), (dict(mean=torch.zeros(B, 2, Hh, Ww)), "mean is a finite"),
                    (dict(mean=mean + float("nan")), "mean is a finite"), (dict(lam=torch.ones(B, 3)), "lam is a finite"),
                    (dict(lam=torch.zeros(B, 2)), "lam is a finite")):
        with pytest.raises(ValueError, match=msg):
            mk(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mk()


# ---- the case tables -------------------------------------------------------------------------------------------------------------------
def test_case_tables_reach_both_load_paths_and_every_sector_count():
    import tmg_hip
    for name, tab in (("integer", P.INT_TABLE), ("real", P.REAL_TABLE)):
        seen = set()
        for c in tab:
            S, B, Cc, hw, NB, kind, padded = c[:7]
            q = tmg_hip.ens_phase_plan(S, B, Cc, hw[0] * hw[1], NB)
            vec = q["vec"] and not padded                                    # a channel slice of a wider buffer is never dense
            seen.add("vector" if vec else "scalar")
            seen.add("NB=%d" % NB)
            seen.add("C=%d" % Cc)
            seen.add("chunking %d" % kind)
            tile = 1024 if vec else 256
            HW = hw[0] * hw[1]
            seen.add(("%s: " % ("vector" if vec else "scalar")) + ("one tile exactly" if HW == tile else "one thread over a tile" if HW in (tile + 1, tile + 4)
                                                                 else "ragged tiles" if HW > tile and HW % tile else "inside a tile"))
        assert seen >= {"vector", "scalar", "NB=4", "NB=8", "NB=16", "NB=32", "chunking 0", "chunking 1", "chunking 2"}, (name, seen)
        if name == "integer":
            assert seen >= {"C=2", "C=3", "C=4", "vector: one tile exactly", "scalar: one tile exactly", "vector: one thread over a tile",
                            "scalar: one thread over a tile", "vector: ragged tiles", "scalar: ragged tiles", "scalar: inside a tile"}, seen
    ints = P.INT_TABLE
    assert {c[3] for c in ints} >= {(1, 1), (5, 7)} and {c[0] for c in ints} >= {1, 17, 70} and {c[1] for c in ints} == {1, 3}
    assert {c[7] for c in ints} == {"one", "never", "alt", "skip"} and {c[6] for c in ints} == {False, True}
    assert P.MAX_CASE[0] == 1024 and P.MAX_CASE[3][0] * P.MAX_CASE[3][1] <= 8
    assert {(c[0], c[1], c[2]) for c in P.LABEL_TABLE} >= {(NB, B, S) for NB, B, S in ((4, 1, 1), (8, 3, 17), (32, 1, 70))}
    assert {c[0] for c in P.LABEL_TABLE} == {4, 8, 32} and {c[1] for c in P.LABEL_TABLE} == {1, 3} and {c[2] for c in P.LABEL_TABLE} == {1, 17, 70}
    assert all(sum(P.chunk_sizes(S, kind)) == S for S in (1, 5, 17, 70, 1024) for kind in (0, 1, 2))


def test_integer_and_fp64_references_agree_and_the_checks_are_sensitive():
    S, B, Cc, hw, NB, kind, padded, pattern = P.INT_TABLE[1]
    xs, tgt, m = P.int_inputs(S, B, Cc, hw, 7001)
    lab = P.pattern_labels(pattern, S, B, NB)
    a = P.scales(None, None, B, Cc)
    timed = range(1, P.T)
    ri, rf = P.reference(xs, lab, timed, a, m, NB, integer=True), P.reference(xs, lab, timed, a, m, NB)
    assert ri["raw"].dtype == np.int64 and np.array_equal(ri["raw"].astype(np.float64), rf["raw"]) and np.array_equal(ri["n"], rf["n"])
    mc, skipped = P.counts(lab, timed, NB)
    assert np.array_equal(mc.sum(1), ri["n"]) and np.array_equal(ri["n"].sum(1) + skipped, np.full(B, S * 3))
    acc = ri["raw"].astype(P.F32)
    P.check_integer(acc, ri, "fake")
    assert P.check_bound(acc, rf, Cc, "fake") == 0.0
    off = acc.copy()
    off[B - 1, 3, 2 * Cc, 5] += 1
    with pytest.raises(AssertionError):
        P.check_integer(off, ri, "off")
    for q in (0, Cc, 2 * Cc):                                                # one element of each kind of plane off by twice its bound
        off = acc.copy()
        k = int(np.argmax(rf["n"][0]))
        cr = P.C_ROUND_LIN if q < Cc else P.C_ROUND_PROD
        off[0, k, q, 0] += P.F32(2.0 * (rf["n"][0, k] + cr) * P.U24 * rf["abs"][0, k, q, 0] + 1e-30)
        if off[0, k, q, 0] != acc[0, k, q, 0]:
            with pytest.raises(AssertionError):
                P.check_bound(off, rf, Cc, "off")
    # the target's row through the same reference: S = 1
    rt = P.reference(tgt[:, None], lab[:, :1], timed, a, m, NB, integer=True)
    assert rt["n"].sum() == B * 3 - int((lab[:, 0, 1:] < 0).sum())
