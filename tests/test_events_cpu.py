"""CPU-side checks of the ensemble event verification (Brier, reliability, ROC, fractions skill score): the kernel entries are declared
in their own header, listed apart and exported; the ops / post-processing entry points exist with their signatures and the pinned old
ones are unchanged; the argument errors come in the documented order without a GPU; the C entries return their codes before any
launch; the launch plan's tiles cover every pixel once with halo = the largest w // 2 inside the LDS limit; the numpy simulation of
the tiled summed-area scheme (tests/event_cases.py), driven by the plan, equals the reference; the host formulas of
tmg_ops.event_table_scores / event_fss meet the reference's other formulas inside the float tolerance; every named defect changes the
reference's own outputs on the GPU tests' tables; and those tables reach every plan branch and have no degenerate score."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import event_cases as K

NAMES = ["tmg_ens_event_plan", "tmg_ens_event_count", "tmg_ens_event_step"]
c_i64 = ctypes.c_int64
LDS_LIMIT = 160 * 1024


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_event.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.EVENT_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert len(re.findall(r'^#include "tmglow_hip_event\.h"$', main, re.M)) == 1 and main.count("tmglow_hip_event.h") == 1
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.GRAM_EXPORTS,
                      tmg_hip.SFUN_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert name not in main and hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_event.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_event.hip"))
    assert callable(tmg_hip.ens_event_plan) and callable(tmg_hip.ens_event_count) and callable(tmg_hip.ens_event_step)
    assert re.search(r"for f in [^;]*\btmg_event\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    assert "atomicAdd(float" not in open(os.path.join(tmg_hip.CSRC, "tmg_event.hip")).read()


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredEvents).parameters
    assert list(sig) == old + ["events", "scales"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, ((0, 0.0, "<"),), (1, 3, 5, 9, 17, 33)]
    init = inspect.signature(tmg_ops.EnsembleEvents.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "events", "scales"]
    assert init["u"].default is None and init["events"].default == ((0, 0.0, "<"),) and init["scales"].default == (1, 3, 5, 9, 17, 33)
    add = inspect.signature(tmg_ops.EnsembleEvents.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert add["target"].default is inspect.Parameter.empty
    assert list(inspect.signature(tmg_ops.EnsembleEvents.finalize).parameters) == ["self"]
    assert list(inspect.signature(tmg_ops.event_args).parameters) == ["events", "scales", "C"]
    assert list(inspect.signature(tmg_hip.ens_event_plan).parameters) == ["S", "B", "H", "W", "K", "scales"]
    assert callable(tmg_ops.raw_thresholds)
    # the pinned ones keep their parameter lists
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert list(inspect.signature(utils.modelPredScores).parameters) == old
    assert list(inspect.signature(utils.modelPredEnergy).parameters) == old + ["groups"]
    assert list(inspect.signature(utils.modelPredQuantiles).parameters) == old + ["levels", "exceed"]
    assert list(inspect.signature(utils.modelPredStructure).parameters) == old + ["lags", "weights"]
    assert list(inspect.signature(tmg_ops.EnsembleQuantiles.__init__).parameters) == [
        "self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "levels", "exceed"]
    for doc in (utils.modelPredEvents.__doc__, tmg_ops.EnsembleEvents.__doc__):
        for word in ("rel_count", "brier_res", "roc_area", "fss_raw", "time_fss_uniform", "time_brier_map", "event_scales"):
            assert word in doc, word
    assert "diagonal" in utils.modelPredEvents.__doc__ and "0.5 = no discrimination" in utils.modelPredEvents.__doc__
    assert "O(B K HW)" in tmg_ops.EnsembleEvents.__doc__


def test_raw_thresholds_are_the_quantile_class_expression():
    """(value / u - out_mu) / out_std in fp64, rounded once: the helper both classes use."""
    import tmg_ops
    g = torch.Generator().manual_seed(5)
    mu, sd, u = torch.randn(3, generator=g), 0.5 + torch.rand(3, generator=g), 0.5 + torch.rand(4, 3, generator=g)
    ex = [(0, 0.0, "<"), (2, 1.25, ">"), (1, -0.3, "<")]
    for uu in (u, None):
        got = tmg_ops.raw_thresholds(ex, 4, 3, mu, sd, uu)
        ref = K.thresholds(ex, 4, 3, mu.numpy(), sd.numpy(), None if uu is None else uu.numpy())
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3) and np.array_equal(got.numpy(), ref)


# ---- event_args -------------------------------------------------------------------------------------------------------------------------
def test_event_args_accepts_the_documented_forms():
    import tmg_ops
    ev, sc = tmg_ops.event_args([[0, 0.0, "<"], (2, 1, ">")], [33, 1, 5], 3)
    assert ev == [(0, 0.0, "<"), (2, 1, ">")] and sc == (33, 1, 5)
    assert tmg_ops.event_args(((0, 0.0, "<"),), (1, 3, 5, 7, 9, 11, 13, 15), 2)[1] == (1, 3, 5, 7, 9, 11, 13, 15)
    assert tmg_ops.event_args(((0, 0.0, "<"),), (np.int64(3),), 2)[1] == (3,)


@pytest.mark.parametrize("events,word", [
    ((), "at least one"), (((0, 0.0, "<"),) * 5, "at most 4"), (((3, 0.0, "<"),), "exceed entries are"), (((0, 0.0, ">="),), "exceed entries are"),
    (((0, float("nan"), "<"),), "exceed entries are"), (((True, 0.0, "<"),), "exceed entries are"), (((0, 0.0),), "exceed entries are"),
])
def test_a_bad_event_raises_with_the_quantile_rules(events, word):
    import tmg_ops
    with pytest.raises(ValueError, match=word):
        tmg_ops.event_args(events, (2,), 3)                                   # (the scales are wrong too: the events come first)


@pytest.mark.parametrize("scales,word", [
    ((), "1 to 8"), ((1, 3, 5, 7, 9, 11, 13, 15, 17), "1 to 8"), ((1, 4, 35), "got 4"), ((1, 35, 4), "got 35"), ((0,), "got 0"), ((-3,), "got -3"),
    ((3.0,), r"got 3\.0"), ((True,), "got True"), ((1, 3, 1), "distinct, got 1 twice"), ((3, 3, 2), "distinct, got 3 twice"), (("3",), "got '3'"),
])
def test_a_bad_scale_is_named(scales, word):
    import tmg_ops
    with pytest.raises(ValueError, match=word):
        tmg_ops.event_args(((0, 0.0, "<"),), scales, 3)


# ---- the constructor's error order: every case is wrong in the named argument AND in every later one ---------------------------------
BAD_STD = torch.tensor([1.0, float("nan"), 1.0])
BAD_MU = torch.tensor([0.0, float("inf"), 0.0])
BAD_EV = ((7, 0.0, "<"),)
BAD_SC = (2,)


def _events(members=3, B=2, Cc=3, steps=2, out_mu=None, out_std=None, u=None, events=((0, 0.0, "<"),), scales=(1, 3), device="cpu", hw=(4, 5)):
    import tmg_ops
    return tmg_ops.EnsembleEvents(members, B, Cc, hw[0], hw[1], steps, device, torch.zeros(Cc) if out_mu is None else out_mu,
                                  torch.ones(Cc) if out_std is None else out_std, u=u, events=events, scales=scales)


def test_constructor_errors_come_in_the_documented_order():
    bad_u = torch.tensor([[1.0, -1.0, 1.0]] * 2)
    with pytest.raises(ValueError, match="channels"):
        _events(members=0, Cc=5, steps=0, out_std=BAD_STD, events=BAD_EV, scales=BAD_SC)
    with pytest.raises(ValueError, match="steps >= 1"):
        _events(members=0, steps=0, out_std=BAD_STD, events=BAD_EV, scales=BAD_SC)
    with pytest.raises(ValueError, match="exceed entries are"):
        _events(members=0, out_std=BAD_STD, events=BAD_EV, scales=BAD_SC)
    with pytest.raises(ValueError, match="scales are odd integers"):
        _events(members=0, out_std=BAD_STD, scales=BAD_SC)
    with pytest.raises(ValueError, match="members <= 1024"):
        _events(members=1025, out_std=BAD_STD, out_mu=BAD_MU)
    with pytest.raises(ValueError, match="need 3 entries"):
        _events(out_std=torch.ones(2), u=bad_u)
    with pytest.raises(ValueError, match="out_std must be finite"):
        _events(out_std=BAD_STD, out_mu=BAD_MU, u=bad_u)
    with pytest.raises(ValueError, match="out_mu must be finite"):
        _events(out_mu=BAD_MU, u=bad_u)
    with pytest.raises(ValueError, match="u must be finite"):
        _events(u=bad_u, members=1024, steps=2048)
    with pytest.raises(ValueError, match=r"S\^2 Tk = 1024\^2 \* 2048"):
        _events(members=1024, steps=2048)
    with pytest.raises(ValueError, match=r"S\^2 w_max\^4 HW Tk"):
        _events(members=1024, steps=2047, scales=(33,), hw=(2 ** 15, 2 ** 15))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _events()


# ---- the C entries return their codes with no device ----------------------------------------------------------------------------------
def _plan_rc(dims, scales, plan=True):
    import tmg_hip
    buf = (c_i64 * 12)()
    return tmg_hip.lib().tmg_ens_event_plan(_i64(*dims) if dims else None, _i64(*scales) if scales is not None else None,
                                            buf if plan else None)


def test_plan_entry_codes():
    ok = (5, 3, 50, 58, 2, 2)
    assert _plan_rc(ok, (1, 33)) == 0
    for dims in ((0, 3, 50, 58, 2, 2), (5, 0, 50, 58, 2, 2), (5, 3, 0, 58, 2, 2), (5, 3, 50, 0, 2, 2), (5, 3, 50, 58, 0, 2), (5, 3, 50, 58, 5, 2),
                 (5, 3, 50, 58, 2, 0), (5, 3, 50, 58, 2, 9)):
        assert _plan_rc(dims, (1, 33)) == -1, dims
    for sc in ((1, 2), (1, 35), (0, 1), (3, 3), (-1, 3)):
        assert _plan_rc(ok, sc) == -1, sc
    assert _plan_rc((1025, 3, 50, 58, 2, 2), (1, 2)) == -1                    # a bad argument before a size
    assert _plan_rc((1025, 3, 50, 58, 2, 2), (1, 33)) == -2
    assert _plan_rc((5, 65536, 50, 58, 2, 2), (1, 33)) == -2
    assert _plan_rc((5, 3, 2 ** 16, 2 ** 15, 2, 2), (1, 33)) == -2
    assert _plan_rc((1024, 1, 2 ** 15, 2 ** 15, 1, 1), (33,)) == -2           # S^2 w^4 HW = 2^20 * 1.19e6 * 2^30 > 2^63
    assert _plan_rc((1024, 1, 2 ** 15, 2 ** 15, 1, 1), (1,)) == 0
    assert _plan_rc((1025, 3, 50, 58, 2, 2), None) == -2                      # a size before a null pointer
    assert _plan_rc(ok, None) == -3 and _plan_rc(ok, (1, 33), plan=False) == -3 and _plan_rc(None, (1, 33)) == -3


def test_count_and_step_entry_codes_before_any_launch():
    """Pointers are fake non-null values: a code comes back before anything is dereferenced on the device or launched."""
    import tmg_hip
    lib = tmg_hip.lib()
    P = ctypes.c_void_p(4096)
    N = ctypes.c_void_p(0)
    ev = _i64(0, 0, 1, 1)

    def count(dims, y=P, y_d=(4, 1), thr=P, e=ev, cnt=P):
        return lib.tmg_ens_event_count(y, _i64(*y_d) if y_d else None, thr, e, cnt, _i64(*dims), N)

    ok = (2, 3, 20, 3, 5, 0, 2)                                               # k, B, HW, C, S, m0, K
    for dims in ((0, 3, 20, 3, 5, 0, 2), (2, 0, 20, 3, 5, 0, 2), (2, 3, 0, 3, 5, 0, 2), (2, 3, 20, 1, 5, 0, 2), (2, 3, 20, 5, 5, 0, 2),
                 (2, 3, 20, 3, 0, 0, 2), (2, 3, 20, 3, 5, -1, 2), (2, 3, 20, 3, 5, 4, 2), (2, 3, 20, 3, 5, 0, 0), (2, 3, 20, 3, 5, 0, 5)):
        assert count(dims) == -1, dims
    assert count(ok, y_d=(2, 0)) == -1 and count(ok, y_d=(4, 2)) == -1 and count(ok, y_d=(4, -1)) == -1
    assert count(ok, e=_i64(3, 0, 1, 1)) == -1 and count(ok, e=_i64(0, 2, 1, 1)) == -1
    assert count((2, 3, 20, 3, 1025, 0, 2)) == -2 and count((2, 65536, 20, 3, 5, 0, 2)) == -2 and count((2, 3, 2 ** 31, 3, 5, 0, 2)) == -2
    assert count((2, 3, 20, 3, 1025, 0, 2), y=N) == -2                        # a size before a null pointer
    assert count(ok, y=N) == -3 and count(ok, thr=N) == -3 and count(ok, cnt=N) == -3 and count(ok, e=None) == -3 and count(ok, y_d=None) == -3

    def step(dims, scales=(1, 33), cnt=P, tgt=P, t_d=(4, 1), thr=P, e=ev, rc=P, rh=P, fss=P, ts=P, o_d=(100, 100)):
        return lib.tmg_ens_event_step(cnt, tgt, _i64(*t_d) if t_d else None, thr, e, _i64(*scales) if scales is not None else None, rc, rh,
                                      fss, ts, _i64(*o_d) if o_d else None, _i64(*dims), N)

    ok = (5, 3, 50, 58, 3, 2, 2, 0, 1)                                        # S, B, H, W, C, K, NS, t_before, flags
    for i, v in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (4, 5), (5, 0), (5, 5), (6, 0), (6, 9), (7, -1)):
        dims = list(ok)
        dims[i] = v
        assert step(dims) == -1, dims
    assert step(ok, scales=(1, 2)) == -1 and step(ok, scales=(3, 3)) == -1 and step(ok, scales=(1, 35)) == -1
    assert step(ok, t_d=(2, 0)) == -1 and step(ok, t_d=(4, 2)) == -1
    assert step(ok, e=_i64(3, 0, 1, 1)) == -1
    assert step(ok, o_d=(11, 100)) == -1 and step(ok, o_d=(100, 11)) == -1     # K (S + 1) = 12, 3 K NS = 12
    assert step((1025, 3, 50, 58, 3, 2, 2, 0, 1), o_d=(3000, 100)) == -2 and step((5, 65536, 50, 58, 3, 2, 2, 0, 1)) == -2
    assert step((1024, 1, 50, 58, 3, 2, 2, 2047, 1), o_d=(3000, 100)) == -2    # S^2 (t_before + 1) = 2^31
    assert step((1024, 1, 50, 58, 3, 2, 2, 2047, 0), o_d=(3000, 100), cnt=N) == -3   # ... only when the sums advance
    assert step((1025, 3, 50, 58, 3, 2, 2, 0, 1), o_d=(3000, 100), cnt=N) == -2     # a size before a null pointer
    for kw in ("cnt", "tgt", "thr", "rc", "rh", "fss", "ts"):
        assert step(ok, **{kw: N}) == -3, kw
    assert step(ok, e=None) == -3 and step(ok, scales=None) == -3 and step(ok, t_d=None) == -3 and step(ok, o_d=None) == -3


def test_step_without_time_flag_does_not_need_the_sums():
    """With flags = 0 a null tsum is not an error: the next missing pointer is reported instead."""
    import tmg_hip
    P, N = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    rc = tmg_hip.lib().tmg_ens_event_step(N, P, _i64(4, 1), P, _i64(0, 0), _i64(1), P, P, P, N, _i64(100, 100),
                                          _i64(5, 3, 50, 58, 3, 1, 1, 0, 0), N)
    assert rc == -3                                                           # cnt is null; with cnt given the call would launch


# ---- plan geometry ---------------------------------------------------------------------------------------------------------------------
def _cases():
    return [(i, c) for i, c in enumerate(K.INT_TABLE + [K.LONG_CASE])]


def _plan(case):
    import tmg_hip
    S, B, Cc, hw, t_start, kind, padded, Kn, scales = case
    return tmg_hip.ens_event_plan(S, B, hw[0], hw[1], Kn, scales)


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE) + 1))
def test_plan_geometry_covers_every_pixel_once_inside_the_lds_limit(idx):
    case = (K.INT_TABLE + [K.LONG_CASE])[idx]
    S, B, Cc, hw, t_start, kind, padded, Kn, scales = case
    q = _plan(case)
    assert q["halo"] == max(scales) // 2 and q["threads"] == 256 and q["ws"] == 0 and q["scales"] == list(scales)
    assert q["NTY"] == -(-hw[0] // q["TH"]) and q["NTX"] == -(-hw[1] // q["TW"]) and q["blocks"] == q["NTY"] * q["NTX"] * Kn * B
    assert q["TH"] * q["TW"] % q["threads"] == 0                              # whole pixels per thread
    assert q["rows"] == q["TH"] + 2 * q["halo"] + 1 and q["pitch"] >= q["TW"] + 2 * q["halo"] + 1
    assert q["pitch"] % 2 == 1                                                # the row pass strides by pitch: odd keeps 32 rows on 32 banks
    assert len({(r * q["pitch"]) % 32 for r in range(32)}) == 32
    assert q["lds"] == 4 * (2 * q["rows"] * q["pitch"] + 2 * (S + 1)) + 8 * 4 * 24 and q["lds"] <= LDS_LIMIT
    assert S * q["rows"] * q["pitch"] < 2 ** 31                               # a table entry stays in int32
    seen = np.zeros(hw, np.int64)
    for ty in range(q["NTY"]):
        for tx in range(q["NTX"]):
            seen[ty * q["TH"]:(ty + 1) * q["TH"], tx * q["TW"]:(tx + 1) * q["TW"]] += 1
    assert bool((seen == 1).all())


def test_largest_plan_stays_inside_the_lds_limit():
    import tmg_hip
    q = tmg_hip.ens_event_plan(1024, 1, 100, 100, 4, (1, 3, 5, 7, 9, 17, 25, 33))
    assert q["halo"] == 16 and q["lds"] <= 64 * 1024 <= LDS_LIMIT


def test_the_tables_reach_every_plan_branch():
    plans = {i: _plan(c) for i, c in _cases()}
    cases = dict(_cases())
    one = [i for i, q in plans.items() if q["NTY"] == 1 and q["NTX"] == 1 and min(cases[i][3]) > 1]
    both = [i for i, q in plans.items() if q["NTY"] >= 2 and q["NTX"] >= 2 and cases[i][3][0] % q["TH"] and cases[i][3][1] % q["TW"]]
    assert one and both
    assert any(c[3][0] == 1 for c in cases.values()) and any(c[3][1] == 1 for c in cases.values())
    assert any(max(c[8]) // 2 >= max(c[3]) for c in cases.values())           # a halo wider than the field
    assert any(c[3] == (7, 9) and 33 in c[8] for c in cases.values())
    assert any(len(c[8]) == 1 for c in cases.values()) and any(len(c[8]) == 8 for c in cases.values())
    assert {c[0] for c in cases.values()} == {1, 2, 5, 17, 64, 130, 1024}
    assert {c[5] for c in cases.values()} == {0, 1, 2} and {c[2] for c in cases.values()} == {2, 3, 4} and {c[1] for c in cases.values()} == {1, 3}
    assert {c[6] for c in cases.values()} == {False, True} and {c[4] for c in cases.values()} == {0, 1}
    assert any(c[7] == 4 for c in cases.values())
    ev = K.int_events(3, 4)
    assert ev[0][0] == ev[1][0] and {ev[0][2], ev[1][2]} == {">", "<"}        # both directions on one channel
    assert {c[3] for c in cases.values()} | {c[3] for c in K.REAL_TABLE} == K.FIELDS
    assert {c[4] for c in K.REAL_TABLE} == {"gauss", "smooth", "biased"} and {c[5] for c in K.REAL_TABLE} == {False, True}
    assert K.LONG_CASE[0] == 2 and K.LONG_CASE[3] == (181, 183)


# ---- reference, simulation, host formulas, defects -----------------------------------------------------------------------------------
def test_no_table_case_is_degenerate():
    """Apart from the fields with HW < 8, every case has a finite roc_area and fss at every step and event (the seeds are chosen so)."""
    n = 0
    for idx, case in _cases():
        if case[3][0] * case[3][1] < 8:
            continue
        ref = K.int_reference(idx)
        for key in ("roc_area", "fss", "time_roc_area", "time_fss"):
            assert bool(np.isfinite(ref[key]).all()), (idx, key)
        n += 1
    for idx in range(len(K.REAL_TABLE)):
        ref = K.real_reference(idx)
        for key in ("roc_area", "fss", "time_roc_area", "time_fss"):
            assert bool(np.isfinite(ref[key]).all()), ("real", idx, key)
    assert n == len(K.INT_TABLE) + 1 - 3                                      # all but (1, 2), (2, 1) and (1, 5)


def test_thresholds_fall_on_values_so_that_strictness_shows():
    for idx, case in _cases():
        xs, tgt, events, t_start = K.int_case_inputs(case, idx)
        assert set(np.unique(xs)) <= set(range(-3, 4))
        for ch, v, _ in events:
            assert float(v) in set(np.unique(xs[:, :, :, ch]).tolist()) or xs[:, :, :, ch].size < 8


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE) + 1))
def test_the_tiled_summed_area_simulation_equals_the_reference(idx):
    case = (K.INT_TABLE + [K.LONG_CASE])[idx]
    S, B, Cc, hw, t_start, kind, padded, Kn, scales = case
    q = _plan(case)
    ref = K.int_reference(idx)
    n, o = ref["n"], ref["o"]
    for t in range(n.shape[0] if idx < len(K.INT_TABLE) else 1):
        for b in range(B):
            for k in range(Kn):
                cnt, hit, raw, seen = K.simulate(n[t, b, k], o[t, b, k], S, scales, q)
                assert bool((seen == 1).all())
                assert np.array_equal(cnt, ref["rel_count"][b, t, k]) and np.array_equal(hit, ref["rel_hit"][b, t, k])
                assert np.array_equal(raw, ref["fss_raw"][b, t, k]), (idx, t, b, k)


@pytest.mark.parametrize("idx", [3, 5, 7, 11])
def test_host_formulas_meet_the_reference_inside_the_float_tolerance(idx):
    """tmg_ops.event_table_scores / event_fss on the reference's own tables and raw sums against the reference's other formulas."""
    import tmg_ops
    S, scales, t_start = K.INT_TABLE[idx][0], K.INT_TABLE[idx][8], K.INT_TABLE[idx][4]
    ref = K.int_reference(idx)
    cnt, hit, raw = (torch.from_numpy(np.ascontiguousarray(ref[k])) for k in ("rel_count", "rel_hit", "fss_raw"))
    got = {k: v.to(torch.float32).numpy() for k, v in tmg_ops.event_table_scores(cnt, hit, S).items() if k in K.STEP_KEYS}
    got["fss"] = tmg_ops.event_fss(raw, S).to(torch.float32).numpy()
    sc = tmg_ops.event_table_scores(cnt[:, t_start:].sum(1), hit[:, t_start:].sum(1), S)
    for key in ("brier", "brier_rel", "brier_res", "brier_unc", "base_rate", "roc_area"):
        got["time_" + key] = sc[key].to(torch.float32).numpy()
    got["time_fss_uniform"] = (0.5 + sc["base_rate"] / 2).to(torch.float32).numpy()
    got["time_rel_obs_freq"] = sc["obs_freq"].to(torch.float32).numpy()
    got["time_roc_hit_rate"], got["time_roc_false_rate"] = sc["roc_hit_rate"].to(torch.float32).numpy(), sc["roc_false_rate"].to(torch.float32).numpy()
    got["time_fss"] = tmg_ops.event_fss(raw[:, t_start:].sum(1), S).to(torch.float32).numpy()
    got["time_brier_map"] = ref["time_brier_map"].astype(np.float32)
    worst = K.check_floats(got, ref, "host formulas %d" % idx)
    got.update({k: ref[k] for k in ("rel_count", "rel_hit", "fss_raw")})
    K.check_identities(got, S, scales, K.INT_TABLE[idx][3], "host formulas %d" % idx)
    print("case %d: worst share of the float tolerance %.3f" % (idx, worst))


def test_degenerate_tables_give_nan_where_documented():
    import tmg_ops
    cnt = torch.tensor([[4, 0, 2], [4, 0, 2], [0, 0, 0]])
    hit = torch.tensor([[0, 0, 0], [4, 0, 2], [0, 0, 0]])
    sc = tmg_ops.event_table_scores(cnt, hit, 2)
    assert bool(torch.isnan(sc["roc_area"]).all())                            # no event, no non-event, no pixel
    assert sc["brier"][0].item() == (2 * 4) / (4 * 6) and sc["brier_unc"][1].item() == 0.0
    assert torch.isnan(sc["obs_freq"][0, 1]) and sc["obs_freq"][0, 0].item() == 0.0
    assert torch.isnan(tmg_ops.event_fss(torch.zeros(3, dtype=torch.int64), 2))
    assert tmg_ops.event_fss(torch.tensor([8, 4, 2]), 2).item() == 1.0


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_every_named_defect_changes_the_reference_outputs_on_the_gpu_tables(defect):
    """What the GPU tests compare for equality (tables, raw sums, per-pixel sums) or inside the float tolerance (the derived
    scores) moves under every defect, on the tables' own cases."""
    changed, applicable = 0, 0
    for idx, case in _cases():
        S, B, Cc, hw, t_start, kind, padded, Kn, scales = case
        if hw[0] * hw[1] < 8 or idx == len(K.INT_TABLE):
            continue
        if defect in ("even_window", "wrap") and max(scales) == 1:
            continue
        if defect == "drop_last" and max(hw) < 32:
            continue
        applicable += 1
        xs, tgt, events, ts = K.int_case_inputs(case, idx)
        bad = K.reference(xs, tgt, K.thresholds(events, B, Cc), events, scales, ts, defect=defect)
        ref = K.int_reference(idx)
        moved = any(not np.array_equal(bad[k], ref[k]) for k in ("rel_count", "rel_hit", "fss_raw", "tsum_steps"))
        if not moved:
            for key in K.FLOAT_KEYS:
                r, g = ref[key], bad[key]
                ok = ~np.isnan(r) & ~np.isnan(g)
                moved = moved or not np.array_equal(np.isnan(r), np.isnan(g)) or bool((np.abs(g[ok] - r[ok]) > K.U24 * np.abs(r[ok]) + K.TOL_ABS).any())
        changed += moved
    assert applicable >= 3 and changed == applicable, "%s: %d of %d cases changed" % (defect, changed, applicable)
