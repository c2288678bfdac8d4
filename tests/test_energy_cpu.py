"""CPU-side checks of the ensemble energy score: the kernel entries are declared in their own header, listed apart and exported; the
ops / post-processing entry points exist with their signatures; the argument errors come in the documented order without a GPU; the
C entries return their codes before any launch; the launch plan covers every row macro-tile pair and every pixel exactly once inside
its workspace cap; the float32 simulation of the scheme (tests/energy_cases.py) equals the integer reference and stays inside the
rounding bound; and reference and bound are sensitive to the defects the GPU comparison has to catch, on the GPU tests' own tables."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import energy_cases as K

NAMES = ["tmg_ens_gram_plan", "tmg_ens_gram_step", "tmg_ens_gram_traj"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_gram.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.GRAM_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert len(re.findall(r'^#include "tmglow_hip_gram\.h"$', main, re.M)) == 1 and main.count("tmglow_hip_gram.h") == 1
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert name not in main and hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_gram.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_gram.hip"))
    assert callable(tmg_hip.ens_gram_step) and callable(tmg_hip.ens_gram_plan) and callable(tmg_hip.ens_gram_traj)
    assert "tmg_gram" in open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read()


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredEnergy).parameters
    assert list(sig) == old + ["groups"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, ((0, 1), (2,))]
    init = inspect.signature(tmg_ops.EnsembleEnergy.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_std", "u", "groups"]
    assert init["u"].default is None and init["groups"].default is None
    add = inspect.signature(tmg_ops.EnsembleEnergy.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert add["target"].default is inspect.Parameter.empty
    assert list(inspect.signature(tmg_ops.EnsembleEnergy.finalize).parameters) == ["self"]
    assert list(inspect.signature(tmg_hip.ens_gram_plan).parameters) == ["S", "B", "C", "HW"]
    assert list(inspect.signature(tmg_hip.ens_gram_step).parameters) == [
        "xs", "target", "a2", "groups", "r", "ws", "traj", "outf", "outi", "t", "t_before", "flags"]
    assert list(inspect.signature(tmg_hip.ens_gram_traj).parameters) == ["traj", "outf", "outi"]
    # the pinned ones keep their parameter lists
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert list(inspect.signature(utils.modelPredScores).parameters) == old
    doc = utils.modelPredEnergy.__doc__
    assert "target_dist_mean" in doc and "pair_dist_mean" in doc and "calibrated" in doc


# ---- the constructor's error order: every case is wrong in the named argument AND in every later one ---------------------------------
BAD_STD = torch.tensor([1.0, float("nan"), 1.0])
BAD_GROUPS = ((0, 0),)


def _energy(members=3, B=2, Cc=3, steps=2, out_std=None, u=None, groups=None, device="cpu"):
    import tmg_ops
    return tmg_ops.EnsembleEnergy(members, B, Cc, 4, 5, steps, device, torch.ones(Cc) if out_std is None else out_std, u=u, groups=groups)


@pytest.mark.parametrize("Cc", [1, 5])
def test_bad_channel_count_raises_first(Cc):
    with pytest.raises(ValueError, match="channels"):
        _energy(members=0, Cc=Cc, out_std=BAD_STD, groups=BAD_GROUPS)


@pytest.mark.parametrize("members", [0, 1025, -1])
def test_bad_member_count_raises_second(members):
    with pytest.raises(ValueError, match="members"):
        _energy(members=members, out_std=BAD_STD[:2], groups=BAD_GROUPS)


def test_short_out_std_raises_third():
    with pytest.raises(ValueError, match="entries"):
        _energy(out_std=BAD_STD[:2], u=torch.zeros(2, 3), groups=BAD_GROUPS)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_out_std_then_bad_u_raise_before_the_groups(bad):
    with pytest.raises(ValueError, match=r"^out_std must"):
        _energy(out_std=torch.tensor([1.0, bad, 2.0]), u=torch.full((2, 3), bad), groups=BAD_GROUPS)
    u = torch.ones(2, 3)
    u[1, 2] = bad
    with pytest.raises(ValueError, match=r"^u must"):
        _energy(u=u, groups=BAD_GROUPS)


@pytest.mark.parametrize("groups", [(), ((),), ((0, 0),), ((0, 1), (1,)), ((3,),), ((-1,),), ((0.0,),), ((True,),), (0, 1)])
def test_bad_groups_raise_before_the_device(groups):
    with pytest.raises(ValueError, match="^groups"):
        _energy(groups=groups)


@pytest.mark.parametrize("members,groups", [(1, None), (1024, ((2, 0), (1,))), (5, ((1,),))])
def test_cpu_device_raises_last(members, groups):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _energy(members=members, u=torch.full((2, 3), 0.5), groups=groups)


def test_default_groups():
    import tmg_ops
    assert tmg_ops.energy_groups(((0, 1), (2,)), 3) == ((0, 1), (2,))
    assert tmg_ops.energy_groups([[2], [1, 0]], 4) == ((2,), (1, 0))


def _tiny_model_and_loader():
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    return m, [(x, torch.zeros(2, 3, 3, 16, 16), torch.ones(2))]


LOG = SimpleNamespace(log=lambda *a, **k: None)


def test_model_pred_energy_bad_groups_raise_first_and_the_cpu_last():
    from utils import utils
    m, loader = _tiny_model_and_loader()
    with pytest.raises(ValueError, match="^groups"):
        utils.modelPredEnergy(SimpleNamespace(device=None), m, loader, LOG, samples=2, tmax=2, groups=((0, 3),))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredEnergy(SimpleNamespace(device=None), m, loader, LOG, samples=2, tmax=2)


# ---- the C entries' return codes: all of them return before any launch ---------------------------------------------------------------
PTRS = ("xs", "target", "a2", "r", "ws", "traj", "outf", "outi")
GRP = (0, 1, -1, -1, 2, -1, -1, -1) + (-1,) * 8


def _call(dims, grp=GRP, t_d=(3, 0), ws_floats=None, ptrs=None, null_grp=False, null_td=False):
    """tmg_ens_gram_step with dims = (S, B, HW, C, Gn, Tk, t, t_before, flags); ptrs: the device-side pointers by name, null by default."""
    import tmg_hip
    p = dict.fromkeys(PTRS, None)
    p.update(ptrs or {})
    v = lambda n: ctypes.c_void_p(p[n])                                       # noqa: E731
    i64 = lambda vals: (c_i64 * max(1, len(vals)))(*vals)                     # noqa: E731
    return tmg_hip.lib().tmg_ens_gram_step(v("xs"), v("target"), None if null_td else i64(t_d), v("a2"), None if null_grp else i64(grp),
                                           v("r"), v("ws"), c_i64((1 << 40) if ws_floats is None else ws_floats), v("traj"), v("outf"),
                                           v("outi"), i64(dims), ctypes.c_void_p(0))


GOOD = (4, 2, 35, 3, 2, 3, 1, 0, 0)


@pytest.mark.parametrize("dims,kw", [
    ((4, 2, 35, 1, 2, 3, 1, 0, 0), {}), ((4, 2, 35, 5, 2, 3, 1, 0, 0), {}),                          # C outside 2..4
    ((0, 2, 35, 3, 2, 3, 1, 0, 0), {}), ((4, 0, 35, 3, 2, 3, 1, 0, 0), {}), ((4, 2, 0, 3, 2, 3, 1, 0, 0), {}),
    ((4, 2, 35, 3, 0, 3, 1, 0, 0), {}), ((4, 2, 35, 3, 5, 3, 1, 0, 0), {}),                          # Gn outside 1..4
    ((4, 2, 35, 3, 2, 0, 0, 0, 0), {}), ((4, 2, 35, 3, 2, 3, 3, 0, 0), {}), ((4, 2, 35, 3, 2, 3, -1, 0, 0), {}),   # Tk, t
    ((4, 2, 35, 3, 2, 3, 1, -1, 0), {}),
    (GOOD, {"grp": (0, 1, -1, -1, 1, -1, -1, -1) + (-1,) * 8}), (GOOD, {"grp": (0, 3, -1, -1, 2, -1, -1, -1) + (-1,) * 8}),   # twice; range
    (GOOD, {"grp": (0, 1, -1, -1) + (-1,) * 12}), (GOOD, {"grp": (-1, 0, -1, -1, 2, -1, -1, -1) + (-1,) * 8}),   # empty; a gap
    (GOOD, {"t_d": (2, 0)}), (GOOD, {"t_d": (4, 2)}),                                                # the target's stride / offset
])
def test_step_returns_minus_one_for_bad_dims(dims, kw):
    # also wrong in what the later codes check (S > 1024 where S is not the subject, null pointers throughout): -1 comes first
    if dims[0] == 4:
        dims = (2000,) + dims[1:]
    assert _call(dims, **kw) == -1


def test_step_returns_minus_one_for_a_workspace_under_the_plan():
    import tmg_hip
    need = tmg_hip.ens_gram_plan(4, 2, 3, 35)["ws"]
    assert _call(GOOD, ws_floats=need - 1, ptrs=dict.fromkeys(PTRS, 0x1000)) == -1
    assert _call(GOOD, ws_floats=need) == -3                                  # enough: the null pointers are next


@pytest.mark.parametrize("dims,kw", [
    ((1025,) + GOOD[1:], {}), ((4, 30000, 35, 3, 2, 3, 1, 0, 0), {}), ((4, 2, (1 << 31) - 256, 3, 2, 3, 1, 0, 0), {}),
    ((1024, 16000, 1 << 20, 4, 2, 3, 1, 0, 0), {"t_d": (4, 0)}),                                                  # S B C HW >= 2^40
    (GOOD, {"t_d": (1 << 31, 0)}),
])
def test_step_returns_minus_two_for_sizes_beyond_the_index_ranges(dims, kw):
    assert _call(dims, **kw) == -2                                           # every pointer is null: -2 comes before -3


def test_step_returns_minus_three_for_null_pointers():
    one = 0x1000                                                             # never dereferenced: every call returns before a launch
    need = {k: one for k in PTRS if k != "traj"}
    for missing in need:
        assert _call(GOOD, ptrs={k: v for k, v in need.items() if k != missing}) == -3, missing
    assert _call(GOOD, ptrs=need, null_grp=True) == -3 and _call(GOOD, ptrs=need, null_td=True) == -3
    assert _call(GOOD[:8] + (1,), ptrs=need) == -3                           # flags & 1 needs traj


def test_plan_and_traj_return_codes():
    import tmg_hip
    L = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                     # noqa: E731
    out = (c_i64 * 7)()
    for dims in ((0, 2, 3, 35), (4, 0, 3, 35), (4, 2, 1, 35), (4, 2, 5, 35), (4, 2, 3, 0)):
        assert L.tmg_ens_gram_plan(i64(*dims), None) == -1
    for dims in ((1025, 2, 3, 35), (4, 30000, 3, 35), (4, 2, 3, (1 << 31) - 256), (1024, 16000, 4, 1 << 20)):
        assert L.tmg_ens_gram_plan(i64(*dims), None) == -2
    assert L.tmg_ens_gram_plan(i64(4, 2, 3, 35), None) == -3 and L.tmg_ens_gram_plan(i64(4, 2, 3, 35), out) == 0
    null = ctypes.c_void_p(0)
    for dims in ((0, 2, 2), (4, 0, 2), (4, 2, 0), (4, 2, 5)):
        assert L.tmg_ens_gram_traj(null, null, null, i64(*dims), null) == -1
    assert L.tmg_ens_gram_traj(null, null, null, i64(1025, 2, 2), null) == -2
    assert L.tmg_ens_gram_traj(null, null, null, i64(4, 2, 2), null) == -3
    with pytest.raises(RuntimeError, match="tmg_ens_gram_plan failed with code -2"):
        tmg_hip.ens_gram_plan(1025, 2, 3, 35)


# ---- the plan query ------------------------------------------------------------------------------------------------------------------
WS_CAP = 1 << 24


@pytest.mark.parametrize("S", [1, 2, 14, 15, 16, 47, 62, 63, 64, 127, 128, 130, 500, 1023, 1024])
def test_plan_covers_every_pair_and_pixel_once_inside_its_cap(S):
    import tmg_hip
    for B, Cc in ((1, 2), (3, 3), (7, 4), (64, 3)):
        for HW in (1, 63, 64, 65, 255, 256, 257, 272, 528, 2900, 8192, 1 << 16, (1 << 20) + 3):
            q = tmg_hip.ens_gram_plan(S, B, Cc, HW)
            NT = (S + 1 + 63) // 64
            assert q["NT"] == NT and q["pairs"] == [(i, j) for i in range(NT) for j in range(i, NT)]     # every I <= J exactly once
            assert len(set(q["pairs"])) == NT * (NT + 1) // 2
            assert q["part"] == (256 if S + 1 <= 16 else 4096)
            P, SL, L = q["P"], q["SL"], q["L"]
            assert P >= 1 and SL % 256 == 0 and (P - 1) * SL < HW <= P * SL   # the slices [s SL, min(HW, (s + 1) SL)) cover 0..HW-1 once
            assert L == SL and L * P >= HW
            base = B * Cc * len(q["pairs"]) * q["part"]
            assert q["ws"] == base * (P + (1 if P > 1 else 0))
            assert q["ws"] <= max(WS_CAP, base), (S, B, Cc, HW, q)
            assert P == 1 or P <= -(-768 // (B * Cc * len(q["pairs"])))          # no more slices than fill the grid


def test_plan_of_the_named_cases():
    import tmg_hip
    q = tmg_hip.ens_gram_plan(*K.LONG_CASE[:3], K.LONG_CASE[3][0] * K.LONG_CASE[3][1])
    assert (q["P"], q["SL"], len(q["pairs"])) == (6, 512, 6)                  # two chunks per wave
    q = tmg_hip.ens_gram_plan(130, 1, 2, 272)
    assert (q["P"], q["SL"], q["NT"]) == (2, 256, 3)                          # 272: a little over one slice
    assert max(tmg_hip.ens_gram_plan(c[0], c[1], c[2], c[3][0] * c[3][1])["P"] for c in K.INT_TABLE) == 3


# ---- the scheme in float32 against the reference ---------------------------------------------------------------------------------------
def _plan(S, B, Cc, hw):
    import tmg_hip
    return tmg_hip.ens_gram_plan(S, B, Cc, hw[0] * hw[1])


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE)))
def test_simulation_equals_the_integer_reference(idx):
    S, B, Cc, hw, groups, t_start, _, _ = K.INT_TABLE[idx]
    xs, tgt, k = K.int_inputs(S, B, Cc, hw, 5000 + idx)
    a, a2 = K.scales(None, None, B, Cc)
    plan = _plan(S, B, Cc, hw)
    sim = K.simulate(xs, tgt, a2, groups, plan, t_start)
    ref = K.reference(xs, tgt, a, groups, t_start, integer=True)
    K.check_integer(sim, ref, k, t_start, "simulated %s" % (K.INT_TABLE[idx],))
    K.check(sim, ref, K.bounds(xs, tgt, sim["r"], a, groups, plan, ref, t_start), S, t_start, "simulated")


@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_simulation_stays_in_the_rounding_bound(idx):
    S, B, Cc, hw, groups, kind, with_u = K.REAL_TABLE[idx]
    xs, tgt = K.real_inputs(S, B, Cc, hw, kind, 6000 + idx)
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))).numpy() if with_u else None
    a, a2 = K.scales(K.SD, u, B, Cc)
    plan = _plan(S, B, Cc, hw)
    sim = K.simulate(xs, tgt, a2, groups, plan, idx % 2)
    ref = K.reference(xs, tgt, a, groups, idx % 2)
    worst = K.check(sim, ref, K.bounds(xs, tgt, sim["r"], a, groups, plan, ref, idx % 2), S, idx % 2, "simulated %s" % kind)
    print("%s %s: the simulation's worst share of the bound %.4f" % (kind, K.REAL_TABLE[idx][:4], worst))


# ---- sensitivity: every defect, put into the simulation, shows on a named case of the GPU tests' tables ------------------------------
def _defective(idx, defect, integer):
    if integer:
        S, B, Cc, hw, groups, t_start, _, _ = K.INT_TABLE[idx]
        xs, tgt, k = K.int_inputs(S, B, Cc, hw, 5000 + idx)
        a, a2 = K.scales(None, None, B, Cc)
    else:
        S, B, Cc, hw, groups, _, _ = K.REAL_TABLE[idx]
        xs, tgt = K.real_inputs(S, B, Cc, hw, K.REAL_TABLE[idx][5], 6000 + idx)
        a, a2 = K.scales(K.SD, None, B, Cc)
        t_start, k = 0, None
    plan = _plan(S, B, Cc, hw)
    sim = K.simulate(xs, tgt, a2, groups, plan, t_start, defect=defect)
    ref = K.reference(xs, tgt, a, groups, t_start, integer=integer)
    good = K.simulate(xs, tgt, a2, groups, plan, t_start)
    bnd = K.bounds(xs, tgt, good["r"], a, groups, plan, ref, t_start)
    return sim, ref, bnd, k, S, t_start


def _share(sim, ref, bnd, name):
    return float((np.abs(sim[name].astype(np.float64) - ref[name]) / np.maximum(bnd[name], 1e-300)).max())


INT_272 = 11                                                                 # (130, 1, 2, 16 x 17): 272 pixels, three macro-tiles
REAL_GAUSS = 0                                                               # (7, 3, 3, 16 x 17), members and target N(0.3, 1)
REAL_CENTRED = 7                                                             # (9, 3, 3, 5 x 13), members 0.5 N(0, 1) around the target
REAL_BIASED = 1                                                              # (7, 3, 3, 16 x 17), members 5 +- 0.1, target 0 +- 1


def test_a_dropped_pixel_run_breaks_integer_equality_and_the_bound():
    assert K.INT_TABLE[INT_272][:4] == (130, 1, 2, K.HWS[272])
    sim, ref, bnd, k, S, t_start = _defective(INT_272, "drop_run", True)
    with pytest.raises(AssertionError):
        K.check_integer(sim, ref, k, t_start, "drop_run")
    sim, ref, bnd, _, S, _ = _defective(REAL_BIASED, "drop_run", False)
    share = float((np.abs(sim["traj_steps"][0].astype(np.float64) - ref["d2"][0]) / np.maximum(bnd["beta"][0], 1e-300)).max())
    print("a dropped run of 16 pixels in 272 moves d2 by %.0f bounds" % share)
    assert share > 100


def test_the_target_counted_into_the_mean_breaks_integer_equality():
    sim, ref, bnd, k, S, t_start = _defective(3, "target_in_mean", True)
    assert not np.array_equal(sim["r"], k.reshape(sim["r"].shape))
    with pytest.raises(AssertionError):
        K.check_integer(sim, ref, k, t_start, "target_in_mean")


def test_a_lost_factor_two_moves_the_biased_case_beyond_its_bound():
    sim, ref, bnd, _, S, _ = _defective(REAL_BIASED, "no_factor_two", False)
    assert _share(sim, ref, bnd, "energy_score") > 10 and _share(sim, ref, bnd, "pair_dist_mean") > 10
    sim, ref, bnd, k, S, t_start = _defective(INT_272, "no_factor_two", True)
    with pytest.raises(AssertionError):
        K.check_integer(sim, ref, k, t_start, "no_factor_two")


def test_s_for_s_minus_one_moves_the_fair_score_beyond_its_bound():
    sim, ref, bnd, _, S, _ = _defective(REAL_BIASED, "fair_s", False)
    assert _share(sim, ref, bnd, "energy_score_fair") > 10 and _share(sim, ref, bnd, "traj_energy_score_fair") > 10
    assert _share(sim, ref, bnd, "energy_score") <= 1.0


def test_the_target_as_a_medoid_candidate_fails_the_comparison_by_value():
    assert K.REAL_TABLE[REAL_CENTRED][5] == "centred"
    sim, ref, bnd, _, S, t_start = _defective(REAL_CENTRED, "target_medoid", False)
    good = _defective(REAL_CENTRED, None, False)[0]
    assert not np.array_equal(sim["medoid"], good["medoid"])
    K.check(good, ref, bnd, S, t_start, "no defect")
    with pytest.raises(AssertionError, match="medoid"):
        K.check(sim, ref, bnd, S, t_start, "target_medoid")
