"""CPU-side checks of the ensemble structure functions and variogram score: the kernel entries are declared in their own header, listed
apart and exported; the ops / post-processing entry points exist with their signatures and the pinned old ones are unchanged; the
argument errors come in the documented order without a GPU; the C entries return their codes before any launch; the launch plan
counts every pair of every lag exactly once inside its workspace, with P and Lc consistent with its geometry; the float32
simulation of the scheme (tests/structure_cases.py) equals the integer reference and stays inside the rounding bounds; reference and
bounds catch every named defect on the GPU tests' own tables; and those tables reach every kernel instance and plan branch."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import structure_cases as K

NAMES = ["tmg_ens_sfun_plan", "tmg_ens_sfun_step"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_sfun.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.SFUN_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert len(re.findall(r'^#include "tmglow_hip_sfun\.h"$', main, re.M)) == 1 and main.count("tmglow_hip_sfun.h") == 1
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.GRAM_EXPORTS,
                      tmg_hip.RET_I64):
            assert name not in other
        assert name not in main and hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_sfun.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_sfun.hip"))
    assert callable(tmg_hip.ens_sfun_step) and callable(tmg_hip.ens_sfun_plan)
    assert "tmg_sfun" in open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read()


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredStructure).parameters
    assert list(sig) == old + ["lags", "weights"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, None, None]
    init = inspect.signature(tmg_ops.EnsembleStructure.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_std", "u", "lags", "weights", "grid"]
    assert init["u"].default is None and init["lags"].default is None and init["weights"].default is None
    assert init["grid"].default == (1.0, 1.0)
    add = inspect.signature(tmg_ops.EnsembleStructure.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert add["target"].default is inspect.Parameter.empty
    assert list(inspect.signature(tmg_ops.EnsembleStructure.finalize).parameters) == ["self"]
    assert list(inspect.signature(tmg_ops.structure_lags).parameters) == ["lags", "H", "W"]
    assert list(inspect.signature(tmg_hip.ens_sfun_plan).parameters) == ["S", "B", "C", "H", "W", "lags"]
    # the pinned ones keep their parameter lists
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert list(inspect.signature(utils.modelPredScores).parameters) == old
    assert list(inspect.signature(utils.modelPredEnergy).parameters) == old + ["groups"]
    assert list(inspect.signature(utils.modelPredQuantiles).parameters)[:9] == old
    assert list(inspect.signature(tmg_ops.EnsembleEnergy.__init__).parameters) == [
        "self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_std", "u", "groups"]
    assert list(inspect.signature(tmg_hip.ens_gram_step).parameters) == [
        "xs", "target", "a2", "groups", "r", "ws", "traj", "outf", "outi", "t", "t_before", "flags"]
    for doc in (utils.modelPredStructure.__doc__, tmg_ops.EnsembleStructure.__doc__):
        assert "vario_score" in doc and "time_flat" in doc and "sf2_std" in doc and "lag_dist" in doc


# ---- structure_lags ---------------------------------------------------------------------------------------------------------------------
def test_default_lags_are_powers_of_two_along_w_then_h():
    import tmg_ops
    assert tmg_ops.structure_lags(None, 64, 128) == ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (32, 0),
                                                     (0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (0, 32))
    assert tmg_ops.structure_lags(None, 16, 17) == ((1, 0), (2, 0), (4, 0), (8, 0), (0, 1), (0, 2), (0, 4), (0, 8))
    assert tmg_ops.structure_lags(None, 1, 5) == ((1, 0), (2, 0)) and tmg_ops.structure_lags(None, 3, 1) == ((0, 1),)
    assert tmg_ops.structure_lags([[3, -2], (0, 1)], 7, 9) == ((3, -2), (0, 1))
    for hw, lags in K.LAGS.items():
        assert tmg_ops.structure_lags(lags, *hw) == tuple(lags)
    with pytest.raises(ValueError, match="^lags"):
        tmg_ops.structure_lags(None, 1, 1)


@pytest.mark.parametrize("lags,word", [
    (((1, 0), (-1, 2)), r"lag \(-1, 2\) is not in canonical"), (((0, 0),), r"lag \(0, 0\) is not in canonical"),
    (((0, -1),), r"lag \(0, -1\) is not in canonical"), (((65, 0),), r"lag \(65, 0\) is beyond"), (((1, -65),), r"lag \(1, -65\) is beyond"),
    (((9, 0),), r"lag \(9, 0\) has no pair"), (((1, 7),), r"lag \(1, 7\) has no pair"), (((1, -7),), r"lag \(1, -7\) has no pair"),
    (((1, 0), (2, 1), (1, 0)), r"lag \(1, 0\) is listed twice"), (((1.0, 0),), r"lag \(1.0, 0\) is not a pair of integers"),
    (((True, 0),), r"lag \(True, 0\) is not a pair"), (((1, 0, 0),), r"lag \(1, 0, 0\) is not a pair"),
])
def test_a_lag_that_breaks_a_rule_is_named(lags, word):
    import tmg_ops
    with pytest.raises(ValueError, match=word):
        tmg_ops.structure_lags(lags, 7, 9)


def test_lag_rules_come_in_order_and_the_list_rules_first():
    import tmg_ops
    with pytest.raises(ValueError, match="1 to 16"):
        tmg_ops.structure_lags((), 7, 9)
    with pytest.raises(ValueError, match="1 to 16"):
        tmg_ops.structure_lags([(1, k) for k in range(-8, 9)], 70, 90)
    with pytest.raises(ValueError, match=r"pairs, got 3"):
        tmg_ops.structure_lags(3, 7, 9)
    with pytest.raises(ValueError, match="canonical"):                        # not canonical AND beyond the range AND outside the field
        tmg_ops.structure_lags(((-70, 80),), 7, 9)
    with pytest.raises(ValueError, match="beyond"):                           # beyond the range AND outside the field
        tmg_ops.structure_lags(((70, 0),), 7, 9)
    with pytest.raises(ValueError, match=r"lag \(0, -3\)"):                    # the first bad lag is the one that is named
        tmg_ops.structure_lags(((1, 0), (0, -3), (99, 0)), 7, 9)


# ---- the constructor's error order: every case is wrong in the named argument AND in every later one ---------------------------------
BAD_STD = torch.tensor([1.0, float("nan"), 1.0])
BAD_LAGS = ((0, 0),)
BAD_W = (-1.0,)
BAD_GRID = (0.0, 1.0)


def _structure(members=3, B=2, Cc=3, steps=2, out_std=None, u=None, lags=None, weights=None, grid=(1.0, 1.0), device="cpu"):
    import tmg_ops
    return tmg_ops.EnsembleStructure(members, B, Cc, 4, 5, steps, device, torch.ones(Cc) if out_std is None else out_std, u=u, lags=lags,
                                     weights=weights, grid=grid)


@pytest.mark.parametrize("Cc", [1, 5])
def test_bad_channel_count_raises_first(Cc):
    with pytest.raises(ValueError, match="channels"):
        _structure(members=0, Cc=Cc, out_std=BAD_STD, lags=BAD_LAGS, weights=BAD_W, grid=BAD_GRID)


@pytest.mark.parametrize("members", [0, 1025, -1])
def test_bad_member_count_raises_second(members):
    with pytest.raises(ValueError, match="members"):
        _structure(members=members, out_std=BAD_STD[:2], lags=BAD_LAGS, weights=BAD_W, grid=BAD_GRID)


def test_short_out_std_raises_third():
    with pytest.raises(ValueError, match="entries"):
        _structure(out_std=BAD_STD[:2], u=torch.zeros(2, 3), lags=BAD_LAGS, weights=BAD_W, grid=BAD_GRID)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_out_std_then_bad_u_raise_before_the_lags(bad):
    with pytest.raises(ValueError, match=r"^out_std must"):
        _structure(out_std=torch.tensor([1.0, bad, 2.0]), u=torch.full((2, 3), bad), lags=BAD_LAGS, weights=BAD_W, grid=BAD_GRID)
    u = torch.ones(2, 3)
    u[1, 2] = bad
    with pytest.raises(ValueError, match=r"^u must"):
        _structure(u=u, lags=BAD_LAGS, weights=BAD_W, grid=BAD_GRID)


def test_bad_lags_then_weights_then_grid_raise_before_the_device():
    with pytest.raises(ValueError, match=r"^lag \(0, 0\)"):
        _structure(lags=BAD_LAGS, weights=BAD_W, grid=BAD_GRID)
    with pytest.raises(ValueError, match=r"^lag \(5, 0\) has no pair"):       # the field is 4 x 5
        _structure(lags=((5, 0),), weights=BAD_W, grid=BAD_GRID)
    for w in (BAD_W, (1.0, 2.0), (0.0,), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError, match="^weights"):
            _structure(lags=((1, 0),), weights=w, grid=BAD_GRID)
    for g in (BAD_GRID, (1.0, float("inf")), (1.0, -2.0), (float("nan"), 1.0), 3.0, (1.0,)):
        with pytest.raises(ValueError, match="^grid"):
            _structure(lags=((1, 0),), weights=(2.0,), grid=g)


@pytest.mark.parametrize("members,lags", [(1, None), (1024, ((4, 3), (0, 1))), (5, ((1, -3),))])
def test_cpu_device_raises_last(members, lags):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _structure(members=members, u=torch.full((2, 3), 0.5), lags=lags)


def _tiny_model_and_loader():
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    return m, [(x, torch.zeros(2, 3, 3, 16, 16), torch.ones(2))]


LOG = SimpleNamespace(log=lambda *a, **k: None)


def test_model_pred_structure_bad_lags_raise_first_and_the_cpu_last():
    from utils import utils
    m, loader = _tiny_model_and_loader()
    args = SimpleNamespace(device=None, dx=0.1, dy=0.1)
    with pytest.raises(ValueError, match=r"^lag \(0, -1\)"):
        utils.modelPredStructure(args, m, loader, LOG, samples=2, tmax=2, lags=((1, 0), (0, -1)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredStructure(args, m, loader, LOG, samples=2, tmax=2)


# ---- the C entries' return codes: all of them return before any launch ---------------------------------------------------------------
PTRS = ("xs", "target", "ws", "mom", "vsum", "tmom", "tvar")
GOOD_LAGS = ((1, 0), (0, 2), (3, -2))
GOOD = (4, 2, 3, 5, 7, 3, 0, 0)                                               # S, B, C, H, W, L, t_before, flags


def _call(dims, lags=GOOD_LAGS, t_d=(3, 0), ws_floats=None, ptrs=None, null_lags=False, null_td=False):
    import tmg_hip
    p = dict.fromkeys(PTRS, None)
    p.update(ptrs or {})
    v = lambda n: ctypes.c_void_p(p[n])                                       # noqa: E731
    i64 = lambda vals: (c_i64 * max(1, len(vals)))(*vals)                     # noqa: E731
    flat = [x for l in lags for x in l] + [0] * 32                            # (room for a wrong L up to 16 lags)
    return tmg_hip.lib().tmg_ens_sfun_step(v("xs"), v("target"), None if null_td else i64(t_d), None if null_lags else i64(flat), v("ws"),
                                           c_i64((1 << 40) if ws_floats is None else ws_floats), v("mom"), v("vsum"), v("tmom"),
                                           v("tvar"), i64(dims), ctypes.c_void_p(0))


@pytest.mark.parametrize("dims,kw", [
    ((4, 2, 1, 5, 7, 3, 0, 0), {}), ((4, 2, 5, 5, 7, 3, 0, 0), {}),                                  # C outside 2..4
    ((0, 2, 3, 5, 7, 3, 0, 0), {}), ((4, 0, 3, 5, 7, 3, 0, 0), {}), ((4, 2, 3, 0, 7, 3, 0, 0), {}), ((4, 2, 3, 5, 0, 3, 0, 0), {}),
    ((4, 2, 3, 5, 7, 0, 0, 0), {}), ((4, 2, 3, 5, 7, 17, 0, 0), {}),                                 # L outside 1..16
    ((4, 2, 3, 5, 7, 3, -1, 0), {}),
    (GOOD, {"lags": ((1, 0), (0, 0), (3, -2))}), (GOOD, {"lags": ((1, 0), (-1, 2), (3, -2))}), (GOOD, {"lags": ((1, 0), (0, -2), (3, -2))}),
    (GOOD, {"lags": ((7, 0), (0, 2), (3, -2))}), (GOOD, {"lags": ((1, 0), (0, 5), (3, -2))}), (GOOD, {"lags": ((1, 0), (0, 2), (3, -5))}),
    (GOOD, {"lags": ((1, 0), (0, 2), (1, 0))}),                                                      # twice
    ((4, 2, 3, 80, 90, 3, 0, 0), {"lags": ((65, 0), (0, 2), (3, -2))}), ((4, 2, 3, 80, 90, 3, 0, 0), {"lags": ((1, 0), (0, 2), (3, -65))}),
    (GOOD, {"t_d": (2, 0)}), (GOOD, {"t_d": (4, 2)}),                                                # the target's stride / offset
])
def test_step_returns_minus_one_for_bad_dims(dims, kw):
    # also wrong in what the later codes check (S > 1024 where S is not the subject, null pointers throughout): -1 comes first
    if dims[0] == 4:
        dims = (2000,) + dims[1:]
    assert _call(dims, **kw) == -1


def test_step_returns_minus_one_for_a_workspace_under_the_plan():
    import tmg_hip
    need = tmg_hip.ens_sfun_plan(*GOOD[:5], GOOD_LAGS)["ws"]
    assert _call(GOOD, ws_floats=need - 1, ptrs=dict.fromkeys(PTRS, 0x1000)) == -1
    assert _call(GOOD, ws_floats=need) == -3                                  # enough: the null pointers are next


@pytest.mark.parametrize("dims,kw", [
    ((1025,) + GOOD[1:], {}), ((4, 30000, 3, 5, 7, 3, 0, 0), {}), ((4, 2, 3, 1 << 16, 1 << 15, 3, 0, 0), {}),
    ((4, 2, 3, 5, 1 << 31, 3, 0, 0), {}), ((1024, 16000, 4, 1 << 10, 1 << 10, 3, 0, 0), {"t_d": (4, 0)}),     # S B C H W >= 2^40
    (GOOD, {"t_d": (1 << 31, 0)}),
])
def test_step_returns_minus_two_for_sizes_beyond_the_index_ranges(dims, kw):
    assert _call(dims, **kw) == -2                                           # every pointer is null: -2 comes before -3


def test_step_returns_minus_three_for_null_pointers():
    one = 0x1000                                                             # never dereferenced: every call returns before a launch
    need = {k: one for k in PTRS if k not in ("tmom", "tvar")}
    for missing in need:
        assert _call(GOOD, ptrs={k: v for k, v in need.items() if k != missing}) == -3, missing
    assert _call(GOOD, ptrs=need, null_lags=True) == -3 and _call(GOOD, ptrs=need, null_td=True) == -3
    timed = GOOD[:7] + (1,)
    assert _call(timed, ptrs=need) == -3                                      # flags & 1 needs tmom and tvar
    assert _call(timed, ptrs=dict(need, tmom=one)) == -3 and _call(timed, ptrs=dict(need, tvar=one)) == -3


def test_plan_return_codes():
    import tmg_hip
    L = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                     # noqa: E731
    out = (c_i64 * 88)()
    lags = i64(1, 0, 0, 2, 3, -2, *([0] * 32))
    for dims in ((0, 2, 3, 5, 7, 3), (4, 0, 3, 5, 7, 3), (4, 2, 1, 5, 7, 3), (4, 2, 5, 5, 7, 3), (4, 2, 3, 0, 7, 3), (4, 2, 3, 5, 0, 3),
                 (4, 2, 3, 5, 7, 0), (4, 2, 3, 5, 7, 17), (4, 2, 3, 2, 7, 3), (4, 2, 3, 5, 3, 3), (2000, 2, 3, 5, 7, 4)):
        assert L.tmg_ens_sfun_plan(i64(*dims), lags, None) == -1, dims        # (the last: a fourth lag (0, 0), before S > 1024)
    for dims in ((1025, 2, 3, 5, 7, 3), (4, 30000, 3, 5, 7, 3), (4, 2, 3, 1 << 16, 1 << 15, 3), (1024, 16000, 4, 1 << 10, 1 << 10, 3)):
        assert L.tmg_ens_sfun_plan(i64(*dims), lags, None) == -2
    assert L.tmg_ens_sfun_plan(i64(4, 2, 3, 5, 7, 3), lags, None) == -3 and L.tmg_ens_sfun_plan(i64(4, 2, 3, 5, 7, 3), None, out) == -3
    assert L.tmg_ens_sfun_plan(i64(4, 2, 3, 5, 7, 3), lags, out) == 0
    with pytest.raises(RuntimeError, match="tmg_ens_sfun_plan failed with code -2"):
        tmg_hip.ens_sfun_plan(1025, 2, 3, 5, 7, GOOD_LAGS)
    with pytest.raises(RuntimeError, match="tmg_ens_sfun_plan failed with code -1"):
        tmg_hip.ens_sfun_plan(4, 2, 3, 5, 7, ((7, 0),))


# ---- the plan query ------------------------------------------------------------------------------------------------------------------
WS_CAP = 1 << 24


def _pairs_by_plan(q, H, W):
    """Every (p, p') the kernels count, lag by lag, walking the plan's geometry: slice s, thread t, the thread's pixels in order."""
    HW, SL, th = H * W, q["SL"], q["threads"]
    walked, longest = [], 0
    for s in range(q["P"]):
        end = min(HW, (s + 1) * SL)
        for t in range(th):
            mine = list(range(s * SL + t, end, th))
            longest = max(longest, len(mine))
            walked += mine
    p = np.array(walked, dtype=np.int64)
    i, j = p // W, p % W
    out = []
    for l in range(q["L"]):
        ok = (j < q["jmax"][l]) & (i >= q["ilo"][l]) & (i < q["ihi"][l])
        out.append(list(zip(p[ok].tolist(), (p[ok] + q["off"][l]).tolist())))
    return walked, longest, out


@pytest.mark.parametrize("hw", sorted(K.LAGS))
def test_plan_counts_every_pair_of_every_lag_once(hw):
    import tmg_hip
    H, W = hw
    lags = K.LAGS[hw]
    for S, B, Cc in ((1, 1, 2), (5, 3, 3), (130, 3, 4), (1024, 7, 4)) if H * W < 4000 else ((2, 3, 4),):
        q = tmg_hip.ens_sfun_plan(S, B, Cc, H, W, lags)
        walked, longest, pairs = _pairs_by_plan(q, H, W)
        assert sorted(walked) == list(range(H * W))                           # the slices cover every pixel once
        assert q["SL"] % 256 == 0 and (q["P"] - 1) * q["SL"] < H * W <= q["P"] * q["SL"] and q["threads"] == 256
        assert longest <= q["SL"] // 256 and q["Lc"] == q["SL"] // 256 + 9    # a thread's terms, the butterfly's 6, the waves' 3
        assert q["R"] == S + 1 and q["L"] == len(lags) and q["lags"] == [tuple(l) for l in lags]
        assert q["ws"] == B * Cc * q["P"] * len(lags) * (3 * (S + 1) + 1)
        assert q["P"] == 1 or (q["SL"] >= 512 and q["P"] <= -(-768 // (B * Cc)) and q["ws"] <= WS_CAP)
        for l, (dx, dy) in enumerate(lags):
            want = sorted((i * W + j, (i + dy) * W + j + dx) for i in range(H) for j in range(W)
                          if 0 <= i + dy < H and j + dx < W)
            assert sorted(pairs[l]) == want and len(set(pairs[l])) == len(want) == q["N"][l] == (H - abs(dy)) * (W - dx) >= 1


@pytest.mark.parametrize("S", [1, 16, 130, 1024])
def test_plan_slices_stay_inside_the_workspace_cap(S):
    import tmg_hip
    for B, Cc in ((1, 2), (3, 3), (7, 4), (64, 3)):
        for H, W in ((1, 2), (16, 16), (16, 33), (64, 128), (128, 256), (1000, 1049)):
            for L in (1, 5, 16):
                lags = [(1, 0)] + [(0, k) for k in range(1, L)] if H > L else [(k, 0) for k in range(1, 2)]
                q = tmg_hip.ens_sfun_plan(S, B, Cc, H, W, lags)
                per = B * Cc * len(lags) * (3 * (S + 1) + 1)
                assert q["ws"] == per * q["P"] and q["ws"] <= max(WS_CAP, per), (S, B, Cc, H, W, q["P"])
                assert (q["P"] - 1) * q["SL"] < H * W <= q["P"] * q["SL"] and q["Lc"] == q["SL"] // 256 + 9


def _plan(S, B, Cc, hw):
    import tmg_hip
    return tmg_hip.ens_sfun_plan(S, B, Cc, hw[0], hw[1], K.LAGS[hw])


def test_gpu_tables_reach_every_kernel_instance_and_plan_branch():
    cases = [c[1:5] for c in K.INT_TABLE + [K.LONG_CASE]]
    for tab in (cases, [c[:4] for c in K.REAL_TABLE]):
        reached = [K.plan_branch(_plan(*c)) for c in tab]
        assert {r[0] for r in reached} == K.INSTANCES
        assert {r[1] for r in reached} >= K.PLAN_BRANCHES - ({(True, 3)} if tab is not cases else set())
    assert K.plan_branch(_plan(*K.LONG_CASE[1:5])) == (4, (True, 3))
    # the table's edges: N = 1, H = 1, W = 1, dx = W - 1, dy = +-(H - 1), lag 64 both ways, a lag wider than a slice, 16 lags, one lag
    fields = {c[4] for c in K.INT_TABLE}
    assert {(1, 2), (2, 1), (1, 5), (7, 9), (8, 8), (5, 13), (16, 17), (16, 33), (50, 58), (3, 70), (66, 3)} <= fields
    assert {c[1] for c in K.INT_TABLE} >= {1, 2, 5, 16, 17, 64, 130, 1024} and {c[2] for c in K.INT_TABLE} == {1, 3}
    assert {c[3] for c in K.INT_TABLE} == {2, 3, 4} and {c[5] for c in K.INT_TABLE} == {0, 1} and {c[6] for c in K.INT_TABLE} == {0, 1, 2}
    assert (8, 0) in K.LAGS[(7, 9)] and (0, 6) in K.LAGS[(7, 9)] and (1, -6) in K.LAGS[(7, 9)] and (3, -2) in K.LAGS[(7, 9)]
    assert (64, 0) in K.LAGS[(3, 70)] and (0, 64) in K.LAGS[(66, 3)] and (2, -64) in K.LAGS[(66, 3)]
    q = _plan(2, 3, 4, (50, 58))
    assert q["P"] > 1 and max(abs(o) for o in q["off"]) > q["SL"]             # p' lies beyond the next slice
    assert len(K.LAGS[(16, 17)]) == 16 and len(K.LAGS[(8, 8)]) == 1


# ---- the scheme in float32 against the reference ---------------------------------------------------------------------------------------
def _int_case(case, idx, defect=None):
    mode, S, B, Cc, hw, t_start, _, _ = case
    steps = 2 if case is K.LONG_CASE else K.T
    t_start = min(t_start, steps - 1)
    lags = K.LAGS[hw]
    xs, tgt = K.int_inputs(mode, S, B, Cc, hw, 7000 + idx, steps)
    a, w, N = K.scales(None, None, B, Cc), [1.0] * len(lags), K.pair_counts(lags, hw)
    plan = _plan(S, B, Cc, hw)
    ref = K.reference(xs, tgt, lags, integer=True)
    phys = K.derive(ref["mom"], ref["vsum"], a, w, N, t_start, S)
    bnd = K.bounds(ref, phys, plan, a, w, N, t_start, S)
    sim = K.simulate(xs, tgt, lags, plan, a, w, N, t_start, defect=defect)
    return sim, ref, phys, bnd, mode, S, t_start


# the cases whose variogram sums are exact: binary data and a power of two of members
VARIO_EXACT = {1: True, 2: True, 4: True, 6: True, 8: True, 13: True}


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE) + 1))
def test_simulation_equals_the_integer_reference(idx):
    case = K.INT_TABLE[idx] if idx < len(K.INT_TABLE) else K.LONG_CASE
    sim, ref, phys, bnd, mode, S, t_start = _int_case(case, idx)
    vex = K.check_integer(sim, ref, mode, S, t_start, "simulated %s" % (case,))
    assert vex == (VARIO_EXACT.get(idx, False) or case is K.LONG_CASE)
    K.check(sim, ref, phys, bnd, t_start, "simulated")


def _real_case(idx, defect=None):
    S, B, Cc, hw, kind, with_u = K.REAL_TABLE[idx]
    lags = K.LAGS[hw]
    xs, tgt = K.real_inputs(S, B, Cc, hw, kind, 8000 + idx)
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))).numpy() if with_u else None
    a, w, N = K.scales(K.SD, u, B, Cc), K.weights_of(len(lags)), K.pair_counts(lags, hw)
    plan = _plan(S, B, Cc, hw)
    t_start = idx % 2
    ref = K.reference(xs, tgt, lags)
    phys = K.derive(ref["mom"], ref["vsum"], a, w, N, t_start, S)
    bnd = K.bounds(ref, phys, plan, a, w, N, t_start, S)
    sim = K.simulate(xs, tgt, lags, plan, a, w, N, t_start, defect=defect)
    return sim, ref, phys, bnd, S, t_start


@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_simulation_stays_in_the_rounding_bounds(idx):
    sim, ref, phys, bnd, S, t_start = _real_case(idx)
    worst, cnt = K.check(sim, ref, phys, bnd, t_start, "simulated %s" % (K.REAL_TABLE[idx],))
    print("%s: the simulation's worst share of the bounds %.4f; %d skewness / flatness entries compared" % (K.REAL_TABLE[idx], worst, cnt))
    assert cnt == bnd["qualifies"].size == phys["time_sf2"].size              # every entry of the table qualifies


# ---- sensitivity: every defect, put into the simulation, shows on a named case of the GPU tests' tables ------------------------------
def _share(sim, ref, phys, bnd, name):
    r = ref[name] if name in ref else phys[name]
    return float((np.abs(sim[name].astype(np.float64) - r) / np.maximum(bnd[name], 1e-300)).max())


REAL_GAUSS, REAL_SMOOTH, REAL_BIASED = 0, 1, 2
INT_SMALL, INT_BINARY = 3, 6                                                 # (5, 3, 3, 7 x 9) small, (64, 1, 3, 16 x 17) binary


@pytest.mark.parametrize("defect,names", [
    ("drop_last", ("mom", "sf2", "sf2_mean", "vsum")), ("dy_flip", ("mom", "sf3", "sf4", "vario_score")),
    ("target_in_sbar", ("vsum", "vario_lag", "time_vario_score")), ("s_minus_one", ("vsum", "vario_lag", "time_vario_lag")),
    ("abs_cube", ("mom", "sf3", "time_sf3", "time_skew")), ("n_hw", ("sf2", "sf2_std", "vario_lag", "time_sf4", "time_vario_score")),
])
def test_reference_and_bounds_catch_the_defect_on_real_data(defect, names):
    for idx in (REAL_GAUSS, REAL_SMOOTH, REAL_BIASED):
        sim, ref, phys, bnd, S, t_start = _real_case(idx, defect)
        shares = {n: _share(sim, ref, phys, bnd, n) for n in names}
        print("%s on %s: %s" % (defect, K.REAL_TABLE[idx][4], {n: "%.3g" % v for n, v in shares.items()}))
        assert min(shares.values()) > 100, shares
        with pytest.raises(AssertionError):
            K.check(sim, ref, phys, bnd, t_start, defect)


@pytest.mark.parametrize("defect", ["drop_last", "dy_flip", "abs_cube"])
def test_a_moment_defect_breaks_integer_equality(defect):
    assert K.INT_TABLE[INT_SMALL][:5] == ("small", 5, 3, 3, (7, 9))
    sim, ref, phys, bnd, mode, S, t_start = _int_case(K.INT_TABLE[INT_SMALL], INT_SMALL, defect)
    with pytest.raises(AssertionError, match="mom after step 0"):
        K.check_integer(sim, ref, mode, S, t_start, defect)


@pytest.mark.parametrize("defect", ["drop_last", "target_in_sbar", "s_minus_one"])
def test_a_variogram_defect_breaks_integer_equality(defect):
    assert K.INT_TABLE[INT_BINARY][:5] == ("binary", 64, 1, 3, (16, 17))
    sim, ref, phys, bnd, mode, S, t_start = _int_case(K.INT_TABLE[INT_BINARY], INT_BINARY, defect)
    good = _int_case(K.INT_TABLE[INT_BINARY], INT_BINARY)[0]
    assert not np.array_equal(sim["vsum"], good["vsum"])
    with pytest.raises(AssertionError):
        K.check_integer(sim, ref, mode, S, t_start, defect)


def test_n_hw_leaves_the_raw_sums_and_moves_every_physical_output():
    sim, ref, phys, bnd, mode, S, t_start = _int_case(K.INT_TABLE[INT_SMALL], INT_SMALL, "n_hw")
    K.check_integer(sim, ref, mode, S, t_start, "n_hw")                       # the raw sums do not know N_l
    with pytest.raises(AssertionError, match="sf2"):
        K.check(sim, ref, phys, bnd, t_start, "n_hw")
