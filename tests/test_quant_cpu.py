"""CPU-side checks of the ensemble prediction intervals: the kernel entry is declared in its own header, listed apart and exported; the
ops / post-processing entry points exist with their signatures; the argument errors come in the documented order without a GPU; the C
entry returns its codes before any launch; the host level table is the fp64 statement; the numpy float32 mirror of the kernel
(tests/test_quant_gpu.py) stays inside 7 u s of np.quantile in fp64 and reproduces numpy's stable sort; and the mirror is sensitive
to the defects the GPU comparison has to catch, on the GPU tests' own inputs."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import test_quant_gpu as G

NAME = "tmg_ens_quant_step"
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_in_its_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_quant.h")).read())
    assert decl == [("int", NAME)] and tmg_hip.QUANT_EXPORTS == [NAME]
    for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.RET_I64):
        assert NAME not in other
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert len(re.findall(r'^#include "tmglow_hip_quant\.h"$', main, re.M)) == 1 and main.count("tmglow_hip_quant.h") == 1
    assert NAME not in main
    lib = ctypes.CDLL(tmg_hip.build())
    assert hasattr(lib, NAME)
    assert tmg_hip.lib().tmg_ens_quant_step.restype is ctypes.c_int
    assert "tmg_quant.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_quant.hip"))
    assert callable(tmg_hip.ens_quant_step)


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredQuantiles).parameters
    assert list(sig) == old + ["levels", "exceed"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, (0.05, 0.5, 0.95), ()]
    init = inspect.signature(tmg_ops.EnsembleQuantiles.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "levels", "exceed"]
    assert init["u"].default is None and init["levels"].default == (0.05, 0.5, 0.95) and init["exceed"].default == ()
    add = inspect.signature(tmg_ops.EnsembleQuantiles.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["target"].default is None and add["time"].default is True
    assert list(inspect.signature(tmg_ops.EnsembleQuantiles.finalize).parameters) == ["self"]
    assert list(inspect.signature(tmg_ops.quantile_levels).parameters) == ["S", "levels"]
    assert list(inspect.signature(tmg_hip.ens_quant_step).parameters) == [
        "xs", "target", "u", "out_mu", "out_std", "lo", "hi", "w", "thr", "ex", "quant", "exceed", "taggs", "ostrides", "t_before", "flags"]
    # the pinned ones keep their parameter lists
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert list(inspect.signature(utils.modelPredScores).parameters) == old


# ---- the constructor's error order: every case is wrong in the named argument AND in every later one ---------------------------------
BAD_STD = torch.tensor([1.0, float("nan"), 1.0])
BAD_LEVELS = (0.5, 1.5)
BAD_EXCEED = ((7, 0.0, "<"),)


def _quant(members=3, B=2, Cc=3, steps=2, out_mu=None, out_std=None, u=None, levels=(0.05, 0.5, 0.95), exceed=(), device="cpu"):
    import tmg_ops
    return tmg_ops.EnsembleQuantiles(members, B, Cc, 4, 5, steps, device, torch.zeros(Cc) if out_mu is None else out_mu,
                                     torch.ones(Cc) if out_std is None else out_std, u=u, levels=levels, exceed=exceed)


@pytest.mark.parametrize("Cc", [1, 5])
def test_bad_channel_count_raises_first(Cc):
    with pytest.raises(ValueError, match="channels"):
        _quant(members=0, Cc=Cc, steps=0, out_std=BAD_STD, levels=BAD_LEVELS, exceed=BAD_EXCEED)


def test_bad_steps_raise_second():
    with pytest.raises(ValueError, match="steps"):
        _quant(members=0, steps=0, out_std=BAD_STD[:2], levels=BAD_LEVELS, exceed=BAD_EXCEED)


@pytest.mark.parametrize("levels", [(), (0.5, 1.5), (-0.1,), (float("nan"),), (float("inf"),), tuple([0.5] * 9)])
def test_bad_levels_raise_third(levels):
    with pytest.raises(ValueError, match="^levels"):
        _quant(members=0, out_std=BAD_STD[:2], levels=levels, exceed=BAD_EXCEED)


@pytest.mark.parametrize("exceed", [((7, 0.0, "<"),), ((-1, 0.0, "<"),), ((0, float("nan"), "<"),), ((0, float("inf"), ">"),),
                                    ((0, 0.0, ">="),), ((0, 0.0),), ((0.0, 0.0, "<"),), tuple([(0, 0.0, "<")] * 5)])
def test_bad_exceed_entries_raise_fourth(exceed):
    with pytest.raises(ValueError, match="^exceed"):
        _quant(members=0, out_std=BAD_STD[:2], exceed=exceed)


@pytest.mark.parametrize("members", [0, 1025, -1])
def test_bad_member_count_raises_fifth(members):
    with pytest.raises(ValueError, match="members"):
        _quant(members=members, out_std=BAD_STD[:2], exceed=((2, 0.0, "<"),))


def test_short_out_std_or_out_mu_raises_sixth():
    with pytest.raises(ValueError, match="entries"):
        _quant(out_std=BAD_STD[:2])
    with pytest.raises(ValueError, match="entries"):
        _quant(out_mu=torch.zeros(2), out_std=BAD_STD)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_bad_out_std_out_mu_or_u_raises_before_the_device(bad):
    sd = torch.tensor([1.0, bad, 2.0])
    with pytest.raises(ValueError, match=r"^out_std must"):
        _quant(out_std=sd, u=torch.full((2, 3), bad))
    if not np.isfinite(bad):
        with pytest.raises(ValueError, match=r"^out_mu must"):
            _quant(out_mu=torch.tensor([0.0, bad, 0.0]), u=torch.full((2, 3), bad))
    u = torch.ones(2, 3)
    u[1, 2] = bad
    with pytest.raises(ValueError, match=r"^u must"):
        _quant(u=u)


@pytest.mark.parametrize("members", [1, 1024])
def test_cpu_device_raises_last(members):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _quant(members=members, u=torch.full((2, 3), 0.5), levels=G.LEVELS, exceed=((0, 0.0, "<"), (2, 1.5, ">")))


def _tiny_model_and_loader():
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    return m, [(x, torch.zeros(2, 3, 3, 16, 16), torch.ones(2))]


LOG = SimpleNamespace(log=lambda *a, **k: None)


def test_model_pred_quantiles_bad_levels_raise_first():
    from utils import utils
    m, loader = _tiny_model_and_loader()
    with pytest.raises(ValueError, match="^levels"):
        utils.modelPredQuantiles(SimpleNamespace(device=None), m, loader, LOG, samples=2, tmax=2, levels=BAD_LEVELS, exceed=BAD_EXCEED)


def test_model_pred_quantiles_bad_exceed_raises_second():
    from utils import utils
    m, loader = _tiny_model_and_loader()
    with pytest.raises(ValueError, match="^exceed"):
        utils.modelPredQuantiles(SimpleNamespace(device=None), m, loader, LOG, samples=2, tmax=2, exceed=((3, 0.0, "<"),))


def test_model_pred_quantiles_on_cpu_raises_last():
    from utils import utils
    m, loader = _tiny_model_and_loader()
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredQuantiles(SimpleNamespace(device=None), m, loader, LOG, samples=2, tmax=2, exceed=((0, 0.0, "<"),))


# ---- the C entry's return codes: all of them return before any launch ----------------------------------------------------------------
def _call(dims, lohi=(0, 1), w=(0.5,), ex=(), o_d=None, t_d=(3, 0), ptrs=None):
    """tmg_ens_quant_step with dims = (S, B, HW, C, Q, K, t_before, flags); ptrs: the 11 device-side pointers in the entry's order
    (xs, target, u, out_mu, out_std, thr, quant, exceed, tquant, tbelow, texceed), null by default."""
    import tmg_hip
    S, B, HW, Cc, Q, K = dims[:6]
    p = dict.fromkeys(("xs", "target", "u", "out_mu", "out_std", "thr", "quant", "exceed", "tquant", "tbelow", "texceed"), None)
    p.update(ptrs or {})
    v = lambda n: ctypes.c_void_p(p[n])                                       # noqa: E731
    o_d = (Q * Cc * HW, K * HW) if o_d is None else o_d
    i64 = lambda vals: (c_i64 * max(1, len(vals)))(*vals)                     # noqa: E731
    return tmg_hip.lib().tmg_ens_quant_step(v("xs"), v("target"), i64(t_d), v("u"), v("out_mu"), v("out_std"), i64(lohi),
                                            (ctypes.c_float * max(1, len(w)))(*w), v("thr"), i64(ex), v("quant"), v("exceed"),
                                            v("tquant"), v("tbelow"), v("texceed"), i64(o_d), i64(dims), ctypes.c_void_p(0))


GOOD = (4, 2, 35, 3, 1, 0, 0, 0)


@pytest.mark.parametrize("dims,kw", [
    ((4, 2, 35, 1, 1, 0, 0, 0), {}), ((4, 2, 35, 5, 1, 0, 0, 0), {}),                              # C outside 2..4
    ((4, 2, 35, 3, 0, 0, 0, 0), {}), ((4, 2, 35, 3, 9, 0, 0, 0), {"lohi": (0,) * 18, "w": (0.0,) * 9}),   # Q outside 1..8
    ((4, 2, 35, 3, 1, 5, 0, 0), {"ex": (0, 1) * 5}), ((4, 2, 35, 3, 1, -1, 0, 0), {}),             # K outside 0..4
    ((0, 2, 35, 3, 1, 0, 0, 0), {}), ((4, 0, 35, 3, 1, 0, 0, 0), {}), ((4, 2, 0, 3, 1, 0, 0, 0), {}),
    ((4, 2, 35, 3, 1, 0, -1, 0), {}),
    (GOOD, {"lohi": (0, 4)}), (GOOD, {"lohi": (-1, 0)}),                                            # lo / hi outside 0..S-1
    ((4, 2, 35, 3, 1, 1, 0, 0), {"ex": (3, 1)}), ((4, 2, 35, 3, 1, 1, 0, 0), {"ex": (-1, 0)}),     # a channel outside 0..C-1
    ((4, 2, 35, 3, 1, 1, 0, 0), {"ex": (0, 2)}),                                                    # a direction outside 0..1
    (GOOD, {"o_d": (3 * 35 - 1, 0)}), ((4, 2, 35, 3, 1, 2, 0, 0), {"ex": (0, 1, 2, 0), "o_d": (3 * 35, 2 * 35 - 1)}),   # strides too small
    ((4, 2, 35, 3, 1, 0, 0, 2), {"t_d": (2, 0)}), ((4, 2, 35, 3, 1, 0, 0, 2), {"t_d": (4, 2)}),    # the target's stride / offset
])
def test_entry_returns_minus_one_for_bad_dims(dims, kw):
    # also wrong in what the later codes check (S > 1024 where S is not the subject, null pointers throughout): -1 comes first
    if dims[0] == 4 and "lohi" not in kw:
        dims = (2000,) + dims[1:]
    assert _call(dims, **kw) == -1


@pytest.mark.parametrize("dims,kw", [
    ((1025, 2, 35, 3, 1, 0, 0, 0), {}), ((4, 65536, 35, 3, 1, 0, 0, 0), {}), ((4, 2, (1 << 31) - 256, 3, 1, 0, 0, 0), {}),
    ((1024, 65535, 1 << 20, 4, 1, 0, 0, 0), {}),                                                    # S B C HW >= 2^40
    ((4, 2, 35, 3, 1, 0, 0, 0), {"o_d": (1 << 39, 0)}),                                             # B o_d[0] >= 2^40
    ((4, 2, 35, 3, 1, 0, 0, 2), {"t_d": (1 << 31, 0)}),
])
def test_entry_returns_minus_two_for_sizes_beyond_the_index_ranges(dims, kw):
    assert _call(dims, **kw) == -2                                           # every pointer is null: -2 comes before -3


def test_entry_returns_minus_three_for_null_pointers():
    one = 0x1000                                                             # never dereferenced: every call returns before a launch
    need = {"xs": one, "out_mu": one, "out_std": one, "quant": one}
    for missing in need:
        assert _call(GOOD, ptrs={k: v for k, v in need.items() if k != missing}) == -3, missing
    # flags & 2 needs the target; K > 0 thr and exceed; flags & 1 tquant, with a target tbelow, with K > 0 texceed
    assert _call((4, 2, 35, 3, 1, 0, 0, 2), ptrs=need) == -3
    k1 = dict(dims=(4, 2, 35, 3, 1, 1, 0, 0), ex=(0, 1))
    assert _call(ptrs=dict(need, thr=one), **k1) == -3 and _call(ptrs=dict(need, exceed=one), **k1) == -3
    assert _call((4, 2, 35, 3, 1, 0, 0, 1), ptrs=need) == -3
    assert _call((4, 2, 35, 3, 1, 0, 0, 3), ptrs=dict(need, target=one, tquant=one)) == -3
    assert _call((4, 2, 35, 3, 1, 1, 0, 1), ex=(0, 1), ptrs=dict(need, thr=one, exceed=one, tquant=one)) == -3


# ---- the level table ---------------------------------------------------------------------------------------------------------------
def test_level_table_is_the_fp64_statement():
    import tmg_ops
    for S in (1, 2, 5, 8, 9, 1024):
        lo, hi, w = tmg_ops.quantile_levels(S, G.LEVELS)
        rlo, rhi, rw = G.level_table(S, G.LEVELS)
        assert lo.dtype == np.int64 and hi.dtype == np.int64 and w.dtype == np.float32
        assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi) and np.array_equal(w, rw)
        assert bool(((0 <= lo) & (lo <= hi) & (hi <= S - 1) & (0 <= w) & (w < 1)).all())
    q = lambda S, v: tuple(float(a[0]) for a in tmg_ops.quantile_levels(S, (v,)))   # noqa: E731
    assert q(9, 0.0) == (0, 1, 0.0) and q(9, 1.0) == (8, 8, 0.0)             # the ends; q = 1: lo = hi = S - 1, w = 0
    assert q(9, 0.5) == (4, 5, 0.0) and q(8, 0.5) == (3, 4, 0.5)             # the median at odd and even S
    assert q(1, 0.0) == q(1, 0.3) == q(1, 1.0) == (0, 0, 0.0)                # one member
    assert q(5, 0.25) == (1, 2, 0.0) and q(9, 0.75) == (6, 7, 0.0)           # a level whose h is an integer
    assert q(5, 0.05) == (0, 1, float(np.float32(0.05 * 4)))
    with pytest.raises(ValueError):
        tmg_ops.quantile_levels(5, (1.5,))


# ---- the fp32 mirror against np.quantile in fp64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7, 8, 9, 17, 33, 64, 130, 1024])
def test_fp32_mirror_stays_in_seven_roundings_of_np_quantile(S):
    g = np.random.default_rng(100 + S)
    n = 4000 if S <= 130 else 300
    x = (g.standard_normal((S, n)) + 0.3).astype(np.float32)
    rank = G.ranks(x)
    assert np.array_equal(np.sort(rank, axis=0), np.broadcast_to(np.arange(S).reshape(S, 1), rank.shape))    # a permutation
    srt = G.order_stats(x, rank)
    assert np.array_equal(srt, np.sort(x, axis=0))
    lo, hi, w = G.level_table(S, G.LEVELS)
    a, b = srt[lo], srt[hi]
    q32 = a + (w.reshape(-1, 1) * (b - a).astype(np.float32)).astype(np.float32)
    assert q32.dtype == np.float32
    q64 = np.quantile(x.astype(np.float64), G.LEVELS, axis=0, method="linear")
    bnd = 7 * G.U24 * np.abs(x.astype(np.float64)).max(0)
    share = float((np.abs(q32.astype(np.float64) - q64) / bnd).max())
    print("S=%d: the mirror's worst share of 7 u s: %.3f" % (S, share))
    assert share <= 1.0


def test_rank_count_reproduces_numpys_stable_sort_on_ties():
    xs, _ = G.tie_inputs()
    x = np.ascontiguousarray(np.moveaxis(xs, 1, 0))
    rank = G.ranks(x)
    order = np.argsort(x, axis=0, kind="stable")                             # order[r] = the member of rank r
    inv = np.empty_like(order)
    np.put_along_axis(inv, order, np.broadcast_to(np.arange(x.shape[0]).reshape(-1, 1, 1, 1, 1, 1), x.shape), axis=0)
    assert np.array_equal(rank, inv)
    assert np.array_equal(G.order_stats(x, rank), np.sort(x, axis=0))


# ---- sensitivity: every defect, put into the mirror, shows on a named case of the GPU tests' inputs ----------------------------------
def _moved(ref, bad, xs):
    """The largest move of quant in units of the 7 u s bound (NaN in the defective result: infinite)."""
    s = np.abs(xs.astype(np.float64)).max(1).transpose(1, 0, 2, 3, 4)[:, :, None]
    d = np.abs(bad["quant"].astype(np.float64) - ref["quant"].astype(np.float64)) / np.maximum(7 * G.U24 * s, 1e-300)
    return float(np.where(np.isnan(d), np.inf, d).max())


SWEEP_CASE = G.SWEEP.index((9, 3, 3, (16, 17)))


def test_a_rank_off_by_one_moves_the_sweep():
    xs, tgt = G.inputs(SWEEP_CASE)
    ex = G.thresholds(3)
    assert _moved(G.mirror(xs, tgt, G.LEVELS, ex, 0), G.mirror(xs, tgt, G.LEVELS, ex, 0, defect="rank_off"), xs) > 10


def test_swapped_lo_and_hi_move_the_sweep():
    xs, tgt = G.inputs(SWEEP_CASE)
    ex = G.thresholds(3)
    assert _moved(G.mirror(xs, tgt, G.LEVELS, ex, 0), G.mirror(xs, tgt, G.LEVELS, ex, 0, defect="swap"), xs) > 10


def test_unbroken_ties_leave_a_slot_nan_on_the_tie_case():
    xs, tgt = G.tie_inputs()
    bad = G.mirror(xs, tgt, G.LEVELS, G.TIE_THRESHOLDS, 1, defect="no_tiebreak")
    assert np.isnan(bad["quant"]).any()
    assert _moved(G.mirror(xs, tgt, G.LEVELS, G.TIE_THRESHOLDS, 1), bad, xs) > 10


def test_a_loose_below_count_changes_the_tie_case():
    xs, tgt = G.tie_inputs()
    ref, bad = (G.mirror(xs, tgt, G.LEVELS, G.TIE_THRESHOLDS, 1, defect=d) for d in (None, "below_le"))
    assert np.array_equal(ref["quant"], bad["quant"]) and not np.array_equal(ref["time_below_count"], bad["time_below_count"])


def test_a_loose_exceedance_count_changes_the_tie_case():
    xs, tgt = G.tie_inputs()
    ref, bad = (G.mirror(xs, tgt, G.LEVELS, G.TIE_THRESHOLDS, 1, defect=d) for d in (None, "exceed_ge"))
    assert not np.array_equal(ref["time_exceed_count"], bad["time_exceed_count"])
    assert not np.array_equal(ref["exceed_prob"], bad["exceed_prob"])
