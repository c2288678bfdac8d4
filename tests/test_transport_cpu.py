"""CPU-side checks of the ensemble's Lagrangian transport: the kernel entries are declared in their own header, listed apart and
exported; the signatures of the three Python layers; the launch plan and the codes the entries return before any launch; every
argument error without a GPU; the float32 mirror of tests/transport_cases.py against the int64 reference on integer data and
inside the counted bound of the fp64 scheme; the known answers on the mirror's state; and the sensitivity of the measure: every
deliberate mistake in the mirror is caught."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import transport_cases as K

NAMES = ["tmg_ens_lagr_plan", "tmg_ens_lagr_advect", "tmg_ens_lagr_store", "tmg_ens_lagr_finalize"]
c_i64 = ctypes.c_int64
F32 = np.float32


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_lagr.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.LAGR_EXPORTS == NAMES
    assert "lagr" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert tmg_hip.SOURCES[-1] == "tmg_lagr.hip" and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_lagr.hip"))
    assert "tmg_lagr.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_lagr.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_lagr\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_lagr.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)                                       # (the header comment says "no atomics")
    assert not re.search(r"atomic|\basm\b|__shared__", code)
    assert src.count("#pragma clang fp contract(off)") >= 4
    # nothing that reaches the state divides, takes a root or calls a transcendental: the advect and store kernels and their helper
    # (the one integer division splits a particle's index into its lattice row and column)
    state_code = code[code.index("lagr_inside"):code.index("struct LagrFl")].replace("const int i = p / g.Gw", "")
    assert not re.search(r"/|\b(r?sqrt|log|exp|pow|sin|cos|tan|__f)\w*\s*\(", state_code)


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredTransport).parameters
    assert list(sig) == old + ["dt", "seed_stride", "seed_origin", "substeps", "boxes", "per_member", "keep_paths"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, None, (2, 2), None, 1, (), False, False]
    init = inspect.signature(tmg_ops.EnsembleTransport.__init__).parameters
    assert list(init)[:10] == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std"]
    assert set(list(init)[10:]) == {"u", "grid", "step_dt", "seed_stride", "seed_origin", "substeps", "boxes", "per_member", "keep_paths"}
    add = inspect.signature(tmg_ops.EnsembleTransport.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleTransport, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.transport_args).parameters) == ["seed_stride", "seed_origin", "substeps", "boxes", "C", "Hh", "Ww",
                                                                          "grid", "step_dt"]
    assert list(inspect.signature(tmg_hip.ens_lagr_plan).parameters) == ["S", "B", "Hh", "Ww", "P"]
    assert list(inspect.signature(tmg_hip.ens_lagr_advect).parameters)[:7] == ["y", "a", "o", "prev", "pos", "exit_", "res"]
    assert list(inspect.signature(tmg_hip.ens_lagr_store).parameters) == ["y", "a", "o", "prev", "k", "row0"]
    assert list(inspect.signature(tmg_hip.ens_lagr_finalize).parameters)[:5] == ["pos", "exit_", "res", "fl", "outs"]
    assert set(tmg_hip.LAGR_OUTS) == set(K.FIELD_KEYS + K.RES_KEYS + K.MEMBER_KEYS)
    doc = utils.modelPredTransport.__doc__
    for word in ("Not supported", "backward-time", "RK4", "periodic", "re-seeding", "non-finite", "Heun", "T_int", "inside"):
        assert word in doc, word


def test_plan_covers_the_particles_and_the_pixels_once_and_names_the_path():
    import tmg_hip
    shapes = [K.FIELDS[c[2]] for c in K.CASES] + [K.MAX_CASE[2], ((256, 256), (2, 2)), ((256, 256), (1, 1)), ((64, 257), (3, 5))]
    for hw, stride in shapes:
        Gh, Gw = K.lattice_of(hw, stride)[:2]
        P, HW = Gh * Gw, hw[0] * hw[1]
        for S, B in ((1, 1), (1024, 3)):
            q = tmg_hip.ens_lagr_plan(S, B, hw[0], hw[1], P)
            assert q["tile"] == 256 and q["tiles"] * 256 >= P > (q["tiles"] - 1) * 256 and q["grid"] == (q["tiles"], B)
            assert q["vec"] == (hw[1] % 4 == 0) and q["store_tile"] == (1024 if q["vec"] else 256)
            assert q["store_tiles"] * q["store_tile"] >= HW > (q["store_tiles"] - 1) * q["store_tile"]
            assert q["bytes"] == (S + 1) * B * (12 * P + 8 * HW)
    paths = set()
    for c in K.CASES:
        hw, stride = K.FIELDS[c[2]]
        Gh, Gw = K.lattice_of(hw, stride)[:2]
        q = tmg_hip.ens_lagr_plan(c[0], c[1], hw[0], hw[1], Gh * Gw)
        paths.add((q["vec"], q["store_tiles"] > 1, q["tiles"] > 1))
    assert paths >= {(True, True, True), (False, True, True), (False, False, False)}


def test_entries_return_their_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                    # noqa: E731
    plan = (c_i64 * 6)()
    ok = (4, 2, 5, 7, 6)
    assert lib.tmg_ens_lagr_plan(i64(*ok), plan) == 0 and list(plan) == [256, 1, 256, 1, 0, 5 * 2 * (72 + 280)]
    for pos, v in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 0), (4, 36)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_lagr_plan(i64(*d), plan) == -1, (pos, v)
    for pos, v in ((0, 1025), (1, 65536), (2, 1 << 31), (3, (1 << 31) - 1)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_lagr_plan(i64(*d), plan) == -2, (pos, v)
    assert lib.tmg_ens_lagr_plan(i64(*ok), None) == -3 and lib.tmg_ens_lagr_plan(None, plan) == -3
    # the launches: a non-null dummy pointer is never dereferenced by a call that returns a code
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    seeds_ok = (2, 2, 1, 1, 2, 3, 1, 2, 0, 4, 0, 6) + (0,) * 12                # 5 x 7: seeds (1, 1), (1, 4), (3, 1), (3, 4); one box
    hs = (ctypes.c_float * 11)(*([0.0, 0.5, 1.0] + [0.0] * 6 + [0.5, 0.25]))

    def advect(dims=(2, 4, 2, 5, 7, 0, 0), td=(3, 0), seeds=seeds_ok, ptr=p, hsp=hs):
        return lib.tmg_ens_lagr_advect(ptr, i64(*td) if td else None, p, p, p, p, p, p, i64(*seeds) if seeds else None, hsp, i64(*dims), None)

    assert advect(dims=(0, 4, 2, 5, 7, 0, 0)) == -1 and advect(dims=(2, 0, 2, 5, 7, 0, 0)) == -1 and advect(dims=(2, 4, 2, 1, 7, 0, 0)) == -1
    assert advect(dims=(2, 4, 2, 5, 7, -1, 0)) == -1 and advect(dims=(2, 4, 2, 5, 7, 4, 0)) == -1 and advect(dims=(2, 4, 2, 5, 7, 0, -1)) == -1
    assert advect(td=(1, 0)) == -1 and advect(td=(4, 3)) == -1 and advect(td=(3, -1)) == -1
    for pos, v in ((0, 0), (0, 3), (1, 3), (2, -1), (2, 3), (3, 4), (4, 0), (5, 0), (6, 5), (6, -1), (7, 0), (7, 9), (9, 5), (8, 5), (11, 7),
                   (10, -1)):
        s = list(seeds_ok)
        s[pos] = v
        assert advect(seeds=s) == -1, (pos, v)
    assert advect(dims=(2, 1025, 2, 5, 7, 0, 0)) == -2 and advect(dims=(2, 4, 65536, 5, 7, 0, 0)) == -2 and advect(td=(1 << 31, 0)) == -2
    assert advect(ptr=None) == -3 and advect(td=None) == -3 and advect(seeds=None) == -3 and advect(hsp=None) == -3
    store = lambda dims=(2, 4, 2, 5, 7, 0), td=(3, 0), ptr=p: lib.tmg_ens_lagr_store(ptr, i64(*td), p, p, p, i64(*dims), None)   # noqa: E731
    assert store(dims=(0, 4, 2, 5, 7, 0)) == -1 and store(dims=(2, 4, 2, 5, 7, 4)) == -1 and store(td=(1, 0)) == -1
    assert store(dims=(2, 1025, 2, 5, 7, 0)) == -2 and store(ptr=None) == -3
    table = (ctypes.c_void_p * 17)(*([p.value] * 14 + [None] * 3))

    def fin(dims=(4, 2, 5, 7), fl=(0.5, 0.25, 0.1, 0.3), seeds=seeds_ok, ptr=p, outs=table):
        return lib.tmg_ens_lagr_finalize(ptr, p, p, (ctypes.c_double * 4)(*fl) if fl else None, outs, i64(*seeds), i64(*dims), None)

    assert fin(dims=(0, 2, 5, 7)) == -1 and fin(dims=(4, 2, 5, 1)) == -1 and fin(seeds=(3,) + seeds_ok[1:]) == -1
    for fl in ((0.0, 0.25, 0.1, 0.3), (0.5, -1.0, 0.1, 0.3), (0.5, 0.25, float("nan"), 0.3), (0.5, 0.25, 0.1, float("inf")), (0.5, 0.25, 0.1, 0.0)):
        assert fin(fl=fl) == -1, fl
    assert fin(dims=(1025, 2, 5, 7)) == -2 and fin(ptr=None) == -3 and fin(fl=None) == -3 and fin(outs=None) == -3
    assert fin(outs=(ctypes.c_void_p * 17)(*([p.value] * 15 + [None] * 2))) == -3     # the member arrays: all three or none
    assert fin(outs=(ctypes.c_void_p * 17)(*([p.value] * 9 + [None] * 3 + [p.value] * 2 + [None] * 3))) == -3   # one box: res_time_* needed


def test_host_constants_are_single_roundings():
    import tmg_hip
    for n in range(1, 9):
        hs = list(tmg_hip.ens_lagr_steps(n))
        assert hs[:n + 1] == [float(F32(j / n)) for j in range(n + 1)] and hs[9] == float(F32(1.0 / n)) and hs[10] == float(F32(0.5 / n))
    assert list(tmg_hip.ens_lagr_seeds((2, 3, 1, 0, 2, 2), ((0, 1, 2, 3),), 4)) == [2, 3, 1, 0, 2, 2, 1, 4, 0, 1, 2, 3] + [0] * 12


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_transport_args_names_every_error_and_fills_the_defaults():
    import tmg_ops as ops
    ok = dict(seed_stride=(2, 2), seed_origin=None, substeps=1, boxes=(), C=3, Hh=5, Ww=7, grid=(0.5, 0.25), step_dt=0.1)
    assert ops.transport_args(**ok) == ((2, 3, 1, 1, 2, 2), 1, (), 0.5, 0.25, 0.1)
    assert ops.transport_args(**dict(ok, seed_stride=(2, 3)))[0] == K.lattice_of((5, 7), (2, 3)) == (2, 2, 1, 1, 2, 3)
    assert ops.transport_args(**dict(ok, seed_stride=[1, 1], seed_origin=(0, 0)))[0] == (5, 7, 0, 0, 1, 1)
    assert ops.transport_args(**dict(ok, seed_origin=(4, 6)))[0] == (1, 1, 4, 6, 2, 2)
    assert ops.transport_args(**dict(ok, Hh=None, Ww=None, boxes=[[0, 90, 0, 5]], substeps=8))[:3] == ((None, None, 1, 1, 2, 2), 8, ((0, 90, 0, 5),))
    assert ops.transport_args(**dict(ok, boxes=((0, 4, 0, 6), (2, 2, 3, 3)), C=2))[2] == ((0, 4, 0, 6), (2, 2, 3, 3))
    for hw, stride in K.FIELDS:
        assert ops.transport_args(stride, None, 1, K.boxes_of(hw), 3, hw[0], hw[1], K.GRID, K.STEP_DT)[0] == K.lattice_of(hw, stride)
    bad = [dict(C=1), dict(C=5), dict(Hh=1), dict(Ww=1), dict(grid=(1.0,)), dict(grid=(1.0, 0.0)), dict(grid=(-1.0, 1.0)),
           dict(grid=(1.0, float("inf"))), dict(grid=1.0), dict(grid=(True, 1.0)), dict(step_dt=0.0), dict(step_dt=float("nan")),
           dict(step_dt=None), dict(step_dt=-1.0), dict(seed_stride=2), dict(seed_stride=(2,)), dict(seed_stride=(0, 1)),
           dict(seed_stride=(1.5, 1)), dict(seed_stride=(True, 1)), dict(seed_origin=(0,)), dict(seed_origin=(-1, 0)), dict(seed_origin=(0.5, 0)),
           dict(seed_origin=(5, 0)), dict(seed_origin=(0, 7)), dict(seed_origin=3), dict(substeps=0), dict(substeps=9), dict(substeps=1.0),
           dict(substeps=True), dict(boxes=((0, 1, 0, 1),) * 5), dict(boxes=((0, 1, 0),)), dict(boxes=((1, 0, 0, 1),)), dict(boxes=((0, 1, 2, 1),)),
           dict(boxes=((-1, 1, 0, 1),)), dict(boxes=((0, 5, 0, 1),)), dict(boxes=((0, 1, 0, 7),)), dict(boxes=((0.0, 1, 0, 1),)), dict(boxes=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.transport_args(**dict(ok, **kw))


def test_constructor_validates_before_it_touches_a_device():
    import tmg_ops as ops
    ok = dict(members=3, B=2, C=3, Hh=5, Ww=7, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3), grid=(0.5, 0.25),
              step_dt=0.1)
    bad = [dict(members=0), dict(members=1025), dict(C=1), dict(Hh=1), dict(steps=1), dict(B=0), dict(grid=(0.0, 1.0)), dict(step_dt=0.0),
           dict(substeps=9), dict(boxes=((0, 5, 0, 1),)), dict(seed_origin=(5, 0)), dict(out_std=torch.tensor([1.0, 0.0, 1.0])),
           dict(out_mu=torch.tensor([0.0, float("nan"), 0.0])), dict(u=torch.zeros(2, 3))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.EnsembleTransport(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.EnsembleTransport(**dict(ok, device="cpu"))


def test_model_pred_transport_raises_its_value_errors_before_any_device_work():
    from utils import utils
    args = SimpleNamespace(dx=0.5, dy=0.25)
    ok = dict(dt=0.1, tmax=4)
    for a, kw in ((args, dict(dt=None)), (args, dict(dt=0.0)), (args, dict(dt=float("nan"))), (SimpleNamespace(dx=0.0, dy=1.0), {}),
                  (args, dict(tmax=1)), (args, dict(tmax=4, stride=2, t_start=1)), (args, dict(tmax=4, t_start=3)), (args, dict(substeps=0)),
                  (args, dict(seed_stride=(0, 1))), (args, dict(boxes=((1, 0, 0, 0),))), (args, dict(seed_origin=(-1, 0)))):
        with pytest.raises(ValueError):
            utils.modelPredTransport(a, None, None, None, **dict(ok, **kw))   # model None: any device work would fail otherwise


# ---- the mirror against the int64 reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4])
def test_mirror_equals_the_int64_reference_on_integer_data(n):
    died = moved = 0
    for i, (S, B, fi, padded, _n, Tn) in enumerate(K.CASES):
        hw, stride = K.FIELDS[fi]
        lat, boxes, timed = K.lattice_of(hw, stride), K.boxes_of(hw), range(1, Tn + 1)
        vel = K.int_velocities(S, B, Tn + 1, 300 + i)
        ref = K.int_reference(vel, hw, lat, boxes, n, timed)
        ones, zeros = np.ones((B, 2), F32), np.zeros((B, 2), F32)
        got = K.mirror(K.uniform_fields(vel, hw), ones, zeros, lat, boxes, n, timed)[-1]
        assert got["pos"].dtype == F32 and np.array_equal(got["pos"].astype(np.float64), ref["pos"]), (i, n)
        assert np.array_equal(got["exit"], ref["exit"]) and np.array_equal(got["res"], ref["res"]), (i, n)
        died += int((ref["exit"] >= 0).sum())
        moved += int((ref["exit"] < 0).sum())
    assert died > 0 and moved > 0


def test_the_trapezoid_of_a_velocity_linear_in_time_is_exact():
    """Uniform velocity c t at timed step t: one advection from t - 1 to t moves by c (t - 1/2) for every substep count."""
    hw, lat = (9, 33), (1, 1, 4, 2, 1, 1)
    c = np.array([2, 0], np.int64)
    Tn = 4
    vel = np.zeros((Tn + 1, 2, 1, 2), np.int64)
    for t in range(1, Tn + 1):
        vel[t, :, 0] = c * (t - 1)
    vel[0] = 9
    for n in (1, 2, 4):
        got = K.mirror(K.uniform_fields(vel, hw), np.ones((1, 2), F32), np.zeros((1, 2), F32), lat, (), n, range(1, Tn + 1))[-1]
        want = 2 + sum(2 * (t - 1.5) for t in range(2, Tn + 1))              # 2 + 1 + 3 + 5
        assert got["pos"][0, 0, 0, 0] == want == 11.0 and got["pos"][0, 0, 1, 0] == 4.0
        assert np.array_equal(got["pos"].astype(np.float64), K.int_reference(vel, hw, lat, (), n, range(1, Tn + 1))["pos"])


# ---- the mirror against the fp64 scheme ------------------------------------------------------------------------------------------------
def test_mirror_stays_inside_the_counted_bound_of_the_fp64_scheme():
    worst = 0.0
    for i, case in enumerate(K.CASES):
        xs, a, o, lat, boxes, n, timed = K.bound_case(i)
        trace = []
        ref = K.scheme(xs, a, o, lat, boxes, n, timed, np.float64, trace=trace)[-1]
        # the property of the inputs: in the fp64 scheme every particle stays at least 2^-10 pixel inside at every substep
        assert len(trace) == 2 * n * (len(timed) - 1) and min(trace) >= K.FRAME_MARGIN, (i, min(trace))
        got = K.mirror(xs, a, o, lat, boxes, n, timed)[-1]
        assert (ref["exit"] < 0).all() and (got["exit"] < 0).all()           # equal alive sets: nobody is excluded
        G, Vm = K.slope_and_size(xs, a, o, timed)
        bound = K.position_bound(G, Vm, float(max(xs.shape[-2:])), n, len(timed) - 1)
        assert bound < K.FRAME_MARGIN
        err = float(np.abs(got["pos"].astype(np.float64) - ref["pos"]).max())
        assert err <= bound, "case %d: the mirror is off by %.3g, bound %.3g" % (i, err, bound)
        assert np.array_equal(got["res"], ref["res"]) or err > 0             # (a box edge may be crossed only inside the error)
        worst = max(worst, err / bound)
    print("mirror against the fp64 scheme: worst share of the bound %.4f" % worst)
    assert worst > 0                                                         # the two schemes do differ: the check is not vacuous


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------
def _mutation_setup():
    """A 6 x 9 field whose velocity changes in space and time; substeps 2, three advections."""
    hw, Tn, n = (6, 9), 4, 2
    Hh, Ww = hw
    yy, xx = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(Ww, dtype=np.float64), indexing="ij")
    xs = np.zeros((Tn + 1, 2, 1, 3, Hh, Ww))
    for t in range(Tn + 1):
        xs[t, :, 0, 0] = 0.125 * yy + 0.0625 * t + 0.03125 * xx
        xs[t, :, 0, 1] = 0.0625 * xx - 0.125 * t
    return xs.astype(F32), np.ones((1, 2), F32), np.zeros((1, 2), F32), K.lattice_of(hw, (1, 2)), ((0, 2, 0, 8),), n, range(1, Tn + 1)


def test_every_mutation_of_the_mirror_is_caught():
    xs, a, o, lat, boxes, n, timed = _mutation_setup()
    good = K.mirror(xs, a, o, lat, boxes, n, timed)[-1]
    ref = K.scheme(xs, a, o, lat, boxes, n, timed, np.float64)[-1]
    live = (good["exit"] < 0) & (ref["exit"] < 0)
    assert live.sum() > 10
    G, Vm = K.slope_and_size(xs, a, o, timed)
    bound = K.position_bound(G, Vm, 9.0, n, len(timed) - 1)
    keep = np.broadcast_to(live[:, :, None], good["pos"].shape)
    assert np.abs(good["pos"].astype(np.float64) - ref["pos"])[keep].max() <= bound
    for mut in ("store_first", "no_h", "fxfy"):
        bad = K.mirror(xs, a, o, lat, boxes, n, timed, mut=mut)[-1]
        both = np.broadcast_to(((bad["exit"] < 0) & live)[:, :, None], good["pos"].shape)
        assert np.abs(bad["pos"].astype(np.float64) - ref["pos"])[both].max() > 1000 * bound, mut
    # the inclusive edge: integer data that puts a particle exactly on the last column
    hw, lat1 = (4, 6), (1, 1, 2, 3, 1, 1)
    vel = np.zeros((3, 2, 1, 2), np.int64)
    vel[:, :, 0, 0] = 2                                                      # 3 -> 5 = W - 1: inside, on the frame
    args = (K.uniform_fields(vel, hw), a, o, lat1, (), 1, range(1, 3))
    ref_i = K.int_reference(vel, hw, lat1, (), 1, range(1, 3))
    assert (ref_i["exit"] == -1).all() and ref_i["pos"][0, 0, 0, 0] == 5.0
    assert np.array_equal(K.mirror(*args)[-1]["exit"], ref_i["exit"])
    assert (K.mirror(*args, mut="exclusive")[-1]["exit"] == 0).all()


# ---- known answers on the mirror's state -----------------------------------------------------------------------------------------------
def test_simple_shear_known_answer():
    xs, gs = K.kat_shear()
    Tn, (Hh, Ww) = xs.shape[0] - 1, xs.shape[-2:]
    a, o = K.tables(np.ones(3, F32), np.zeros(3, F32), None, 1, K.KAT_GRID, K.KAT_DT)
    assert np.array_equal(a, [[1.0, 2.0]]) and not o.any()
    lat = K.lattice_of((Hh, Ww), (2, 2))
    st = K.mirror(xs, a, o, lat, (), 1, range(1, Tn + 1))[-1]
    Gh, Gw = lat[:2]
    ii, jj = np.divmod(np.arange(Gh * Gw), Gw)
    x0, y0 = 1.0 + 2 * jj, 1.0 + 2 * ii
    fl = (K.KAT_GRID[0], K.KAT_GRID[1], K.KAT_DT, (Tn - 1) * K.KAT_DT)
    out, err = K.restate(st["pos"], st["exit"], st["res"], lat, fl)
    for r, g in enumerate(gs):
        alive = st["exit"][r, 0] < 0
        assert alive.any() and not alive.all()
        assert np.array_equal(st["pos"][r, 0, 0][alive], (x0 + g * y0 * (Tn - 1))[alive]) and np.array_equal(st["pos"][r, 0, 1], y0)
        q = g * (Tn - 1) * K.KAT_GRID[0] / K.KAT_GRID[1]
        want = np.log((2.0 + q * q + q * np.sqrt(q * q + 4.0)) / 2.0) / (2.0 * fl[3])
        f = (out["member_ftle"][0, r] if r < len(gs) - 1 else out["target_ftle"][0])
        e = (err["member_ftle"][0, r] if r < len(gs) - 1 else err["target_ftle"][0])
        ok = np.isfinite(f)
        assert ok.sum() >= 4 and (np.abs(f[ok] - want) <= e[ok] + 4 * K.E53 * abs(want)).all(), r


def test_steady_saddle_known_answer():
    al = 0.25
    xs, (cy, cx) = K.kat_saddle(al)
    Tn = xs.shape[0] - 1
    a, o = K.tables(np.ones(3, F32), np.zeros(3, F32), None, 1, K.KAT_GRID, K.KAT_DT)
    lat = K.lattice_of(xs.shape[-2:], (2, 2), (0, 0))
    st = K.mirror(xs, a, o, lat, (), 1, range(1, Tn + 1))[-1]
    fl = (K.KAT_GRID[0], K.KAT_GRID[1], K.KAT_DT, (Tn - 1) * K.KAT_DT)
    out, err = K.restate(st["pos"], st["exit"], st["res"], lat, fl)
    Gh, Gw = lat[:2]
    ii, jj = np.divmod(np.arange(Gh * Gw), Gw)
    gx, gy = 1 + al + al * al / 2, 1 - al + al * al / 2
    alive = st["exit"][0, 0] < 0
    assert np.array_equal(st["pos"][0, 0, 0][alive], (cx + (2 * jj - cx) * gx ** (Tn - 1))[alive])      # dyadic: exact in fp32
    assert np.array_equal(st["pos"][0, 0, 1][alive], (cy + (2 * ii - cy) * gy ** (Tn - 1))[alive])
    want = np.log(gx) / K.KAT_DT
    f, e = out["target_ftle"][0], err["target_ftle"][0]
    ok = np.isfinite(f)
    assert ok.sum() >= 4 and (np.abs(f[ok] - want) <= e[ok] + 4 * K.E53 * want).all()
    # the member equals the target: no spread, no error
    assert not np.nan_to_num(out["end_spread"]).any() and not np.nan_to_num(out["end_err_mean"]).any()
    assert np.array_equal(np.isnan(out["end_err_mean"][0]), ~alive.reshape(Gh, Gw))
