"""CPU-side checks of the ensemble TKE budget: the kernel entries are declared in their own header, listed apart and exported; the
signatures of the three Python layers; the launch plan and the codes the entries return before any launch; every argument error
without a GPU; the float32 mirror of the raw state against the fp64 reference by direct definition inside the counted bounds of
tests/budget_cases.py; two known answers (production in a uniform mean shear, dissipation of a single wave) on the definition and on
the shift-formula restatement; and the sensitivity of the measure: every deliberate mistake in the reference exceeds the bound."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import budget_cases as K

NAMES = ["tmg_ens_budget_plan", "tmg_ens_budget_accum", "tmg_ens_budget_terms"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_budget.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.BUDGET_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert "budget" not in main
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.GRAM_EXPORTS,
                      tmg_hip.SFUN_EXPORTS, tmg_hip.EVENT_EXPORTS, tmg_hip.PDF_EXPORTS, tmg_hip.POD_EXPORTS, tmg_hip.PHASE_EXPORTS,
                      tmg_hip.SPOD_EXPORTS, tmg_hip.LAYOUT_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert len(tmg_hip.RET_I64) == 4
    assert "tmg_budget.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_budget.hip"))
    assert "tmg_budget.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_budget.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_budget\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_budget.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)                                       # (the header comment says "no atomics")
    assert not re.search(r"atomic|\basm\b|__shared__", code)
    assert src.count("#pragma clang fp contract(off)") >= 2


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredBudget).parameters
    assert list(sig) == old + ["nu", "rho", "per_member"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, None, 1.0, False]
    init = inspect.signature(tmg_ops.EnsembleBudget.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid", "nu", "rho", "mean",
                          "per_member"]
    assert init["u"].default is None and init["rho"].default == 1.0 and init["mean"].default is None and init["per_member"].default is False
    add = inspect.signature(tmg_ops.EnsembleBudget.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleBudget, tmg_ops.EnsembleFeed)
    assert tmg_ops.BUDGET_TERMS == K.TERMS == ("conv", "prod", "turb", "pres", "visc", "diss", "resid")
    assert list(inspect.signature(tmg_hip.ens_budget_plan).parameters) == ["S", "B", "Hh", "Ww"]
    assert list(inspect.signature(tmg_hip.ens_budget_accum).parameters)[:4] == ["y", "a", "m", "raw"]
    assert list(inspect.signature(tmg_hip.ens_budget_terms).parameters)[:3] == ["raw", "M", "fl"]
    doc = utils.modelPredBudget.__doc__
    for word in ("resid", "NaN", "14 * 4", "not an error", "Not supported", "5x5", "phase-conditioned", "non-finite"):
        assert word in doc, word


def test_plan_covers_the_pixels_once_and_names_the_path():
    import tmg_hip
    shapes = [c[2] for c in K.CASES] + [K.MAX_CASE[2], (3, 1024), (256, 256), (64, 257), (3, 3), (1025, 3), (4, 256), (3, 1 << 20)]
    for Hh, Ww in shapes:
        for S, B in ((1, 1), (1024, 3)):
            q = tmg_hip.ens_budget_plan(S, B, Hh, Ww)
            HW = Hh * Ww
            assert q["vec"] == (Ww % 4 == 0) and q["tile"] == (1024 if q["vec"] else 256) and q["ws"] == 0
            assert q["grid"] == (q["tiles"], B)
            assert q["tiles"] * q["tile"] >= HW and (q["tiles"] - 1) * q["tile"] < HW      # every pixel in exactly one block
            assert q == dict(tmg_hip.ens_budget_plan(1, B, Hh, Ww))                         # not a function of the rows
    # the case tables reach both paths and cross a block on each
    paths = {(tmg_hip.ens_budget_plan(c[0], c[1], *c[2])["vec"], tmg_hip.ens_budget_plan(c[0], c[1], *c[2])["tiles"] > 1) for c in K.CASES}
    assert paths >= {(True, True), (False, True), (False, False)}


def test_entries_return_their_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                    # noqa: E731
    plan = (c_i64 * 4)()
    ok = (4, 2, 5, 7)
    assert lib.tmg_ens_budget_plan(i64(*ok), plan) == 0 and list(plan) == [256, 1, 0, 0]
    for pos, v in ((0, 0), (1, 0), (2, 2), (3, 2), (2, 0), (3, -1)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_budget_plan(i64(*d), plan) == -1, (pos, v)
    for pos, v in ((0, 1025), (1, 65536), (2, 1 << 31), (3, (1 << 31) - 1)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_budget_plan(i64(*d), plan) == -2, (pos, v)
    assert lib.tmg_ens_budget_plan(i64(*ok), None) == -3 and lib.tmg_ens_budget_plan(None, plan) == -3
    # the launches: a non-null dummy pointer is never dereferenced by a call that returns a code
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    accum = lambda dims=(2, 4, 2, 5, 7, 0, 0), td=(3, 0), ptr=p: lib.tmg_ens_budget_accum(ptr, i64(*td), p, p, p, i64(*dims), None)   # noqa: E731
    assert accum(dims=(0, 4, 2, 5, 7, 0, 0)) == -1 and accum(dims=(2, 0, 2, 5, 7, 0, 0)) == -1 and accum(dims=(2, 4, 2, 2, 7, 0, 0)) == -1
    assert accum(dims=(2, 4, 2, 5, 7, -1, 0)) == -1 and accum(dims=(2, 4, 2, 5, 7, 4, 0)) == -1 and accum(dims=(2, 4, 2, 5, 7, 0, -1)) == -1
    assert accum(td=(2, 0)) == -1 and accum(td=(5, 3)) == -1 and accum(td=(3, -1)) == -1
    assert accum(dims=(2, 1025, 2, 5, 7, 0, 0)) == -2 and accum(dims=(2, 4, 65536, 5, 7, 0, 0)) == -2 and accum(td=(1 << 31, 0)) == -2
    assert accum(ptr=None) == -3 and lib.tmg_ens_budget_accum(p, None, p, p, p, i64(2, 4, 2, 5, 7, 0, 0), None) == -3
    f64 = lambda *v: (ctypes.c_double * 4)(*v)                               # noqa: E731
    terms = lambda dims=(4, 2, 5, 7, 3), fl=(0.5, 0.25, 0.01, 1.0), ptr=p: lib.tmg_ens_budget_terms(   # noqa: E731
        ptr, p, f64(*fl) if fl else None, p, p, p, p, p, p, None, i64(*dims), None)
    assert terms(dims=(0, 2, 5, 7, 3)) == -1 and terms(dims=(4, 2, 5, 2, 3)) == -1 and terms(dims=(4, 2, 5, 7, 0)) == -1
    for fl in ((0.0, 0.25, 0.01, 1.0), (0.5, -1.0, 0.01, 1.0), (0.5, 0.25, -0.01, 1.0), (0.5, 0.25, 0.01, 0.0),
               (float("nan"), 0.25, 0.01, 1.0), (0.5, float("inf"), 0.01, 1.0), (0.5, 0.25, float("inf"), 1.0), (0.5, 0.25, 0.01, float("nan"))):
        assert terms(fl=fl) == -1, fl
    assert terms(dims=(1025, 2, 5, 7, 3)) == -2 and terms(dims=(4, 2, 5, 7, 1 << 31)) == -2
    assert terms(ptr=None) == -3 and terms(fl=None) == -3


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_budget_args_names_every_error():
    import tmg_ops as ops
    assert ops.budget_args(3, 3, 3, (0.5, 0.25), 0, 1) == (0.5, 0.25, 0.0, 1.0)
    assert ops.budget_args(3, 64, 128, [1, 2], 0.01, 1.3) == (1.0, 2.0, 0.01, 1.3)
    bad = [dict(C=2), dict(C=4), dict(Hh=2), dict(Ww=2), dict(grid=(1.0,)), dict(grid=(1.0, 0.0)), dict(grid=(-1.0, 1.0)),
           dict(grid=(1.0, float("inf"))), dict(grid=(float("nan"), 1.0)), dict(grid=1.0), dict(grid=(1.0, 2.0, 3.0)), dict(grid=("a", 1.0)),
           dict(grid=(True, 1.0)), dict(nu=-1e-9), dict(nu=float("inf")), dict(nu=float("nan")), dict(nu=None), dict(nu=True),
           dict(rho=0.0), dict(rho=-1.0), dict(rho=float("inf")), dict(rho=float("nan")), dict(rho="1")]
    for kw in bad:
        full = dict(C=3, Hh=5, Ww=7, grid=(0.5, 0.25), nu=0.01, rho=1.0)
        full.update(kw)
        with pytest.raises(ValueError):
            ops.budget_args(**full)


def test_constructor_validates_before_it_touches_a_device():
    import tmg_ops as ops
    ok = dict(members=3, B=2, C=3, Hh=5, Ww=7, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3), grid=(0.5, 0.25), nu=0.01)
    bad = [dict(members=0), dict(members=1025), dict(C=2), dict(Hh=2), dict(Ww=1), dict(steps=0), dict(B=0), dict(grid=(0.0, 1.0)),
           dict(nu=-1.0), dict(rho=0.0), dict(out_std=torch.tensor([1.0, 0.0, 1.0])), dict(out_std=torch.ones(2)),
           dict(out_mu=torch.tensor([0.0, float("nan"), 0.0])), dict(u=torch.zeros(2, 3)), dict(u=torch.full((2, 3), float("inf"))),
           dict(mean=torch.zeros(2, 3, 5, 6)), dict(mean=torch.full((2, 3, 5, 7), float("nan"))), dict(mean=torch.zeros(2, 2, 5, 7))]
    for kw in bad:
        full = dict(ok)
        full.update(kw)
        with pytest.raises(ValueError):
            ops.EnsembleBudget(**full)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.EnsembleBudget(**dict(ok, device="cpu"))


def test_model_pred_budget_validates_nu_and_the_grid_first():
    from types import SimpleNamespace
    from utils import utils
    for args, kw in ((SimpleNamespace(dx=0.0, dy=1.0, nu=0.01), {}), (SimpleNamespace(dx=1.0, dy=1.0, nu=-1.0), {}),
                     (SimpleNamespace(dx=1.0, dy=1.0, nu=0.01), dict(nu=float("nan"))), (SimpleNamespace(dx=1.0, dy=1.0, nu=0.01), dict(rho=0.0))):
        with pytest.raises(ValueError):
            utils.modelPredBudget(args, None, None, None, **kw)


# ---- the mirror against the definition ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_cases():
    """Every case of the table once: inputs, tables, the mirror's snapshots and the definition's reference."""
    out = []
    for i, (S, B, hw, padded, T) in enumerate(K.CASES):
        xs, m, sd, mu, u = K.real_inputs(S, B, hw, T, 100 + i)
        a = K.scales(sd, u, B)
        M, fl, timed = K.phys_mean(a, m, u, mu), K.fl_of(i), range(1, T + 1)
        out.append(dict(S=S, B=B, hw=hw, T=T, xs=xs, m=m, a=a, M=M, fl=fl, timed=timed, snaps=K.mirror(xs, a, m, timed),
                        ref=K.definition(xs, a, m, timed, M, fl)))
    return out


def test_mirror_agrees_with_the_definition_inside_the_counted_bounds(real_cases):
    worst_raw = worst = 0.0
    for i, c in enumerate(real_cases):
        raw = c["snaps"][-1]
        assert c["snaps"][0] is None                                         # the untimed first step
        assert raw.dtype == K.F32 and np.abs(raw[np.abs(raw) > 0]).min() > 1e-30        # nothing near the subnormal range
        worst_raw = max(worst_raw, K.check_raw(raw, c["ref"], "case %d" % i))
        rows = K.restate(raw, c["T"], c["M"], c["fl"], c["hw"])
        mags = K.restate(c["ref"]["mags"], c["T"], c["M"], c["fl"], c["hw"], mag=True)
        got = {k: v.astype(K.F32) for k, v in K.outputs_from_rows(*rows).items()}
        worst = max(worst, K.check_fields(got, (c["ref"]["terms"], c["ref"]["stress"]), mags, c["S"], "case %d" % i, rel=K.rel_definition(c["T"])))
    print("mirror against the definition: worst share of the raw bound %.4f, of the term bound %.4f" % (worst_raw, worst))


def test_mirror_of_integer_data_is_exact():
    for i, (S, B, hw, padded, T) in enumerate(K.CASES):
        xs, m = K.int_inputs(S, B, hw, T, 300 + i)
        a = np.ones((B, 3), K.F32)
        ref = K.definition(xs, a, m, range(1, T + 1), np.zeros((B, 2) + hw), K.FL)
        raw = K.mirror(xs, a, m, range(1, T + 1))[-1]
        assert np.abs(ref["mags"]).max() < 2 ** 15 and np.array_equal(raw.astype(np.float64), ref["sums"])


# ---- known answers -------------------------------------------------------------------------------------------------------------------------
def _known(xs, m, want, what):
    """A known-answer field through the definition and through the mirror + restatement -> the worst shares."""
    a, sd, mu, u = K.kat_tables()
    M = K.phys_mean(a, m, u, mu)
    timed = range(1, K.KAT_T + 1)
    ref = K.definition(xs, a, m, timed, M, K.KAT_FL, pad=K.kat_pad(xs, m, a))
    magt, _ = K.restate(ref["mags"], K.KAT_T, M, K.KAT_FL, K.KAT_HW, mag=True)
    s0 = K.check_known(ref["terms"], want, magt, K.KAT_T, what + ": definition")
    rows, _ = K.restate(K.mirror(xs, a, m, timed)[-1], K.KAT_T, M, K.KAT_FL, K.KAT_HW)
    s1 = K.check_known(rows, want, magt, K.KAT_T, what + ": restatement of the mirror")
    return s0, s1


def test_known_answer_production_in_a_uniform_mean_shear():
    xs, m, want = K.kat_shear()
    assert (want[:, :, 1] < -0.05).all() and not want[:, :, [0, 2, 3, 4, 5]].any()
    print("mean shear: worst shares %.4f (definition), %.4f (restatement)" % _known(xs, m, want, "mean shear"))


def test_known_answer_dissipation_and_viscous_diffusion_of_a_wave():
    xs, m, want = K.kat_wave()
    inner = want[:, :, :, 1:-1, 1:-1]
    assert (inner[:, :, 5] <= 0).all() and inner[:, :, 5].min() < -1e-3 and np.abs(inner[:, :, 4]).max() > 1e-3
    print("wave: worst shares %.4f (definition), %.4f (restatement)" % _known(xs, m, want, "wave"))


# ---- the sensitivity of the measure ------------------------------------------------------------------------------------------------------
MUTATIONS = ["sign:conv", "sign:prod", "sign:turb", "sign:pres", "sign:visc", "sign:diss", "half", "dxdy", "sy", "uuv", "gx"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_a_mistake_in_the_reference_exceeds_the_bound(real_cases, mut):
    caught = 0
    for i, c in enumerate(real_cases):
        bad = K.definition(c["xs"], c["a"], c["m"], c["timed"], c["M"], c["fl"], mut=mut)
        rows = K.restate(c["snaps"][-1], c["T"], c["M"], c["fl"], c["hw"])
        mags = K.restate(c["ref"]["mags"], c["T"], c["M"], c["fl"], c["hw"], mag=True)
        got = {k: v.astype(K.F32) for k, v in K.outputs_from_rows(*rows).items()}
        try:
            K.check_fields(got, (bad["terms"], bad["stress"]), mags, c["S"], "case %d" % i, rel=K.rel_definition(c["T"]))
        except AssertionError:
            caught += 1
    assert caught >= 1, "the bound lets %s through on every case" % mut
