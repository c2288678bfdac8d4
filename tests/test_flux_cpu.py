"""CPU-side checks of the ensemble energy flux: the kernel entries are declared in their own header, listed apart and exported; the
signatures of the three Python layers; the launch plan (every valid pixel in one tile, every branch reached by the case table) and
the codes the entries return before any launch; every argument error without a GPU; the float32 mirror of the state against the fp64
direct sums and the reference by direct definition inside the counted bounds of tests/flux_cases.py, exact on integer data; the two
known answers (pure strain, diagonal ramp) on the references; and the sensitivity of the measure: every deliberate mistake in the
reference exceeds the bound."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import flux_cases as K

NAMES = ["tmg_ens_flux_plan", "tmg_ens_flux_accum", "tmg_ens_flux_terms"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_flux.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.FLUX_EXPORTS == NAMES
    assert "flux" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.QUANT_EXPORTS, tmg_hip.GRAM_EXPORTS,
                      tmg_hip.SFUN_EXPORTS, tmg_hip.EVENT_EXPORTS, tmg_hip.PDF_EXPORTS, tmg_hip.POD_EXPORTS, tmg_hip.PHASE_EXPORTS,
                      tmg_hip.SPOD_EXPORTS, tmg_hip.LAYOUT_EXPORTS, tmg_hip.BUDGET_EXPORTS, tmg_hip.CORR_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == tmg_hip.FLUX_ARGTYPES[name]
    assert len(tmg_hip.EXPORTS) == 89 and len(tmg_hip.RET_I64) == 4
    assert "tmg_flux.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_flux.hip"))
    assert "tmg_flux.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_flux.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_flux\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_flux.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)                                       # (the header comment says "no atomics")
    assert not re.search(r"atomic|\basm\b", code) and "TMG_LDS_OPTIN" in code
    assert src.count("#pragma clang fp contract(off)") >= 3


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredFlux).parameters
    assert list(sig) == old + ["widths", "per_member"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, None, False]
    init = inspect.signature(tmg_ops.EnsembleFlux.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid", "widths", "per_member"]
    assert init["u"].default is None and init["grid"].default == (1.0, 1.0) and init["widths"].default is None
    assert init["per_member"].default is False
    add = inspect.signature(tmg_ops.EnsembleFlux.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleFlux, tmg_ops.EnsembleFeed)
    assert tmg_ops.FLUX_WIDTHS == K.DEFAULT_WIDTHS and tmg_ops.FLUX_PLANES == K.Q == 7
    assert list(inspect.signature(tmg_hip.ens_flux_plan).parameters) == ["S", "B", "Hh", "Ww", "widths"]
    assert list(inspect.signature(tmg_hip.ens_flux_accum).parameters)[:5] == ["y", "a", "kk", "raw", "widths"]
    assert list(inspect.signature(tmg_hip.ens_flux_terms).parameters)[:3] == ["raw", "k64", "outs"]
    assert set(tmg_hip.FLUX_OUTS) == set(K.FIELD_KEYS) | {"member_flux"}
    doc = utils.modelPredFlux.__doc__
    for word in ("backscatter", "NaN", "28 L", "Not supported", "Gaussian", "one-sided", "over 33", "more than 8", "per-step", "non-finite",
                 "pressure", "boxes"):
        assert word in doc, word
    assert np.array_equal(tmg_ops.flux_factors((3, 33), 0.5, 0.25).numpy(), K.factors((3, 33), (0.5, 0.25)))


def test_plan_covers_every_valid_pixel_once_and_the_cases_reach_every_branch():
    import tmg_hip
    shapes = [(c[2], c[3]) for c in K.CASES] + [(K.MAX_CASE[2], K.MAX_CASE[3]), ((64, 128), K.DEFAULT_WIDTHS), ((5, 1 << 20), (3,)),
                                                ((36, 36), (3,)), ((37, 37), (3,)), ((17, 300), (13,)), ((17, 300), (15,))]
    for (Hh, Ww), widths in shapes:
        for S, B in ((1, 1), (1024, 3)):
            q = tmg_hip.ens_flux_plan(S, B, Hh, Ww, widths)
            r0, rmax = widths[0] // 2, widths[-1] // 2
            assert q["tile"] == (32, 32) and q["halo"] == rmax + 1
            rows = 32 + 2 * q["halo"]
            assert q["lds"] == 4 * (2 * rows * 66 + 5 * rows * 34 + 2 * 34 * 34) and q["optin"] == (q["lds"] > 65536) == (rmax >= 7)
            assert q["lds"] <= 160 * 1024
            nty, ntx = q["tiles"]
            vh, vw = Hh - 2 - 2 * r0, Ww - 2 - 2 * r0                          # the valid region of the smallest width
            assert nty * 32 >= vh > (nty - 1) * 32 and ntx * 32 >= vw > (ntx - 1) * 32     # every valid pixel in exactly one tile
            assert q["blocks"] == nty * ntx * B
            one = tmg_hip.ens_flux_plan(1, 1, Hh, Ww, widths)                   # not a function of the rows
            assert {k: v for k, v in q.items() if k != "blocks"} == {k: v for k, v in one.items() if k != "blocks"}
    # the case table reaches: LDS under and over 64 KB, one tile and several in each direction, a field narrower than a tile
    plans = [tmg_hip.ens_flux_plan(c[0], c[1], c[2][0], c[2][1], c[3]) for c in K.CASES]
    assert {p["optin"] for p in plans} == {False, True}
    assert {(p["tiles"][0] > 1, p["tiles"][1] > 1) for p in plans} >= {(False, False), (True, False), (False, True), (True, True)}
    assert any(c[2][1] < 32 for c in K.CASES) and any(len(c[3]) == 8 for c in K.CASES) and any(c[3][-1] == 33 for c in K.CASES)


def test_entries_return_their_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                    # noqa: E731
    plan = (c_i64 * 8)()
    ok, w = (4, 2, 9, 11, 2), (3, 5)
    assert lib.tmg_ens_flux_plan(i64(*ok), i64(*w), plan) == 0 and list(plan) == [32, 32, 3, 1, 1, 4 * (2 * 38 * 66 + 5 * 38 * 34 + 2 * 34 * 34), 0, 2]
    for pos, v in ((0, 0), (1, 0), (2, 4), (3, 4), (2, 0), (3, -1), (4, 0), (4, 9)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_flux_plan(i64(*d), i64(*(w + (7,) * 7)), plan) == -1, (pos, v)
    for bad in ((3, 4), (5, 3), (3, 3), (1, 3), (3, 35), (3, 9), (2, 5), (-3, 5)):       # even, decreasing, equal, < 3, > 33, over min(H, W) - 2
        assert lib.tmg_ens_flux_plan(i64(*ok), i64(*bad), plan) == -1, bad
    for pos, v in ((0, 1025), (1, 65536), (2, 1 << 31), (3, (1 << 31) - 1)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_flux_plan(i64(*d), i64(*w), plan) == -2, (pos, v)
    assert lib.tmg_ens_flux_plan(i64(*ok), i64(*w), None) == -3 and lib.tmg_ens_flux_plan(None, i64(*w), plan) == -3
    assert lib.tmg_ens_flux_plan(i64(*ok), None, plan) == -3
    # the launches: a non-null dummy pointer is never dereferenced by a call that returns a code
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = (2, 4, 2, 9, 11, 0, 0, 2)
    accum = lambda dims=good, td=(3, 0), ptr=p, ww=w: lib.tmg_ens_flux_accum(ptr, i64(*td), p, p, p, i64(*ww) if ww else None, i64(*dims), None)   # noqa: E731
    edit = lambda pos, v: tuple(v if i == pos else x for i, x in enumerate(good))   # noqa: E731
    for pos, v in ((0, 0), (1, 0), (2, 0), (3, 4), (4, 4), (5, -1), (5, 4), (6, -1), (7, 0), (7, 9)):
        assert accum(dims=edit(pos, v)) == -1, (pos, v)
    assert accum(td=(1, 0)) == -1 and accum(td=(4, 3)) == -1 and accum(td=(3, -1)) == -1 and accum(ww=(3, 9)) == -1 and accum(ww=(5, 3)) == -1
    assert accum(dims=edit(1, 1025)) == -2 and accum(dims=edit(2, 65536)) == -2 and accum(td=(1 << 31, 0)) == -2
    assert accum(ptr=None) == -3 and accum(ww=None) == -3 and lib.tmg_ens_flux_accum(p, None, p, p, p, i64(*w), i64(*good), None) == -3
    table = lambda skip=None: (ctypes.c_void_p * 14)(*[None if i == skip else p.value for i in range(14)])   # noqa: E731
    tgood = (4, 2, 9, 11, 3, 2)
    terms = lambda dims=tgood, ptr=p, outs=None, ww=w: lib.tmg_ens_flux_terms(   # noqa: E731
        ptr, p, table() if outs is None else outs, p, i64(*ww) if ww else None, i64(*dims), None)
    tedit = lambda pos, v: tuple(v if i == pos else x for i, x in enumerate(tgood))   # noqa: E731
    for pos, v in ((0, 0), (1, 0), (2, 4), (3, 4), (4, 0), (5, 0), (5, 9)):
        assert terms(dims=tedit(pos, v)) == -1, (pos, v)
    assert terms(ww=(3, 4)) == -1
    assert terms(dims=tedit(0, 1025)) == -2 and terms(dims=tedit(4, 1 << 31)) == -2
    assert terms(ptr=None) == -3 and terms(ww=None) == -3 and terms(outs=table(skip=0)) == -3 and terms(outs=table(skip=13)) == -3
    assert lib.tmg_ens_flux_terms(p, p, None, p, i64(*w), i64(*tgood), None) == -3 and lib.tmg_ens_flux_terms(p, p, table(), None, i64(*w), i64(*tgood), None) == -3


# ---- validation --------------------------------------------------------------------------------------------------------------------------
def test_flux_args_names_every_error():
    import tmg_ops as ops
    assert ops.flux_args(None, 3, 64, 128, (0.5, 0.25)) == ((3, 5, 9, 17, 33), 0.5, 0.25)
    assert ops.flux_args(None, 2, 11, 40, [1, 2]) == ((3, 5, 9), 1.0, 2.0)
    assert ops.flux_args(None, 4, 5, 5, (1.0, 1.0))[0] == (3,) and ops.flux_args(None, 3, 35, 35, (1.0, 1.0))[0] == K.DEFAULT_WIDTHS
    assert ops.flux_args([5, 7], 3, 9, 9, (1.0, 1.0))[0] == (5, 7) and ops.flux_args(np.array([3, 33]), 3, None, None, (1.0, 1.0))[0] == (3, 33)
    assert ops.flux_args(None, 3, None, None, (1.0, 1.0))[0] == K.DEFAULT_WIDTHS
    bad = [dict(C=1), dict(C=5), dict(Hh=4), dict(Ww=4), dict(grid=(1.0,)), dict(grid=(1.0, 0.0)), dict(grid=(-1.0, 1.0)),
           dict(grid=(1.0, float("inf"))), dict(grid=(float("nan"), 1.0)), dict(grid=1.0), dict(grid=(1.0, 2.0, 3.0)), dict(grid=("a", 1.0)),
           dict(grid=(True, 1.0)), dict(widths=()), dict(widths=(3, 5, 7, 9, 11, 13, 15, 17, 19)), dict(widths=(4,)), dict(widths=(1,)),
           dict(widths=(35,)), dict(widths=(5, 3)), dict(widths=(3, 3)), dict(widths=(3.0,)), dict(widths=(True,)), dict(widths=3),
           dict(widths=("3",)), dict(widths=(3, 21)), dict(widths=(19,), Hh=40, Ww=20)]
    for kw in bad:
        full = dict(widths=None, C=3, Hh=21, Ww=22, grid=(0.5, 0.25))
        full.update(kw)
        with pytest.raises(ValueError):
            ops.flux_args(**full)
    with pytest.raises(ValueError, match="min\\(H, W\\) - 2"):
        ops.flux_args((3, 21), 3, 21, 22, (1.0, 1.0))


def test_constructor_validates_before_it_touches_a_device():
    import tmg_ops as ops
    ok = dict(members=3, B=2, C=3, Hh=9, Ww=11, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3), grid=(0.5, 0.25))
    bad = [dict(members=0), dict(members=1025), dict(C=1), dict(C=5), dict(Hh=4), dict(Ww=3), dict(steps=0), dict(B=0), dict(grid=(0.0, 1.0)),
           dict(widths=(9,)), dict(widths=(4,)), dict(widths=(5, 3)), dict(out_std=torch.tensor([1.0, 0.0, 1.0])), dict(out_std=torch.ones(2)),
           dict(out_mu=torch.tensor([0.0, float("nan"), 0.0])), dict(u=torch.zeros(2, 3)), dict(u=torch.full((2, 3), float("inf")))]
    for kw in bad:
        full = dict(ok)
        full.update(kw)
        with pytest.raises(ValueError):
            ops.EnsembleFlux(**full)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.EnsembleFlux(**dict(ok, device="cpu"))


def test_model_pred_flux_validates_the_widths_and_the_grid_first():
    from types import SimpleNamespace
    from utils import utils
    good = SimpleNamespace(dx=1.0, dy=1.0)
    for args, kw in ((SimpleNamespace(dx=0.0, dy=1.0), {}), (SimpleNamespace(dx=1.0, dy=float("nan")), {}), (good, dict(widths=(4,))),
                     (good, dict(widths=(5, 3))), (good, dict(widths=(35,))), (good, dict(widths=tuple(range(3, 22, 2)))), (good, dict(widths=()))):
        with pytest.raises(ValueError):
            utils.modelPredFlux(args, None, None, None, **kw)


# ---- the mirror against the references ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_cases():
    return [K.case_refs(i) for i in range(len(K.CASES))]


def fields_of(c, raw):
    """The published fields the finalize formulas give from a state (fp64 restatement, rounded to fp32 as the device does)."""
    rows = K.restate(raw, c["T"], c["widths"], c["k64"], c["hw"])
    got = {}
    for key, (nm, ns, nt) in {"flux": ("flux_mean", "flux_std", "target_flux"), "tstd": ("flux_tstd_mean", None, "target_flux_tstd"),
                              "back": ("backscatter_mean", "backscatter_std", "target_backscatter"),
                              "sgs": ("sgs_mean", "sgs_std", "target_sgs")}.items():
        got[nm], got[nt] = rows[key][:-1].mean(0).astype(K.F32), rows[key][-1].astype(K.F32)
        if ns:
            got[ns] = rows[key][:-1].std(0).astype(K.F32)
    got["member_flux"] = np.ascontiguousarray(np.moveaxis(rows["flux"][:-1], 0, 1)).astype(K.F32)
    fc, ec = K.curves(rows, c["widths"], c["hw"])
    got["flux_curve"], got["sgs_energy_curve"] = fc.astype(K.F32), ec.astype(K.F32)
    return got


def test_mirror_agrees_with_the_references_inside_the_counted_bounds(real_cases):
    worst_raw = worst = 0.0
    for i, c in enumerate(real_cases):
        raw = c["snaps"][-1]
        assert c["snaps"][0] is None                                         # the untimed first step
        fin = raw[np.isfinite(raw)]
        assert raw.dtype == K.F32 and np.abs(fin[np.abs(fin) > 0]).min() > 1e-30        # nothing near the subnormal range
        worst_raw = max(worst_raw, K.check_raw(raw, c["ref"], "case %d" % i))
        worst = max(worst, K.check_against_definition(c, fields_of(c, raw), c["rows"], "case %d" % i))
        assert np.nanmax(c["rows"]["back"]) > 0 and np.nanmin(c["rows"]["back"]) < 1    # both signs of the flux occur
    print("mirror: worst share of the raw bound %.4f, of the field bound against the definition %.4f" % (worst_raw, worst))


def test_mirror_of_integer_data_is_exact():
    for i, (S, B, hw, widths, padded, T) in enumerate(K.CASES):
        for planes, amp, ws, Tn, keep in (("Q", 2, widths, min(T, 3), [4, 5, 6]),
                                          ("AB", 1, tuple(w for w in (3, 5) if w <= min(hw) - 2), T, [0, 1, 3, 4, 5, 6])):
            xs = K.int_inputs(S, B, hw, Tn, 300 + i, amp)
            ref = K.int_reference(xs, ws, range(1, Tn + 1), planes)
            raw = K.mirror(xs, np.ones((B, 2), K.F32), ws, K.factors(ws, K.GRID_INT).astype(K.F32), range(1, Tn + 1))[-1]
            valid = np.isfinite(raw[:, :, :, keep])
            assert valid.any() and np.array_equal(np.where(valid, raw[:, :, :, keep], 0).astype(np.int64), ref[:, :, :, keep]), (i, planes)


# ---- known answers -------------------------------------------------------------------------------------------------------------------------
def known(xs, want, what):
    """A known-answer field through the definition and through the mirror + restatement -> the worst shares."""
    a, sd, mu, u = K.kat_tables()
    off, k64, timed = K.offset(mu, u, 1), K.factors(K.KAT_WIDTHS, K.KAT_GRID), range(1, K.KAT_T + 1)
    ref = K.direct(xs, a, K.KAT_WIDTHS, k64, timed, k=K.KAT_K)
    bnd = K.definition_bounds(ref, ref, want, K.KAT_T, K.KAT_WIDTHS, k64, K.KAT_HW)
    rows = K.definition(xs, a, off, K.KAT_WIDTHS, K.KAT_GRID, timed)
    s0 = K.check_known(rows, want, bnd, K.KAT_WIDTHS, K.KAT_HW, what + ": definition")
    raw = K.mirror(xs, a, K.KAT_WIDTHS, k64.astype(K.F32), timed)[-1]
    s1 = K.check_known(K.restate(raw, K.KAT_T, K.KAT_WIDTHS, k64, K.KAT_HW), want, bnd, K.KAT_WIDTHS, K.KAT_HW, what + ": restatement of the mirror")
    return s0, s1


def test_known_answer_pure_strain():
    xs, want = K.kat_strain()
    assert (np.abs(want["flux"]) > 1e-3).all() and not want["sgs"][:, :, :, 1].any() and (want["back"] == 1).all()      # dx > dy
    print("pure strain: worst shares %.4f (definition), %.4f (restatement)" % known(xs, want, "pure strain"))


def test_known_answer_diagonal_ramp():
    xs, want = K.kat_ramp()
    assert (want["flux"] < -1e-4).all() and (want["sgs"] > 0).all()
    print("diagonal ramp: worst shares %.4f (definition), %.4f (restatement)" % known(xs, want, "diagonal ramp"))


# ---- the sensitivity of the measure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", ["dxdy", "uv", "sign", "shift", "nonorm"])
def test_a_mistake_in_the_reference_exceeds_the_bound(real_cases, mut):
    caught = 0
    for i, c in enumerate(real_cases):
        bad = K.definition(c["xs"], c["a"], c["off"], c["widths"], K.GRID, c["timed"], mut=mut)
        try:
            K.check_against_definition(c, fields_of(c, c["snaps"][-1]), bad, "case %d" % i)
        except AssertionError:
            caught += 1
    assert caught >= 1, "the bound lets %s through on every case" % mut
