"""The launch-plan queries of the direct convolution kernels (tmg_conv_fwd_plan, tmg_conv_wgrad_plan, tmg_conv_rep_border_plan), the
instance coverage of the case tables of test_conv_kernels.py (conv_cases.py), and the sensitivity of its two error measures.  No
device: the queries launch nothing, dereference nothing, and plan for 256 compute units when there is no device to ask.

Sweep (SWEEP_*): strides 1 and 2, k = 1 and 3, 16 image shapes from 1 x 7 to 16 x 128 x 128 pixels, 21 input and 17 output channel
counts, aligned and misaligned operands.  The case tables must reach, by name, every instance the sweep reaches.

Compiled instances that NO shape of the sweep reaches (asserted below; recorded in LAB_NOTES.md for a later clean-up):
  conv_fwd_kernel<MT, 2, 4, 2>, <MT, 1, 4, 2>, <MT, 2, 2, 4>, <MT, 1, 2, 4> (MT = 1, 2, 4): conv_fwd_lean takes NTW = 3 or 4
  whenever WN > 1 (more than 4 output-channel tiles), so the (NTW <= 2, WN > 1) instances of TMG_FWD_CASE are never selected.
  conv_mfma_kernel and conv_wgrad_kernel: none - all 8 x 3 fallback instances and all 11 (NP, NCO) x {LEAN, non-LEAN} are reached.

Which case catches which reverted piece of the kernels (shown on the fp64 references, test_reverted_*):
  the last channel chunk of conv_fwd_kernel dropped       -> test_conv_kernels.py::test_conv_fwd[lean_chunks2_cin104-*]
  the ci_off1 term of conv_wgrad_reduce_kernel dropped    -> test_conv_kernels.py::test_conv_wgrad[wg_ci_split_off1-*]
  the corner classes of conv_rep_border_mfma_kernel       -> test_conv_kernels.py::test_conv_rep_border[bd_nt1-*] (and every bd_ case)
"""
import os
import re

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import conv_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _H():
    import tmg_hip as H
    H.lib()
    return H


def _src():
    return open(os.path.join(ROOT, "deep-turbulence_amd", "csrc", "tmg_conv.hip")).read()


# ---------------------------------------------------------------------------------------------------------------------------------
# exports and signatures
# ---------------------------------------------------------------------------------------------------------------------------------
def _header_params(name):
    txt = open(os.path.join(ROOT, "include", "tmglow_hip.h")).read() + open(os.path.join(ROOT, "include", "tmglow_hip_plan.h")).read()
    m = re.search(r"\bint\s+%s\(([^;]*?)\);" % name, txt, re.S)
    assert m, "include/tmglow_hip.h does not declare %s" % name
    out = []
    for prm in m.group(1).split(","):
        words = prm.replace("*", " * ").split()
        out.append(" ".join(words[:-1]))     # the type without the parameter's name
    return out


@pytest.mark.parametrize("plan_fn,launch_fn,extra", [
    ("tmg_conv_fwd_plan", "tmg_conv_fwd_add", ["int64_t *"]),
    ("tmg_conv_wgrad_plan", "tmg_conv_wgrad", ["int64_t", "int64_t *"]),
    ("tmg_conv_rep_border_plan", "tmg_conv_rep_border_fix", ["int64_t *"]),
    ("tmg_c1x2_fwd_plan", "tmg_c1x2_fwd", ["int64_t *"]),
    ("tmg_c1_fwd_plan", "tmg_c1_fwd_add", ["int64_t *"]),
    ("tmg_conv_wgrad_thin_grouped_plan", "tmg_conv_wgrad_thin_grouped", ["int64_t *"]),
    ("tmg_mix_wgrad_grouped_plan", "tmg_mix_wgrad_grouped", ["int64_t *"]),
])
def test_plan_exports_and_signatures(plan_fn, launch_fn, extra):
    import ctypes
    H = _H()
    assert plan_fn in H.PLAN_EXPORTS and plan_fn not in H.EXPORTS and hasattr(H.lib(), plan_fn)
    prm = _header_params(plan_fn)
    assert prm == _header_params(launch_fn) + extra, "a plan query takes its launch's arguments plus %s" % extra
    want = [ctypes.c_int64 if t == "int64_t" else ctypes.c_void_p for t in prm]
    assert all(t == "int64_t" or t.endswith("*") or t == "tmg_stream_t" for t in prm), prm
    assert H.PLAN_ARGTYPES[plan_fn] == want
    assert getattr(H.lib(), plan_fn).argtypes == want and getattr(H.lib(), plan_fn).restype is ctypes.c_int


def test_plan_header_declares_exactly_the_plan_exports():
    """tmglow_hip.h declares the operations (tmg_hip.EXPORTS, test_boundary_cpu) and includes tmglow_hip_plan.h, which declares the
    queries (tmg_hip.PLAN_EXPORTS)."""
    H = _H()
    main = open(os.path.join(ROOT, "include", "tmglow_hip.h")).read()
    assert main.count('#include "tmglow_hip_plan.h"') == 1
    plan = open(os.path.join(ROOT, "include", "tmglow_hip_plan.h")).read()
    assert sorted(re.findall(r"\bint\s+(tmg_\w+)\s*\(", plan)) == sorted(H.PLAN_EXPORTS) == sorted(H.PLAN_ARGTYPES)
    assert not set(H.PLAN_EXPORTS) & set(H.EXPORTS)


def _all_written(p):
    """The queries prefill the plan with -1 and no field's value is negative: after rc == 0 none may be left."""
    return p["rc"] == 0 and all(v >= 0 for v in p.values())


def test_a_declined_query_leaves_the_plan_unwritten():
    H = _H()
    p = H.conv_fwd_plan([_d((2, 8, 8), 0, 8)], 16, 5, 1, [_d((2, 8, 8), 4, 16)])
    assert p["rc"] == -2 and all(p[f] == -1 for f in H.FWD_PLAN_FIELDS)
    q = H.conv_wgrad_plan([_d((2, 8, 8), 0, 8)], _d((2, 8, 8), 4, 16), 5, 1)
    assert q["rc"] == -2 and all(q[f] == -1 for f in H.WGRAD_PLAN_FIELDS)


# ---------------------------------------------------------------------------------------------------------------------------------
# sweep
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = ((1, 1, 7), (3, 33, 1), (1, 3, 5), (1, 8, 8), (1, 13, 9), (2, 16, 16), (2, 5, 40), (3, 20, 24), (2, 32, 32), (2, 40, 72),
                (4, 64, 64), (1, 128, 128), (2, 128, 128), (4, 128, 128), (8, 128, 128), (16, 128, 128))
SWEEP_CIN = (4, 6, 8, 12, 16, 20, 24, 28, 32, 40, 48, 64, 72, 96, 104, 112, 128, 136, 160, 192, 256)
SWEEP_COUT = (4, 6, 8, 16, 18, 24, 32, 48, 64, 80, 96, 112, 124, 128, 192, 256, 480)
SWEEP_KS = ((3, 1), (1, 1), (3, 2), (1, 2))


def _d(shape, slot, n, mis=0):
    return CC.descr(shape, CC.seg(n, n, 0, mis), slot)


@pytest.fixture(scope="module")
def sweep():
    H = _H()
    fwd, wg, wgf, bd = set(), set(), set(), set()
    for k, s in SWEEP_KS:
        for (B, Hh, Ww) in SWEEP_SHAPES:
            Ho, Wo = CC.out_hw(Hh, Ww, s)
            for cin in SWEEP_CIN:
                for cout in SWEEP_COUT:
                    for mis in (0, 1):
                        p = H.conv_fwd_plan([_d((B, Hh, Ww), 0, cin, mis)], cout, k, s, [_d((B, Ho, Wo), 4, cout)])
                        if p["rc"] == 0:
                            assert _all_written(p), p
                            fwd.add(CC.fwd_instance(p))
                        q = H.conv_wgrad_plan([_d((B, Hh, Ww), 0, cin, mis)], _d((B, Ho, Wo), 4, cout), k, s)
                        if q["rc"] == 0:
                            assert _all_written(q), q
                            wg.add(CC.wg_instance(q))
                            wgf.add(("ksplit", q["ksplit"]))
                            wgf.add(("ppg_rebalanced", int(q["PPG"] % (k * k) != 0)))
                            wgf.add(("mpix", min(q["MPIX"], 129)))
    for (B, Hh, Ww) in SWEEP_SHAPES:
        for cdy in (8, 16, 128, 192):
            for cx in (4, 6, 12, 28, 44, 60, 76, 92, 108, 124, 128, 136):
                for mis in (0, 1):
                    p = H.conv_rep_border_plan(_d((B, Hh, Ww), 0, cdy, mis), [_d((B, Hh, Ww), 4, cx)])
                    assert _all_written(p), p
                    bd.add((p["mfma"], p["NT"], int(p["S"] > 1)))
    return dict(fwd=fwd, wg=wg, wgf=wgf, bd=bd)


def _compiled_fwd():
    src = _src()
    lean = [(0, mt) + tuple(int(v) for v in m) for m in re.findall(r"TMG_FWD_CASE\((\d), (\d), (\d)\)", src) for mt in (1, 2, 4)]
    fb = [(1, mt) + tuple(int(v) for v in m) for m in re.findall(r"TMG_CONV_CASE\((\d), (\d), (\d)\)", src) for mt in (1, 2, 4)]
    assert len(lean) == 36 and len(fb) == 24
    return set(lean + fb)


def _compiled_wg():
    inst = [tuple(int(v) for v in m) for m in re.findall(r"TMG_WG_CASE\((\d), (\d)\)", _src())]
    assert len(inst) == 11 and set(inst) == set(CC.WG_INSTANCES)
    return {i + (l,) for i in inst for l in (0, 1)}


def test_unreachable_instances_are_the_listed_ones(sweep):
    dead = _compiled_fwd() - sweep["fwd"]
    assert dead == {(k, mt, a, b, c) for (k, a, b, c) in CC.FWD_UNREACHABLE for mt in (1, 2, 4)}, sorted(dead)
    assert sweep["fwd"] <= _compiled_fwd()
    assert sweep["wg"] == _compiled_wg()
    assert sweep["bd"] == {(0, 0, 0)} | {(1, nt, sp) for nt in range(1, 9) for sp in (0, 1)}


def test_forward_cases_reach_every_reachable_instance(sweep):
    H = _H()
    got = {}
    for case in CC.FWD_CASES:
        B, p = CC.resolve_fwd(H, case)
        got.setdefault(CC.fwd_instance(p), []).append(case["name"])
        assert ("_mt%d" % p["MT"]) in case["name"] or p["MT"] == case["want"][1]
    missing = sweep["fwd"] - set(got)
    assert not missing, "no forward case runs on %s" % sorted(missing)
    by = {n: CC.resolve_fwd(H, CC.FWD_BY_NAME[n])[1] for n in ("lean_chunks2_cin104", "lean_chunks3_cin136", "lean_chunks_by_patch",
                                                               "lean_persistent", "fb_chunks_40k", "fb_chunks_64k")}
    assert by["lean_chunks2_cin104"]["nchunks"] == 2 and by["lean_chunks3_cin136"]["nchunks"] == 3
    assert by["lean_chunks_by_patch"]["nchunks"] == 2 and by["lean_chunks_by_patch"]["KCH"] < 64
    pp = by["lean_persistent"]
    tpi = pp["tiles_x"] * pp["tiles_y"]
    assert 24 * tpi > pp["grid_x"] and pp["grid_x"] % tpi != 0, "a block's tiles must lie in different images"
    assert by["fb_chunks_40k"]["lds_bytes"] <= 40000 and 40000 < by["fb_chunks_64k"]["lds_bytes"] <= 65536
    # every operand switch is on in at least two cases and off in at least two, and one case has all of them
    for sw in CC.SWITCHES:
        on = sum(sw in c["sw"] for c in CC.FWD_CASES)
        assert on >= 2 and len(CC.FWD_CASES) - on >= 2, sw
    for kern in (0, 1):
        assert any(c["sw"] == set(CC.SWITCHES) and c["want"][0] == kern for c in CC.FWD_CASES)


def test_wgrad_cases_reach_every_reachable_instance(sweep):
    H = _H()
    plans = {c["name"]: CC.wg_plan(H, c) for c in CC.WG_CASES}
    got = {CC.wg_instance(p) for p in plans.values()}
    assert got == sweep["wg"], "no weight-gradient case runs on %s" % sorted(sweep["wg"] - got)
    vals = list(plans.values())
    assert {p["ksplit"] for p in vals} == {0, 1}
    assert {min(p["MPIX"], 129) for p in vals} == {64, 128, 129} == {v for f, v in sweep["wgf"] if f == "mpix"}
    assert any(p["PPG"] % 9 for n, p in plans.items() if CC.WG_BY_NAME[n]["k"] == 3), "no case with a rebalanced PPG"
    assert any(p["gz"] > 1 for p in vals) and any(p["gx"] > 32 and p["slab"] for p in vals) and any(p["gx"] == 1 for p in vals)
    for np_ in (3, 5, 7, 8, 9):
        assert {p["slab"] for p in vals if p["NP"] == np_} == {0, 1}, "NP = %d needs a slab case and an atomics case" % np_
    for c in CC.WG_CASES:
        assert not any(CC.wino_routed(H, c, m) for m in ("int", "gauss")), "%s would be routed to the Winograd kernel by tmg_hip.conv_wgrad" % c["name"]


def test_border_cases_reach_every_reachable_instance(sweep):
    H = _H()
    got = set()
    for c in CC.BD_CASES:
        p = CC.bd_plan(H, c)
        got.add((p["mfma"], p["NT"]))
        got.add(("S>1", p["S"] > 1))
    assert got >= {(1, nt) for nt in range(1, 9)} | {(0, 0), ("S>1", True), ("S>1", False)}


def test_declined_shapes_by_plan():
    H = _H()
    x, o = _d((2, 8, 8), 0, 8), _d((2, 8, 8), 4, 16)
    assert H.conv_fwd_plan([x], 16, 5, 1, [o])["rc"] == -2
    assert H.conv_fwd_plan([x, x, x, x], 16, 3, 1, [o])["rc"] == -3
    assert H.conv_fwd_plan([x], 20, 3, 1, [o])["rc"] == -4
    assert H.conv_wgrad_plan([x], o, 5, 1)["rc"] == -2
    assert H.conv_wgrad_plan([x], o, 3, 1, use_ws=False, ngroups=2)["rc"] == -100     # grouped launches need the workspace
    assert H.conv_wgrad_plan([x], o, 3, 1, ngroups=2)["rc"] == 0
    assert H.conv_wgrad_plan([_d((2, 8, 8), 0, 8, 1)], o, 3, 1, ngroups=2)["rc"] == -100  # ... and the lean staging path


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity of the measures (fp64 references alone)
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32(t):
    return t.float()


def _check_fault(ref_g, S_g, ref_gf, ref_i, ref_if, K, what, frac):
    """Gaussian mode: the faulted reference exceeds the bound on the affected elements - the largest by 10x, and the fraction `frac` of
    them at all.  `frac` cannot be 1 for a fault that removes FEW Gaussian products from an element: the removed amount |x w| (or a
    sum of 16 of them) has a density that is positive at 0, so some affected elements move by less than any bound; for one dropped
    product of K = 936 the bound is (K + 8) u S ~ 0.03 against a median |x w| of ~0.4, which leaves well over half of the elements
    above it, and that is what is asserted there (0.5).  A fault that removes or replaces a large part of an element's terms (a
    channel chunk, a shifted quad) must show on practically every element: 0.99.  Integer mode: equality fails."""
    sh = CC.affected_shares(ref_gf, ref_g, S_g, K)
    assert sh.numel() > 0, what
    assert float(sh.max()) > 10.0 and float((sh > 1.0).double().mean()) > frac, (what, float(sh.max()), float((sh > 1).double().mean()))
    assert CC.gauss_share(_f32(ref_gf), ref_g, S_g, K) > 10.0, what
    assert not CC.bit_equal(_f32(ref_if), ref_i), what


@pytest.fixture(scope="module")
def fwd_refs():
    case = CC.FWD_BY_NAME["lean_chunks2_cin104"]
    out = {}
    for mode in ("gauss", "int"):
        d = CC.fwd_data(case, 2, mode)
        out[mode] = (d,) + CC.fwd_ref(case, d)
    return case, out


@pytest.mark.parametrize("fault", [("tap", 7, 2, 1), ("quad", 1), ("chunk", 64, 104)], ids=["tap", "quad", "last_chunk"])
def test_forward_measure_detects(fwd_refs, fault):
    case, r = fwd_refs
    (dg, ref_g, S_g), (di, ref_i, S_i) = r["gauss"], r["int"]
    assert case["gauss"] and CC.int_terms_ok(S_i, CC.gran_of(di))
    _check_fault(ref_g, S_g, CC.fwd_ref(case, dg, fault)[0], ref_i, CC.fwd_ref(case, di, fault)[0], case["K"], fault,
                 0.5 if fault[0] == "tap" else 0.99)


def test_forward_measure_accepts_the_rounded_reference(fwd_refs):
    case, r = fwd_refs
    (dg, ref_g, S_g), (di, ref_i, S_i) = r["gauss"], r["int"]
    assert CC.gauss_share(_f32(ref_g), ref_g, S_g, case["K"]) <= 1.0
    assert CC.bit_equal(_f32(ref_i), ref_i)
    nan = _f32(ref_g).clone()
    nan[0, 0, 0, 0] = float("nan")
    assert CC.gauss_share(nan, ref_g, S_g, case["K"]) == float("inf") and not CC.bit_equal(nan, ref_g)


def test_wgrad_measure_detects_a_dropped_16_pixel_unit():
    case = CC.WG_BY_NAME["wg_ppg_rebalanced"]          # K = 2048: the largest a Gaussian case may have
    assert case["K"] == CC.KMAX_GAUSS and case["gauss"]
    dg, di = CC.wg_data(case, "gauss"), CC.wg_data(case, "int")
    Wg, Sg, bg, Sbg, _ = CC.wg_ref(case, dg)
    Wi, Si, bi, Sbi, _ = CC.wg_ref(case, di)
    assert CC.int_terms_ok(Si) and CC.int_terms_ok(Sbi)
    fault = ("unit16", 1, 31, 16)                      # the last unit of the last tile
    Wgf, _, bgf, _, _ = CC.wg_ref(case, dg, fault)
    Wif, _, bif, _, _ = CC.wg_ref(case, di, fault)
    _check_fault(Wg, Sg, Wgf, Wi, Wif, case["K"], "dW", 0.5)          # 16 of 2048 products dropped: few, see _check_fault
    _check_fault(bg, Sbg, bgf, bi, bif, case["K"], "dbias", 0.5)
    assert CC.gauss_share(_f32(Wg), Wg, Sg, case["K"]) <= 1.0 and CC.bit_equal(_f32(Wi), Wi)
    assert CC.gauss_share(_f32(bg), bg, Sbg, case["K"]) <= 1.0 and CC.bit_equal(_f32(bi), bi)


def test_reverted_ci_off1_fails_wg_ci_split_off1():
    for name in ("wg_ci_split_off1", "wg_ci_split_off1_atomics"):
        case = CC.WG_BY_NAME[name]
        dg, di = CC.wg_data(case, "gauss"), CC.wg_data(case, "int")
        Wg, Sg, _, _, touched = CC.wg_ref(case, dg)
        assert touched.tolist() == [False, True, True] + [False] * 4 + [True] * 4 + [False] * 3
        assert CC.gauss_share(_f32(CC.wg_ref(case, dg, ("off1",))[0]), Wg, Sg, case["K"]) > 10.0
        assert not CC.bit_equal(_f32(CC.wg_ref(case, di, ("off1",))[0]), CC.wg_ref(case, di)[0])


def test_reverted_last_chunk_fails_lean_chunks2_cin104(fwd_refs):
    case, r = fwd_refs
    (dg, ref_g, S_g), (di, ref_i, _) = r["gauss"], r["int"]
    H = _H()
    p = CC.resolve_fwd(H, case)[1]
    c0 = (p["nchunks"] - 1) * p["KCH"]
    assert 0 < c0 < 104
    assert CC.gauss_share(_f32(CC.fwd_ref(case, dg, ("chunk", c0, 104))[0]), ref_g, S_g, case["K"]) > 10.0
    assert not CC.bit_equal(_f32(CC.fwd_ref(case, di, ("chunk", c0, 104))[0]), ref_i)


@pytest.mark.parametrize("name", ["bd_nt1", "bd_split_k", "bd_h2_w2", "bd_partial_tile"])
def test_reverted_corner_classes_fail_the_border_cases(name):
    case = CC.BD_BY_NAME[name]
    dg, di = CC.bd_data(case, "gauss"), CC.bd_data(case, "int")
    ref_g, S_g = CC.bd_ref(case, dg)
    ref_i, S_i = CC.bd_ref(case, di)
    assert CC.int_terms_ok(S_i)
    if case["gauss"]:
        assert CC.gauss_share(_f32(CC.bd_ref(case, dg, "corners")[0]), ref_g, S_g, case["K"]) > 10.0
        assert CC.gauss_share(_f32(ref_g), ref_g, S_g, case["K"]) <= 1.0
    assert not CC.bit_equal(_f32(CC.bd_ref(case, di, "corners")[0]), ref_i)
    assert CC.bit_equal(_f32(ref_i), ref_i)


def test_pack_reference_layout():
    """pack_ref against the layout comment on a hand-checked entry: mode 0 element (tap 5, channel 17, n 3), mode 1 its transpose."""
    w = torch.arange(6 * 20 * 9, dtype=torch.float64).reshape(6, 20, 3, 3)
    p0 = CC.pack_ref(w, 0).reshape(9, 2, 16, 16)
    assert float(p0[5, 1, 3, 1]) == float(w[3, 17].reshape(9)[5]) and float(p0[5, 1, 6, 1]) == 0 and float(p0[5, 1, 3, 4]) == 0
    p1 = CC.pack_ref(w, 1).reshape(9, 1, 32, 16)
    assert float(p1[5, 0, 17, 3]) == float(w[3, 17].reshape(9)[3]) and float(p1[5, 0, 20, 3]) == 0
    pm = CC.pack_ref(w, 0, cin_eff=16, cmap=(10, 4, 6)).reshape(9, 1, 16, 16)
    assert float(pm[2, 0, 1, 3]) == float(w[1, 3].reshape(9)[2]) and float(pm[2, 0, 1, 4]) == float(w[1, 10].reshape(9)[2])
    assert float(pm[2, 0, 1, 10]) == 0
