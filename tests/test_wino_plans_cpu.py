"""The launch-plan queries of the Winograd launchers (tmg_conv_wino_fwd_plan, _fwd3_plan, _narrow_plan, _wgrad_plan), the instance
coverage and the budgets of the case tables of test_wino_kernels.py (wino_cases.py), and the sensitivity of its two error measures.  No
device: the queries launch nothing, dereference nothing, and plan for 256 compute units when there is no device to ask.

Sweep: 18 image shapes from 1 x 1 to 16 x 128 x 128 pixels, 15 input and 22 output channel counts, through all four queries (the
weight gradient also grouped).  The case tables must reach, by name, every kernel instance, reduce width and plan feature the sweep reaches.

Compiled instances that no shape reaches: none.  tmg_wino.hip instantiates exactly wino_fwdp_kernel<1>, wino_fwd_kernel<2>,
wino_fwd3_kernel<1> / <2>, wino_nn_kernel<1> / <2> / <3>, the nine wino_wgrad_kernel<CIT, NCO, DB> (DB = false on <4, 4> only) and
wino_wgrad_reduce_kernel<4> / <8> / <16>, and the sweep reaches all of them.  wino_fwd_kernel<1> is NOT instantiated (asserted below): the
`NPW == 1` branches of wino_fwd_kernel (TMG_WN_PIN, LEAD = 3, the third ring slot at k = 0) are template text no object code comes from,
and the same holds for the `NPW == 2` text of wino_fwdp_kernel - a later clean-up can drop the parameter from both.

Which case catches which defect (shown on the fp64 restatement of the algorithm, test_defect_*: integer mode loses bit-equality, Gaussian
mode exceeds its bound):
  the last channel quad of a half-full chunk dropped         -> test_wino_fwd[f_cin48_cout72-*]
  the -V sign at nu = 3 dropped                              -> test_wino_fwd[f_cin4_cout64-*] (and every forward case)
  one tile of a block's second round dropped                 -> test_wino_fwd[p_fwdp_two_tiles-*-int]
  the ci_off1 term of wino_wgrad_reduce_kernel dropped       -> test_wino_wgrad[w_ci_split_off1-*]
  one group's dy_goff dropped                                -> test_wino_wgrad_grouped[g2_cin20_cg32-*]
The old check of test_hip_ops.py::test_winograd_* (max |diff| / max |ref| <= 2e-5) is evaluated on the first defect as well.  It does NOT
miss it: four dropped channels of 48 move the outputs by ~0.1 of max |ref| (test_defect_dropped_quad asserts the figure), and at these
channel counts 2e-5 max |ref| is in fact a SMALLER absolute allowance than the derived elementwise bound (K + c) u S^W.  What those
tests lacked is not tolerance but reach: none of the five defects lies on a path their case lists execute with valid data (no second
tile per block, no ci_off1, no grouped launch, the last quad of their half-full chunks is padding), and none of them is bit-exact.
"""
import os
import re

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import conv_cases as CC
import wino_cases as WC
from test_conv_plans_cpu import _header_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _H():
    import tmg_hip as H
    H.lib()
    return H


def _src():
    return open(os.path.join(ROOT, "deep-turbulence_amd", "csrc", "tmg_wino.hip")).read()


def _d(shape, slot, n):
    return CC.descr(shape, CC.seg(n), slot)


# ---------------------------------------------------------------------------------------------------------------------------------
# exports and signatures
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan_fn,launch_fn,extra", [
    ("tmg_conv_wino_fwd_plan", "tmg_conv_wino_fwd", ["int64_t *"]),
    ("tmg_conv_wino_fwd3_plan", "tmg_conv_wino_fwd3", ["int64_t *"]),
    ("tmg_conv_wino_narrow_plan", "tmg_conv_wino_narrow", ["int64_t *"]),
    ("tmg_conv_wino_wgrad_plan", "tmg_conv_wino_wgrad", ["int64_t", "int64_t *"]),
])
def test_plan_exports_and_signatures(plan_fn, launch_fn, extra):
    import ctypes
    H = _H()
    assert plan_fn in H.PLAN_EXPORTS and plan_fn not in H.EXPORTS and launch_fn in H.EXPORTS and hasattr(H.lib(), plan_fn)
    prm = _header_params(plan_fn)
    assert prm == _header_params(launch_fn) + extra, "a plan query takes its launch's arguments plus %s" % extra
    want = [ctypes.c_int64 if t == "int64_t" else ctypes.c_void_p for t in prm]
    assert H.PLAN_ARGTYPES[plan_fn] == want
    assert getattr(H.lib(), plan_fn).argtypes == want and getattr(H.lib(), plan_fn).restype is ctypes.c_int
    # the definition in the source has the header's parameter list
    m = re.search(r'extern "C" int %s\(([^)]*)\)' % plan_fn, _src(), re.S)
    assert m and [" ".join(q.replace("*", " * ").split()[:-1]).replace("hipStream_t", "tmg_stream_t") for q in m.group(1).split(",")] == prm


def test_plan_header_speaks_of_both_kernel_families():
    head = open(os.path.join(ROOT, "include", "tmglow_hip_plan.h")).read()
    assert "direct and Winograd" in head.split("*/")[0]
    H = _H()
    assert len(H.WINO_FWD_PLAN_FIELDS) == 13 and len(H.WINO_WGRAD_PLAN_FIELDS) == 11 and len(H.WINO_KERNELS) == 4
    assert re.search(r"#define TMG_WINO_FWD_PLAN_N 13\b", _src()) and re.search(r"#define TMG_WINO_WG_PLAN_N 11\b", _src())


def test_a_declined_query_leaves_the_plan_unwritten():
    H = _H()
    x, o = _d((2, 8, 8), 0, 8), _d((2, 8, 8), 4, 32)
    for fn in (H.conv_wino_fwd_plan, H.conv_wino_fwd3_plan, H.conv_wino_narrow_plan):
        p = fn([x], 32, [o])
        assert p["rc"] == -100 and all(p[f] == -1 for f in H.WINO_FWD_PLAN_FIELDS)
    q = H.conv_wino_wgrad_plan([_d((2, 8, 8), 0, 16)], o)
    assert q["rc"] == -100 and all(q[f] == -1 for f in H.WINO_WGRAD_PLAN_FIELDS)
    # an empty batch is "nothing to do": code 0, and nothing planned
    p = H.conv_wino_fwd_plan([_d((0, 8, 8), 0, 8)], 64, [_d((0, 8, 8), 4, 64)])
    assert p["rc"] == 0 and all(p[f] == -1 for f in H.WINO_FWD_PLAN_FIELDS)


def test_declined_by_plan():
    """The codes of wino_cases.DECLINED_* and their order (-3 for counts and channel sums before -100 for the envelope), from the
    queries: a query and its launch are one function body that returns these codes before the point where a launch would happen."""
    H = _H()
    for name, entry, ins, outs, cin, cout, bias_mis, code in WC.DECLINED_FWD:
        rc, buf = WC.raw_fwd(H, entry, [WC.spec_addr(s, i) for i, s in enumerate(ins)], [WC.spec_addr(s, 4 + i) for i, s in enumerate(outs)],
                             16, 0 if bias_mis is None else 4096 + 4 * bias_mis, cin if cin is not None else sum(s[0] for s in ins),
                             cout if cout is not None else sum(s[0] for s in outs), plan=True)
        assert rc == code and all(v == -1 for v in buf), (name, rc, code, buf)
    for name, ins, dys, cin, wsk, ng, code in WC.DECLINED_WG:
        if ng == "nogtab":
            continue            # the grouped entry's own test (no table): only a launch has it
        cin_ = cin if cin is not None else sum(s[0] for s in ins)
        need = int(H.lib().tmg_conv_wino_wgrad_ws_floats(H._i64(*(WC.DECL_SHAPE + (cin_, dys[0], 0, 0, 0, 0, 0, 0, 0)))))
        ws, wsn = {"ok": (4096, 1 << 21), "null": (0, 1 << 21), "short": (4096, max(need - 1, 0)), "misaligned": (4100, 1 << 21)}[wsk]
        rc, buf = WC.raw_wg(H, [WC.spec_addr(s, i) for i, s in enumerate(ins)], WC.spec_addr(dys, 4), 16, 16, ws, wsn, cin_, dys[0], plan=True)
        assert rc == code and all(v == -1 for v in buf), (name, rc, code, buf)
    # every condition the issue lists has an entry
    names = {e[0] for e in WC.DECLINED_FWD} | {"wg_" + e[0] for e in WC.DECLINED_WG}
    assert names >= {"wide_cout32", "narrow_cout52", "narrow_cin60", "cin6", "in_stride10", "in_misaligned", "bias_misaligned",
                     "no_input_segment", "four_input_segments", "no_output_segment", "four_output_segments", "cin_sum_disagrees",
                     "cout_sum_disagrees", "wg_ws_null", "wg_ws_short", "wg_ws_misaligned", "wg_cit1", "wg_cin_sum_disagrees"}
    # the comment above wino_fwd_setup states the order that is asserted here
    assert "The channel-sum test comes before the envelope test" in _src()


# ---------------------------------------------------------------------------------------------------------------------------------
# sweep
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = ((1, 1, 1), (1, 1, 7), (3, 17, 1), (1, 3, 5), (1, 8, 16), (2, 9, 17), (7, 8, 16), (2, 32, 32), (33, 8, 16), (64, 8, 16),
                (4, 64, 64), (1, 128, 128), (128, 8, 16), (2, 128, 128), (257, 8, 16), (513, 3, 5), (8, 128, 128), (16, 128, 128))
SWEEP_CIN = (4, 8, 16, 20, 32, 36, 48, 52, 64, 68, 72, 80, 104, 112, 256)
SWEEP_COUT = (4, 8, 16, 20, 32, 36, 44, 48, 52, 64, 68, 72, 76, 80, 128, 132, 248, 256, 260, 264, 480, 1920)


def _all_written(p):
    return p["rc"] == 0 and all(v >= 0 for v in p.values())


def _fwd_features(p):
    return {("inst", p["kernel"], p["NPW"]), ("gy>1", p["kernel"], p["grid_y"] > 1), ("tiles", p["kernel"], p["NPW"], min(p["max_tiles"], 3)),
            ("last_groups", p["kernel"], p["last_groups"]), ("odd_ntt", p["kernel"], p["NPW"] == 2 and p["ntt"] % 2 == 1),
            ("chunks", p["kernel"], min(p["nchunks"], 4))}


@pytest.fixture(scope="module")
def sweep():
    H = _H()
    fwd, wg = set(), set()
    for shp in SWEEP_SHAPES:
        for cin in SWEEP_CIN:
            x = _d(shp, 0, cin)
            for cout in SWEEP_COUT:
                o = _d(shp, 4, cout)
                for fn in (H.conv_wino_fwd_plan, H.conv_wino_fwd3_plan, H.conv_wino_narrow_plan):
                    p = fn([x], cout, [o])
                    if p["rc"] == 0:
                        assert _all_written(p), p
                        assert p["grid_x"] * p["max_tiles"] >= p["ntiles"] > p["grid_x"] * (p["max_tiles"] - 1)
                        fwd |= _fwd_features(p)
                    else:
                        assert p["rc"] == -100
                for ng in (1, 3):
                    q = H.conv_wino_wgrad_plan([x], o, ngroups=ng)
                    if q["rc"] == 0:
                        assert _all_written(q) and q["gy"] == ng * q["bpg"], q
                        wg |= {("inst", q["CIT"], q["NCO"], q["DB"]), ("NG", q["NG"]), ("gz>1", q["gz"] > 1), ("bpg>1", q["bpg"] > 1),
                               ("gx1", q["gx"] == 1), ("grouped", ng > 1)}
    return dict(fwd=fwd, wg=wg)


def test_compiled_instances_are_the_reached_ones(sweep):
    src = _src()
    inst = lambda feats: {f[1:] for f in feats if f[0] == "inst"}      # noqa: E731
    # what the launchers instantiate (a kernel template is instantiated where its address is taken for the launch)
    compiled = set()
    for name, k in (("wino_fwd_kernel", 0), ("wino_fwdp_kernel", 1), ("wino_fwd3_kernel", 2)):
        compiled |= {(k, int(n)) for n in re.findall(r"hipLaunchKernelGGL\(\(?%s<(\d)>" % name, src)}
    compiled |= {(3, int(n)) for n in re.findall(r"return launch_wino_nn<(\d)>", src)}
    assert compiled == {(0, 2), (1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 3)} == inst(sweep["fwd"])
    assert "wino_fwd_kernel<1>" not in src and "wino_fwdp_kernel<2>" not in src, "see the module docstring: not instantiated"
    ww = {tuple(int(v) for v in m) for m in re.findall(r"TMG_WW_CASE\((\d), (\d)\)", src)}
    assert ww == {(c, n) for c in (2, 3, 4) for n in (2, 3, 4)}
    assert inst(sweep["wg"]) == set(WC.WG_INSTANCES) == {(c, n, int(2 * 4 * (180 * (c * 16 + 8) + 128 * (n * 16 + 8)) <= 160 * 1024)) for c, n in ww}
    assert {int(n) for n in re.findall(r"hipLaunchKernelGGL\(wino_wgrad_reduce_kernel<(\d+)>", src)} == {4, 8, 16} == {
        f[1] for f in sweep["wg"] if f[0] == "NG"}
    # section 4 of the issue: the envelope in the comment, and the switch that no longer exists
    assert "FEW output channels (Cout <= 48)" in src and "Cout <= 64" not in src
    assert "getenv" not in src and "TMG_WN_NOSKEW" not in src


def test_forward_cases_reach_everything_the_sweep_reaches(sweep):
    H = _H()
    got = set()
    for case in WC.FWD_CASES:
        for arith in ("f32", "bf16x3"):
            got |= _fwd_features(WC.resolve_fwd(H, case, arith)[1])
    for case in WC.NARROW_CASES:
        got |= _fwd_features(WC.resolve_fwd(H, case)[1])
    missing = sweep["fwd"] - got
    assert not missing, "no forward case has %s" % sorted(missing, key=str)
    # every persistent case really has >= 2 tiles in some block at 256 compute units, and blocks with unequal counts
    pers = [c for c in WC.FWD_CASES + WC.NARROW_CASES if c["name"].startswith("p_")]
    assert {(WC.want_kernel(c, a), c["npw"]) for c in pers for a in ("f32", "bf16x3")} >= {(0, 2), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3)}
    for c in pers:
        for arith in (("f32",) if c["narrow"] else ("f32", "bf16x3")):
            B, p = WC.resolve_fwd(H, c, arith)
            assert p["max_tiles"] >= 2 and p["ntiles"] % p["grid_x"] != 0 and p["grid_x"] * p["grid_y"] <= WC.CU_DEFAULT, (c["name"], p)
            assert p["tiles_x"] * p["tiles_y"] == 1 and B == p["ntiles"], "a block's consecutive tiles lie in different images"
    for k in (0, 1, 2, 3):
        mine = [WC.resolve_fwd(H, c, a)[1] for c in pers for a in ("f32", "bf16x3") if WC.want_kernel(c, a) == k and not (c["narrow"] and a != "f32")]
        assert {p["max_tiles"] for p in mine} >= {2, 3}, k
        assert {p["nchunks"] for p in mine} >= {1, 3} or k == 3, k            # (wino_nn_kernel: Cin >= 64, two chunks or more)
        assert any(p["nchunks"] % 2 == 1 and p["max_tiles"] >= 2 for p in mine), "an odd stage total"
        assert any(p["last_groups"] == 1 and p["max_tiles"] >= 2 for p in mine) or k == 2, "a half-full last chunk with two tiles"


def test_forward_tables_cover_the_listed_edges():
    wide, nar = WC.FWD_CASES, WC.NARROW_CASES
    assert {c["cin"] for c in wide} >= {4, 8, 20, 48, 104} and {c["cin"] % 32 for c in wide} >= {4, 16, 20}
    assert {c["cout"] % 16 for c in wide} >= {4, 8, 12}
    for tab, pads in ((wide, ("zero", "rep")), (nar, ("zero", "rep"))):
        for hw in WC.SMALL_HW:
            for pad in pads:
                assert any(c["hw"] == hw and ("rep" in c["sw"]) == (pad == "rep") for c in tab), (hw, pad)
    assert {v for hw in WC.SMALL_HW for v in hw} >= {1, 2, 3, 7, 9, 17}
    assert {len(c["ins"]) for c in wide} == {1, 2, 3} and {len(c["outs"]) for c in wide} == {1, 2, 3}
    assert any(len(c["outs"]) == 3 for c in nar)
    # segment boundaries: inside a chunk at a quad that is no 16-multiple; inside a 16-channel output tile; slices with stride > n, offset > 0
    assert any(len(c["ins"]) > 1 and c["ins"][0][0] % 16 for c in wide) and any(len(c["outs"]) > 1 and c["outs"][0][0] % 16 for c in wide)
    assert any(sp[1] > sp[0] and sp[2] > 0 for c in wide for sp in c["ins"]) and any(sp[1] > sp[0] and sp[2] > 0 for c in wide for sp in c["outs"])
    for sw in ("bias", "relu_in", "rep"):
        on = sum(sw in c["sw"] for c in wide)
        assert on >= 3 and len(wide) - on >= 3, sw
    for sw in WC.SWITCHES:
        on = sum(sw in c["sw"] for c in nar)
        assert on >= 3 and len(nar) - on >= 3, sw
    assert {c["npw"] for c in nar} == {1, 2, 3} and 64 in {c["cin"] for c in nar} and any(c["cin"] % 32 == 16 for c in nar)
    dg = [c for c in nar if c["dgrad"]]
    assert dg and all(c["dgrad"][1] < c["dgrad"][0] and c["cin"] % 16 for c in dg), "mode 1 with nvalid < Cin and K % 16 != 0"


def test_wgrad_cases_reach_everything_the_sweep_reaches(sweep):
    H = _H()
    got, plans = set(), {}
    for c in WC.WG_CASES:
        B, p = WC.resolve_wg(H, c)
        plans[c["name"]] = (B, p)
        got |= {("inst", p["CIT"], p["NCO"], p["DB"]), ("NG", p["NG"]), ("gz>1", p["gz"] > 1), ("gx1", p["gx"] == 1), ("bpg>1", False),
                ("grouped", False)}
    for c in WC.GROUPED_CASES:
        p = WC.resolve_wg(H, c, ngroups=c["G"])[1]
        got |= {("inst", p["CIT"], p["NCO"], p["DB"]), ("NG", p["NG"]), ("gz>1", p["gz"] > 1), ("bpg>1", p["bpg"] > 1), ("grouped", True)}
    missing = sweep["wg"] - got
    assert not missing, "no weight-gradient case has %s" % sorted(missing, key=str)
    vals = [p for _, p in plans.values()]
    assert any(p["gy"] > 1 for p in vals) and any(p["gz"] > 1 for p in vals)
    assert any(p["gx"] > 1 and p["ntiles"] % p["gx"] for p in vals), "an odd tile share"
    assert {p["ntiles"] for p in vals if p["gx"] == 1} >= {1, 3}
    assert {(p["CIT"], p["NCO"]) for p in vals if p["DB"] == 0} == {(4, 4)}
    lay = [c["layout"] for c in WC.WG_CASES]
    assert any(l[0] > 32 and l[3] for l in lay) and any(l[2] and l[4] for l in lay) and any(0 < l[1] < 32 and not l[2] for l in lay)
    assert any(c["dy"][1] > c["dy"][0] and c["dy"][2] == 4 for c in WC.WG_CASES) and any(len(c["ins"]) == 3 for c in WC.WG_CASES)
    assert any(c["cin"] % 16 and c["cout"] % 16 for c in WC.WG_CASES)
    assert {c["G"] for c in WC.GROUPED_CASES} == {2, 3} and {c["cin"] for c in WC.GROUPED_CASES} >= {20, 36, 68}
    assert {c["cout"] for c in WC.GROUPED_CASES} >= {32, 64}
    # Gaussian cases: K <= 2048
    for c in WC.WG_CASES:
        B, _ = plans[c["name"]]
        assert not c["gauss"] or WC.wg_dy_tiles((B,) + c["shape"][1:]) <= CC.KMAX_GAUSS, c["name"]
    assert all(WC.wg_dy_tiles(c["shape"]) <= CC.KMAX_GAUSS for c in WC.GROUPED_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# budgets; the restatement against the plain reference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_integer_budget_and_gauss_range_of_every_case():
    """4 S^W < 2^24 for every integer case (at the batch 256 compute units resolve to); K <= 2048 for every Gaussian one."""
    H = _H()
    for c in WC.FWD_CASES + WC.NARROW_CASES:
        B, p = WC.resolve_fwd(H, c)
        d = WC.fwd_data(c, B, "int")
        xp = WC.activate(d["x"], "relu_in" in c["sw"], "rep" in c["sw"])
        assert CC.int_terms_ok(WC.wino_fwd(xp, d["w_eff"], d["bias"], absolute=True), WC.GRAN), c["name"]
        assert WC.cin_pad(c, "bf16x3") <= CC.KMAX_GAUSS
        if "relu_in" in c["sw"]:
            assert bool((d["x"] < 0).any()), "relu_in must really clip"
    for c in WC.WG_CASES:
        B, p = WC.resolve_wg(H, c)
        d = WC.wg_data(c, B, "int")
        _, SW, _, Sb, _ = WC.wg_ref(c, d)
        assert CC.int_terms_ok(SW, WC.GRAN) and CC.int_terms_ok(Sb), c["name"]
    for c in WC.GROUPED_CASES:
        for _, SW, _, Sb, _ in WC.grouped_ref(c, WC.grouped_data(c, "int")):
            assert CC.int_terms_ok(SW, WC.GRAN) and CC.int_terms_ok(Sb), c["name"]


def test_bf16_parts_two_is_exercised_by_the_two_named_cases():
    """Small integers leave parts 2 and 3 of the bf16x3 split zero: bf3_parts_v makes the transformed V, bf3_parts_u the operand U need
    more than 8 significant bits (from the fp64 restatement), inside the integer budget."""
    plain = WC.FWD_BY_NAME["f_cin48_cout72"]
    for name, which in (("bf3_parts_v", "V"), ("bf3_parts_u", "U"), ("f_cin48_cout72", None)):
        c = WC.FWD_BY_NAME[name]
        assert 16 <= c["cin"] <= 48
        d = WC.fwd_data(c, c["B"], "int")
        xp = WC.activate(d["x"], "relu_in" in c["sw"], "rep" in c["sw"])
        V = WC._two_sided(WC.BT, WC.patches(xp)[0])
        U = WC._two_sided(WC.G, d["w_eff"])
        v2, u2 = WC.split_bf16(V)[1], WC.split_bf16(U)[1]
        assert bool((v2 != 0).any()) == (which == "V") and bool((u2 != 0).any()) == (which == "U"), name
        assert torch.equal(sum(WC.split_bf16(V)), V) and torch.equal(sum(WC.split_bf16(U)), U)
        assert CC.int_terms_ok(WC.wino_fwd(xp, d["w_eff"], d["bias"], absolute=True), WC.GRAN)
    assert plain["amp"] == (3, 2)


@pytest.mark.parametrize("name", ["f_cin48_cout72", "f2_cin20_cout264", "f_hw1x1_rep", "n3_dgrad_k72_nvalid36", "n2_hw1x17_zero"])
def test_forward_restatement_equals_the_plain_reference(name):
    c = WC.FWD_BY_NAME.get(name) or WC.NARROW_BY_NAME[name]
    for mode in ("int", "gauss"):
        d = WC.fwd_data(c, c["B"], mode)
        ref, S = WC.fwd_ref(c, d)
        win, _ = WC.fwd_ref(c, d, winograd=True)
        assert bool((S >= ref.abs() * (1 - 1e-12)).all()), "S^W bounds |ref|"
        if mode == "int":
            assert torch.equal(win, ref)
        else:
            assert bool(((win - ref).abs() <= 1e-13 * S).all())
        # the measures accept the reference rounded to fp32 and refuse a NaN
        K, cc = WC.cin_pad(c, "f32"), WC.fwd_c(3 if c["narrow"] else 0, 1)
        assert CC.gauss_share(ref.float(), ref, S, K + cc - 8) <= 1.0
        bad = ref.float().clone()
        bad.view(-1)[0] = float("nan")
        assert CC.gauss_share(bad, ref, S, K + cc - 8) == float("inf") and not CC.bit_equal(bad, ref)


@pytest.mark.parametrize("name", ["w_cit2_nco2", "w_cit3_nco4_gz2", "w_hw1x1", "w_hw17x1", "w_ci_split_off1"])
def test_wgrad_restatement_equals_the_plain_reference(name):
    c = WC.WG_BY_NAME[name]
    for mode in ("int", "gauss"):
        d = WC.wg_data(c, c["shape"][0], mode)
        Wr, SW, br, Sb, touched = WC.wg_ref(c, d)
        Ww = WC.wg_ref(c, d, winograd=True)[0]
        assert bool((SW >= Wr.abs() * (1 - 1e-12)).all())
        assert torch.equal(Ww, Wr) if mode == "int" else bool(((Ww - Wr).abs() <= 1e-13 * SW).all())
        assert torch.equal(Wr[:, ~touched], d["prevW"][:, ~touched])


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity of the measures (fp64 restatement alone)
# ---------------------------------------------------------------------------------------------------------------------------------
def _caught(ref_g, S_g, bad_g, ref_i, bad_i, Kc, what, frac):
    """Gaussian mode: the defective result exceeds the bound - by 10x at its worst element and on the fraction `frac` of the elements it
    changes (a defect that removes few Gaussian products leaves some elements within any bound: conv_cases' test of the same name).
    Integer mode: equality fails."""
    sh = CC.affected_shares(bad_g, ref_g, S_g, Kc - 8)
    assert sh.numel() > 0, what
    assert float(sh.max()) > 10.0 and float((sh > 1.0).double().mean()) > frac, (what, float(sh.max()), float((sh > 1).double().mean()))
    assert CC.gauss_share(bad_g.float(), ref_g, S_g, Kc - 8) > 10.0, what
    assert not CC.bit_equal(bad_i.float(), ref_i), what
    assert CC.gauss_share(ref_g.float(), ref_g, S_g, Kc - 8) <= 1.0 and CC.bit_equal(ref_i.float(), ref_i)


def _fwd_defect(name, fault, B=None):
    H = _H()
    c = WC.FWD_BY_NAME[name]
    B0, p = WC.resolve_fwd(H, c)
    out = {}
    for mode in ("gauss", "int"):
        d = WC.fwd_data(c, B or B0, mode)
        ref, S = WC.fwd_ref(c, d, winograd=True)       # (the restatement itself: the defect is the only difference, bit for bit)
        out[mode] = (ref, S, WC.fwd_ref(c, d, fault=fault)[0])
    return c, p, out


def test_defect_dropped_quad_of_a_half_full_chunk():
    c, p, r = _fwd_defect("f_cin48_cout72", ("chan", 44, 48))
    assert p["nchunks"] == 2 and p["last_groups"] == 1 and p["Cin_pad"] == c["cin"] == 48, "the last quad of the half-full chunk is valid data"
    (ref_g, S_g, bad_g), (ref_i, _, bad_i) = r["gauss"], r["int"]
    _caught(ref_g, S_g, bad_g, ref_i, bad_i, p["Cin_pad"] + WC.fwd_c(p["kernel"], p["nchunks"]), "dropped quad", 0.9)
    # the old check, max |diff| / max |ref| <= 2e-5, on the same defect: it does not miss it (module docstring)
    old = float((bad_g - ref_g).abs().max() / ref_g.abs().max())
    assert 0.02 < old < 1.0, old
    # and per element the old allowance 2e-5 max |ref| is the SMALLER one here: the derived bound is no tighter than the old tolerance,
    # the integer mode is
    new_abs = (p["Cin_pad"] + WC.fwd_c(p["kernel"], p["nchunks"])) * CC.U24 * S_g
    assert float(new_abs.median()) > 2e-5 * float(ref_g.abs().max())


def test_defect_dropped_sign_at_nu3():
    c, p, r = _fwd_defect("f_cin4_cout64", ("nu3",))
    (ref_g, S_g, bad_g), (ref_i, _, bad_i) = r["gauss"], r["int"]
    _caught(ref_g, S_g, bad_g, ref_i, bad_i, p["Cin_pad"] + WC.fwd_c(p["kernel"], p["nchunks"]), "nu = 3 sign", 0.99)


def test_defect_dropped_tile_of_the_second_round():
    H = _H()
    c = WC.FWD_BY_NAME["p_fwdp_two_tiles"]
    B, p = WC.resolve_fwd(H, c)
    assert p["max_tiles"] == 2 and p["ntiles"] == p["grid_x"] + 1
    c_, _, r = _fwd_defect("p_fwdp_two_tiles", ("tile", p["grid_x"]))      # block 0's second tile
    (ref_g, S_g, bad_g), (ref_i, _, bad_i) = r["gauss"], r["int"]
    assert bool((bad_i[:p["grid_x"]] == ref_i[:p["grid_x"]]).all()) and bool((bad_i[p["grid_x"]] != ref_i[p["grid_x"]]).any())
    _caught(ref_g, S_g, bad_g, ref_i, bad_i, p["Cin_pad"] + WC.fwd_c(p["kernel"], p["nchunks"]), "second-round tile", 0.99)


def test_defect_dropped_ci_off1():
    H = _H()
    c = WC.WG_BY_NAME["w_ci_split_off1"]
    B, p = WC.resolve_wg(H, c)
    dg, di = WC.wg_data(c, B, "gauss"), WC.wg_data(c, B, "int")
    Wg, Sg, _, _, touched = WC.wg_ref(c, dg)
    Wi = WC.wg_ref(c, di)[0]
    assert touched.tolist() == [False] + [True] * 12 + [False] * 8 + [True] * 16 + [False] * 3
    Kc = WC.wg_dy_tiles((B,) + c["shape"][1:]) + WC.wg_c(p)
    _caught(Wg, Sg, WC.wg_ref(c, dg, off1_fault=True)[0], Wi, WC.wg_ref(c, di, off1_fault=True)[0], Kc, "ci_off1", 0.99)


def test_defect_dropped_dy_goff():
    H = _H()
    c = WC.GROUPED_BY_NAME["g2_cin20_cg32"]
    B, p = WC.resolve_wg(H, c, ngroups=c["G"])
    dg, di = WC.grouped_data(c, "gauss"), WC.grouped_data(c, "int")
    rg, ri = WC.grouped_ref(c, dg), WC.grouped_ref(c, di)
    bg, bi = WC.grouped_ref(c, dg, goff_fault=1), WC.grouped_ref(c, di, goff_fault=1)
    Kc = WC.wg_dy_tiles(c["shape"]) + WC.wg_c(p)
    assert torch.equal(bg[0][0], rg[0][0]), "group 0 has no offset to lose"
    _caught(rg[1][0], rg[1][1], bg[1][0], ri[1][0], bi[1][0], Kc, "dy_goff dW", 0.99)
    _caught(rg[1][2], rg[1][3], bg[1][2], ri[1][2], bi[1][2], WC.wg_kb(p) + 1, "dy_goff dbias", 0.9)


def test_pack_reference_layout():
    """pack_ref / pack3_unpack against the layout comments on hand-checked entries."""
    w = torch.arange(6 * 20 * 9, dtype=torch.float64).reshape(6, 20, 3, 3)
    U = WC.pack_ref(w, 0).reshape(16, 2, 16, 16)                         # [pos][k / 16][n][k % 16]
    assert float(U[0, 1, 3, 1]) == float(w[3, 17, 0, 0]) and float(U[15, 1, 3, 1]) == float(w[3, 17, 2, 2])
    assert float(U[5, 0, 2, 7]) == float(0.25 * (w[2, 7].sum()))        # position (1, 1): G row 1 on both sides
    assert float(U[0, 1, 3, 4]) == 0 and float(U[0, 0, 6, 0]) == 0       # k = 20, n = 6: padding
    U1 = WC.pack_ref(w, 1, 12).reshape(16, 1, 16, 16)                    # K = 6 weight output channels, N = 12 input channels
    assert float(U1[0, 0, 11, 5]) == float(w[5, 11, 2, 2]) and float(U1[15, 0, 11, 5]) == float(w[5, 11, 0, 0])
    assert float(U1[0, 0, 12, 5]) == 0 and float(U1[0, 0, 11, 6]) == 0
    # pack3_unpack inverts the documented lane order
    K, N = 40, 20
    nch, ntt = 2, 2
    t = torch.zeros(16, nch, ntt, 3, 64, 8, dtype=torch.int16)
    k, n, pos, part = 37, 18, 9, 1
    t[pos, k // 32, n // 16, part, 16 * ((k % 32) // 8) + n % 16, k % 8] = 0x3f80          # bf16 1.0
    back = WC.pack3_unpack(t.reshape(-1), K, N)
    assert float(back[part, pos, k // 16, n, k % 16]) == 1.0 and float(back.sum()) == 1.0
