"""The launch-plan queries of the growth-layer forwards and the thin / mix weight gradients (tmg_c1x2_fwd_plan, tmg_c1_fwd_plan,
tmg_conv_wgrad_thin_grouped_plan, tmg_mix_wgrad_grouped_plan), the coverage of the case tables of test_thin_kernels.py
(thin_cases.py), their budgets and the sensitivity of the two error measures.  No device: the queries launch nothing and dereference
nothing.

Sweep: 19 image shapes from 1 x 1 to 64 x 128 x 128 pixels, the supported channel counts (and the unaligned ones of the scalar
staging path), G = 1 .. 16 groups.  The case tables must reach, by name, every (instance, plan feature) pair the sweep reaches, and
the sweep every kernel instance the sources instantiate.

Return paths that NO shape reaches (asserted below):
  tmg_c1x2_fwd's -2 of the ring check (2 (TW + 2) + 2 TH > 256 / CG): the launcher's tile shapes are (TW, TH) in {(8, 32), (16, 16),
  (32, 8)} at CG = 1, {(8, 16), (16, 8), (32, 4)} at CG = 2 and {(8, 8), (16, 4)} at CG = 4 (TW_log2 5 is reduced to 4), whose rings hold
  84, 68, 84 / 52, 52, 76 / 36, 44 pixels.  The only -2 left is the misaligned output.
Reachable and named: empty partitions of mix_wgrad_kernel (p0 >= npix) whenever P = ceil(2048 / G) and ceil(npix / P) lies just above
a multiple of 16 U (m16_g16_empty_partitions, m32_g16_empty_partitions, m32_g15_p137_pair): such a block adds zeros.

Which case catches which defect (each applied to the fp64 restatement; it must break integer equality in the named cases, only there):
  d1 not zeroed on ring pixels outside the image      -> every c1x2 case (*_plus1_xcd_uneven, *_h1w1, x_cg1_cq2_xcd_uneven, ..)
  one CG lane's channel quads dropped                  -> x_cg2_cq4_b512, x_cg4_cin64_norelu, .. (not x_cg2_cin12_seg3, x_cg1_*)
  the second chunk's last quad dropped                 -> the nchunks >= 2 cases of c1x2 and c1_fwd (not c_cin44_rows36)
  thin group index with the plain mapping, P % 8 == 0  -> the xcd cases with even G (t_ch*_dyc4_few, t_walk_in_images; one-to-one at G = 15)
  z / w of a compact dy pair not zeroed                -> rows 2, 3 of the dyc = 2 cases with G > 1
  the last partition's ragged pixels dropped           -> m16_p4_last1, m16_p4_last2_pair, m32_p8_last3_pair, m32_p8_last1, ..
  the second dy half read at the first half's stride   -> every `pair` case
  a looping block's second round of pixels dropped     -> the four mx_*_cap_* cases
"""
import os
import re

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import conv_cases as CC
import thin_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deep-turbulence_amd", "csrc")


def _H():
    import tmg_hip as H
    H.lib()
    return H


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# ---------------------------------------------------------------------------------------------------------------------------------
# exports and signatures
# ---------------------------------------------------------------------------------------------------------------------------------
def _header_params(name):
    txt = open(os.path.join(ROOT, "include", "tmglow_hip.h")).read() + open(os.path.join(ROOT, "include", "tmglow_hip_plan.h")).read()
    m = re.search(r"\bint\s+%s\(([^;]*?)\);" % name, txt, re.S)
    assert m, "the headers do not declare %s" % name
    return [" ".join(prm.replace("*", " * ").split()[:-1]) for prm in m.group(1).split(",")]


@pytest.mark.parametrize("plan_fn,launch_fn,fields", [
    ("tmg_c1x2_fwd_plan", "tmg_c1x2_fwd", "C1X2_PLAN_FIELDS"),
    ("tmg_c1_fwd_plan", "tmg_c1_fwd_add", "C1_PLAN_FIELDS"),
    ("tmg_conv_wgrad_thin_grouped_plan", "tmg_conv_wgrad_thin_grouped", "THIN_PLAN_FIELDS"),
    ("tmg_mix_wgrad_grouped_plan", "tmg_mix_wgrad_grouped", "MIX_WGRAD_PLAN_FIELDS"),
])
def test_plan_exports_and_signatures(plan_fn, launch_fn, fields):
    import ctypes
    H = _H()
    assert plan_fn in H.PLAN_EXPORTS and plan_fn not in H.EXPORTS and hasattr(H.lib(), plan_fn)
    prm = _header_params(plan_fn)
    assert prm == _header_params(launch_fn) + ["int64_t *"], "a plan query takes its launch's arguments plus the plan"
    want = [ctypes.c_int64 if t == "int64_t" else ctypes.c_void_p for t in prm]
    assert H.PLAN_ARGTYPES[plan_fn] == want
    assert getattr(H.lib(), plan_fn).argtypes == want and getattr(H.lib(), plan_fn).restype is ctypes.c_int
    # the header's field list is the wrapper's
    hdr = open(os.path.join(ROOT, "include", "tmglow_hip_plan.h")).read()
    m = re.search(r"%s[^:]*: plan\[(\d+)\] = \{([^}]*)\}" % plan_fn, hdr, re.S)
    assert m and int(m.group(1)) == len(getattr(H, fields))
    names = [re.sub(r"\s*\(.*", "", f.strip(" *\n"), flags=re.S) for f in re.sub(r"\([^)]*\)", "", m.group(2)).split(",")]
    assert tuple(n.split()[0] for n in names) == getattr(H, fields)


def test_a_declined_query_leaves_the_plan_unwritten():
    H = _H()
    p = T.thin_plan(H, T.THIN_BY_NAME["t_declined_cin16"])
    assert p["rc"] == -100 and all(p[f] == -1 for f in H.THIN_PLAN_FIELDS)
    q = T.mixwg_plan(H, T.MIXWG_BY_NAME["m_declined_c24"])
    assert q["rc"] == -100 and all(q[f] == -1 for f in H.MIX_WGRAD_PLAN_FIELDS)
    B, Hh, Ww = 2, 5, 7
    r = H.c1x2_fwd_plan([T.descr((B, Hh, Ww), T.seg(8), 0)], T.descr((B, Hh, Ww), T.seg(4, 4, 0, 1), 6))      # output 4 bytes off
    assert r["rc"] == -2 and all(r[f] == -1 for f in H.C1X2_PLAN_FIELDS)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases reach the plans they name
# ---------------------------------------------------------------------------------------------------------------------------------
def _plan_of(H, case):
    return {"c1x2": T.c1x2_plan, "c1": T.c1_plan, "thin": T.thin_plan, "mixwg": T.mixwg_plan}[case["fam"]](H, case)


QUERIED = T.C1X2_CASES + T.C1_CASES + T.THIN_CASES + T.MIXWG_CASES


@pytest.mark.parametrize("case", QUERIED, ids=lambda c: c["name"])
def test_case_reaches_its_plan(case):
    p = _plan_of(_H(), case)
    assert p["rc"] == case.get("rc", 0), p
    if p["rc"] == 0:
        assert all(v >= 0 for v in p.values())
        assert all(p[k] == v for k, v in case["plan"].items()), (case["plan"], p)
        if case["fam"] == "c1x2":
            assert p["CG"] == case["CG"], p
            assert p["nring"] == 2 * ((1 << p["TW_log2"]) + 2) + 2 * p["TH"] <= 256 // p["CG"]
        if case["fam"] == "thin":
            assert (p["SL"], p["CS"], p["TH"]) == T.THIN_INST[case["cin"]] and p["grid"] == p["P"] * case["G"] and p["lds_bytes"] <= 65536


def test_mix_plan_restates_the_launchers():
    """thin_cases.MIX32_INST / MIX16_INST are the switch tables of tmg_mix_f32 / tmg_mix_f16, the grid formula launch_mix32's and
    launch_mix16's."""
    src = _src("tmg_mix16.hip")
    for fn, table in (("launch_mix32", T.MIX32_INST), ("launch_mix16", T.MIX16_INST)):
        got, pending = {}, []
        body = src[src.index('extern "C" int tmg_mix_f%s(' % ("32" if fn == "launch_mix32" else "16")):]
        body = body[:body.index("\n}\n")]
        for ln in body.splitlines():
            pending += [int(v) for v in re.findall(r"case (\d+):", ln)]
            m = re.search(r"return %s<(\d+), (\d+)>\(p, st\)" % fn, ln)
            if m:
                if "default" in ln:
                    pending = [k for k in table if k not in got]
                for k in pending:
                    got[k] = (int(m.group(1)), int(m.group(2)))
                pending = []
        assert got == table, (fn, got)
        assert re.search(r"static int %s\(const Mix16P& p, hipStream_t st\) \{.*?const long groups = \(p\.npix \+ 64L \* NP - 1\) / \(64L \* NP\);\s*"
                         r"const int grid = \(int\)\(groups < 2048 \? \(groups < 1 \? 1 : groups\) : 2048\);" % fn, src, re.S)
    assert T.mix_plan("f32", 68, 2048 * 64 + 101) == (6, 1, 2048, 2) and T.mix_plan("f16", 16, 17) == (1, 8, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# sweep, coverage, instances
# ---------------------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPES = ((1, 1, 1), (3, 1, 1), (2, 3, 5), (1, 8, 8), (2, 11, 5), (3, 9, 12), (2, 16, 16), (5, 9, 33), (5, 5, 33), (2, 40, 40), (41, 40, 40), (8, 64, 64),
                (130, 16, 16), (512, 5, 7), (1024, 5, 7), (1027, 5, 7), (4, 128, 128), (16, 128, 128), (64, 128, 128))
SWEEP_CIN = (3, 4, 6, 8, 10, 12, 16, 18, 32, 36, 44, 64)
SWEEP_G = tuple(range(1, 17))


@pytest.fixture(scope="module")
def sweep():
    H = _H()
    out = dict(c1x2=set(), c1=set(), thin=set(), mixwg=set(), mix=set(), rc=set())
    for shp in SWEEP_SHAPES:
        npix = shp[0] * shp[1] * shp[2]
        for cin in SWEEP_CIN + (68, 70):
            for mis in (0, 1):
                ins = [T.descr(shp, T.seg(cin, cin, 0, mis), 0)]
                if cin <= 64:
                    p = H.c1x2_fwd_plan(ins, T.descr(shp, T.seg(4), 6), w2_d1_row=cin)
                    out["rc"].add(("c1x2", p["rc"]))
                    out["c1x2"] |= T.c1x2_features(p)
                q = H.c1_fwd_plan(ins, T.descr(shp, T.seg(1, 4, 0), 6))
                out["rc"].add(("c1", q["rc"]))
                out["c1"] |= T.c1_features(q)
        for G in SWEEP_G:
            for ch in (8, 16, 32, 64):
                for dyc in (2, 4):
                    p = H.conv_wgrad_thin_grouped_plan(shp, (ch, 4), G, CC.BASE, dyc * G, dyc)
                    out["rc"].add(("thin", p["rc"]))
                    out["thin"] |= T.thin_features(p)
            for Cn in (16, 32):
                p = H.mix_wgrad_grouped_plan(npix, Cn, G)
                out["rc"].add(("mixwg", p["rc"]))
                out["mixwg"] |= T.mixwg_features(p, npix)
        for kind, cmax in (("f32", 128), ("f16", 256)):
            for Cn in range(4, cmax + 1, 4):
                for sw in ("bias", "transposed", ""):
                    out["mix"] |= T.mix_features(T.mix_case("s", kind, Cn, npix, sw=sw))
    return out


def _case_pairs(H):
    got = dict(c1x2=set(), c1=set(), thin=set(), mixwg=set(), mix=set())
    for c in T.C1X2_CASES:
        got["c1x2"] |= T.c1x2_features(T.c1x2_plan(H, c))
    for c in T.C1_CASES:
        got["c1"] |= T.c1_features(T.c1_plan(H, c))
    for c in T.THIN_CASES:
        if c["rc"] == 0:
            got["thin"] |= T.thin_features(T.thin_plan(H, c))
    for c in T.MIXWG_CASES:
        if c["rc"] == 0:
            got["mixwg"] |= T.mixwg_features(T.mixwg_plan(H, c), c["npix"])
    for c in T.MIX_CASES:
        if c["rc"] == 0:
            got["mix"] |= T.mix_features(c)
    return got


def test_cases_cover_every_instance_and_plan_feature_of_the_sweep(sweep):
    got = _case_pairs(_H())
    for fam in got:
        missing = sorted(sweep[fam] - got[fam])
        assert not missing, "%s: (instance, feature) pairs the sweep reaches and no case names: %s" % (fam, missing)


def test_sweep_reaches_every_instantiated_kernel(sweep):
    pw, th, mx = _src("tmg_pointwise.hip"), _src("tmg_thin.hip"), _src("tmg_mix16.hip")
    inst = {"c1x2<%s>" % m for m in re.findall(r"hipLaunchKernelGGL\(c1x2_fwd_kernel<(\d+)>", pw)}
    assert inst == {"c1x2<1>", "c1x2<2>", "c1x2<4>"} == {i for i, _ in sweep["c1x2"]}
    assert "hipLaunchKernelGGL(c1_fwd_kernel," in pw and {i for i, _ in sweep["c1"]} == {"c1_fwd"}
    inst = {"thin<%s,%s,%s>" % m for m in re.findall(r"launch_thin<(\d+), (\d+), (\d+)>\(p", th)}
    assert len(inst) == 4 and inst == {i for i, _ in sweep["thin"]}
    inst = {"mix_wgrad<%s>" % m for m in re.findall(r"hipLaunchKernelGGL\(mix_wgrad_kernel<(\d+)>", th)}
    assert inst == {"mix_wgrad<1>", "mix_wgrad<2>"} == {i for i, _ in sweep["mixwg"]}
    inst = {"mix32<%s,%s,0>" % m for m in re.findall(r"launch_mix32<(\d+), (\d+)>\(p", mx)} | {"mix16<%s,%s>" % m for m in re.findall(r"launch_mix16<(\d+), (\d+)>\(p", mx)}
    assert len(inst) == 6 + 8 and inst == {i for i, _ in sweep["mix"] if "loop" not in i}
    assert {i for i, f in sweep["mix"] if f == "loops"} == {"mix32 loop", "mix16 loop", "mix16 loop NT > 8"}


def test_unreachable_return_paths(sweep):
    """No shape of the sweep is declined by a supported channel count: the ring check's -2 of tmg_c1x2_fwd in particular is dead."""
    assert sweep["rc"] == {("c1x2", 0), ("c1", 0), ("thin", 0), ("mixwg", 0)}
    for cg in (1, 2, 4):
        for twl in (3, 4, 5):
            t = twl
            while ((256 // cg) >> t) < 4 and t > 3:
                t -= 1
            assert 2 * ((1 << t) + 2) + 2 * ((256 // cg) >> t) <= 256 // cg


def test_empty_partitions_are_reachable(sweep):
    assert ("mix_wgrad<1>", "empty_partitions") in sweep["mixwg"] and ("mix_wgrad<2>", "empty_partitions") in sweep["mixwg"]
    H = _H()
    for name in ("m16_g16_empty_partitions", "m32_g16_empty_partitions"):
        c = T.MIXWG_BY_NAME[name]
        p = T.mixwg_plan(H, c)
        assert (p["P"] - 1) * p["per"] >= c["npix"]


# ---------------------------------------------------------------------------------------------------------------------------------
# budgets and measures
# ---------------------------------------------------------------------------------------------------------------------------------
ALL_CASES = QUERIED + T.PLANES_CASES + T.MIX_CASES


def test_budgets():
    assert len({c["name"] for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        by, fl = T.case_cost(c)
        assert by <= T.BYTES_CAP and fl <= T.REF_FLOP_CAP, (c["name"], by, fl)
    big = [c["name"] for c in ALL_CASES if c.get("big")]
    assert sorted(big) == sorted(["m16_g16_empty_partitions", "m32_g16_empty_partitions", "m32_g15_p137_pair", "mx_f32_cap_np1_c68",
                                  "mx_f16_cap_6x2_c96", "mx_f16_cap_nt12_c192", "mx_f32_cap_np8_c16"]), big


def _refs(case, mode="int"):
    """(reference tensors, S tensors) of a case on the CPU."""
    fam = case["fam"]
    if fam == "c1x2":
        ref, S = T.c1x2_ref(case, T.fwd_data(case, mode))
        return [ref], [S["S2"], S["S1"]]
    if fam == "c1":
        ref, S = T.c1_ref(case, T.c1_data(case, mode))
        return [ref], [S]
    if fam == "thin":
        ref, S = T.thin_ref(case, T.thin_data(case, mode))
        return [ref], [S]
    if fam == "mixwg":
        dW, SW, db, Sb = T.mixwg_ref(case, T.mixwg_data(case, mode))
        return [dW, db], [SW, Sb]
    ref, S = T.mix_ref(case, T.mix_data(case, mode))
    return [ref], [S]


@pytest.mark.parametrize("case", [c for c in QUERIED + T.MIX_CASES if c.get("rc", 0) == 0], ids=lambda c: c["name"])
def test_integer_premise(case):
    """S < 2^24 in integer mode for every case, every element: no element is left out of the exact check.  The Gaussian bound is
    applied only where K <= KMAX_GAUSS (2048)."""
    if case["fam"] == "mix" and case.get("big"):
        S = [torch.tensor(float(case["C"] * 3 * 2 + 8))]         # |x| <= 3, |W| <= 2, |bias| <= 8
    else:
        refs, S = _refs(case)
        assert all(bool(torch.isfinite(r).all()) for r in refs)
    assert all(T.int_terms_ok(s) for s in S), [float(s.max()) for s in S]
    if case["fam"] == "mix" and case["kind"] == "f16" and not case.get("big"):
        d = T.mix_data(case, "int")
        assert bool((T.f16(d["x"]) == d["x"]).all()) and bool((T.f16(d["W"]) == d["W"]).all())
    if case["fam"] in ("thin", "mixwg"):
        assert case["gauss"] == (case["K"] <= T.KMAX_GAUSS)
    assert case["K"] <= T.KMAX_GAUSS or case["fam"] in ("thin", "mixwg")


def test_gaussian_bound_is_tighter_than_a_dropped_product():
    """Where the bound is applied, (K + c) u S stays below S / (4 K): K^2 u <= 1/4."""
    for c in QUERIED + T.MIX_CASES:
        if c.get("rc", 0) == 0 and c["gauss"] and c["K"] <= T.KMAX_GAUSS:
            assert (c["K"] + 16) * T.U24 * c["K"] <= 0.26, c["name"]


def test_restatements_agree():
    """The block-wise restatement of the thin kernel (the carrier of the mapping defect) equals the plain reference."""
    H = _H()
    for name in ("t_ch8_dyc4_few", "t_walk_in_images", "t_ch32_dyc2_walk_g15", "t_ch8_dyc2_p4"):
        c = T.THIN_BY_NAME[name]
        d = T.thin_data(c, "int")
        ref, _ = T.thin_ref(c, d)
        blk, _ = T.thin_ref(c, d, fault=("map",), plan=dict(T.thin_plan(H, c), P=7))     # P = 7: the plain mapping either way
        assert bool((blk == ref).all()), name


# ---------------------------------------------------------------------------------------------------------------------------------
# defects: each is applied to the fp64 restatement and must break integer equality in the cases it names, and only there
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL_X = [c for c in T.C1X2_CASES if c["B"] <= 16 and c["hw"] != (128, 128)]


def _differs(a, b):
    return not bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_defect_d1_not_zeroed_outside_the_image():
    """Every case: all have tiles whose ring leaves the image (named: the *_plus1_xcd_uneven and *_h1w1 geometry cases and
    x_cg1_cq2_xcd_uneven)."""
    for c in SMALL_X + [T.C1X2_BY_NAME["x_cg1_cq2_xcd_uneven"]]:
        d = T.fwd_data(c, "int")
        ref, _ = T.c1x2_ref(c, d)
        bad, _ = T.c1x2_ref(c, d, fault=("ring",))
        assert _differs(bad[..., 1], ref[..., 1]) and not _differs(bad[..., 0], ref[..., 0]), c["name"]


def test_defect_one_lane_of_a_pixel_dropped():
    """Lane CG - 1 of a pixel's CG lanes: breaks every CG = 2 / 4 case with a weighted channel quad q, q % CG == CG - 1, and no other
    (x_cg2_cin12_seg3: only the first quad carries weight)."""
    H = _H()
    hit, clean = [], []
    for c in SMALL_X + [T.C1X2_BY_NAME[n] for n in ("x_cg2_cq4_b512", "x_cg1_cq2_b1024")]:
        cg = T.c1x2_plan(H, c)["CG"]
        d = T.fwd_data(c, "int")
        ref, _ = T.c1x2_ref(c, d)
        bad, _ = T.c1x2_ref(c, d, fault=("lane", cg, cg - 1)) if cg > 1 else (ref, None)
        w_rows = T._w_params(c)[0]
        expect = cg > 1 and any((ch // 4) % cg == cg - 1 for ch in range(min(w_rows, c["cin"])))
        assert _differs(bad, ref) == expect, c["name"]
        (hit if expect else clean).append(c["name"])
    assert "x_cg2_cq4_b512" in hit and "x_cg4_cin64_norelu" in hit and "x_cg2_cin12_seg3" in clean and "x_cg1_cq2_b1024" in clean


def test_defect_last_quad_of_the_second_chunk_dropped():
    """Channels Cpad - 4 .. of a two-chunk plan: breaks the two-chunk cases of c1x2 and c1_fwd whose last quad carries weight."""
    H = _H()
    for c in SMALL_X + [T.C1X2_BY_NAME["x_cg1_chunks2_cin36"], T.C1X2_BY_NAME["x_cg2_chunks2_cin36"]] + T.C1_CASES:
        x2 = c["fam"] == "c1x2"
        p = T.c1x2_plan(H, c) if x2 else T.c1_plan(H, c)
        c0 = ((c["cin"] + 3) & ~3) - 4 if p["nchunks"] >= 2 else 10000
        d = T.fwd_data(c, "int") if x2 else T.c1_data(c, "int")
        ref = (T.c1x2_ref if x2 else T.c1_ref)(c, d)[0]
        bad = (T.c1x2_ref if x2 else T.c1_ref)(c, d, fault=("quad", c0))[0]
        w_rows = (T._w_params(c) if x2 else T._c1_params(c))[0]
        assert _differs(bad, ref) == (p["nchunks"] >= 2 and c0 < w_rows), c["name"]
    assert T._c1_params(T.C1_BY_NAME["c_cin44_rows36"])[0] == 36        # its last quad carries no weight: not broken


def test_defect_thin_group_index_with_the_wrong_mapping():
    """The group from the plain block mapping, the partition from the XCD-aware one: breaks the xcd cases whose G shares a factor with 8
    (t_ch*_dyc4_few, t_walk_in_images: G = 2), no other - at G = 15 the mixed mapping is still one-to-one."""
    import math
    H = _H()
    for c in T.THIN_CASES:
        if c["rc"] or c["K"] > 2000:
            continue
        p = T.thin_plan(H, c)
        d = T.thin_data(c, "int")
        ref, _ = T.thin_ref(c, d)
        bad, _ = T.thin_ref(c, d, fault=("map",), plan=p)
        assert _differs(bad, ref) == (p["xcd"] == 1 and math.gcd(c["G"], 8) > 1), c["name"]


def test_defect_compact_dy_pair_not_zero_extended():
    """z / w of a compact pair taken from the bytes behind it: breaks rows 2, 3 of every dyc = 2 case with two groups or more."""
    for c in T.THIN_CASES:
        if c["rc"] or c["K"] > 1500:
            continue
        d = T.thin_data(c, "int")
        ref, _ = T.thin_ref(c, d)
        bad, _ = T.thin_ref(c, d, fault=("zw",))
        assert _differs(bad[:, 2:], ref[:, 2:]) == (c["dyc"] == 2 and c["G"] > 1), c["name"]
        assert not _differs(bad[:, :2], ref[:, :2])


def test_defect_ragged_pixels_of_the_last_partition_dropped():
    H = _H()
    hit = []
    for c in T.MIXWG_CASES:
        if c["rc"]:
            continue
        p = T.mixwg_plan(H, c)
        d = T.mixwg_data(c, "int")
        ref = T.mixwg_ref(c, d)
        bad = T.mixwg_ref(c, d, fault=("ragged",), plan=p)
        p0 = (c["npix"] - 1) // p["per"] * p["per"]
        expect = (c["npix"] - p0) % 4 != 0
        assert _differs(bad[0], ref[0]) == expect and _differs(bad[2], ref[2]) == expect, c["name"]
        if expect:
            hit.append(c["name"])
    assert {"m16_p4_last1", "m16_p4_last2_pair", "m32_p8_last3_pair", "m32_p8_last1", "m16_p1_px511_pair"} <= set(hit)
    assert "m16_g15_p2" not in hit


def test_defect_second_dy_half_at_the_first_halfs_stride():
    """Applies where dy is a pair (the halves' pixel strides differ by test_thin_kernels.PAIR_STRIDES): breaks every such case."""
    for c in T.MIXWG_CASES:
        if c["rc"] or "pair" not in c["sw"]:
            continue
        d = T.mixwg_data(c, "int")
        ref = T.mixwg_ref(c, d)
        s1, s2 = T.PAIR_STRIDES(c["C"])
        bad = T.mixwg_ref(c, d, fault=("stride", s1, s2))
        assert _differs(bad[0], ref[0]) and (c["npix"] == 1 or _differs(bad[2], ref[2])), c["name"]
        h = c["C"] // 2
        assert not _differs(bad[0][:, :h], ref[0][:, :h])


def test_defect_second_round_of_a_looping_block_dropped():
    """Breaks the four grid-cap cases (the only ones whose blocks loop), no other."""
    for c in T.MIX_CASES:
        if c["rc"]:
            continue
        if c.get("big"):
            assert c["rounds"] == 2 and c["grid"] == T.GRID_CAP
            n2 = c["npix"] - 64 * c["NP"] * c["grid"]          # pixels of the second round
            assert 0 < n2 <= 64 * c["NP"] + 37
            continue
        d = T.mix_data(c, "int")
        ref, _ = T.mix_ref(c, d)
        bad, _ = T.mix_ref(c, d, fault=("round", c["grid"], c["NP"]))
        assert c["rounds"] == 1 and not _differs(bad, ref), c["name"]
    c = dict(T.MIX_BY_NAME["mx_f32_cap_np1_c68"])
    d = T.mix_data(c, "int")
    ref, _ = T.mix_ref(c, d)
    bad, _ = T.mix_ref(c, d, fault=("round", c["grid"], c["NP"]))
    changed = (bad != ref).any(1)
    assert int(changed.sum()) == c["npix"] - 64 * c["grid"] and bool(changed[64 * c["grid"]:].all())
