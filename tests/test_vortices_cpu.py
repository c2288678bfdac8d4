"""CPU-side checks of the ensemble vortex census: the kernel entries are declared in their own header, listed apart and exported;
the signatures of the three Python layers; the plan query's values and the codes the entries return before any launch; every
argument error without a GPU; the float32 mirror of tests/vortex_cases.py against its fp64 restatement inside the counted bound;
the reference labeller against scipy where it is installed; the known answers on the mirror; the identities of the finalize
restatement and tmg_ops.vortex_finalize against it; and the sensitivity of the measure: every named mutation is caught."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import pdf_cases as P
import vortex_cases as K

NAMES = ["tmg_ens_vortex_plan", "tmg_ens_vortex_classify", "tmg_ens_vortex_label", "tmg_ens_vortex_census"]
c_i64 = ctypes.c_int64
F32 = np.float32


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_vortex.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.VORTEX_EXPORTS == NAMES
    assert "vortex" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_vortex.hip" in tmg_hip.SOURCES and "tmg_vortex.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_vortex.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_vortex\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_vortex.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in src
    # integer atomics only, no inline assembly, nothing printed or asserted in a kernel, no block waits on another
    assert not re.search(r"\basm\b|printf|assert\s*\(|atomicAdd\s*\(\s*\(?\s*float|atomicExch|atomicCAS|while\s*\(", code)
    # every access to the label plane inside the merge and root kernels is an agent-scope atomic
    merge = code[code.index("ens_vortex_merge_kernel"):code.index("extern \"C\" int tmg_ens_vortex_label")]
    assert not re.search(r"\blabel\s*\[|\blab\s*\[", merge) and merge.count("__HIP_MEMORY_SCOPE_AGENT") >= 3


def test_signatures():
    from utils import utils
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredVortices).parameters
    new = ["threshold", "qscale", "min_area", "max_vortices", "circ_bins", "circ_range", "per_member"]
    assert list(sig) == old + new
    assert [sig[n].default for n in new] == [None, None, 4, 64, 16, None, False]
    init = inspect.signature(tmg_ops.EnsembleVortices.__init__).parameters
    assert list(init)[:10] == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std"]
    assert set(list(init)[10:]) == {"u", "grid"} | set(new)
    assert issubclass(tmg_ops.EnsembleVortices, tmg_ops.EnsembleFeed)
    doc = utils.modelPredVortices.__doc__
    for word in ("8-connectivity", "tracking", "lambda-2", "pixel boxes", "256 vortices", "periodic", "512 per side"):
        assert word in doc, word


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,S,B,hw,Kk,Tn", [(1, 1, 1, (3, 3), 1, 1), (4, 8, 2, (40, 72), 64, 3), (5, 1024, 1, (33, 65), 256, 2),
                                            (2, 5, 3, (512, 512), 16, 41), (64, 64, 1, (64, 32), 64, 1)])
def test_plan_values(k, S, B, hw, Kk, Tn):
    import tmg_hip
    p = tmg_hip.ens_vortex_plan(k, S, B, hw[0], hw[1], Kk, Tn)
    TH, TW, thr = p["TH"], p["TW"], p["threads"]
    HW = hw[0] * hw[1]
    assert (TH, TW, thr) == (32, 32, 256)
    assert p["NTH"] == -(-hw[0] // TH) and p["NTW"] == -(-hw[1] // TW) and p["tile_blocks"] == p["NTH"] * p["NTW"]
    pairs = (p["NTW"] - 1) * hw[0] + (p["NTH"] - 1) * hw[1]
    assert p["merge_blocks"] == -(-pairs // thr) and p["pixel_blocks"] == -(-HW // thr)
    assert p["lds_label"] == 5 * TH * TW and p["lds_census"] == max(64 * Kk, 4 * 1024 + 16) and p["lds_census"] <= 65536
    assert p["ws_bytes"] == 17 * k * B * HW                                  # 9 bytes per pixel plus the area and the slot planes
    assert p["state_bytes"] == 64 * Kk * (S + 1) * B * Tn + 2 * 8 * B * HW


def test_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    plan = (c_i64 * 12)()
    good = [2, 5, 2, 8, 9, 64, 3]
    assert lib.tmg_ens_vortex_plan(_i64(*good), plan) == 0
    for pos, bad in ((0, 0), (0, 7), (1, 0), (2, 0), (3, 2), (4, 2), (5, 0), (5, 257), (6, 0)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_vortex_plan(_i64(*d), plan) == -1, (pos, bad)
    for pos, bad in ((1, 1025), (3, 513), (4, 513)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_vortex_plan(_i64(*d), plan) == -2, (pos, bad)
    assert lib.tmg_ens_vortex_plan(_i64(1025, 1024, 64, 8, 9, 64, 3), plan) == -2    # k B > 65535
    assert lib.tmg_ens_vortex_plan(None, plan) == -3 and lib.tmg_ens_vortex_plan(_i64(*good), None) == -3
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                                  # never dereferenced: every code comes before a launch
    fl = (ctypes.c_float * 2)(0.5, 0.25)
    cl = lambda dims, td=(3, 0), f=fl, rows=one: lib.tmg_ens_vortex_classify(rows, _i64(*td), nul, one, one, one, one, one, one, one, f,  # noqa: E731
                                                                             _i64(*dims), nul)
    assert cl((0, 1, 8, 9, 3)) == -1 and cl((1, 1, 2, 9, 3)) == -1 and cl((1, 1, 8, 9, 5)) == -1 and cl((1, 1, 8, 9, 3), td=(2, 0)) == -1
    assert cl((1, 1, 8, 9, 3), f=(ctypes.c_float * 2)(0.0, 1.0)) == -1 and cl((1, 1, 8, 9, 3), f=(ctypes.c_float * 2)(1.0, float("nan"))) == -1
    assert cl((1, 1, 513, 9, 3)) == -2 and cl((1, 1, 8, 9, 3), rows=nul) == -3
    lb = lambda dims, c=one, s=one: lib.tmg_ens_vortex_label(c, one, s, _i64(*dims), nul)   # noqa: E731
    assert lb((0, 5, 7)) == -1 and lb((1, 0, 7)) == -1 and lb((1, 5, 513)) == -2 and lb((65536, 5, 7)) == -2
    assert lb((1, 5, 7), c=nul) == -3 and lb((1, 5, 7), s=nul) == -3
    cs = lambda dims, t=one: lib.tmg_ens_vortex_census(one, one, one, one, one, one, t, one, one, _i64(*dims), nul)   # noqa: E731
    assert cs((1, 1, 8, 9, 64, 0)) == -1 and cs((1, 1, 8, 9, 257, 4)) == -1 and cs((1, 1, 2, 9, 64, 4)) == -1
    assert cs((1, 1, 513, 9, 64, 4)) == -2 and cs((1, 1, 8, 9, 64, 4), t=nul) == -3


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_vortex_args_errors_and_defaults():
    import tmg_ops as ops
    ok = dict(threshold=0.5, qscale=1024.0, min_area=4, max_vortices=64, circ_bins=16, circ_range=None, C=3, Hh=24, Ww=40, grid=(0.5, 0.25))
    thr, qs, ma, Kk, nb, cr, dx, dy = ops.vortex_args(B=2, **ok)
    assert thr.tolist() == [0.5, 0.5] and qs.tolist() == [1024.0, 1024.0] and (ma, Kk, nb, cr, dx, dy) == (4, 64, 16, None, 0.5, 0.25)
    assert ops.vortex_args(B=2, **dict(ok, threshold=None, qscale=None))[:2] == (None, None)
    assert ops.vortex_args(B=2, **dict(ok, circ_range=(0.0, 2.0)))[5].tolist() == [[0.0, 2.0], [0.0, 2.0]]
    assert ops.vortex_args(B=2, **dict(ok, threshold=[0.0, 1.0], qscale=[2.0 ** -3, 2.0 ** 30]))[0].tolist() == [0.0, 1.0]
    bad = [dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=[0.5, 0.5, 0.5]), dict(threshold="x"), dict(qscale=3.0),
           dict(qscale=0.0), dict(qscale=-2.0), dict(qscale=float("inf")), dict(qscale=[2.0]), dict(min_area=0), dict(min_area=1.5),
           dict(min_area=True), dict(max_vortices=0), dict(max_vortices=257), dict(max_vortices=8.0), dict(circ_bins=0), dict(circ_bins=33),
           dict(circ_range=(1.0, 1.0)), dict(circ_range=(-1.0, 1.0)), dict(circ_range=(0.0, float("inf"))), dict(circ_range=(0.0, 1.0, 2.0)),
           dict(C=1), dict(C=5), dict(Hh=2), dict(Ww=513), dict(grid=(0.0, 1.0)), dict(grid=(1.0,)), dict(grid=1.0), dict(grid=(1.0, float("nan")))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.vortex_args(B=2, **dict(ok, **kw))
    # H = W = None: the field's limits are skipped (modelPredVortices checks before the field is known)
    assert ops.vortex_args(None, None, 1, 256, 32, None, 3, None, None, (1.0, 1.0))[2:5] == (1, 256, 32)
    # the accumulator's own errors come before any device work: it is refused here although no GPU exists
    kw = dict(members=2, B=2, C=3, Hh=24, Ww=40, steps=2, device="cuda", out_mu=[0.0] * 3, out_std=[1.0] * 3)
    for extra in (dict(threshold=None, qscale=2.0), dict(threshold=0.1, qscale=None), dict(threshold=0.1, qscale=3.0),
                  dict(threshold=0.1, qscale=2.0, min_area=0), dict(threshold=0.1, qscale=2.0, members=1025)):
        with pytest.raises(ValueError):
            ops.EnsembleVortices(**dict(kw, **extra))
    with pytest.raises(ValueError, match="does not vary"):
        ops.vortex_defaults(torch.ones(1, 2, 3, 8, 9), (1.0, 1.0))


def test_vortex_defaults_match_the_restatement():
    import tmg_ops as ops
    xs, sd, mu, u = K.real_inputs(1, 2, (24, 40), 3, 5)
    tp = P.physical(xs[:, 1], mu, sd, u, np.float64).transpose(1, 0, 2, 3, 4)
    thr, qs = ops.vortex_defaults(torch.from_numpy(tp), K.GRID)
    rthr, rqs = K.defaults(tp, K.GRID)
    assert np.allclose(thr.numpy(), rthr, rtol=1e-12, atol=0) and np.array_equal(qs.numpy(), rqs)
    frac, _ = np.frexp(qs.numpy())
    assert (frac == 0.5).all()


# ---- the mirror -------------------------------------------------------------------------------------------------------------------------
REAL = [(1, 2, (24, 40), 3, 5), (3, 1, (33, 65), 3, 6), (2, 2, (40, 72), 2, 7)]


@pytest.mark.parametrize("S,B,hw,steps,seed", REAL)
def test_mirror_against_fp64_inside_the_counted_bound(S, B, hw, steps, seed):
    """The vorticity is pdf_cases.derived's bit for bit; against fp64 the class differs only where the fp64 ow lies within the counted
    bound of the threshold, and at most NEAR_CAP of the interior pixels lie there (checked here for the seeds the GPU test uses)."""
    xs, sd, mu, u = K.real_inputs(S, B, hw, steps, seed)
    thr, qs = K.real_defaults(xs, sd, mu, u, K.GRID, range(steps))
    m = K.classify(xs, mu, sd, u, K.GRID, thr, qs, F32)
    d = K.classify(xs, mu, sd, u, K.GRID, F32(thr).astype(np.float64), qs, np.float64)
    assert np.array_equal(m["om"], P.derived(xs, mu, sd, u, K.GRID, F32)[1])
    near = np.abs(d["ow"] - F32(thr).astype(np.float64).reshape(B, 1, 1)) <= K.near_bound(xs, mu, sd, u, K.GRID)
    assert not ((m["cls"] != d["cls"]) & ~near).any()
    assert np.abs(m["ow"].astype(np.float64) - d["ow"]).max() <= K.near_bound(xs, mu, sd, u, K.GRID).max()
    assert (np.abs(m["ow"].astype(np.float64) - d["ow"]) <= K.near_bound(xs, mu, sd, u, K.GRID)).all()
    share = near[..., 1:-1, 1:-1].mean()
    assert share <= K.NEAR_CAP, share
    assert (m["cls"] == 1).any() and (m["cls"] == -1).any() and not m["rej"].any()


def test_reference_labeller_against_scipy_and_its_own_properties():
    have = K.scipy_label(np.zeros((3, 3), np.int8)) is not None
    for hw in K.mask_shapes(32, 32) + [(64, 64)]:
        for name, m in K.masks(hw, 32, 32).items():
            lab = K.label(m)
            assert ((lab >= 0) == (m != 0)).all(), name
            on = lab >= 0
            assert (lab[on] <= np.arange(m.size).reshape(hw)[on]).all(), name
            roots = np.unique(lab[on])
            assert (lab.reshape(-1)[roots] == roots).all(), name
            if have:
                assert np.array_equal(lab, K.scipy_label(m)), (name, hw)
    m = K.masks((9, 11), 32, 32)
    assert len(np.unique(K.label(m["checkerboard"]))) - 1 == (9 * 11) // 2
    assert len(np.unique(K.label(m["all_one"]))) == 1 and len(np.unique(K.label(m["serpentine"]))) - 1 == 1
    assert len(np.unique(K.label(m["diagonal_touch"]))) - 1 == 2 and len(np.unique(K.label(m["opposite_signs_on_border"]))) - 1 == 2


def _known(i):
    hw, vort, noise, counts, areas = K.KNOWN[i]
    x = K.gauss_field(hw, vort, noise)[None]                                  # [B = 1, 3, H, W]
    thr, qs = K.defaults(x[None].astype(np.float64).transpose(1, 0, 2, 3, 4), (1.0, 1.0))
    return hw, vort, counts, areas, x, thr, qs


@pytest.mark.parametrize("i", range(len(K.KNOWN)))
def test_known_answers_on_the_mirror(i):
    hw, vort, counts, areas, x, thr, qs = _known(i)
    r = K.classify(x, [0, 0, 0], [1, 1, 1], None, (1.0, 1.0), thr, qs, F32)
    lab = K.label(r["cls"][0])
    table, found, _ = K.census(lab, r["cls"][0], r["om"][0], float(qs[0]), 64, 4)
    assert tuple(found) == counts
    kept = table[table[:, 0] >= 0]
    assert tuple(kept[kept[:, 4] > 0, 1]) == areas[0] and tuple(kept[kept[:, 4] < 0, 1]) == areas[1]
    for row in kept:
        cx, cy = row[5] / row[4], row[6] / row[4]
        assert min(np.hypot(cx - v[1], cy - v[0]) for v in vort if (v[2] > 0) == (row[4] > 0)) <= 0.5
    if K.scipy_label(r["cls"][0]) is not None:
        assert np.array_equal(lab, K.scipy_label(r["cls"][0]))


# ---- finalize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,hw,steps,seed", REAL)
@pytest.mark.parametrize("circ_range", [None, (0.5, 6.0)])
def test_finalize_identities_and_the_torch_finalize(S, B, hw, steps, seed, circ_range):
    import tmg_ops as ops
    xs, sd, mu, u = K.real_inputs(S, B, hw, steps, seed)
    thr, qs = K.real_defaults(xs, sd, mu, u, K.GRID, range(steps))
    Kk, nb = 6, 5
    ref = K.reference(xs, mu, sd, u, K.GRID, thr, qs, Kk, 4, range(steps))
    f = K.finalize(ref["table"], ref["found"], ref["core"], S, hw, K.GRID, qs, nb, circ_range, steps)
    K.check_identities(f, ref["table"], ref["found"], S, hw, Kk, "case %d" % seed)
    assert (ref["found"].sum(-1) > 0).all() and np.isfinite(f["match_dist_mean"]).any()
    cr = None if circ_range is None else torch.tensor([circ_range] * B, dtype=torch.float64)
    got = ops.vortex_finalize(torch.from_numpy(ref["table"]), torch.from_numpy(ref["found"]), S, hw[0], hw[1], K.GRID[0], K.GRID[1],
                              torch.from_numpy(np.asarray(qs, np.float64)), nb, cr)
    g = {k: v.numpy() for k, v in got.items()}
    assert np.array_equal(g["area_hist"], f["area_hist"]) and np.array_equal(g["circ_hist"], f["circ_hist"])
    K.check_floats(g, f, "torch finalize", keys=[k for k in K.FLOAT_KEYS if k not in ("core_prob", "target_core_freq")] + ["vortex_circ_edges"])


def test_members_equal_to_the_target_match_it_exactly():
    xs, sd, mu, u = K.real_inputs(3, 2, (24, 40), 2, 11)
    xs = np.repeat(xs[:, 3:], 4, axis=1)
    thr, qs = K.real_defaults(xs, sd, mu, u, K.GRID, range(2))
    ref = K.reference(xs, mu, sd, u, K.GRID, thr, qs, 8, 4, range(2))
    f = K.finalize(ref["table"], ref["found"], ref["core"], 3, (24, 40), K.GRID, qs, 8, None, 2)
    for key in ("match_dist_mean", "match_miss_frac", "time_area_w1", "time_circ_w1", "count_std"):
        assert np.nanmax(np.abs(f[key])) == 0 and np.isfinite(f[key]).any(), key


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
def test_every_mutation_is_caught_by_the_check_meant_for_it():
    """conn8 / nosign: labels of the diagonal-touch and the opposite-sign masks; ge: a pixel whose ow equals the threshold; frame: a
    field whose criterion holds on the frame; area_after: small components ahead of a large one with K = 2."""
    m = K.masks((40, 72), 32, 32)
    assert not np.array_equal(K.label(m["diagonal_touch"]), K.label(m["diagonal_touch"], "conn8"))
    assert np.array_equal(K.label(m["opposite_signs_on_border"]), K.label(m["opposite_signs_on_border"], "conn8"))
    assert not np.array_equal(K.label(m["opposite_signs_on_border"]), K.label(m["opposite_signs_on_border"], "nosign"))
    assert not np.array_equal(K.label(m["sign_stripes"]), K.label(m["sign_stripes"], "nosign"))
    xs = K.int_inputs(0, 1, (9, 11), 1, 3)
    base = K.classify(xs[0], [0, 0, 0], [1, 1, 1], None, (1.0, 1.0), [0.0], [8.0], F32)
    val = np.unique(base["ow"][0, 0, 1:-1, 1:-1])
    val = val[val > 0]
    a = K.classify(xs[0], [0, 0, 0], [1, 1, 1], None, (1.0, 1.0), [val[0]], [8.0], F32)
    assert not np.array_equal(a["cls"], K.classify(xs[0], [0, 0, 0], [1, 1, 1], None, (1.0, 1.0), [val[0]], [8.0], F32, "ge")["cls"])
    assert not np.array_equal(base["cls"], K.classify(xs[0], [0, 0, 0], [1, 1, 1], None, (1.0, 1.0), [0.0], [8.0], F32, "frame")["cls"])
    cls = np.zeros((8, 12), np.int8)
    cls[1, 1] = cls[1, 3] = cls[1, 5] = 1                                    # three single pixels, then a 2 x 3 block
    cls[4:6, 2:5] = 1
    om = np.where(cls != 0, F32(1.0), F32(0.0))
    lab = K.label(cls)
    good, bad = K.census(lab, cls, om, 8.0, 2, 4), K.census(lab, cls, om, 8.0, 2, 4, "area_after")
    assert good[0][0, 0] == 4 * 12 + 2 and good[0][0, 1] == 6 and tuple(good[1]) == (1, 0)
    assert not np.array_equal(good[0], bad[0])
    for mut in K.MUTATIONS:                                                  # and on a whole reference: every mutation moves an integer
        xi = K.int_inputs(2, 1, (33, 35), 2, 17)
        r0 = K.reference(xi, None, None, None, (1.0, 1.0), [1.0], [8.0], 4, 2, range(2))
        r1 = K.reference(xi, None, None, None, (1.0, 1.0), [1.0], [8.0], 4, 2, range(2), mut)
        assert any(not np.array_equal(r0[k], r1[k]) for k in ("table", "found", "core")), mut


def test_integer_data_is_exact_in_the_mirror():
    xi = K.int_inputs(1, 2, (9, 11), 2, 5)
    a = K.classify(xi, None, None, None, (1.0, 1.0), [1.0, 2.0], [8.0, 8.0], F32)
    d = K.classify(xi, None, None, None, (1.0, 1.0), [1.0, 2.0], [8.0, 8.0], np.float64)
    assert np.array_equal(a["om"].astype(np.float64), d["om"]) and np.array_equal(a["cls"], d["cls"])
    assert np.array_equal(a["qf"], np.rint(a["qf"]))
