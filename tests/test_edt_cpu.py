"""CPU-side checks of the distance-map verification: the kernel entries are declared in their own header, listed apart and exported;
the signatures of the three Python layers; the plan query's values and the codes the entries return before any launch; every argument
error without a GPU; the reference of tests/edt_cases.py against its second statements (the all-pairs minimum, and scipy's transform
where it imports); the integer square root fix-up of the kernels against math.isqrt; tmg_ops.dist_outputs against independently
written fp64 formulas, with every NaN, inf and empty-set convention; hand cases; and the sensitivity of the comparison the GPU test
uses: every named mutation that can change an output is caught, and the two that cannot are shown to change none."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import common as C
import edt_cases as K

NAMES = ["tmg_ens_edt_plan", "tmg_ens_edt_chunk", "tmg_ens_edt_step", "tmg_ens_edt_fixed"]
c_i64 = ctypes.c_int64
P64 = ctypes.POINTER(c_i64)
vp = ctypes.c_void_p


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    hdr = open(os.path.join(inc, "tmglow_hip_edt.h")).read()
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", hdr)
    assert decl == [("int", n) for n in NAMES] and tmg_hip.EDT_EXPORTS == NAMES
    assert "edt" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    want = {"tmg_ens_edt_plan": [P64, P64], "tmg_ens_edt_chunk": [vp, P64, vp, P64, vp, P64, vp, vp, vp, vp, vp, vp, P64, vp],
            "tmg_ens_edt_step": [vp, vp, vp, vp, P64, vp], "tmg_ens_edt_fixed": [P64, c_i64, c_i64, P64]}
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.EDT_ARGTYPES[name] == want[name]
        # the header's parameter list, read as ctypes: a pointer to int64_t, an int64_t by value, any other pointer, the stream
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        kinds = [P64 if "int64_t*" in q.replace(" *", "*") else c_i64 if "int64_t" in q else vp for q in params]
        assert kinds == want[name], name
    assert "tmg_edt.hip" in tmg_hip.SOURCES and "tmg_edt.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_edt.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_edt\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    code = re.sub(r"//[^\n]*", "", open(os.path.join(tmg_hip.CSRC, "tmg_edt.hip")).read())
    # integer outputs only: no float atomics, no inline assembly, nothing printed or asserted in a kernel, no memset
    assert not re.search(r"\basm\b|printf|assert\s*\(|atomicAdd\s*\(\s*\(float|double|hipMemset", code)


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredDistance).parameters
    assert list(sig) == old + ["events", "cutoff", "quantiles"]
    assert sig["events"].default == ((0, 0.0, "<"),) and sig["cutoff"].default is None and sig["quantiles"].default == (0.5, 0.75, 0.9)
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleDistance.__init__).parameters
    isc = list(inspect.signature(tmg_ops.EnsembleIntensityScale.__init__).parameters)
    assert list(init) == isc[:isc.index("events") + 1] + ["cutoff", "quantiles"]
    assert init["events"].default == ((0, 0.0, "<"),) and init["cutoff"].default is None and init["u"].default is None
    assert list(inspect.signature(tmg_ops.EnsembleDistance.add).parameters) == ["self", "y", "m0", "target", "time"]
    assert issubclass(tmg_ops.EnsembleDistance, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.dist_args).parameters) == ["events", "cutoff", "quantiles", "C", "H", "W"]
    out = inspect.signature(tmg_ops.dist_outputs).parameters
    assert list(out) == ["pair_raw", "hist_raw", "S", "H", "W", "cutoff", "quantiles", "steps"] and out["steps"].default == 1
    plan = inspect.signature(tmg_hip.ens_edt_plan).parameters
    assert list(plan) == ["S", "B", "H", "W", "K", "c", "code"] and plan["code"].default is False
    assert inspect.signature(tmg_hip.ens_edt_chunk).parameters["code"].default is False
    assert inspect.signature(tmg_hip.ens_edt_step).parameters["code"].default is False
    assert "8 (S + 1) B K H ceil(W / 64)" in tmg_ops.EnsembleDistance.__doc__   # the device memory is stated
    for doc in (utils.modelPredDistance.__doc__, tmg_ops.EnsembleDistance.__doc__):
        for word in ("Not supported", "anisotropic", "periodic", "Pratt", "1 / 256 pixel", "not a mean of ratios"):
            assert word in doc, word
    assert tmg_ops.DIST_PAIR == K.PAIR and tmg_ops.DIST_SUMMARY == K.SUMMARY and tmg_ops.DIST_FLOAT_KEYS == K.FLOAT_KEYS
    assert tmg_ops.DIST_INF == K.INF == 2 ** 30


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,Hh,Ww,Kk,c", [(1, 1, 1, 1, 1, 1), (5, 2, 3, 130, 2, 5), (2, 3, 64, 64, 1, 255), (5, 2, 65, 63, 4, 1),
                                            (16, 4, 256, 256, 1, 64), (1024, 65535, 4096, 4096, 4, 255)])
def test_plan_values(S, B, Hh, Ww, Kk, c):
    import tmg_hip
    p = tmg_hip.ens_edt_plan(S, B, Hh, Ww, Kk, c)
    sx, by = -(-Ww // 64), -(-Hh // 64)
    assert (p["band"], p["tile_w"]) == K.TILE == (64, 64) and p["threads"] == 256 and (p["strips"], p["bands"]) == (sx, by)
    assert p["grid"] == (sx * by * Kk, S, B) and p["blocks"] == sx * by * Kk * S * B
    # a source tile of 64 x 64 row distances as uint16, two int32 histograms of 256 bins, nine 64-bit sums, two int32 maxima, and the
    # tile's 64 rows of indicator words
    assert p["lds_bytes"] == 2 * 64 * 64 + 4 * 2 * 256 + 8 * 9 + 4 * 2 + 8 * 64 * sx <= 64 * 1024
    assert p["mask_grid_x"] == -(-(Hh * sx) // 4)
    assert p["scratch_words"] == (S + 1) * B * Kk * Hh * sx and p["pair_words"] == 11 * B * Kk * S
    assert p["hist_words"] == 2 * (c + 1) * B * Kk * S and p["count_words"] == B * Kk * (S + 1) and p["map_words"] == B * Kk * Hh * Ww


def test_plan_codes():
    import tmg_hip
    code = lambda *a: tmg_hip.ens_edt_plan(*a, code=True)[1]                  # noqa: E731
    assert code(1, 1, 1, 1, 1, 1) == 0 and code(1024, 65535, 4096, 4096, 4, 255) == 0
    for bad in ((0, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 5, 1),
                (1, 1, 1, 1, 1, 0), (1, 1, 1, 1, 1, 256), (1025, 1, 1, 1, 5, 1)):
        assert code(*bad) == -1, bad
    for big in ((1025, 1, 1, 1, 1, 1), (1, 65536, 1, 1, 1, 1), (1, 1, 4097, 1, 1, 1), (1, 1, 1, 4097, 1, 1)):
        assert code(*big) == -2, big
    lib = tmg_hip.lib()
    assert lib.tmg_ens_edt_plan(None, _i64(*[0] * 16)) == -3 and lib.tmg_ens_edt_plan(_i64(1, 1, 1, 1, 1, 1), None) == -3
    assert lib.tmg_ens_edt_plan(_i64(0, 1, 1, 1, 1, 1), None) == -1            # the limits come first
    with pytest.raises(RuntimeError, match="tmg_ens_edt_plan failed with code -1"):
        tmg_hip.ens_edt_plan(1, 1, 1, 1, 1, 0)


def test_every_code_of_the_launching_entries_comes_before_a_launch():
    """No device here: an entry that got as far as a launch would fail differently.  Dummy non-null pointers are never read."""
    import tmg_hip
    lib = tmg_hip.lib()
    p, nul = vp(64), vp(0)
    yd = _i64(3, 0)
    ev = _i64(0, 0, 2, 1)
    good = [2, 2, 5, 7, 3, 3, 0, 2, 5]                                        # k, B, H, W, C, S, m0, K, c

    def chunk(dims=good, y=p, y_d=yd, tg=p, t_d=yd, thr=p, evs=ev, bufs=(p,) * 6):
        return lib.tmg_ens_edt_chunk(y, y_d, tg, t_d, thr, evs, *bufs, _i64(*dims), nul)
    edit = lambda i, v: [v if j == i else x for j, x in enumerate(good)]      # noqa: E731
    for dims in (edit(4, 1), edit(4, 5), edit(0, 0), edit(6, -1), edit(6, 2), edit(5, 0), edit(7, 0), edit(7, 5), edit(8, 0), edit(8, 256),
                 edit(1, 0), edit(2, 0), edit(3, 0)):
        assert chunk(dims) == -1, dims
    assert chunk(y_d=_i64(2, 0)) == -1 and chunk(t_d=_i64(3, 1)) == -1 and chunk(y_d=_i64(4, -1)) == -1
    assert chunk(evs=_i64(0, 0, 3, 1)) == -1 and chunk(evs=_i64(0, 2, 1, 1)) == -1 and chunk(evs=_i64(-1, 0, 1, 1)) == -1
    assert chunk(edit(5, 1025)) == -2 and chunk(edit(1, 65536)) == -2 and chunk(edit(2, 4097)) == -2 and chunk(edit(3, 4097)) == -2
    assert chunk(y_d=_i64(2 ** 31, 0)) == -2
    assert lib.tmg_ens_edt_chunk(p, yd, p, yd, p, ev, p, p, p, p, p, p, None, nul) == -3
    assert chunk(y_d=None) == -3 and chunk(t_d=None) == -3 and chunk(evs=None) == -3
    assert chunk(y=nul) == -3 and chunk(tg=nul) == -3 and chunk(thr=nul) == -3
    for i in range(6):
        assert chunk(bufs=tuple(nul if j == i else p for j in range(6))) == -3, i
    assert chunk(edit(4, 1), y=nul) == -1 and chunk(edit(5, 1025), y=nul) == -2     # -1 before -2 before -3
    step = lambda dims, bufs=(p,) * 4: lib.tmg_ens_edt_step(*bufs, None if dims is None else _i64(*dims), nul)   # noqa: E731
    assert step(None) == -3 and step((0, 5, 7, 2, 5)) == -1 and step((2, 5, 7, 5, 5)) == -1 and step((2, 5, 7, 2, 256)) == -1
    assert step((65536, 5, 7, 2, 5)) == -2 and step((2, 4097, 7, 2, 5)) == -2
    for i in range(4):
        assert step((2, 5, 7, 2, 5), tuple(nul if j == i else p for j in range(4))) == -3, i
    assert lib.tmg_ens_edt_fixed(_i64(1), 1, 0, _i64(0)) == -1 and lib.tmg_ens_edt_fixed(_i64(1), 1, 256, _i64(0)) == -1
    assert lib.tmg_ens_edt_fixed(_i64(-1), 1, 5, _i64(0)) == -1 and lib.tmg_ens_edt_fixed(_i64(2 ** 30 + 1), 1, 5, _i64(0)) == -1
    assert lib.tmg_ens_edt_fixed(None, 1, 5, _i64(0)) == -3 and lib.tmg_ens_edt_fixed(_i64(1), 1, 5, None) == -3


# ---- the arguments ---------------------------------------------------------------------------------------------------------------------
def test_dist_args_errors_each_with_its_message():
    from tmg_ops import dist_args
    ev = ((0, 0.0, "<"),)
    assert dist_args(ev, None, (0.5,), 3, 64, 300) == ([(0, 0.0, "<")], 75, (0.5,))
    assert dist_args(ev, None, (0.5,), 3, 1, 3)[1] == 1 and dist_args(ev, None, (0.5,), 3, 4096, 7)[1] == 255
    assert dist_args(ev, 255, (1.0, 0.25), 3, 8, 8)[1:] == (255, (1.0, 0.25))
    for cut in (0, 256, -1, 2.0, True, "5"):
        with pytest.raises(ValueError, match=r"cutoff is an integer in 1\.\.255"):
            dist_args(ev, cut, (0.5,), 3, 8, 8)
    with pytest.raises(ValueError, match="cutoff=None needs H, W >= 1"):
        dist_args(ev, None, (0.5,), 3, 0, 8)
    with pytest.raises(ValueError, match="quantiles is a sequence"):
        dist_args(ev, 5, 0.5, 3, 8, 8)
    for ql in ((), (0.1,) * 9):
        with pytest.raises(ValueError, match="quantiles takes 1 to 8 probabilities"):
            dist_args(ev, 5, ql, 3, 8, 8)
    for q in (0.0, 1.5, -0.1, True, float("nan"), "a"):
        with pytest.raises(ValueError, match=r"quantiles are probabilities in \(0, 1\]"):
            dist_args(ev, 5, (0.5, q), 3, 8, 8)
    with pytest.raises(ValueError, match="events needs at least one entry"):
        dist_args((), 5, (0.5,), 3, 8, 8)
    for bad in (((3, 0.0, "<"),), ((0, 0.0, ">="),), ((0, float("inf"), "<"),), ((True, 0.0, "<"),)):
        with pytest.raises(ValueError, match="exceed entries are"):
            dist_args(bad, 5, (0.5,), 3, 8, 8)
    with pytest.raises(ValueError):
        dist_args(ev * 5, 5, (0.5,), 3, 8, 8)


def test_constructor_limits_come_before_the_device():
    import tmg_ops as ops
    mk = lambda S=2, B=2, Cc=3, Hh=8, Ww=8, T=2, **kw: ops.EnsembleDistance(S, B, Cc, Hh, Ww, T, kw.pop("device", "cpu"), torch.zeros(Cc),  # noqa: E731
                                                                            kw.pop("sd", torch.ones(Cc)), **kw)
    for kw, msg in ((dict(Cc=1), "2 <= C <= 4"), (dict(Cc=5), "2 <= C <= 4"), (dict(T=0), "steps >= 1"), (dict(T=True), "steps >= 1"),
                    (dict(B=0), "B, H, W >= 1"), (dict(Hh=0), "B, H, W >= 1"), (dict(S=0), "1 <= members <= 1024"),
                    (dict(S=1025), "1 <= members <= 1024"), (dict(B=65536), "at most 65535 cases"), (dict(Hh=4097), "H, W <= 4096"),
                    (dict(Ww=4097), "H, W <= 4096"), (dict(cutoff=0), "cutoff is an integer"), (dict(quantiles=(2.0,)), "probabilities in"),
                    (dict(events=((3, 0.0, "<"),)), "exceed entries are"), (dict(sd=torch.zeros(3)), "strictly positive"),
                    (dict(u=torch.zeros(2, 3)), "u must be finite")):
        with pytest.raises(ValueError, match=msg):
            mk(**kw)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        mk()


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", K.SHAPES)
def test_the_reference_agrees_with_its_second_statements(hw):
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    try:
        import scipy  # noqa: F401
        third = True
    except ImportError:
        third = False
    for d in K.DENSITIES:
        m = rng.random(hw) < d
        a = K.edt2(m)
        assert a.dtype == np.int64 and np.array_equal(a, K.edt2_all_pairs(m)), (hw, d)
        assert bool((a == K.INF).all()) == (not m.any()) and (m.any() or True)
        if third:
            assert np.array_equal(a, K.edt2_scipy(m)), (hw, d)
    one = np.zeros(hw, bool)
    one[-1, -1] = True                                                        # the far diagonal
    assert K.edt2(one)[0, 0] == (hw[0] - 1) ** 2 + (hw[1] - 1) ** 2 and np.array_equal(K.edt2(one), K.edt2_all_pairs(one))


def test_the_kernels_integer_square_root_fix_up_is_exact():
    import tmg_hip
    n = 255 * 255
    w = tmg_hip.ens_edt_fixed(range(n), 255)
    assert w == [math.isqrt(65536 * v) for v in range(n)] and max(w) < 2 ** 16
    for c in (1, 5, 255):
        d2 = list(range(0, c * c + 3)) + [2 ** 30 - 1, 2 ** 30]
        assert tmg_hip.ens_edt_fixed(d2, c) == K.fixed(d2, c).tolist() == [256 * c if v >= c * c else math.isqrt(65536 * v) for v in d2]
    assert tmg_hip.ens_edt_fixed([], 5) == []
    with pytest.raises(RuntimeError, match="tmg_ens_edt_fixed failed with code -1"):
        tmg_hip.ens_edt_fixed([1], 0)


def test_the_two_equivalent_mutations_change_no_output():
    """The bin w >> 8 is min(floor(sqrt(d2)), c), and the cutoff compared with > gives the same w, for every d2 and cutoff."""
    d2 = np.concatenate([np.arange(255 * 255 + 2), [2 ** 20, 2 ** 30 - 1, 2 ** 30]])
    for c in sorted({1, 2, 5, 254, 255} | {case[5] for case in K.TABLE}):
        assert np.array_equal(K.fixed(d2, c) >> 8, K.whole(d2, c)) and np.array_equal(K.whole(d2, c, "hist_w8"), K.whole(d2, c))
        assert np.array_equal(K.fixed(d2, c, "cutoff_gt"), K.fixed(d2, c))
    for idx in (1, 8, 12):
        for mu in K.EQUIVALENT:
            assert all(np.array_equal(v, K.case_reference(idx, mu)[k]) for k, v in K.case_reference(idx).items()), (idx, mu)


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_every_mutation_is_caught_by_the_comparison(mutation):
    caught = []
    for idx, case in enumerate(K.TABLE):
        S, B, Cc, hw, Kk, c, kind, _ = case
        want = K.full_reference(K.case_reference(idx), S, hw[0], hw[1], c, K.QUANTILES)
        bad = K.full_reference(K.case_reference(idx, mutation), S, hw[0], hw[1], c, K.QUANTILES)
        if K.mismatches(bad, want, K.INT_KEYS):
            caught.append(idx)
    assert len(caught) >= 3, (mutation, caught)


def test_the_cases_the_issue_names():
    sizes = {c[3] for c in K.TABLE}
    assert {(1, 1), (1, 7), (3, 130), (2, 300), (64, 64), (65, 63), (70, 70)} <= sizes
    assert max(-(-h // 64) for h, _ in sizes) >= 3 and max(-(-w // 64) for _, w in sizes) >= 3       # more than two bands and strips
    assert {c[5] for c in K.TABLE} == {1, 5, 255} and {c[2] for c in K.TABLE} == {2, 3, 4} and {c[0] for c in K.TABLE} == {1, 2, 3, 5}
    assert {c[6] for c in K.TABLE} == {"int", "smooth", "checker", "corners", "blobs", "cutoff", "empty", "nonfinite", "edges", "sparse"}
    assert any(c[7] for c in K.TABLE) and not any(c[7] and c[2] == 4 for c in K.TABLE)
    assert K.chunk_sizes(5, 0) == [5] and K.chunk_sizes(5, 1) == [1] * 5 and K.chunk_sizes(5, 2) == [2, 3]
    assert len(K.TIMED) == 3 and sum(K.TIMED) == 2
    # the empty case meets every combination, and the cutoff case a pair exactly the cutoff apart
    emp = K.case_reference(6)["pair"]
    nA, nO = emp[..., 0] == 0, emp[..., 1] == 0
    assert (nA & nO).any() and (nA & ~nO).any() and (~nA & nO).any() and (~nA & ~nO).any() and (emp[..., 0] == 70 * 70).any()
    assert (emp[..., 9] == K.INF).any() and (emp[..., 9] == -1).any() and (emp[..., 10] == K.INF).any()
    cut = K.case_reference(8)["pair"]
    assert (cut[..., 9] == 25).any() and (cut[..., 9] == 20).any()
    edges = K.inputs(2)
    m = K.in_event(edges[1][0, 0, 2], -0.5, "<")                              # the target's set of the word-edge case
    assert m[:, [63, 64, 127, 128]].any(0).all()


# ---- the host outputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_dist_outputs_against_the_fp64_restatement(idx):
    import tmg_ops as ops
    S, B, Cc, hw, Kk, c, kind, _ = K.TABLE[idx]
    ref = K.case_reference(idx)
    want = K.full_reference(ref, S, hw[0], hw[1], c, K.QUANTILES)
    got = ops.dist_outputs(torch.from_numpy(ref["pair"]), torch.from_numpy(ref["hist"]), S, hw[0], hw[1], c, K.QUANTILES)
    assert set(got) == set(K.FLOAT_KEYS) | {"dist_valid"}
    g = {k: v.numpy() for k, v in got.items()}
    assert not K.mismatches(g, want, ("dist_valid",))
    K.check_floats(g, want, K.FLOAT_KEYS, str(K.TABLE[idx]))
    on = [t for t, f in enumerate(K.TIMED) if f]
    tp, th = ops.dist_pool(torch.from_numpy(ref["pair"])[:, on], torch.from_numpy(ref["hist"])[:, on], 1)
    assert np.array_equal(tp.numpy(), want["time_dist_pair_raw"]) and np.array_equal(th.numpy(), want["time_dist_hist_raw"])
    gt = {"time_" + k: v.numpy() for k, v in ops.dist_outputs(tp, th, S, hw[0], hw[1], c, K.QUANTILES, len(on)).items()}
    assert not K.mismatches(gt, want, ("time_dist_valid",))
    K.check_floats(gt, want, tuple("time_" + k for k in K.FLOAT_KEYS), "pooled " + str(K.TABLE[idx]))


def test_dist_outputs_conventions_for_empty_sets():
    import tmg_ops as ops
    nan, inf = float("nan"), float("inf")
    c, HW = 5, 64
    full = 256 * c
    # member 0: both sets hold pixels; 1: A empty, O holds 4; 2: O empty, A holds 3; 3: both empty
    pair = torch.tensor([[3, 4, 2, 512, 70000, 256, 65536, 1000, 90000, 4, 1],
                         [0, 4, 0, 4 * full, 4 * full * full, 0, 0, HW * full, HW * full * full, K.INF, -1],
                         [3, 0, 0, 0, 0, 3 * full, 3 * full * full, HW * full, HW * full * full, -1, K.INF],
                         [0, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1]], dtype=torch.int64)
    hist = torch.zeros(4, 2, c + 1, dtype=torch.int64)
    hist[0, 0, 0], hist[0, 0, 2], hist[0, 1, 1], hist[1, 0, c], hist[2, 1, c] = 2, 2, 3, 4, 3
    o = {k: v.tolist() for k, v in ops.dist_outputs(pair, hist, 4, 8, 8, c, (0.5, 0.51, 1.0)).items()}
    same = lambda a, b: all((math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a, b))     # noqa: E731
    assert same(o["dist_med_miss"], [0.5, 5.0, nan, nan]) and same(o["dist_med_false"], [np.float32(1 / 3), nan, 5.0, nan])
    assert same(o["dist_med"], [0.5, nan, nan, nan])
    assert same(o["dist_hausdorff_miss"], [2.0, inf, inf, 0.0]) and same(o["dist_hausdorff_false"], [1.0, inf, inf, 0.0])
    assert same(o["dist_hausdorff"], [2.0, inf, inf, 0.0])
    assert same(o["dist_csi"], [0.4000000059604645, 0.0, 0.0, nan])
    assert same(o["dist_baddeley"][1:], [5.0, 5.0, 0.0]) and same(o["dist_baddeley1"][1:], [5.0, 5.0, 0.0])
    q = o["dist_hausdorff_q"]
    assert q[0] == [[0.0, 2.0, 2.0], [1.0, 1.0, 1.0]] and q[1][0] == [5.0, 5.0, 5.0] and same(q[1][1], [nan] * 3)
    assert same(q[2][0], [nan] * 3) and q[2][1] == [5.0, 5.0, 5.0] and same(q[3][0] + q[3][1], [nan] * 6)
    assert o["dist_valid"] == [2, 2, 1, 2, 4, 3]                               # non-finite values are dropped from the summary
    assert o["dist_mean"][3] == 1.0 and o["dist_std"][3] == 1.0                # the Hausdorff distances 2 and 0
    allnan = ops.dist_outputs(pair[3:], hist[3:], 1, 8, 8, c, (0.5,))
    assert allnan["dist_valid"].tolist() == [0, 0, 0, 1, 1, 0] and math.isnan(float(allnan["dist_mean"][0]))
    # pooling: a -1 stays only when every step's is -1, and an INF of one step makes the pooled distance infinite
    steps = torch.stack([pair[0], pair[3], pair[1]])[None]                     # [1, 3 steps, 11] of one member -> [1, S = 1, 11]
    tp, _ = ops.dist_pool(steps.unsqueeze(2), hist[[0, 3, 1]][None].unsqueeze(2), 1)
    assert tp[0, 0].tolist() == [3, 8, 2, 512 + 4 * full, 70000 + 4 * full * full, 256, 65536, 1000 + HW * full, 90000 + HW * full * full,
                                 K.INF, 1]
    with pytest.raises(ValueError, match="dist_outputs takes int64 tables"):
        ops.dist_outputs(pair.int(), hist, 4, 8, 8, c, (0.5,))
    with pytest.raises(ValueError, match="dist_outputs takes int64 tables"):
        ops.dist_outputs(pair, hist[..., :c], 4, 8, 8, c, (0.5,))


# ---- hand cases --------------------------------------------------------------------------------------------------------------------------
def _pair(a, o, c):
    return K.pair_of(K.edt2(a), K.edt2(o), c)


def test_one_pixel_against_one_pixel():
    import tmg_ops as ops
    a, o = np.zeros((9, 12), bool), np.zeros((9, 12), bool)
    a[2, 3], o[5, 7] = True, True                                              # 3 rows and 4 columns apart: 5 pixels
    pair, hist = _pair(a, o, 8)
    assert pair[:3].tolist() == [1, 1, 0] and pair[3:7].tolist() == [1280, 1280 ** 2, 1280, 1280 ** 2] and pair[9:].tolist() == [25, 25]
    assert hist[0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0] == hist[1].tolist()
    out = ops.dist_outputs(torch.from_numpy(pair)[None], torch.from_numpy(hist)[None], 1, 9, 12, 8, (0.5,))
    assert [float(out[k][0]) for k in ("dist_med_miss", "dist_med_false", "dist_med", "dist_hausdorff", "dist_rms_miss")] == [5.0] * 5
    assert float(out["dist_csi"][0]) == 0.0 and out["dist_hausdorff_q"].tolist() == [[[5.0], [5.0]]]
    cut = _pair(a, o, 5)[0]                                                   # exactly the cutoff: the cut value is the distance
    assert cut[3:7].tolist() == [1280, 1280 ** 2, 1280, 1280 ** 2]
    assert _pair(a, o, 4)[0][3:7].tolist() == [1024, 1024 ** 2, 1024, 1024 ** 2] and _pair(a, o, 4)[0][9:].tolist() == [25, 25]


def test_a_set_against_itself_has_every_distance_zero():
    rng = np.random.default_rng(5)
    a = rng.random((20, 33)) < 0.3
    pair, hist = _pair(a, a, 5)
    n = int(a.sum())
    assert pair.tolist() == [n, n, n, 0, 0, 0, 0, 0, 0, 0, 0] and hist.tolist() == [[n, 0, 0, 0, 0, 0]] * 2


@pytest.mark.parametrize("shift", [(0, 6), (4, 0), (3, 4), (6, 8)])
def test_the_hausdorff_distance_of_a_shifted_convex_blob_is_the_shift(shift):
    import tmg_ops as ops
    i, j = np.mgrid[0:40, 0:48]
    a = (i - 12) ** 2 + (j - 14) ** 2 <= 36                                    # a disc, away from the border
    o = np.roll(a, shift, (0, 1))
    pair, hist = _pair(a, o, 20)
    want = shift[0] ** 2 + shift[1] ** 2
    assert pair[9] == want == pair[10]
    out = ops.dist_outputs(torch.from_numpy(pair)[None], torch.from_numpy(hist)[None], 1, 40, 48, 20, (1.0,))
    assert float(out["dist_hausdorff"][0]) == math.sqrt(want) and float(out["dist_hausdorff_q"][0, 0, 0]) == math.isqrt(want)
    assert 0 < float(out["dist_med"][0]) < math.sqrt(want)
