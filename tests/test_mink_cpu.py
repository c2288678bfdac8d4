"""CPU-side checks of the excursion-set morphology: the kernel entries are declared in their own header, listed apart and exported;
the signatures of the three Python layers; the plan query's values and the codes the entries return before any launch; every argument
error without a GPU; the reference of tests/mink_cases.py against its second statement (pieces and holes by flood fill, and scipy's
labeller where it imports) and against the identities of the counts; tmg_ops.mink_outputs against independently written fp64
formulas; and the sensitivity of the comparison the GPU test uses: every named mutation is caught."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import mink_cases as K

NAMES = ["tmg_ens_mink_plan", "tmg_ens_mink_chunk"]
c_i64 = ctypes.c_int64


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    hdr = open(os.path.join(inc, "tmglow_hip_mink.h")).read()
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", hdr)
    assert decl == [("int", n) for n in NAMES] and tmg_hip.MINK_EXPORTS == NAMES
    assert "mink" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    P64 = ctypes.POINTER(c_i64)
    vp = ctypes.c_void_p
    want = {"tmg_ens_mink_plan": [P64, P64], "tmg_ens_mink_chunk": [vp, P64, vp, P64, vp, P64, vp, P64, vp]}
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.MINK_ARGTYPES[name] == want[name]
        # the header's parameter list, read as ctypes: a pointer to int64_t, any other pointer, the stream
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        kinds = [P64 if "int64_t*" in q.replace(" *", "*") else vp for q in params]
        assert kinds == want[name], name
    assert "tmg_mink.hip" in tmg_hip.SOURCES and "tmg_mink.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_mink.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_mink\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_mink.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    # integer arithmetic only: no float atomics, no inline assembly, nothing printed or asserted in a kernel, no unbounded loop
    assert not re.search(r"\basm\b|printf|assert\s*\(|while\s*\(|atomicAdd\s*\(\s*\(float|double|hipMemset", code)
    # no lane leaves before the exchanges and barriers: the kernel has no return statement
    body = code[code.index("void ens_mink_chunk_kernel"):code.index("static int mink_fields")]
    assert body.count("__syncthreads") == 3 and "__shfl_down" in body and not re.search(r"\breturn\b", body)


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredMorphology).parameters
    assert list(sig) == old + ["fields", "thresholds", "levels"]
    assert sig["fields"].default == (0,) and sig["thresholds"].default is None and sig["levels"].default == 16
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleMorphology.__init__).parameters
    isc = list(inspect.signature(tmg_ops.EnsembleIntensityScale.__init__).parameters)
    assert list(init) == isc[:isc.index("events")] + ["fields", "thresholds", "grid"]
    assert init["fields"].default == (0,) and init["grid"].default == (1.0, 1.0) and init["u"].default is None
    assert list(inspect.signature(tmg_ops.EnsembleMorphology.add).parameters) == ["self", "y", "m0", "target", "time"]
    assert issubclass(tmg_ops.EnsembleMorphology, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.mink_args).parameters) == ["fields", "thresholds", "C"]
    out = inspect.signature(tmg_ops.mink_outputs).parameters
    assert list(out)[:6] == ["raw", "S", "H", "W", "grid", "steps"] and out["steps"].default == 1
    plan = inspect.signature(tmg_hip.ens_mink_plan).parameters
    assert list(plan) == ["S", "B", "H", "W", "F", "J", "code"] and plan["code"].default is False
    assert inspect.signature(tmg_hip.ens_mink_chunk).parameters["code"].default is False
    assert "40 Tk B F (S + 1) J bytes" in tmg_ops.EnsembleMorphology.__doc__       # the device memory is stated
    for word in ("speckle", "diagonal", "Not supported", "vorticity", "periodic", "Gaussian", "not a mean of ratios"):
        assert word in utils.modelPredMorphology.__doc__, word
    assert tmg_ops.MINK_CURVES == K.CURVES and tmg_ops.MINK_INT_KEYS == K.INT_KEYS and tmg_ops.MINK_FLOAT_KEYS == K.FLOAT_KEYS


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,Hh,Ww,F,J", [(1, 1, 1, 1, 1, 1), (5, 2, 3, 130, 4, 32), (2, 3, 64, 63, 1, 6), (5, 2, 65, 62, 4, 31),
                                           (32, 4, 256, 256, 3, 16), (1024, 65535, 70, 69, 4, 32)])
def test_plan_values(S, B, Hh, Ww, F, J):
    import tmg_hip
    p = tmg_hip.ens_mink_plan(S, B, Hh, Ww, F, J)
    tx, ty = -(-Ww // 63), -(-Hh // 64)
    G = K.group(tx * ty * B, S)
    assert (p["tile_h"], p["tile_w"]) == K.TILE == (64, 63) and p["threads"] == 256 and p["group"] == G
    assert (p["tiles_x"], p["tiles_y"]) == (tx, ty)
    assert p["grid"] == (tx * ty, -(-S // G) + 1, B) and p["blocks"] == tx * ty * (-(-S // G) + 1) * B
    # five histograms of 33 bins per member of a group and field, the sorted ladders and the ladders as given
    assert p["lds_bytes"] == 4 * 4 * 4 * 5 * 33 + 4 * 4 * 34 + 4 * 4 * 32
    assert p["table_words"] == B * F * (S + 1) * J * 5


def test_the_member_groups_the_gpu_cases_assume():
    import tmg_hip
    assert [K.group(K.planes(c), c[0]) for c in K.GROUP_CASES] == [4, 2] and all(c[0] == 5 for c in K.GROUP_CASES)
    # the chunkings (5,), (1, .., 1), (2, 3) put 1, 2, 3 and 5 members on every side of the groups of 2 and 4
    assert {K.group(K.planes(K.GROUP_CASES[0]), k) for k in (1, 2, 3, 5)} == {1, 2, 4}
    assert {K.group(K.planes(K.GROUP_CASES[1]), k) for k in (1, 2, 3, 5)} == {1, 2}
    assert {K.group(K.planes(c), k) for c in K.TABLE for k in range(1, c[0] + 1)} == {1}
    assert {c[0] for c in K.TABLE} == {1, 2, 3, 5}
    assert K.group(80, 16) == 1 and K.group(128, 16) == 2 and K.group(256, 16) == 4 and K.group(1024, 3) == 3 and K.group(1, 1024) == 1
    for case in K.TABLE + K.GROUP_CASES:
        S, B, Cc, hw, F, J, kind, _ = case
        assert tmg_hip.ens_mink_plan(S, B, hw[0], hw[1], F, J)["group"] == K.group(K.planes(case), S)


def test_the_cases_the_issue_names():
    th, tw = K.TILE
    sizes = {c[3] for c in K.TABLE}
    assert {(1, 1), (1, 7), (2, 2), (3, 130), (th, tw), (th + 1, tw - 1), (th + 6, tw + 6)} <= sizes
    assert {c[5] for c in K.TABLE} >= {1, 2, 31, 32} and {c[2] for c in K.TABLE} == {2, 3, 4}
    assert all(c[4] in (1, c[2]) for c in K.TABLE if c[3] in ((1, 1), (1, 7), (2, 2), (3, 130), (th, tw)))
    assert {c[6] for c in K.TABLE} == {"int", "smooth", "allin", "nonein", "ties", "decr", "nonfinite"}
    assert any(c[7] for c in K.TABLE) and not any(c[7] and c[2] == 4 for c in K.TABLE)
    assert K.chunk_sizes(5, 0) == [5] and K.chunk_sizes(5, 1) == [1] * 5 and K.chunk_sizes(5, 2) == [2, 3]
    assert len(K.TIMED) == 3 and sum(K.TIMED) == 2
    assert K.tile_corners((70, 69)) == [(63, 62)] and K.tile_corners((3, 130)) == [(0, 62), (0, 125)] and K.tile_corners((64, 63)) == []
    for case in K.TABLE:
        thr = K.raw_ladder(case)
        d = np.diff(thr, axis=-1)
        assert bool((d <= 0).all() and (d < 0).any()) if case[6] == "decr" else bool((d >= 0).all())
        assert bool((d == 0).any()) == (case[6] == "ties")
    x = np.zeros((70, 69), np.float32)
    for variant, n in ((0, 4), (1, 2), (2, 4), (3, 2)):
        K.plant(x, variant)
        assert int((x == K.HIGH).sum()) == n, variant


def test_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    plan = (c_i64 * 12)()
    good = [5, 2, 9, 8, 2, 3]                                                 # S, B, H, W, F, J
    assert lib.tmg_ens_mink_plan(_i64(*good), plan) == 0
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 5), (5, 0), (5, 33), (5, -1)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_mink_plan(_i64(*d), plan) == -1, (pos, bad)
    for pos, bad in ((0, 1025), (1, 65536), (2, 1 << 31), (3, 1 << 31)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_mink_plan(_i64(*d), plan) == -2, (pos, bad)
    for pos, edge in ((0, 1024), (1, 65535), (4, 4), (5, 32)):                # the limits themselves are taken
        d = list(good)
        d[pos] = edge
        assert lib.tmg_ens_mink_plan(_i64(*d), plan) == 0, (pos, edge)
    assert lib.tmg_ens_mink_plan(_i64(5, 2, 1 << 16, (1 << 15) - 1, 2, 3), plan) == 0
    assert lib.tmg_ens_mink_plan(_i64(5, 2, 1 << 16, 1 << 15, 2, 3), plan) == -2   # H W >= 2^31 - 256
    assert lib.tmg_ens_mink_plan(_i64(5, 2, 1, (1 << 31) - 257, 2, 3), plan) == 0
    assert lib.tmg_ens_mink_plan(_i64(5, 2, 1, (1 << 31) - 256, 2, 3), plan) == -2
    assert lib.tmg_ens_mink_plan(None, plan) == -3 and lib.tmg_ens_mink_plan(_i64(*good), None) == -3
    assert tmg_hip.ens_mink_plan(0, 1, 5, 5, 1, 4, code=True)[1] == -1
    assert tmg_hip.ens_mink_plan(1025, 1, 5, 5, 1, 4, code=True)[1] == -2
    with pytest.raises(RuntimeError):
        tmg_hip.ens_mink_plan(1, 1, 5, 5, 1, 33)
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                                  # never dereferenced: every code comes before a launch
    k, B, Hh, Ww, Cc, S, F, J = 2, 2, 9, 8, 3, 5, 2, 3
    base = [k, B, Hh, Ww, Cc, S, 0, F, J]                                      # k, B, H, W, C, S, m0, F, J

    def chunk(dims=base, y=one, yd=(4, 1), tgt=one, td=(4, 1), thr=one, fields=(0, 2), table=one):
        return lib.tmg_ens_mink_chunk(y, _i64(*yd) if yd else None, tgt, _i64(*td) if td else None, thr, _i64(*fields) if fields else None,
                                      table, _i64(*dims) if dims else None, nul)

    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (4, 5), (5, 0), (6, -1), (6, 4), (7, 0), (7, 5), (8, 0), (8, 33)):
        d = list(base)
        d[pos] = bad
        assert chunk(d) == -1, (pos, bad)
    for bad in ((2, 0), (4, -1), (4, 2)):
        assert chunk(yd=bad) == -1 and chunk(td=bad) == -1, bad
    for fields in ((3, 0), (0, -1), (1, 1)):                                  # out of range, or twice
        assert chunk(fields=fields) == -1, fields
    for pos, bad in ((5, 1025), (1, 65536), (2, 1 << 31)):
        d = list(base)
        d[pos] = bad
        assert chunk(d) == -2, (pos, bad)
    assert chunk(yd=(1 << 31, 0)) == -2 and chunk(td=(1 << 31, 0)) == -2
    assert chunk(yd=None) == -3 and chunk(td=None) == -3 and chunk(fields=None) == -3 and chunk(dims=None) == -3
    for name in ("y", "tgt", "thr", "table"):
        assert chunk(**{name: nul}) == -3, name


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_mink_args_give_an_error_for_each_bad_argument():
    import tmg_ops as ops
    fl, th = ops.mink_args([2, 0], [[-1, 0.5], (0.0, np.float32(2.0))], 3)
    assert fl == (2, 0) and th == ((-1.0, 0.5), (0.0, 2.0)) and all(type(v) is float for t in th for v in t) and type(fl[0]) is int
    assert ops.mink_args((np.int64(1),), ((0.0,),), 2) == ((1,), ((0.0,),))
    assert len(ops.mink_args((0,), [list(range(32))], 3)[1][0]) == 32
    for fields, thr, msg in ((7, [[0.0]], "sequence of channel"), ((), [], "1 to 4 channels"), ((0, 1, 2, 3, 0), [[0.0]] * 5, "1 to 4 channels"),
                             ((3,), [[0.0]], r"0\.\.2"), ((-1,), [[0.0]], r"0\.\.2"), ((True,), [[0.0]], r"0\.\.2"), ((1.0,), [[0.0]], r"0\.\.2"),
                             ((0, 0), [[0.0], [0.0]], "distinct"), ((0,), 3.0, "one sequence of values per field"),
                             ((0,), [3.0], "one sequence of values per field"), ((0, 1), [[0.0]], "one ladder per field"),
                             ((0,), [[]], "1 to 32 levels"), ((0,), [list(range(33))], "1 to 32 levels"),
                             ((0, 1), [[0.0, 1.0], [0.0]], "same number of levels"), ((0,), [[0.0, float("nan")]], "finite"),
                             ((0,), [[float("inf")]], "finite"), ((0,), [[True]], "finite"), ((0,), [["1"]], "finite"),
                             ((0,), [[0.0, 0.0]], "strictly ascending"), ((0,), [[1.0, 0.0]], "strictly ascending")):
        with pytest.raises(ValueError, match=msg):
            ops.mink_args(fields, thr, 3)


def test_constructor_limits_come_with_their_numbers_before_any_device_work():
    import tmg_ops as ops
    from utils import utils
    ok = dict(members=5, B=2, C=3, Hh=8, Ww=9, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3))
    for kw, msg in ((dict(C=1), "2 <= C <= 4"), (dict(C=5, out_mu=torch.zeros(5), out_std=torch.ones(5)), "2 <= C <= 4"),
                    (dict(steps=0), "steps >= 1"), (dict(steps=True), "steps >= 1"), (dict(steps=2.0), "steps >= 1"),
                    (dict(members=0), "members"), (dict(members=1025), "1024"), (dict(B=0), "B, H, W >= 1"), (dict(Hh=0), "B, H, W >= 1"),
                    (dict(B=65536), "at most 65535 cases, got 65536"), (dict(Hh=1 << 16, Ww=1 << 15), r"H W < 2\^31 - 256"),
                    (dict(fields=(3,)), r"0\.\.2"), (dict(fields=(0, 1)), "one ladder per field"), (dict(thresholds=((1.0, 0.0),)), "ascending"),
                    (dict(thresholds=torch.zeros(3, 1, 1)), r"per case are \[2, F, J\]"), (dict(thresholds=torch.zeros(2, 1, 2)), "ascending"),
                    (dict(grid=(0.0, 1.0)), "finite and positive"), (dict(grid=(1.0, float("nan"))), "finite and positive"),
                    (dict(out_std=torch.tensor([1.0, 0.0, 1.0])), "strictly positive"), (dict(u=torch.zeros(2, 3)), "strictly positive")):
        with pytest.raises(ValueError, match=msg):
            ops.EnsembleMorphology(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="not a GPU"):
        ops.EnsembleMorphology(**dict(ok, device="cpu"))
    with pytest.raises(ValueError):                                           # the argument error wins over the device error
        ops.EnsembleMorphology(**dict(ok, device="cpu", fields=(0, 0)))
    for kw in (dict(fields=()), dict(fields=(3,)), dict(fields=7), dict(levels=0), dict(levels=33), dict(levels=2.0), dict(levels=True),
               dict(thresholds=((1.0, 0.0),)), dict(fields=(0, 1), thresholds=((0.0,),))):
        with pytest.raises(ValueError):
            utils.modelPredMorphology(None, None, None, None, **kw)
    raw = torch.zeros(1, 3, 2, 5, dtype=torch.int64)
    ops.mink_outputs(raw, 2, 3, 4, (1.0, 1.0))
    for a in ((raw.double(), 2, 3, 4, (1.0, 1.0)), (raw, 3, 3, 4, (1.0, 1.0)), (raw[..., :4], 2, 3, 4, (1.0, 1.0)), (raw, 2, 0, 4, (1.0, 1.0)),
              (raw, 2, 3, 4, (1.0, 1.0), 0), (raw, 2, 3, 4, (0.0, 1.0)), (raw[..., :0, :], 2, 3, 4, (1.0, 1.0)),
              (raw, 2, 3, 4, (1.0, 1.0), 1, torch.zeros(3))):
        with pytest.raises(ValueError):
            ops.mink_outputs(*a)


def test_the_raw_ladder_follows_raw_thresholds_rule():
    import tmg_ops as ops
    rng = np.random.default_rng(3)
    B, Cc, fields = 3, 3, (2, 0)
    mu, sd = torch.tensor([0.3, -1.1, 2.0]), torch.tensor([0.7, 1.9, 0.05])
    u = torch.from_numpy(rng.uniform(0.5, 2.0, (B, Cc)).astype(np.float32))
    lv = torch.from_numpy(np.sort(rng.normal(size=(B, 2, 5)), -1))
    for uu in (None, u):
        thr = ops.mink_raw_ladder(lv, fields, mu, sd, uu)
        assert thr.dtype == torch.float32 and tuple(thr.shape) == (B, 2, 5)
        for b in range(B):                                                    # entry by entry through raw_thresholds itself
            for f, ch in enumerate(fields):
                want = ops.raw_thresholds([(ch, float(v), ">") for v in lv[b, f]], B, Cc, mu, sd, uu)[b]
                assert torch.equal(thr[b, f], want)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
def _some_levels(J):
    return sorted({0, J // 2, J - 1})


@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_the_reference_equals_the_second_statement_and_the_identities(idx):
    """On every case: N does not increase with the level and the counts are bounded by their all-in values; per (step, row, field) of
    case 0 the Euler characteristics of the masks equal pieces minus holes and the edge count the differences of the padded mask, by
    scipy's labeller on every level where it imports, and by the flood fill of tests/mink_cases.py on the target's rows (three levels,
    every level of the small fields)."""
    case = K.TABLE[idx]
    S, B, Cc, hw, F, J, kind, _ = case
    Hh, Ww = hw
    xs, tgt = K.inputs(idx)
    ref = K.case_reference(idx)
    thr = K.raw_ladder(case)
    fields = K.fields_for(Cc, F)
    Tk = len(K.TIMED)
    assert ref.shape == (B, Tk, F, S + 1, J, 5) and ref.dtype == np.int64 and bool((ref >= 0).all())
    N, Nh, Nv, Nq, Nd = (ref[..., i] for i in range(5))
    assert bool((np.diff(N, axis=-1) <= 0).all()) and bool((np.diff(Nq, axis=-1) <= 0).all())
    full = (Hh * Ww, Hh * (Ww - 1), (Hh - 1) * Ww, (Hh - 1) * (Ww - 1))
    assert all(bool((v <= m).all()) for v, m in zip((N, Nh, Nv, Nq), full)) and bool((Nq + Nd <= full[3]).all())
    if kind == "allin":
        assert all(bool((v == m).all()) for v, m in zip((N, Nh, Nv, Nq), full)) and not Nd.any()
        assert bool((K.curves(ref)[..., 2:, :] == 1).all())
    if kind == "nonein":
        assert not ref.any()
    cur = K.curves(ref)
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    small = Hh * Ww <= 500
    for t in range(Tk):
        for f, ch in enumerate(fields):
            for m in range(S + 1):
                x = tgt[t, 0, ch] if m == S else xs[t, m, 0, ch]
                for j in range(J) if (have_scipy or small) else (_some_levels(J) if m == S else ()):
                    mask = K.mask_of(x, thr[0, f], j)
                    got = tuple(int(v) for v in cur[0, t, f, m, 2:, j])
                    assert int(cur[0, t, f, m, 1, j]) == K.edges_by_differences(mask)
                    if have_scipy:
                        assert got == K.euler_by_labels(mask, K.scipy_count), (t, f, m, j)
                    if m == S and t == 0 and (small or j in _some_levels(J)):
                        assert got == K.euler_by_labels(mask), (t, f, m, j)


def test_the_labeller_and_the_counts_on_shapes_known_by_hand():
    ring = np.ones((5, 5), bool)
    ring[1:4, 1:4] = False
    ring[2, 2] = True                                                         # a ring with an island in its hole
    assert K.label_count(ring, 4) == 2 and K.label_count(~ring, 4) == 1 and K.euler_by_labels(ring) == (1, 1)
    check = (np.add.outer(np.arange(6), np.arange(7)) % 2) == 0               # a checkerboard: every quad is a diagonal pair
    x = np.where(check, 1.0, -1.0).astype(np.float32)
    c = K.counts(x, np.array([0.0], np.float32))[0]
    assert tuple(c) == (21, 0, 0, 0, 5 * 6)
    assert K.euler_by_labels(check) == (21, 1 - 10)                            # 21 pieces by edges; one by corners, with the 10 interior gaps as holes
    assert tuple(K.curves(c[None])[:, 0]) == (21, 84, 21, 21 - 30) and K.edges_by_differences(check) == 84
    try:
        for mask in (ring, check, ~check):
            for conn in (4, 8):
                assert K.label_count(mask, conn) == K.scipy_count(mask, conn)
    except ImportError:
        pass
    full = K.counts(np.ones((4, 9), np.float32), np.array([0.0, 1.0], np.float32))
    assert tuple(full[0]) == (36, 32, 27, 24, 0) and not full[1].any()          # all in; 1 > 1 is false: strict
    assert tuple(K.curves(full)[:, 0]) == (36, 2 * (4 + 9), 1, 1)
    weird = np.array([np.nan, np.inf, -np.inf, 0.0], np.float32).reshape(1, 4)
    assert K.counts(weird, np.array([-1.0, 1.0], np.float32))[:, 0].tolist() == [2, 1]     # NaN and -Inf rank 0, +Inf rank J, 0.0 rank 1


@pytest.mark.parametrize("mutation", K.MUTATIONS + K.CURVE_MUTATIONS)
def test_every_mutation_of_the_reference_is_caught(mutation):
    """The comparison of the GPU test (bitwise equality of mink_raw, and of the integer outputs) tells every mutation from the
    reference: the tile-edge ones on every case whose field has a tile edge, the others on at least two cases of the kinds that can
    show them (one for NaN; a case may hide one: the planted windows clear the row ends of the 3 x 130 field)."""
    shows = {"nonstrict": ("int", "ties"), "row_wrap": ("int", "smooth"), "tile_edge_dropped": None, "tile_edge_twice": None,
             "nd_three": ("int", "smooth"), "nan_in": ("nonfinite",), "chi8_plus": ("int", "smooth")}[mutation]
    caught = 0
    for idx, case in enumerate(K.TABLE):
        S, B, Cc, hw, F, J, kind, _ = case
        if shows is None:
            if not K.tile_corners(hw) or kind in ("allin", "nonein"):
                continue
        elif kind not in shows or hw[0] < 2 or hw[1] < 2:
            continue
        ref = K.case_reference(idx)
        if mutation in K.CURVE_MUTATIONS:
            want = K.full_reference(ref, S, hw[0], hw[1], K.GRID, K.levels_of(case))
            mut = K.full_reference(ref, S, hw[0], hw[1], K.GRID, K.levels_of(case), mutation=mutation)
            caught += bool(K.mismatches(mut, want, ("mink_euler8",)))
        else:
            xs, tgt = K.inputs(idx)
            mut = K.reference(xs[:1], tgt[:1], K.raw_ladder(case), K.fields_for(Cc, F), mutation)
            hit = bool(K.mismatches({"mink_raw": mut}, {"mink_raw": ref[:, :1]}, ("mink_raw",)))
            assert hit or shows is not None, case
            caught += hit
            assert not K.mismatches({"mink_raw": K.reference(xs[:1], tgt[:1], K.raw_ladder(case), K.fields_for(Cc, F))},
                                    {"mink_raw": ref[:, :1]}, ("mink_raw",))
    assert caught >= (1 if mutation == "nan_in" else 2)


# ---- the host outputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [1, 3, 6, 10, 12])
def test_mink_outputs_follow_the_fp64_formulas_and_the_rank_counts_are_exact(idx):
    import tmg_ops as ops
    case = K.TABLE[idx]
    S, B, Cc, hw, F, J, kind, _ = case
    ref = K.case_reference(idx)
    lv = K.levels_of(case)
    want = K.full_reference(ref, S, hw[0], hw[1], K.GRID, lv)
    raw = torch.from_numpy(np.array(ref))
    got = {k: v.numpy() for k, v in ops.mink_outputs(raw, S, hw[0], hw[1], K.GRID, 1, torch.from_numpy(np.array(lv)).unsqueeze(1)).items()}
    timed = raw[:, [t for t, on in enumerate(K.TIMED) if on]].sum(1)
    got.update({"time_" + k: v.numpy() for k, v in ops.mink_outputs(timed, S, hw[0], hw[1], K.GRID, sum(K.TIMED), torch.from_numpy(np.array(lv))).items()})
    keys = [p + k for p in ("", "time_") for k in K.INT_KEYS]
    assert set(got) == set(K.ALL_KEYS) - {"mink_raw", "time_mink_raw", "mink_levels"}
    assert all(got[k].dtype == np.int64 for k in keys) and not K.mismatches(got, want, keys)
    K.check_floats(got, want, [p + k for p in ("", "time_") for k in K.FLOAT_KEYS], str(case))
    # the exact rank of the target: below + equal + above = S, counted on the integers
    assert bool(((got["mink_below"] >= 0) & (got["mink_below"] + got["mink_equal"] <= S)).all())
    cur = K.curves(ref)
    for q in range(4):
        assert np.array_equal(got["mink_below"][..., q, :], (cur[..., :S, q, :] < cur[..., S:, q, :]).sum(-2))
    assert got["mink_l1"].shape == (B, len(K.TIMED), F, S, 4) and got["time_mink_l1"].shape == (B, F, S, 4)
    assert bool((got["mink_l1"] >= 0).all())
    # without the ladder there is no integral; with one level it is 0
    assert "mink_l1" not in ops.mink_outputs(raw, S, hw[0], hw[1], K.GRID)
    one = ops.mink_outputs(raw[..., :1, :], S, hw[0], hw[1], K.GRID, 1, torch.zeros(1))
    assert tuple(one["mink_l1"].shape) == (B, len(K.TIMED), F, S, 4) and not bool(one["mink_l1"].any())
