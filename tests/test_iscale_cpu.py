"""CPU-side checks of the intensity-scale verification: the kernel entries are declared in their own header, listed apart and
exported; the signatures of the three Python layers; the plan query's values and the codes the entries return before any launch;
every argument error without a GPU; the reference of tests/iscale_cases.py against its second statement (explicit Haar components by
np.kron of block means) and against the identities of the method; tmg_ops.iscale_outputs against independently written fp64
formulas and against event_table_scores' Brier score of the same data; and the sensitivity of the comparison the GPU test uses:
every named mutation is caught."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import iscale_cases as K

NAMES = ["tmg_ens_iscale_plan", "tmg_ens_iscale_chunk", "tmg_ens_iscale_step"]
c_i64 = ctypes.c_int64


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_iscale.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.ISCALE_EXPORTS == NAMES
    assert "iscale" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    P64 = ctypes.POINTER(c_i64)
    vp = ctypes.c_void_p
    want = {"tmg_ens_iscale_plan": [P64, P64], "tmg_ens_iscale_chunk": [vp, P64, vp, P64, vp, P64, vp, vp, vp, vp, P64, vp],
            "tmg_ens_iscale_step": [vp, vp, P64, vp, P64, vp, P64, vp]}
    hdr = open(os.path.join(inc, "tmglow_hip_iscale.h")).read()
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.ISCALE_ARGTYPES[name] == want[name]
        # the header's parameter list, read as ctypes: a pointer to int64_t, any other pointer, the stream
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        kinds = [P64 if "int64_t*" in q.replace(" *", "*") else vp for q in params]
        assert kinds == want[name], name
    assert "tmg_iscale.hip" in tmg_hip.SOURCES and "tmg_iscale.hip" not in tmg_hip.NO_PACKED_F32
    assert tmg_hip.SOURCES.index("tmg_spell.hip") < tmg_hip.SOURCES.index("tmg_iscale.hip") < tmg_hip.SOURCES.index("tmg_lagr.hip")
    assert "tmglow_hip_iscale.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_iscale\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_iscale.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    # integer arithmetic only: no float atomics, no inline assembly, nothing printed or asserted in a kernel, no unbounded loop
    assert not re.search(r"\basm\b|printf|assert\s*\(|while\s*\(|atomicAdd\s*\(\s*\(float|double", code)
    # no lane leaves before the exchanges and barriers: the kernels have no return statement
    for name, end in (("ens_iscale_chunk_kernel", "ens_iscale_step_kernel"), ("ens_iscale_step_kernel", "static int iscale_events")):
        body = code[code.index("void " + name):code.index(end, code.index("void " + name) + 10)]
        assert "__syncthreads" in body and "isc_up" in body and not re.search(r"\breturn\b", body), name


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredIntensityScale).parameters
    assert list(sig) == old + ["events", "levels"] and sig["events"].default == ((0, 0.0, "<"),) and sig["levels"].default is None
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleIntensityScale.__init__).parameters
    ev_init = inspect.signature(tmg_ops.EnsembleEvents.__init__).parameters
    assert list(init) == [("levels" if n == "scales" else n) for n in ev_init] and init["levels"].default is None
    assert list(inspect.signature(tmg_ops.EnsembleIntensityScale.add).parameters) == ["self", "y", "m0", "target", "time"]
    assert issubclass(tmg_ops.EnsembleIntensityScale, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.iscale_args).parameters) == ["events", "levels", "C", "H", "W"]
    out = inspect.signature(tmg_ops.iscale_outputs).parameters
    assert list(out) == ["member_raw", "target_raw", "ens_raw", "S", "HW", "steps"] and out["steps"].default == 1
    plan = inspect.signature(tmg_hip.ens_iscale_plan).parameters
    assert list(plan) == ["S", "B", "H", "W", "K", "L", "code"] and plan["code"].default is False
    for fn in (tmg_hip.ens_iscale_chunk, tmg_hip.ens_iscale_step):
        assert inspect.signature(fn).parameters["code"].default is False
    assert "4 B K HW bytes" in tmg_ops.EnsembleIntensityScale.__doc__             # the device memory is stated
    for word in ("remainder", "Casati", "not a mean of ratios"):
        assert word in utils.modelPredIntensityScale.__doc__, word
    assert tmg_ops.ISCALE_RAW_KEYS == K.RAW_KEYS and set(tmg_ops.ISCALE_FLOAT_KEYS) == set(K.FLOAT_KEYS)


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,Hh,Ww,Kn,L", [(1, 1, 1, 1, 1, 1), (5, 2, 3, 130, 4, 3), (2, 3, 64, 64, 1, 6), (5, 2, 65, 63, 4, 6),
                                            (32, 4, 256, 256, 2, 6), (1024, 65535, 70, 70, 4, 6)])
def test_plan_values(S, B, Hh, Ww, Kn, L):
    import tmg_hip
    p = tmg_hip.ens_iscale_plan(S, B, Hh, Ww, Kn, L)
    tx, ty = -(-Ww // 64), -(-Hh // 64)
    assert p["tile"] == 64 and p["threads"] == 256 and p["group"] == K.group(tx * ty * Kn * B, S) and (p["tiles_x"], p["tiles_y"]) == (tx, ty)
    assert p["grid"] == (tx * ty, Kn, B) and p["blocks"] == tx * ty * Kn * B
    # the chunk kernel: 64 row masks per member of a group and for the target, the per-wave sums; the step kernel: its per-wave sums
    assert p["lds_bytes"] == 8 * (8 + 1) * 64 + 4 * (4 * 8 * 6 * 2 + 8 * 4 + 4 * 6 + 4) and p["step_lds_bytes"] == 8 * 4 * 6 * 2 + 4 * 8
    assert p["member_words"] == B * Kn * S * (L + 1) * 2 and p["target_words"] == B * Kn * (L + 1) and p["ens_words"] == B * Kn * (L + 1) * 2


def test_the_member_groups_the_gpu_cases_assume():
    import tmg_hip
    assert [K.group(K.planes(c), c[0]) for c in K.GROUP_CASES] == [4, 8]
    assert {K.group(K.planes(c), k) for c in K.TABLE for k in range(1, c[0] + 1)} == {1, 2}
    assert K.group(64, 16) == 2 and K.group(64, 64) == 8 and K.group(1024, 16) == 8 and K.group(256, 3) == 2 and K.group(512, 1) == 1
    for case in K.TABLE + K.GROUP_CASES:
        S, B, Cc, hw, Kn, L, kind, _ = case
        assert tmg_hip.ens_iscale_plan(S, B, hw[0], hw[1], Kn, L)["group"] == K.group(K.planes(case), S)


def test_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    plan = (c_i64 * 14)()
    good = [5, 2, 9, 8, 2, 3]                                                 # S, B, H, W, K, L
    assert lib.tmg_ens_iscale_plan(_i64(*good), plan) == 0
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (4, 5), (5, 0), (5, 7), (5, -1)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_iscale_plan(_i64(*d), plan) == -1, (pos, bad)
    for pos, bad in ((0, 1025), (1, 65536), (2, 1 << 31), (3, 1 << 31)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_iscale_plan(_i64(*d), plan) == -2, (pos, bad)
    assert lib.tmg_ens_iscale_plan(_i64(5, 2, 1 << 16, (1 << 15) - 1, 2, 3), plan) == 0
    assert lib.tmg_ens_iscale_plan(_i64(5, 2, 1 << 16, 1 << 15, 2, 3), plan) == -2   # H W >= 2^31 - 256
    # S^2 4^L H_pad W_pad >= 2^63: 2^20 * 2^12 * (64 * 2^25) = 2^63 is refused, one level less is taken
    assert lib.tmg_ens_iscale_plan(_i64(1024, 1, 1, 1 << 25, 1, 6), plan) == -2
    assert lib.tmg_ens_iscale_plan(_i64(1024, 1, 1, 1 << 25, 1, 5), plan) == 0
    assert lib.tmg_ens_iscale_plan(_i64(1023, 1, 1, 1 << 25, 1, 6), plan) == 0
    assert lib.tmg_ens_iscale_plan(None, plan) == -3 and lib.tmg_ens_iscale_plan(_i64(*good), None) == -3
    assert tmg_hip.ens_iscale_plan(0, 1, 5, 5, 1, 4, code=True)[1] == -1
    assert tmg_hip.ens_iscale_plan(1025, 1, 5, 5, 1, 4, code=True)[1] == -2
    with pytest.raises(RuntimeError):
        tmg_hip.ens_iscale_plan(1, 1, 5, 5, 1, 7)
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                                  # never dereferenced: every code comes before a launch
    k, B, Hh, Ww, Cc, S, Kn, L = 2, 2, 9, 8, 3, 5, 2, 3
    base = [k, B, Hh, Ww, Cc, S, 0, Kn, L]                                     # k, B, H, W, C, S, m0, K, L

    def chunk(dims=base, y=one, yd=(4, 1), tgt=one, td=(4, 1), thr=one, ev=(0, 0, 2, 1), cnt=one, mem=one, tt=one, ens=one):
        return lib.tmg_ens_iscale_chunk(y, _i64(*yd) if yd else None, tgt, _i64(*td) if td else None, thr, _i64(*ev) if ev else None, cnt,
                                        mem, tt, ens, _i64(*dims), nul)

    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 1), (4, 5), (5, 0), (6, -1), (6, 4), (7, 0), (7, 5), (8, 0), (8, 7)):
        d = list(base)
        d[pos] = bad
        assert chunk(d) == -1, (pos, bad)
    for bad in ((2, 0), (4, -1), (4, 2)):
        assert chunk(yd=bad) == -1 and chunk(td=bad) == -1, bad
    for ev in ((3, 0, 2, 1), (0, 2, 2, 1), (-1, 0, 2, 1)):
        assert chunk(ev=ev) == -1, ev
    for pos, bad in ((5, 1025), (1, 65536), (2, 1 << 31)):
        d = list(base)
        d[pos] = bad
        assert chunk(d) == -2, (pos, bad)
    assert chunk(yd=(1 << 31, 0)) == -2 and chunk(td=(1 << 31, 0)) == -2
    assert chunk(yd=None) == -3 and chunk(td=None) == -3 and chunk(ev=None) == -3
    for name in ("y", "tgt", "thr", "cnt", "mem", "tt", "ens"):
        assert chunk(**{name: nul}) == -3, name
    assert lib.tmg_ens_iscale_chunk(one, _i64(4, 1), one, _i64(4, 1), one, _i64(0, 0, 2, 1), one, one, one, one, None, nul) == -3
    sbase = [S, B, Hh, Ww, Cc, Kn, L]                                          # S, B, H, W, C, K, L

    def step(dims=sbase, cnt=one, tgt=one, td=(4, 1), thr=one, ev=(0, 0, 2, 1), ens=one):
        return lib.tmg_ens_iscale_step(cnt, tgt, _i64(*td) if td else None, thr, _i64(*ev) if ev else None, ens,
                                       _i64(*dims) if dims else None, nul)

    for pos, bad, code in ((0, 0, -1), (1, 0, -1), (2, 0, -1), (4, 1, -1), (4, 5, -1), (5, 5, -1), (6, 0, -1), (6, 7, -1), (0, 1025, -2),
                           (1, 65536, -2)):
        d = list(sbase)
        d[pos] = bad
        assert step(d) == code, (pos, bad)
    assert step(td=(2, 0)) == -1 and step(ev=(3, 0, 2, 1)) == -1 and step(td=(1 << 31, 0)) == -2
    assert step(dims=None) == -3 and step(td=None) == -3 and step(ev=None) == -3
    assert step(cnt=nul) == -3 and step(tgt=nul) == -3 and step(thr=nul) == -3 and step(ens=nul) == -3


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_iscale_args_follow_the_event_rules_and_check_levels():
    import tmg_ops as ops
    ev, L = ops.iscale_args([(0, 0.0, "<"), (2, 1.5, ">")], 5, 3, 64, 64)
    assert [tuple(e) for e in ev] == [(0, 0.0, "<"), (2, 1.5, ">")] and L == 5 and type(L) is int
    assert ops.iscale_args(((0, 0.0, "<"),), np.int64(6), 3, 1, 1)[1] == 6
    for hw, want in (((1, 1), 1), ((3, 130), 1), ((4, 4), 2), ((7, 9), 2), ((63, 65), 5), ((64, 64), 6), ((70, 70), 6), ((512, 1024), 6)):
        assert ops.iscale_args(((0, 0.0, "<"),), None, 3, *hw)[1] == want, hw
    for events in ((), ((3, 0.0, "<"),), ((0, float("nan"), "<"),), ((0, 0.0, "="),), ((True, 0.0, "<"),), ((0, 0.0, "<"),) * 5):
        with pytest.raises(ValueError) as a:
            ops.iscale_args(events, 3, 3, 8, 8)
        with pytest.raises(ValueError) as b:
            ops.event_args(events, (1,), 3)
        assert str(a.value) == str(b.value)                                   # event_args' own messages
    for bad in (0, 7, -1, True, 4.0, "4"):
        with pytest.raises(ValueError, match=r"levels is an integer in 1\.\.6"):
            ops.iscale_args(((0, 0.0, "<"),), bad, 3, 8, 8)


def test_constructor_limits_come_with_their_numbers_before_any_device_work():
    import tmg_ops as ops
    from utils import utils
    ok = dict(members=5, B=2, C=3, Hh=8, Ww=9, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3))
    for kw, msg in ((dict(C=1), "2 <= C <= 4"), (dict(C=5, out_mu=torch.zeros(5), out_std=torch.ones(5)), "2 <= C <= 4"),
                    (dict(steps=0), "steps >= 1"), (dict(steps=True), "steps >= 1"), (dict(steps=2.0), "steps >= 1"),
                    (dict(members=0), "members"), (dict(members=1025), "1024"), (dict(B=0), "B, H, W >= 1"), (dict(Hh=0), "B, H, W >= 1"),
                    (dict(B=65536), "at most 65535 cases, got 65536"),
                    (dict(members=1024, Hh=1, Ww=1 << 25, levels=6), r"S\^2 4\^L H_pad W_pad = 1024\^2 \* 4\^6 \* 2147483648"),
                    (dict(members=32, Hh=1024, Ww=1024, steps=64), r"S HW Tk = 32 \* 1048576 \* 64"),
                    (dict(levels=0), "levels"), (dict(levels=7), "levels"), (dict(levels=2.0), "levels"), (dict(events=()), "at least one"),
                    (dict(out_std=torch.tensor([1.0, 0.0, 1.0])), "strictly positive"), (dict(u=torch.zeros(2, 3)), "strictly positive")):
        with pytest.raises(ValueError, match=msg):
            ops.EnsembleIntensityScale(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="not a GPU"):
        ops.EnsembleIntensityScale(**dict(ok, device="cpu"))
    with pytest.raises(ValueError):                                           # the argument error wins over the device error
        ops.EnsembleIntensityScale(**dict(ok, device="cpu", levels=0))
    for kw in (dict(events=()), dict(events=((3, 0.0, "<"),)), dict(levels=0), dict(levels=2.0), dict(levels=True)):
        with pytest.raises(ValueError):
            utils.modelPredIntensityScale(None, None, None, None, **kw)
    m = torch.zeros(1, 2, 3, 2, dtype=torch.int64)
    t, e = torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3, 2, dtype=torch.int64)
    ops.iscale_outputs(m, t, e, 2, 7)
    for a in ((m.double(), t, e, 2, 7), (m, t, e, 3, 7), (m, t[..., :2], e, 2, 7), (m, t, e[..., :1], 2, 7), (m, t, e, 2, 0), (m, t, e, 2, 7, 0),
              (m, t, e, 2, 1 << 30), (m[..., :1, :], t[..., :1], e[..., :1, :], 2, 7)):
        with pytest.raises(ValueError):
            ops.iscale_outputs(*a)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.SMALL)
def test_the_reference_equals_the_explicit_haar_components_and_the_identities(case):
    S, B, Cc, hw, Kn, L, kind, _ = case
    xs, tgt = K.make_inputs(case, 7)
    if kind == "smooth":
        K.plant_nonfinite(xs, tgt, 8)
    ev = K.events_for(Cc, Kn)
    thr = K.thresholds(ev, B)
    ref = K.reference(xs, tgt, thr, ev, L)
    Im, o = K.indicators(xs, thr, ev), K.indicators(tgt, thr, ev)               # [Tk, S, B, K, H, W], [Tk, B, K, H, W]
    Tk = xs.shape[0]
    assert ref["iscale_member_raw"].shape == (B, Tk, Kn, S, L + 1, 2) and ref["iscale_ens_raw"].shape == (B, Tk, Kn, L + 1, 2)
    assert ref["iscale_target_raw"].shape == (B, Tk, Kn, L + 1) and all(v.dtype == np.int64 for v in ref.values())
    mism = (Im != o[:, None]).sum((-2, -1)).transpose(2, 0, 3, 1)              # [Tk, S, B, K] -> [B, Tk, K, S]
    K.check_identities(ref, S, hw[0] * hw[1], mism)
    A, X = ref["iscale_member_raw"][..., 0], ref["iscale_member_raw"][..., 1]
    Cc_, AN, XN = ref["iscale_target_raw"], ref["iscale_ens_raw"][..., 0], ref["iscale_ens_raw"][..., 1]
    n = Im.sum(1)
    assert np.array_equal(AN[..., 0], (n * n).sum((-2, -1)).transpose(1, 0, 2))
    for t in range(Tk):
        for b in range(B):
            for k in range(Kn):
                # the sums of the explicit difference fields, and the squared norms of their explicit Haar components
                assert np.array_equal(K.level_sums(o[t, b, k], L), Cc_[b, t, k])
                assert np.array_equal(K.haar_energies(o[t, b, k], L), K.numerators(Cc_[b, t, k]))
                dn = n[t, b, k] - S * o[t, b, k]
                DN = AN[b, t, k] - 2 * S * XN[b, t, k] + S * S * Cc_[b, t, k]
                assert np.array_equal(K.level_sums(dn, L), DN) and np.array_equal(K.haar_energies(dn, L), K.numerators(DN))
                sp = np.zeros(L + 1, np.int64)
                for m in range(S):
                    d = Im[t, m, b, k] - o[t, b, k]
                    D = A[b, t, k, m] - 2 * X[b, t, k, m] + Cc_[b, t, k]
                    assert np.array_equal(K.level_sums(d, L), D) and np.array_equal(K.haar_energies(d, L), K.numerators(D))
                    assert np.array_equal(K.haar_energies(Im[t, m, b, k], L), K.numerators(A[b, t, k, m]))
                    sp += K.haar_energies(S * Im[t, m, b, k] - n[t, b, k], L)   # sum_m |S I_m - n|^2 = S (S sum_m A - AN)
                assert np.array_equal(sp, S * K.numerators(S * A[b, t, k].sum(0) - AN[b, t, k]))


def test_haar_components_are_orthogonal_and_sum_to_the_field():
    rs = np.random.RandomState(3)
    for hw, L in (((5, 7), 2), ((8, 8), 3), ((3, 17), 4), ((1, 1), 1)):
        z = rs.standard_normal(hw)
        comps = K.haar_components(z, L)
        assert len(comps) == L + 1
        total = sum(comps)
        assert np.allclose(total[:hw[0], :hw[1]], z, atol=1e-12) and np.allclose(total.sum(), z.sum(), atol=1e-10)
        for i in range(L + 1):
            for j in range(i):
                assert abs(float((comps[i] * comps[j]).sum())) < 1e-10


def test_known_answers_on_fields_written_by_hand():
    # one pixel in an 4 x 4 field: level sums 1, 1, 1; components 3/4 at size 2, 3/16 at size 4, 1/16 in the remainder
    z = np.zeros((4, 4), np.int64)
    z[1, 2] = 1
    assert K.level_sums(z, 2).tolist() == [1, 1, 1] and K.numerators([1, 1, 1]).tolist() == [3, 3, 1]
    # a 2 x 2 block aligned with the grid lives in the coarser scales only; shifted by one pixel it has energy at size 2
    z = np.zeros((4, 4), np.int64)
    z[0:2, 2:4] = 1
    assert K.level_sums(z, 2).tolist() == [4, 16, 16] and K.numerators([4, 16, 16]).tolist() == [0, 48, 16]
    z = np.zeros((4, 4), np.int64)
    z[1:3, 1:3] = 1
    assert K.level_sums(z, 2).tolist() == [4, 4, 16] and K.numerators([4, 4, 16]).tolist() == [12, 0, 16]
    # a ragged field: the block cut by the border holds fewer pixels
    assert K.level_sums(np.ones((3, 5), np.int64), 2).tolist() == [15, 4 * 4 + 4 * 4 + 2 * 2 + 2 * 2 + 2 * 2 + 1, 12 * 12 + 3 * 3]


@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_the_identities_hold_on_every_case(idx):
    S, B, Cc, hw, Kn, L, kind, _ = K.TABLE[idx]
    xs, tgt = K.inputs(idx)
    ev = K.events_for(Cc, Kn)
    thr = K.thresholds(ev, B)
    ref = K.case_reference(idx)
    mism = (K.indicators(xs, thr, ev) != K.indicators(tgt, thr, ev)[:, None]).sum((-2, -1)).transpose(2, 0, 3, 1)
    K.check_identities(ref, S, hw[0] * hw[1], mism)
    if Kn == 4:                                                               # every pixel in, no pixel in
        assert bool((ref["iscale_target_raw"][:, :, 2, 0] == hw[0] * hw[1]).all()) and bool((ref["iscale_member_raw"][:, :, 3] == 0).all())


# ---- iscale_outputs ---------------------------------------------------------------------------------------------------------------------
def _outputs(ref, S, HW, steps=1):
    import tmg_ops as ops
    return {k: v.numpy() for k, v in ops.iscale_outputs(*[torch.from_numpy(np.array(ref[k])) for k in K.RAW_KEYS], S, HW, steps).items()}


@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_iscale_outputs_agree_with_the_fp64_restatement(idx):
    S, B, Cc, hw, Kn, L, kind, _ = K.TABLE[idx]
    ref = K.case_reference(idx)
    HW = hw[0] * hw[1]
    got = _outputs(ref, S, HW)
    assert set(got) == set(K.FLOAT_KEYS)
    worst = K.check_floats(got, K.host_reference(ref, S, HW), K.FLOAT_KEYS, "case %d" % idx)
    Tk = len(K.TIMED)
    assert got["iscale_mse"].shape == (B, Tk, Kn, S, L + 1) and got["iscale_energy"].shape == (B, Tk, Kn, S + 1, L + 1)
    assert got["iscale_brier"].shape == (B, Tk, Kn, L + 1) and got["iscale_spread_skill"].shape == (B, Tk, Kn, L + 1)
    pooled = {k: ref[k][:, 1:].sum(1) for k in K.RAW_KEYS}
    worst = max(worst, K.check_floats(_outputs(pooled, S, HW, 2), K.host_reference(pooled, S, HW, 2), K.FLOAT_KEYS, "case %d pooled" % idx))
    # the components sum to the level-0 scores, and the spread is the mean member mse minus the brier component
    A, X = ref["iscale_member_raw"][..., 0], ref["iscale_member_raw"][..., 1]
    D0 = (A - 2 * X + ref["iscale_target_raw"][..., None, :])[..., 0]
    assert np.allclose(got["iscale_mse"].astype(np.float64).sum(-1), D0 / HW, rtol=1e-6, atol=1e-9)
    assert np.allclose(got["iscale_spread"], got["iscale_mse"].astype(np.float64).mean(-2) - got["iscale_brier"], rtol=0, atol=1e-6)
    assert bool((got["iscale_spread"] >= 0).all()) and bool((got["iscale_brier"] >= 0).all()) and bool((got["iscale_mse"] >= 0).all())
    print("case %d: worst share of the float tolerance %.3f" % (idx, worst))


@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_the_brier_components_sum_to_the_brier_score_of_the_reliability_tables(idx):
    import tmg_ops as ops
    S, B, Cc, hw, Kn, L, kind, _ = K.TABLE[idx]
    xs, tgt = K.inputs(idx)
    ev = K.events_for(Cc, Kn)
    thr = K.thresholds(ev, B)
    n = K.indicators(xs, thr, ev).sum(1)                                       # [Tk, B, K, H, W]
    o = K.indicators(tgt, thr, ev)
    cnt = np.stack([(n == j).sum((-2, -1)) for j in range(S + 1)], -1)          # the reliability tables of the same data
    hit = np.stack([((n == j) & (o == 1)).sum((-2, -1)) for j in range(S + 1)], -1)
    brier = ops.event_table_scores(torch.from_numpy(cnt), torch.from_numpy(hit), S)["brier"].numpy().transpose(1, 0, 2)    # [B, Tk, K]
    ref = K.case_reference(idx)
    got = _outputs(ref, S, hw[0] * hw[1])
    total = got["iscale_brier"].astype(np.float64).sum(-1)
    # each of the non-negative components is rounded to float32 once: the errors sum to at most 2^-24 of their sum
    assert bool((np.abs(total - brier) <= K.U24 * np.abs(brier) + K.TOL_ABS).all())
    # in integers the sum is exact: sum_c num_c 4^(L - c) = 4^L DN[0], and DN[0] is the tables' numerator
    j = np.arange(S + 1)
    num = (cnt * j * j - 2 * S * hit * j + S * S * hit).sum(-1).transpose(1, 0, 2)
    en, tt = ref["iscale_ens_raw"], ref["iscale_target_raw"]
    assert np.array_equal(en[..., 0, 0] - 2 * S * en[..., 0, 1] + S * S * tt[..., 0], num)
    assert np.array_equal((cnt * j * j).sum(-1).transpose(1, 0, 2), en[..., 0, 0])     # sum n^2 from rel_count is AN[0]


def test_iscale_outputs_known_answers():
    import tmg_ops as ops
    S, L, HW = 2, 2, 16
    # 4 x 4 field; member 0 is the target's aligned 2 x 2 block moved to another aligned place, member 1 equals the target
    o = np.zeros((4, 4), np.int64)
    o[0:2, 0:2] = 1
    m0 = np.zeros((4, 4), np.int64)
    m0[2:4, 2:4] = 1
    I = np.stack([m0, o])
    mem = np.array([[[int((K.block_sums(I[m], l) ** 2).sum()), int((K.block_sums(I[m], l) * K.block_sums(o, l)).sum())] for l in range(L + 1)]
                    for m in range(S)], dtype=np.int64)
    tt = K.level_sums(o, L)
    n = I.sum(0)
    en = np.array([[int((K.block_sums(n, l) ** 2).sum()), int((K.block_sums(n, l) * K.block_sums(o, l)).sum())] for l in range(L + 1)], dtype=np.int64)
    out = ops.iscale_outputs(torch.from_numpy(mem), torch.from_numpy(tt), torch.from_numpy(en), S, HW)
    assert all(v.dtype == torch.float32 for v in out.values()) and set(out) == set(K.FLOAT_KEYS)
    # member 0: 8 mismatched pixels, none of the error at block size 2, all of it at size 4; member 1: no error at all
    assert out["iscale_mse"][0].tolist() == [0.0, 0.5, 0.0] and out["iscale_mse"][1].tolist() == [0.0, 0.0, 0.0]
    assert out["iscale_skill"][0].tolist() == [1.0, 1.0 - 3 * 0.5 / 0.375, 1.0] and out["iscale_skill"][1].tolist() == [1.0, 1.0, 1.0]
    assert out["iscale_energy"].tolist() == [[0.0, 0.1875, 0.0625]] * 3 and out["iscale_energy_bias"][:, 1:].tolist() == [[0.0, 0.0]] * 2
    assert bool(torch.isnan(out["iscale_energy_bias"][:, 0]).all())            # no structure at size 2 on either side: 0 / 0
    assert out["iscale_brier"].tolist() == [0.0, 0.125, 0.0] and out["iscale_spread"].tolist() == [0.0, 0.125, 0.0]
    assert out["iscale_spread_skill"][1] == 1.0 and bool(torch.isnan(out["iscale_spread_skill"][[0, 2]]).all())
    # an event no pixel is in, on both sides: every ratio is 0 / 0
    z = ops.iscale_outputs(torch.zeros(S, L + 1, 2, dtype=torch.int64), torch.zeros(L + 1, dtype=torch.int64),
                           torch.zeros(L + 1, 2, dtype=torch.int64), S, HW)
    for key in ("iscale_skill", "iscale_energy_bias", "iscale_brier_skill", "iscale_spread_skill"):
        assert bool(torch.isnan(z[key]).all()), key
    for key in ("iscale_mse", "iscale_energy", "iscale_brier", "iscale_spread"):
        assert bool((z[key] == 0).all()), key


# ---- NaN placement ----------------------------------------------------------------------------------------------------------------------
def test_nan_is_in_no_event_whatever_the_direction():
    case = (2, 1, 3, (5, 7), 4, 2, "int", False)
    S, B, Cc, hw, Kn, L, _, _ = case
    ev = K.events_for(Cc, Kn)
    thr = K.thresholds(ev, B)
    xs, tgt = K.make_inputs(case, 5)
    xs[:], tgt[:] = np.nan, np.nan                                            # none in: every table is zero
    ref = K.reference(xs, tgt, thr, ev, L)
    assert all(not v.any() for v in ref.values())
    allin = K.reference(xs, tgt, thr, ev, L, "nan_in_event")                   # the mutation: all in, the tables of a full field
    full = K.level_sums(np.ones(hw, np.int64), L)
    assert np.array_equal(allin["iscale_target_raw"], np.broadcast_to(full, allin["iscale_target_raw"].shape))
    assert np.array_equal(allin["iscale_ens_raw"][..., 0], S * S * allin["iscale_target_raw"])


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate", K.MUTATIONS)
def test_named_mutations_are_caught(mutate):
    """Every mutation changes at least one array the GPU test compares, on the case set; the ones that touch ties or NaN alone must
    change nothing on continuous finite data, which shows that they are mutations of that rule and nothing else."""
    caught = []
    for idx, case in enumerate(K.TABLE):
        S, B, Cc, hw, Kn, L, kind, _ = case
        xs, tgt = K.inputs(idx)
        if mutate == "nan_in_event":
            xs, tgt = xs.copy(), tgt.copy()
            K.plant_nonfinite(xs, tgt, 50 + idx)
        ev = K.events_for(Cc, Kn)
        thr = K.thresholds(ev, B)
        ref = K.reference(xs, tgt, thr, ev, L)
        assert not K.mismatches(ref, ref, K.RAW_KEYS)
        bad = K.mismatches(K.reference(xs, tgt, thr, ev, L, mutate), ref, K.RAW_KEYS)
        if kind == "smooth" and mutate == "non_strict":
            assert not bad, (idx, bad)                                        # no ties on continuous data
        caught.append(bool(bad))
    assert any(caught), mutate
    if mutate == "remainder_dropped":
        assert all(caught), (mutate, caught)
    if mutate in ("origin_shifted", "previous_target"):
        assert all(c for c, case in zip(caught, K.TABLE) if case[3] != (1, 1)), (mutate, caught)


def test_the_comparison_sees_one_unit_one_dtype_and_one_key():
    ref = K.case_reference(4)
    for k in K.RAW_KEYS:
        off = {n: v.copy() for n, v in ref.items()}
        off[k].reshape(-1)[-1] += 1
        assert K.mismatches(off, ref, K.RAW_KEYS) == [k]
        cast = dict(ref)
        cast[k] = ref[k].astype(np.int32)
        assert K.mismatches(cast, ref, K.RAW_KEYS) == [k]
    assert K.mismatches({k: v for k, v in ref.items() if k != "iscale_ens_raw"}, ref, K.RAW_KEYS) == ["iscale_ens_raw"]
