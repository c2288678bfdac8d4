"""CPU-side checks of the ensemble field ranks: the kernel entries are declared in their own header, listed apart and exported; the
signatures of the three Python layers; the plan query's values and the codes the step entry returns before any launch; every argument
error without a GPU; the band-depth identity of the reference (tests/fieldrank_cases.py) against a brute-force pair count; the known
answers; tmg_ops.fieldrank_hist and tmg_ops.fieldrank_outputs against their restatements; and the sensitivity of the comparison the
GPU test uses: every named mutation of the reference is caught."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import fieldrank_cases as K

NAMES = ["tmg_ens_frank_plan", "tmg_ens_frank_step"]
c_i64 = ctypes.c_int64


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_frank.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.FRANK_EXPORTS == NAMES
    assert "frank" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    P64 = ctypes.POINTER(c_i64)
    vp = ctypes.c_void_p
    want = {"tmg_ens_frank_plan": [P64, P64], "tmg_ens_frank_step": [vp, vp, c_i64, vp, vp, vp, P64, vp]}
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.FRANK_ARGTYPES[name] == want[name]
    assert "tmg_frank.hip" in tmg_hip.SOURCES and "tmg_frank.hip" not in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_frank.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_frank\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_frank.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in code
    # no atomics, no inline assembly, nothing printed or asserted in a kernel, and no lane leaves before the barriers
    assert not re.search(r"\basm\b|printf|assert\s*\(|atomic|while\s*\(", code)
    step = code[code.index("ens_frank_step_kernel"):code.index("ens_frank_fold_kernel")]
    assert "__syncthreads" in step and not re.search(r"\breturn\b", step)


def test_signatures():
    from utils import utils
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredFieldRanks).parameters
    assert list(sig) == old + ["groups"] and sig["groups"].default == ((0, 1), (2,))
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleFieldRanks.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "groups"] and init["groups"].default == ((0, 1), (2,))
    add = inspect.signature(tmg_ops.EnsembleFieldRanks.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleFieldRanks, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.fieldrank_hist).parameters) == ["below", "equal", "S"]
    import tmg_hip
    assert list(inspect.signature(tmg_hip.ens_frank_plan).parameters)[:4] == ["S", "B", "C", "HW"]
    assert list(inspect.signature(tmg_hip.ens_frank_step).parameters) == ["xs", "ws", "pre_raw", "outside", "tout", "t", "t_before", "flags"]
    for doc in (utils.modelPredFieldRanks.__doc__, tmg_ops.EnsembleFieldRanks.__doc__):
        assert "Non-finite" in doc or "non-finite" in doc
        assert "out_std" in doc                                               # why no scale is an argument
    for word in ("minimum-spanning-tree", "functional boxplot", "pixel boxes", "pooling over cases", "1024 members"):
        assert word in utils.modelPredFieldRanks.__doc__, word


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,Cc,HW", [(1, 1, 2, 1), (7, 3, 3, 35), (8, 2, 4, 256), (33, 3, 3, 257), (1024, 1, 2, 35), (32, 4, 3, 65536)])
def test_plan_values(S, B, Cc, HW):
    import tmg_hip
    p = tmg_hip.ens_frank_plan(S, B, Cc, HW)
    nblk = -(-HW // 256)
    assert p["nblk"] == nblk and p["grid"] == (nblk, Cc, B) and p["threads"] == 256
    assert p["rec_words"] == 2 * (S + 1) + 1 and p["ws_words"] == B * Cc * nblk * (2 * (S + 1) + 1)


def test_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    plan = (c_i64 * 7)()
    good = [5, 2, 3, 72]
    assert lib.tmg_ens_frank_plan(_i64(*good), plan) == 0
    for pos, bad in ((0, 0), (1, 0), (2, 1), (2, 5), (3, 0)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_frank_plan(_i64(*d), plan) == -1, (pos, bad)
    for pos, bad in ((0, 1025), (1, 65536), (3, (1 << 31) - 256)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_frank_plan(_i64(*d), plan) == -2, (pos, bad)
    assert lib.tmg_ens_frank_plan(_i64(1024, 65535, 4, 1 << 20), plan) == -2       # the member buffer is over the index range
    assert lib.tmg_ens_frank_plan(None, plan) == -3 and lib.tmg_ens_frank_plan(_i64(*good), None) == -3
    assert tmg_hip.ens_frank_plan(0, 1, 2, 5, code=True)[1] == -1
    with pytest.raises(RuntimeError):
        tmg_hip.ens_frank_plan(1025, 1, 2, 5)
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                                  # never dereferenced: every code comes before a launch
    S, B, HW, Cc, Tk = 5, 2, 72, 3, 4
    words = tmg_hip.ens_frank_plan(S, B, Cc, HW)["ws_words"]

    def step(dims=(S, B, HW, Cc, Tk, 1, 0, 1), xs=one, ws=one, n=words, pre=one, out=one, tout=one):
        return lib.tmg_ens_frank_step(xs, ws, n, pre, out, tout, _i64(*dims), nul)

    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 1), (3, 5), (4, 0), (5, -1), (5, Tk), (6, -1)):
        d = [S, B, HW, Cc, Tk, 1, 0, 1]
        d[pos] = bad
        assert step(tuple(d)) == -1, (pos, bad)
    for pos, bad in ((0, 1025), (1, 65536), (2, (1 << 31) - 256)):
        d = [S, B, HW, Cc, Tk, 1, 0, 1]
        d[pos] = bad
        assert step(tuple(d)) == -2, (pos, bad)
    assert step((1024, 4, 64, 3, 1 << 28, 1, 0, 1)) == -2                      # pre_raw is over the index range
    assert step(xs=nul) == -3 and step(ws=nul) == -3 and step(pre=nul) == -3 and step(out=nul) == -3 and step(tout=nul) == -3
    assert step((S, B, HW, Cc, Tk, 1, 0, 0), tout=nul, n=words - 1) == -1      # an untimed step without tout passes the null check
    assert step(n=words - 1) == -1 and step(n=0) == -1
    assert lib.tmg_ens_frank_step(one, one, words, one, one, one, None, nul) == -3


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work():
    import tmg_ops as ops
    from utils import utils
    ok = dict(members=5, B=2, C=3, Hh=8, Ww=9, steps=2, device="cuda")
    bad = [dict(C=1), dict(C=5), dict(members=0), dict(members=1025), dict(steps=0), dict(B=0), dict(Hh=0), dict(Ww=0), dict(groups=()),
           dict(groups=((),)), dict(groups=((0, 0),)), dict(groups=((0, 1), (1,))), dict(groups=((3,),)), dict(groups=((-1,),)),
           dict(groups=((True,),)), dict(groups=((0.0,),)), dict(groups=3), dict(C=2), dict(C=2, groups=((0, 1), (2,)))]
    for kw in bad:                                                            # (C = 2 with the default groups names channel 2)
        with pytest.raises(ValueError):
            ops.EnsembleFieldRanks(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="not a GPU"):
        ops.EnsembleFieldRanks(**dict(ok, device="cpu"))
    with pytest.raises(ValueError):                                           # the argument error wins over the device error
        ops.EnsembleFieldRanks(**dict(ok, device="cpu", members=0))
    for groups in ((), ((0, 0),), ((3,),), 7):
        with pytest.raises(ValueError):
            utils.modelPredFieldRanks(None, None, None, None, groups=groups)
    z = torch.zeros(1, 2, 1, dtype=torch.int64)
    for below, equal, S in ((z, z, 0), (z[0], z[0], 3), (z, z[:, :1], 3), (z - 1, z, 3), (z, z - 1, 3), (z + 3, z + 1, 3)):
        with pytest.raises(ValueError):
            ops.fieldrank_hist(below, equal, S)
    raw = torch.zeros(1, 2, 3, 4, 2, dtype=torch.int64)
    oc, tc = torch.zeros(1, 2, 3, dtype=torch.int64), torch.zeros(1, 3, 2, 2, dtype=torch.int64)
    ops.fieldrank_outputs(raw, oc, tc, ((0, 1), (2,)), [1])
    for a in ((raw.double(), oc, tc, ((0,),), [0]), (raw, oc[:, :1], tc, ((0,),), [0]), (raw, oc, tc, ((0,),), []), (raw, oc, tc, ((0,),), [2]),
              (raw, oc, tc, ((3,),), [0]), (raw, oc, tc[0], ((0,),), [0])):
        with pytest.raises(ValueError):
            ops.fieldrank_outputs(*a)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [True, False])
@pytest.mark.parametrize("S", range(1, 10))
def test_band_depth_equals_the_brute_force_pair_count(S, ties):
    xs, tgt = K.make_inputs(S, 2, 2, 3, 5, 40 + S, ties)
    A, D, O = K.pixel_terms(xs, tgt)
    assert np.array_equal(D, K.band_depth_brute(xs, tgt))
    x = np.concatenate([xs, tgt[:, None]], axis=1)
    assert np.array_equal(O, (tgt < xs.min(1)) | (tgt > xs.max(1)))
    if not ties:                                                              # without ties D = lt gt and A = 2 rank
        rank = np.argsort(np.argsort(x, axis=1), axis=1)
        assert np.array_equal(A, 2 * rank) and np.array_equal(D, rank * (S - rank))
    if S == 1:
        assert not D.any()


def _host(ref, groups, t_start):
    """tmg_ops.fieldrank_outputs on the reference's device-side sums -> dict of numpy arrays."""
    import tmg_ops as ops
    out = ops.fieldrank_outputs(*[torch.from_numpy(ref[k]) for k in K.DEVICE_KEYS], groups, list(range(t_start, K.T)))
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("idx,ties", [(K.SWEEP.index((7, 3, 3, (5, 7))), True), (K.SWEEP.index((16, 1, 4, (16, 17))), False),
                                      (K.SWEEP.index((2, 3, 2, (5, 7))), True), (K.SWEEP.index((1, 1, 3, (5, 7))), True)])
def test_host_outputs_equal_the_reference(idx, ties):
    S, B, Cc, hw = K.SWEEP[idx]
    xs, tgt = K.inputs(idx, ties)
    t_start = K.features(idx)[0]
    ref = K.reference(xs, tgt, t_start, K.GROUPS[Cc])
    K.assert_equal(_host(ref, K.GROUPS[Cc], t_start), ref, "host outputs %s" % (K.SWEEP[idx],))
    Gn = len(K.GROUPS[Cc])
    assert ref["avg_rank_hist"].shape == (B, Gn, S + 1) and ref["depth_median"].shape == (B, K.T, Gn)
    assert ref["traj_depth_prerank"].shape == (B, Gn, S + 1) and ref["time_outside_frac"].shape == (B, Cc) + hw


def test_known_answers():
    S, B, Cc, Hh, Ww = 6, 2, 3, 4, 5
    HW = Hh * Ww
    groups = K.GROUPS[Cc]
    xs, tgt = K.make_inputs(S, B, Cc, Hh, Ww, 3)
    # a target above every member everywhere
    high = (xs.max(1) + 1).astype(K.F32)
    out = _host(K.reference(xs, high, 0, groups), groups, 0)
    assert (out["avg_rank_below"] == S).all() and (out["avg_rank_equal"] == 0).all()
    assert (out["depth_prerank"][..., S] == 0).all() and (out["outside_count"] == HW).all() and (out["outside_frac"] == 1.0).all()
    assert (out["depth_rank_below"] == 0).all() and (out["time_outside_count"] == K.T).all()
    assert (out["avg_rank_hist"][..., S] == K.T).all() and (out["avg_rank_hist"][..., :S] == 0).all()
    # all rows equal
    same = np.ascontiguousarray(np.broadcast_to(tgt[:, None], xs.shape))
    A, D, O = K.pixel_terms(same, tgt)
    assert (A == S).all() and (D == K.choose2(S)).all() and not O.any()
    out = _host(K.reference(same, tgt, 1, groups), groups, 1)
    for kind in ("avg", "depth"):
        assert (out[kind + "_rank_equal"] == S).all() and (out[kind + "_rank_below"] == 0).all()
        h = np.zeros(S + 1)
        for _ in range(K.T - 1):
            h += 1.0 / (S + 1)
        assert np.array_equal(out[kind + "_rank_hist"], np.broadcast_to(h, (B, len(groups), S + 1)))
    assert (out["depth_median"] == 0).all() and (out["traj_depth_median"] == 0).all()
    # S = 1: no pair of other rows, D = 0
    one = _host(K.reference(xs[:, :1], tgt, 0, groups), groups, 0)
    assert not one["depth_prerank"].any() and (one["depth_rank_equal"] == 1).all() and (one["depth_rank_hist"] == K.T / 2.0).all()
    assert (one["outside_count"] == HW).all()                                 # continuous data: the target never equals the member


# ---- fieldrank_hist ---------------------------------------------------------------------------------------------------------------------
def test_fieldrank_hist_sums_to_the_steps_and_equals_the_loop():
    import tmg_ops as ops
    g = torch.Generator().manual_seed(5)
    for S in (1, 2, 7, 33):
        below = torch.randint(0, S + 1, (3, 6, 2), generator=g)
        equal = (torch.rand(3, 6, 2, generator=g) * (S - below + 1).double()).floor().long().clamp(max=S)
        equal = torch.minimum(equal, S - below)
        h = ops.fieldrank_hist(below, equal, S)
        assert h.dtype == torch.float64 and tuple(h.shape) == (3, 2, S + 1)
        assert np.array_equal(h.numpy(), K.hist_loop(below.numpy(), equal.numpy(), S))
        assert float((h.sum(-1) - 6).abs().max()) <= 6 * 2.0 ** -50
    assert torch.equal(ops.fieldrank_hist([[[2]]], [[[0]]], 3), torch.tensor([[[0.0, 0.0, 1.0, 0.0]]], dtype=torch.float64))
    assert tuple(ops.fieldrank_hist(torch.zeros(2, 0, 3), torch.zeros(2, 0, 3), 4).shape) == (2, 3, 5)


def test_permuting_the_members_permutes_the_preranks_and_nothing_else():
    idx = K.SWEEP.index((7, 3, 3, (5, 7)))
    groups = K.GROUPS[3]
    for ties in (True, False):
        xs, tgt = K.inputs(idx, ties)
        perm = np.random.RandomState(2).permutation(7)
        a, b = K.reference(xs, tgt, 1, groups), K.reference(np.ascontiguousarray(xs[:, perm]), tgt, 1, groups)
        ha, hb = _host(a, groups, 1), _host(b, groups, 1)
        K.assert_equal(hb, b, "permuted")
        full = np.concatenate([perm, [7]])
        for k, v in ha.items():
            if k == "pre_raw":
                assert np.array_equal(v[:, :, :, full], hb[k])
            elif k.endswith("_prerank"):
                assert np.array_equal(v[..., full], hb[k]), k
            elif k.endswith("depth_median"):
                assert np.array_equal(np.take_along_axis(ha[k.replace("median", "prerank")], v[..., None], -1),
                                      np.take_along_axis(hb[k.replace("median", "prerank")], hb[k][..., None], -1)), k
            else:
                assert np.array_equal(v, hb[k]), k


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate", K.MUTATIONS)
def test_named_mutations_are_caught(mutate):
    """On tie-heavy data every mutation changes what the GPU test compares; on continuous data the ones that touch ties alone
    ('le', 'open') must not, which shows that they are mutations of the tie handling and nothing else."""
    idx = K.SWEEP.index((7, 3, 3, (5, 7)))
    groups = K.GROUPS[3]
    xs, tgt = K.inputs(idx, True)
    ref = K.reference(xs, tgt, 1, groups)
    assert not K.mismatches(ref, ref)
    bad = K.mismatches(K.reference(xs, tgt, 1, groups, mutate), ref)
    assert "pre_raw" in bad, (mutate, bad)
    xc, tc = K.inputs(idx, False)
    cont = K.mismatches(K.reference(xc, tc, 1, groups, mutate), K.reference(xc, tc, 1, groups))
    assert ("pre_raw" in cont) == (mutate not in ("le", "open")), (mutate, cont)


def test_the_comparison_sees_one_unit_one_dtype_and_one_key():
    idx = K.SWEEP.index((2, 1, 2, (5, 7)))
    xs, tgt = K.inputs(idx, True)
    ref = K.reference(xs, tgt, 0, K.GROUPS[2])
    for k in ref:
        off = {n: v.copy() for n, v in ref.items()}
        off[k].reshape(-1)[-1] += 1
        assert K.mismatches(off, ref) == [k]
        cast = dict(ref)
        cast[k] = ref[k].astype(np.float32)
        assert K.mismatches(cast, ref) == [k]
    assert K.mismatches({k: v for k, v in ref.items() if k != "pre_raw"}, ref) == ["pre_raw"]
    assert K.mismatches(dict(ref, extra=ref["pre_raw"]), ref) == ["extra"]
