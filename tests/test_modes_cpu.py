"""CPU-side checks of the ensemble POD: the kernel entries are declared in their own header, listed apart and exported; pod_basis
against numpy's SVD of the snapshot matrix; every argument error without a GPU; the slice plan covers every pixel, does not change
with the row count and returns its codes before any launch; the case tables of tests/modes_cases.py reach every branch of the plan;
and the references and bounds are sensitive to the defects the GPU comparison has to catch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import modes_cases as K

NAMES = ["tmg_ens_pod_plan", "tmg_ens_pod_project"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_pod.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.POD_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert len(re.findall(r'^#include "tmglow_hip_pod\.h"$', main, re.M)) == 1 and main.count("tmglow_hip_pod.h") == 1
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.GRAM_EXPORTS, tmg_hip.PDF_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert name not in main and hasattr(lib, name)
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_pod.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_pod.hip"))
    assert "tmg_pod" in open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read()


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredModes).parameters
    assert list(sig) == old + ["modes", "channels"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, 8, (0, 1)]
    init = inspect.signature(tmg_ops.EnsembleModes.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_std", "u", "channels", "mean", "basis"]
    assert init["u"].default is None and init["channels"].default == (0, 1)
    add = inspect.signature(tmg_ops.EnsembleModes.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleModes, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.pod_basis).parameters)[:4] == ["series", "a", "channels", "K"]
    assert list(inspect.signature(tmg_hip.ens_pod_plan).parameters) == ["S", "B", "Cg", "HW", "K"]


# ---- pod_basis against the SVD of the snapshot matrix ----------------------------------------------------------------------------------
def _svd_case():
    B, Tn, Cc, hw, chs, Kk = 2, 12, 3, (6, 10), (0, 1), 6
    series = K.wave_series(B, Tn, Cc, hw, 5, noise=1e-3)
    a = torch.tensor([[1.7, 0.6, 2.5], [0.9, 1.1, 0.4]], dtype=torch.float64)
    return series, a, chs, Kk


def test_pod_basis_matches_the_svd_of_the_snapshot_matrix():
    import tmg_ops as ops
    series, a, chs, Kk = _svd_case()
    B, Tn = series.shape[:2]
    HW = series.shape[3] * series.shape[4]
    m, psi, lam, lam_total, tc = ops.pod_basis(series, a, chs, Kk)
    assert m.dtype == psi.dtype == lam.dtype == lam_total.dtype == tc.dtype == torch.float64
    assert psi.shape == (B, Kk, len(chs)) + tuple(series.shape[3:]) and lam.shape == (B, Kk) and tc.shape == (B, Tn, Kk)
    x = series[:, :, list(chs)].numpy()
    for b in range(B):
        mean = x[b].mean(0)
        d = (a[b, list(chs)].numpy().reshape(1, -1, 1, 1) * (x[b] - mean)).reshape(Tn, -1)          # snapshots as rows
        assert np.allclose(m[b].numpy(), mean, rtol=0, atol=1e-14)
        U, sv, Vt = np.linalg.svd(d, full_matrices=False)
        ref_lam = sv ** 2 / (HW * Tn)
        assert np.all(np.diff(lam[b].numpy()) <= 0)
        assert np.allclose(lam[b].numpy(), ref_lam[:Kk], rtol=1e-10, atol=0)
        assert abs(float(lam_total[b]) - ref_lam.sum()) <= 1e-10 * ref_lam.sum()
        p = psi[b].reshape(Kk, -1).numpy()
        gram = p @ p.T / HW
        assert np.abs(gram - np.eye(Kk)).max() <= 1e-12                                            # <psi_k, psi_l> = delta_kl
        assert np.abs((p * p).mean(1) * len(chs) - 1.0).max() <= 1e-12                             # RMS 1 over the pixels
        direct = d @ p.T / HW                                                                       # <d_j, psi_k>
        assert np.abs(tc[b].numpy() - direct).max() <= 1e-12 * np.abs(direct).max()
        v = tc[b].numpy() / np.sqrt(Tn * lam[b].numpy())
        assert np.abs((v * v).sum(0) - 1.0).max() <= 1e-12
        for k in range(Kk):                                                                         # the sign rule, and the mode up to it
            top = int(np.abs(v[:, k]).argmax())
            assert v[top, k] > 0
            s = np.sign(U[top, k])
            assert np.abs(p[k] - s * Vt[k] * np.sqrt(HW)).max() <= 1e-8


def test_pod_basis_sign_rule_takes_the_first_entry_on_a_tie():
    import tmg_ops as ops
    # two snapshots: the centred pair is (+e, -e), so v_0 = (1, -1) / sqrt(2) up to sign: a tie, the first entry must be the positive one
    x = torch.zeros(1, 2, 2, 3, 4, dtype=torch.float64)
    x[0, 0, 0, 1, 2], x[0, 1, 0, 1, 2] = -3.0, 5.0
    _, psi, _, _, tc = ops.pod_basis(x, torch.ones(1, 2), (0, 1), 1)
    assert float(tc[0, 0, 0]) > 0 and float(tc[0, 1, 0]) == -float(tc[0, 0, 0]) and float(psi[0, 0, 0, 1, 2]) < 0


# ---- every ValueError ------------------------------------------------------------------------------------------------------------------
def test_pod_basis_errors():
    import tmg_ops as ops
    series, a, chs, _ = _svd_case()
    bad = lambda **kw: pytest.raises(ValueError, match=kw.pop("match"))      # noqa: E731
    with bad(match="modes <= 16"):
        ops.pod_basis(torch.cat([series, series], 1), a, chs, 17)
    with bad(match="modes <= 16"):
        ops.pod_basis(series, a, chs, 0)
    with bad(match="rank at most 11"):
        ops.pod_basis(series, a, chs, 12)
    with bad(match="at least 2 snapshots"):
        ops.pod_basis(series[:, :1], a, chs, 1)
    for c in ((0, 0), (0, 3), (-1,), (), (0, 1, 2, 0, 1), (True,), (0.0,)):
        with bad(match="channels"):
            ops.pod_basis(series, a, c, 2)
    with bad(match="strictly positive"):
        ops.pod_basis(series, -a, chs, 2)
    const = series.clone()
    const[1] = const[1, :1]
    with bad(match=r"modelPredModes: mode 0 of the target of case 5 carries no energy"):
        ops.pod_basis(const, a, chs, 2, name="modelPredModes", case0=4)
    low = series.clone()                                                     # rank 1: mode 1 has no energy
    low[0] = low[0, :1] + torch.arange(12.0).view(12, 1, 1, 1) * torch.ones_like(low[0, :1])
    with bad(match=r"mode 1 of the target of case 0"):
        ops.pod_basis(low, a, chs, 2)


def test_constructor_errors_come_before_the_device():
    import tmg_ops as ops
    B, Cc, Hh, Ww, Kk = 2, 3, 4, 5, 3
    mean, basis = torch.zeros(B, 2, Hh, Ww), torch.ones(B, Kk, 2, Hh, Ww)
    mk = lambda **kw: ops.EnsembleModes(**{**dict(members=4, B=B, C=Cc, Hh=Hh, Ww=Ww, steps=3, device="cpu", out_std=torch.ones(Cc),     # noqa: E731
                                                  mean=mean, basis=basis), **kw})
    for kw, msg in ((dict(C=5), "2 <= C <= 4"), (dict(members=0), "members"), (dict(members=1025), "members"),
                    (dict(out_std=torch.tensor([1.0, 0.0, 1.0])), "strictly positive"), (dict(u=-torch.ones(B, Cc)), "strictly positive"),
                    (dict(channels=(0, 0)), "distinct"), (dict(channels=(0, 3)), "distinct"), (dict(mean=None), "need the tables"),
                    (dict(mean=torch.zeros(B, 3, Hh, Ww)), "mean is a finite"), (dict(mean=mean + float("nan")), "mean is a finite"),
                    (dict(basis=torch.ones(B, 17, 2, Hh, Ww)), "basis is a finite"), (dict(basis=torch.ones(B, 0, 2, Hh, Ww)), "basis is a finite"),
                    (dict(basis=torch.ones(B, Kk, 2, Hh, Ww + 1)), "basis is a finite"), (dict(basis=basis * float("inf")), "basis is a finite"),
                    (dict(steps=0), "steps, B, H, W >= 1")):
        with pytest.raises(ValueError, match=msg):
            mk(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mk()


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def test_plan_covers_the_pixels_and_does_not_change_with_the_row_count():
    import tmg_hip
    for HW in (1, 35, 255, 256, 257, 512, 527, 2048, 8192, 8193, 8281, 65536, 1 << 20):
        for Cg in (1, 2, 4):
            for B in (1, 3):
                base = tmg_hip.ens_pod_plan(1, B, Cg, HW, 5)
                P, SL = base["P"], base["SL"]
                assert P >= 1 and SL % 256 == 0 and P * SL >= HW and (P - 1) * SL < HW and P <= 32
                assert base["L"] == SL * Cg and base["L"] * P >= HW * Cg
                assert P == min((HW + 255) // 256, 32) or SL > 256
                for S in (1, 15, 16, 17, 64, 65, 1024):
                    for Kk in (1, 16):
                        q = tmg_hip.ens_pod_plan(S, B, Cg, HW, Kk)
                        assert (q["P"], q["SL"], q["L"]) == (P, SL, base["L"])             # the slicing: not a function of the rows
                        assert q["ws"] == (P * S * B * 17 if P > 1 else 0)


def test_entries_return_their_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                    # noqa: E731
    plan = (c_i64 * 4)()
    ok = (4, 2, 2, 100, 3)
    assert lib.tmg_ens_pod_plan(i64(*ok), plan) == 0
    for pos, v in ((0, 0), (1, 0), (2, 0), (2, 5), (3, 0), (4, 0), (4, 17)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_pod_plan(i64(*d), plan) == -1, (pos, v)
    for pos, v in ((0, 1025), (1, 65536), (3, (1 << 31) - 256)):
        d = list(ok)
        d[pos] = v
        assert lib.tmg_ens_pod_plan(i64(*d), plan) == -2, (pos, v)
    assert lib.tmg_ens_pod_plan(i64(*ok), None) == -3
    # the projection: a non-null dummy pointer is never dereferenced by a call that returns a code
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dims = (4, 2, 100, 2, 3)
    call = lambda dims=dims, td=(3, 0), ch=(0, 1), od=(36, 9, 12, 3), ptr=p, ws=p, wsn=0: lib.tmg_ens_pod_project(     # noqa: E731
        ptr, i64(*td), i64(*ch), p, p, p, ws, c_i64(wsn), p, p, i64(*od), i64(*dims), None)
    assert call(dims=(0, 2, 100, 2, 3)) == -1 and call(dims=(4, 2, 100, 2, 17)) == -1 and call(dims=(4, 2, 100, 5, 3)) == -1
    assert call(td=(3, 3)) == -1 and call(ch=(0, 3)) == -1 and call(ch=(1, 1)) == -1 and call(od=(36, -1, 12, 3)) == -1
    assert call(dims=(1025, 2, 100, 2, 3)) == -2 and call(td=(1 << 31, 0)) == -2
    assert call(dims=(4, 2, 300, 2, 3), wsn=0) == -1                         # P = 2: the plan's workspace is missing
    assert call(ptr=None) == -3 and call(dims=(4, 2, 300, 2, 3), ws=None, wsn=1 << 20) == -3


# ---- the case tables reach every branch of the plan ------------------------------------------------------------------------------------
def test_case_tables_reach_every_branch_of_the_plan():
    import tmg_hip
    seen = set()
    cases = [(c[0], c[1], len(c[3]), c[4], c[5], c[7]) for c in K.INT_TABLE + [K.LONG_CASE, K.MAX_CASE]]
    cases += [(c[0], c[1], len(c[3]), c[4], c[5], 1) for c in K.REAL_TABLE]
    for S, B, Cg, hw, Kk, kind in cases:
        HW = hw[0] * hw[1]
        q = tmg_hip.ens_pod_plan(S, B, Cg, HW, Kk)
        seen.add("P=1" if q["P"] == 1 else "P>1")
        seen.add("SL=256" if q["SL"] == 256 else "SL>256")
        if q["P"] > 1 and HW == (q["P"] - 1) * q["SL"] + 1:
            seen.add("one pixel over a slice boundary")
        seen.add("scalar psi" if HW % 4 else "float4 psi")
        if HW % 64:
            seen.add("ragged chunk")
        for k in set(K.chunk_sizes(S, kind)):
            seen.add("one tile" if k <= 16 else "four tiles")
            if k > 64:
                seen.add("two member blocks")
            if k % 16:
                seen.add("ragged tile")
        seen.add("K=%d" % Kk if Kk in (1, 16) else "K ragged")
    assert seen >= {"P=1", "P>1", "SL=256", "SL>256", "one pixel over a slice boundary", "scalar psi", "float4 psi", "ragged chunk", "one tile",
                    "four tiles", "two member blocks", "ragged tile", "K=1", "K=16", "K ragged"}, seen
    ints = K.INT_TABLE
    assert {c[4] for c in ints} >= {(1, 1), (5, 7), (16, 16), (17, 31)} and {c[0] for c in ints} >= {1, 15, 16, 17, 33}
    assert {c[5] for c in ints} == {1, 5, 16} and {c[1] for c in ints} == {1, 3} and {c[7] for c in ints} == {0, 1, 2}
    assert {c[3] for c in ints} >= {(0,), (0, 1), (0, 2), (0, 1, 2)} and any(c[2] == 4 and c[3] == (1, 3) for c in ints)
    assert {c[8] for c in ints} == {False, True}
    assert K.MAX_CASE[0] == 1024 and K.MAX_CASE[4] == (1, 5)
    q = tmg_hip.ens_pod_plan(1, 1, 2, 257, 1)
    assert K.HWS[257] == (1, q["SL"] + 1)
    assert all(sum(K.chunk_sizes(S, kind)) == S for S in (1, 15, 16, 17, 33, 70, 1024) for kind in (0, 1, 2))


# ---- the references agree, and the checks are sensitive --------------------------------------------------------------------------------
def _fake_got(ref, hw, t_start):
    """What a perfect device would return: the reference's sums rounded to fp32, divided by HW in fp64 and rounded once."""
    n = float(hw[0] * hw[1])
    got = {"coef_raw": ref["coef_raw"].astype(K.F32), "en_raw": ref["en_raw"].astype(K.F32), "tcoef_raw": ref["tcoef_raw"].astype(K.F32),
           "ten_raw": ref["ten_raw"].astype(K.F32)}
    for raw, out in (("coef_raw", "coef"), ("en_raw", "fluct_energy"), ("tcoef_raw", "target_coef"), ("ten_raw", "target_fluct_energy")):
        got[out] = (got[raw].astype(np.float64) / n).astype(K.F32)
    got.update({k: v.astype(K.F32) for k, v in K.derive(got, t_start).items()})
    return got


def test_integer_and_fp64_references_agree_and_the_checks_are_sensitive():
    S, B, Cc, chs, hw, Kk, t_start, _, _ = K.INT_TABLE[3]
    xs, tgt, m, psi = K.int_inputs(S, B, Cc, chs, hw, Kk, 5003)
    a = K.scales(None, None, B, Cc, chs)
    ri = K.reference(xs, tgt, a, m, psi, chs, integer=True)
    rf = K.reference(xs, tgt, a, m, psi, chs)
    for k in ri:
        assert ri[k].dtype == np.int64 and np.array_equal(ri[k].astype(np.float64), rf[k]), k
    plan = {"P": 3, "SL": 256, "L": 256 * len(chs)}
    got = _fake_got(ri, hw, t_start)
    K.shapes(got, S, B, K.T, Kk)
    K.check_integer(got, ri, hw, "fake")
    assert K.check_bound(got, rf, plan, hw, "fake") <= 1.0 / K.count(plan)      # the one rounding of the quotient
    K.check_derived(got, t_start, "fake")
    off = dict(got)                                                          # one integer sum off by 1
    off["coef_raw"] = got["coef_raw"].copy()
    off["coef_raw"][B - 1, S - 1, 1, Kk - 1] += 1
    with pytest.raises(AssertionError):
        K.check_integer(off, ri, hw, "off")
    off = dict(got)
    off["en_raw"] = got["en_raw"].copy()
    off["en_raw"][0, 0, 0] -= 1
    with pytest.raises(AssertionError):
        K.check_integer(off, ri, hw, "off")
    for name, bkey in (("coef", "abs_coef"), ("target_coef", "abs_tcoef"), ("fluct_energy", "en_raw")):   # one output off by twice its bound
        off = dict(got)
        off[name] = got[name].copy()
        idx = (0,) * off[name].ndim
        off[name][idx] += K.F32(2.0 * K.count(plan) * K.U24 * float(rf[bkey][idx]) / (hw[0] * hw[1]))
        with pytest.raises(AssertionError):
            K.check_bound(off, rf, plan, hw, "off")
    for name in K.DERIVED_KEYS:                                              # one derived output off by four units in the last place
        off = dict(got)
        off[name] = got[name].copy()
        idx = (0,) * off[name].ndim
        off[name][idx] = off[name][idx] * K.F32(1 + 2.0 ** -21) + K.F32(1e-6)
        with pytest.raises(AssertionError):
            K.check_derived(off, t_start, "off")


def test_integer_tables_keep_every_sum_exact():
    for idx, (S, B, Cc, chs, hw, Kk, _, _, _) in enumerate(K.INT_TABLE + [K.LONG_CASE]):
        if S > 33:
            S = 33                                                           # (the members are independent draws: the sums' range is the field's)
        xs, tgt, m, psi = K.int_inputs(S, B, Cc, chs, hw, Kk, 5000 + idx, 1)
        ref = K.reference(xs, tgt, K.scales(None, None, B, Cc, chs), m, psi, chs, integer=True)
        assert max(ref["abs_coef"].max(), ref["abs_tcoef"].max(), ref["en_raw"].max(), ref["ten_raw"].max()) < 2 ** 24
