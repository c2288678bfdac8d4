"""CPU-side checks of the spectral POD: the kernel entries are declared in a header of their own, listed apart and exported; the ops /
post-processing entry points exist with their signatures; the argument errors come in the documented order without a GPU; the C entries
return their codes before any launch; the launch plan covers every row macro-tile pair and every pixel once, and the case tables of
tests/spod_cases.py reach every branch it reports; spod_decompose against numpy; the degenerate cases; and the fp64 reference and the
bounds of the GPU comparison are sensitive to the wrong definitions the comparison has to catch."""
import ctypes
import inspect
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import spod_cases as K

NAMES = ["tmg_ens_spod_plan", "tmg_ens_spod_csd", "tmg_ens_spod_modes"]
c_i64 = ctypes.c_int64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_spod.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.SPOD_EXPORTS == NAMES
    main = open(os.path.join(inc, "tmglow_hip.h")).read()
    assert "spod" not in main                                                  # the main header stays as it was
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NAMES:
        for other in (tmg_hip.EXPORTS, tmg_hip.PLAN_EXPORTS, tmg_hip.TSPEC_EXPORTS, tmg_hip.GRAM_EXPORTS, tmg_hip.POD_EXPORTS,
                      tmg_hip.PHASE_EXPORTS, tmg_hip.RET_I64):
            assert name not in other
        assert hasattr(lib, name) and getattr(tmg_hip.lib(), name).restype is ctypes.c_int
    assert "tmg_spod.hip" in tmg_hip.SOURCES and "tmg_spod.hip" in tmg_hip.NO_PACKED_F32
    assert os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_spod.hip"))
    assert "tmglow_hip_spod.h" in inspect.getsource(tmg_hip.build)
    assert "tmg_spod" in open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read()
    src = open(os.path.join(tmg_hip.CSRC, "tmg_spod.hip")).read()
    assert "atomic" not in src.replace("no atomics", "").replace("No float atomics", "") and "asm" not in src


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredSpod).parameters
    assert list(sig)[:14] == old + ["bins", "modes", "channels", "window", "loo"]
    assert [sig[n].default for n in list(sig)[4:14]] == [1, 1, 1, 0, 64, None, 4, (0, 1), "hann", True]
    init = inspect.signature(tmg_ops.EnsembleSpod.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "bins", "modes", "channels",
                          "window", "dt", "loo"]
    assert [init[n].default for n in list(init)[10:]] == [None, None, 4, (0, 1), "hann", 1.0, True]
    assert list(inspect.signature(tmg_ops.EnsembleSpod.add).parameters) == ["self", "y", "m0", "target"]
    assert list(inspect.signature(tmg_ops.spod_args).parameters) == ["bins", "modes", "channels", "Tn", "C"]
    assert list(inspect.signature(tmg_ops.spod_decompose).parameters) == ["csd_raw", "S", "HW", "kappa", "J", "cnt", "loo"]
    assert list(inspect.signature(tmg_hip.ens_spod_csd).parameters) == ["acc", "cst", "bins", "channels", "ws", "csd_raw", "Tn"]
    assert list(inspect.signature(tmg_hip.ens_spod_modes).parameters) == ["acc", "cst", "bins", "channels", "w", "modes", "Tn"]
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert tmg_ops.SPOD_ROUNDINGS == K.C_ROUNDINGS
    for word in ("eigendecompositions", "all C channels"):
        assert word in tmg_ops.EnsembleSpod.__doc__


# ---- spod_args and the constructor's error order: every case is wrong in the named argument AND in every later one ------------------
def test_spod_args_normalise():
    import tmg_ops
    assert tmg_ops.spod_args(None, 4, (0, 1), 40, 3) == (tuple(range(1, 17)), 4, (0, 1))
    assert tmg_ops.spod_args(None, 1, [2], 5, 3) == ((1, 2), 1, (2,))
    assert tmg_ops.spod_args([1, 4, 8], 8, (2, 0, 1), 16, 3) == ((1, 4, 8), 8, (2, 0, 1))


@pytest.mark.parametrize("bins", [(), (0,), (1, 1), (2, 1), (9,), (1.0,), (True,), tuple(range(1, 18)), 3])
def test_spod_args_bad_bins_raise_first(bins):
    import tmg_ops
    with pytest.raises(ValueError, match="^bins"):
        tmg_ops.spod_args(bins, 0, (0, 0), 16 if bins != tuple(range(1, 18)) else 64, 3)


@pytest.mark.parametrize("modes", [0, 9, 2.0, True, None])
def test_spod_args_bad_modes_raise_before_the_channels(modes):
    import tmg_ops
    with pytest.raises(ValueError, match="modes"):
        tmg_ops.spod_args((1, 2), modes, (0, 0), 16, 3)


@pytest.mark.parametrize("channels", [(), (0, 0), (3,), (-1,), (0.0,), 1, (0, 1, 2, 0)])
def test_spod_args_bad_channels_raise_last(channels):
    import tmg_ops
    with pytest.raises(ValueError, match="^channels"):
        tmg_ops.spod_args(None, 4, channels, 16, 3)


BAD = dict(steps=1, bins=(0,), modes=0, channels=(0, 0), window="boxcar", dt=0.0, members=0, out_std=torch.ones(2), u=torch.ones(5))
ORDER = ["C", "steps", "bins", "modes", "channels", "window", "dt", "members", "out_std", "u"]
MATCH = {"C": "channels", "steps": "steps", "bins": "^bins", "modes": "modes", "channels": "^channels", "window": "^window", "dt": "^dt",
         "members": "members", "out_std": "entries", "u": "^u needs"}


def _spod(Cc=3, device="cpu", **kw):
    import tmg_ops
    a = dict(members=3, steps=8, out_std=torch.ones(Cc), u=None, bins=None, modes=4, channels=(0, 1), window="hann", dt=1.0)
    a.update(kw)
    return tmg_ops.EnsembleSpod(a["members"], 2, Cc, 4, 5, a["steps"], device, torch.zeros(Cc), a["out_std"], u=a["u"], bins=a["bins"],
                                modes=a["modes"], channels=a["channels"], window=a["window"], dt=a["dt"])


@pytest.mark.parametrize("first", ORDER)
def test_constructor_errors_come_in_the_documented_order(first):
    i = ORDER.index(first)
    kw = {k: BAD[k] for k in ORDER[max(i, 1):]}
    with pytest.raises(ValueError, match=MATCH[first]):
        _spod(Cc=5 if first == "C" else 3, **kw)


@pytest.mark.parametrize("members", [0, 256])
def test_member_limit(members):
    with pytest.raises(ValueError, match="members"):
        _spod(members=members)


def test_cpu_device_raises_last():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _spod(members=255, u=torch.full((2, 3), 0.5), bins=(1, 4), modes=8, channels=(2, 0), window=None)


def test_model_pred_spod_bad_arguments_raise_first_and_the_cpu_last():
    from utils import utils
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    x = torch.zeros(2, 5, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    loader = [(x, torch.zeros(2, 5, 3, 16, 16), torch.ones(2))]
    log = SimpleNamespace(log=lambda *a, **k: None)
    args = SimpleNamespace(device=None)
    with pytest.raises(ValueError, match="^bins"):
        utils.modelPredSpod(args, m, loader, log, samples=2, tmax=4, bins=(3,))
    with pytest.raises(ValueError, match="^window"):
        utils.modelPredSpod(args, m, loader, log, samples=2, tmax=4, window="boxcar")
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredSpod(args, m, loader, log, samples=2, tmax=4)


# ---- the C entries' return codes: all of them return before any launch ---------------------------------------------------------------
GOOD = (4, 2, 3, 35, 5, 8, 2, 2, 1 << 40)                                       # S, B, C, HW, NF, Tn, NB, Cg, ws_floats / J


def _call(which, dims, bins=(1, 3), channels=(0, 2), ptr=0, null_lists=False):
    import tmg_hip
    i64 = lambda vals: (c_i64 * max(1, len(vals)))(*vals)                     # noqa: E731
    v = ctypes.c_void_p(ptr)
    fn = getattr(tmg_hip.lib(), "tmg_ens_spod_" + which)
    return fn(v, v, None if null_lists else i64(bins), None if null_lists else i64(channels), v, v, i64(dims), ctypes.c_void_p(0))


@pytest.mark.parametrize("which", ["csd", "modes"])
def test_launchers_return_their_codes_before_any_launch(which):
    last = 4 if which == "modes" else GOOD[8]
    good = GOOD[:8] + (last,)
    sub = lambda i, val: good[:i] + (val,) + good[i + 1:]                      # noqa: E731
    for dims in (sub(0, 0), sub(0, 256), sub(1, 0), sub(2, 1), sub(2, 5), sub(3, 0), sub(4, 1), sub(5, 1), sub(4, 6), sub(6, 0), sub(6, 17),
                 sub(7, 0), sub(7, 4)):
        assert _call(which, dims) == -1, dims
    for kw in (dict(bins=(0, 3)), dict(bins=(3, 1)), dict(bins=(1, 5)), dict(channels=(0, 0)), dict(channels=(0, 3)), dict(channels=(-1, 0))):
        assert _call(which, good, ptr=0x1000, **kw) == -1, kw
    assert _call(which, sub(1, 40000)) == -2 and _call(which, sub(3, (1 << 31) - 256)) == -2
    assert _call(which, good, null_lists=True) == -3 and _call(which, good) == -3
    if which == "csd":
        import tmg_hip
        need = tmg_hip.ens_spod_plan(4, 2, 2, 35, 2)["ws"]
        assert _call(which, good[:8] + (need - 1,), ptr=0x1000) == -1 and _call(which, good[:8] + (need,)) == -3
    else:
        assert _call(which, good[:8] + (0,), ptr=0x1000) == -1 and _call(which, good[:8] + (9,), ptr=0x1000) == -1


def test_plan_return_codes():
    import tmg_hip
    L = tmg_hip.lib()
    i64 = lambda *v: (c_i64 * len(v))(*v)                                     # noqa: E731
    out = (c_i64 * 9)()
    for dims in ((0, 2, 2, 35, 2, 0), (256, 2, 2, 35, 2, 0), (4, 0, 2, 35, 2, 0), (4, 2, 0, 35, 2, 0), (4, 2, 5, 35, 2, 0), (4, 2, 2, 0, 2, 0),
                 (4, 2, 2, 35, 0, 0), (4, 2, 2, 35, 17, 0)):
        assert L.tmg_ens_spod_plan(i64(*dims), None) == -1
    for dims in ((4, 40000, 2, 35, 2, 0), (4, 2, 2, (1 << 31) - 256, 2, 0)):
        assert L.tmg_ens_spod_plan(i64(*dims), None) == -2
    assert L.tmg_ens_spod_plan(i64(4, 2, 2, 35, 2, 0), None) == -3 and L.tmg_ens_spod_plan(i64(4, 2, 2, 35, 2, 0), out) == 0
    with pytest.raises(RuntimeError, match="tmg_ens_spod_plan failed with code -1"):
        tmg_hip.ens_spod_plan(256, 2, 2, 35, 2)


# ---- the plan query ------------------------------------------------------------------------------------------------------------------
WS_CAP = 1 << 24


@pytest.mark.parametrize("S", [1, 6, 7, 8, 30, 31, 32, 63, 64, 127, 128, 255])
def test_plan_covers_every_pair_and_pixel_once_inside_its_cap(S):
    import tmg_hip
    for B, Cg, NB in ((1, 1, 1), (3, 2, 2), (7, 4, 16), (64, 3, 5)):
        for HW in (1, 63, 64, 65, 255, 256, 257, 272, 528, 2900, 8192, 1 << 16, (1 << 20) + 3):
            q = tmg_hip.ens_spod_plan(S, B, Cg, HW, NB)
            NT = (2 * (S + 1) + 63) // 64
            assert q["NT"] == NT and q["pairs"] == [(i, j) for i in range(NT) for j in range(i, NT)]
            assert q["part"] == (256 if 2 * (S + 1) <= 16 else 4096)
            P, SL, L = q["P"], q["SL"], q["L"]
            assert P >= 1 and SL % 256 == 0 and (P - 1) * SL < HW <= P * SL   # the slices [s SL, min(HW, (s + 1) SL)) cover 0..HW-1 once
            assert L == Cg * SL and L * P >= Cg * HW
            base = B * NB * len(q["pairs"]) * q["part"]
            assert q["ws"] == base * (P + (1 if P > 1 else 0))
            assert q["ws"] <= max(WS_CAP, base), (S, B, Cg, HW, q)
            assert P == 1 or P <= -(-768 // (B * NB * len(q["pairs"])))
            assert q["vec"] == (HW % 4 == 0) and q["MB"] == -(-HW // 256)
            assert not tmg_hip.ens_spod_plan(S, B, Cg, HW, NB, acc=0x1004)["vec"]   # a base that is not 16-byte aligned: scalar loads


def _case_plan(c):
    import tmg_hip
    return tmg_hip.ens_spod_plan(c["R"] - 1, c["B"], len(c["channels"]), c["hw"][0] * c["hw"][1], len(c["bins"]))


def test_case_tables_reach_every_branch_the_plan_reports():
    got = {c["name"]: K.csd_branches(_case_plan(c), c["R"]) for c in K.CSD_CASES}
    assert got == K.CSD_BRANCHES                                               # pinned: a removed entry or a changed plan fails here
    sigs = list(got.values())
    assert len(set(sigs)) == len(sigs), "two cases run on the same plan: one of them is redundant"
    assert {s[0] for s in sigs} == {True, False}                               # the one-tile instance and the macro-tile instance
    assert {1, 2} <= {s[1] for s in sigs} and max(s[1] for s in sigs) == 8     # diagonal launch alone, with the off-diagonal one, the limit
    assert any(s[2] and not s[0] and s[1] == 1 for s in sigs)                  # one full macro-tile
    assert any(not s[2] for s in sigs)                                         # a last tile that is not full
    assert {s[3] for s in sigs} == {True, False} and {s[4] for s in sigs} == {True, False}
    # the issue's shapes: R, HW, B, C with channels that reorder and omit, 1 / 2 / 16 bins with non-adjacent ones
    assert {c["R"] for c in K.CSD_CASES} == {2, 8, 9, 32, 33, 129, 256}
    assert {c["hw"] for c in K.CSD_CASES} == {(1, 1), (7, 9), (8, 8), (5, 13), (16, 17), (16, 33)}
    assert {c["B"] for c in K.CSD_CASES} == {1, 3} and {c["C"] for c in K.CSD_CASES} == {2, 3, 4}
    assert {len(c["bins"]) for c in K.CSD_CASES} == {1, 2, 16}
    assert any(len(c["bins"]) == 2 and c["bins"][1] - c["bins"][0] > 1 for c in K.CSD_CASES)
    assert any(list(c["channels"]) != sorted(c["channels"]) for c in K.CSD_CASES) and any(len(c["channels"]) < c["C"] for c in K.CSD_CASES)
    assert {c["gint"] for c in K.CSD_CASES} == {True, False}                   # G = 0 and G != 0
    for c in K.CSD_CASES:                                                      # Tn a power of two: the correction stays exact
        assert c["Tn"] & (c["Tn"] - 1) == 0 and max(c["bins"]) < c["NF"] <= c["Tn"] // 2 + 1
    for name, _ in K.REAL_CASES:
        assert name in K.CSD_BY_NAME
    assert {bool(off) for _, off in K.REAL_CASES} == {True, False}
    # the modes kernel: S below, at and above a multiple of 4; one and two pixel blocks; a tail inside a column tile
    assert {c["S"] % 4 for c in K.MODES_CASES} >= {0, 1} and {(c["hw"][0] * c["hw"][1] + 255) // 256 for c in K.MODES_CASES} == {1, 2}
    assert {c["J"] for c in K.MODES_CASES} >= {1, 8}


def test_integer_cases_are_exact_in_fp32():
    """The scaled integers Tn X of every integer case and their Gram sums stay under 2^24 Tn^2: fp32 holds every partial sum."""
    for i, c in enumerate(K.CSD_CASES):
        acc, cst = K.int_acc(c, 40 + i)
        ref = K.int_csd(acc, cst, c)
        assert int(ref.abs().max()) < (1 << 24), c["name"]                     # Tn^2 raw < 2^24: raw is a multiple of 1 / Tn^2 below 2^24
        r64, _ = K.csd_ref64(acc, cst, c["bins"], c["channels"], c["Tn"])
        assert torch.equal((r64 * c["Tn"] ** 2).round().to(torch.int64), ref) and torch.equal(r64 * c["Tn"] ** 2, ref.double())


# ---- spod_decompose against numpy ------------------------------------------------------------------------------------------------------
def _random_csd(S, N, seed, B=2, NB=3, rank=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, NB, S + 1, N)) + 1j * rng.standard_normal((B, NB, S + 1, N))
    if rank is not None:
        X[:, :, :S] = (rng.standard_normal((B, NB, S, rank)) + 1j * rng.standard_normal((B, NB, S, rank))) @ X[:, :, :rank]
    M = np.einsum("bkme,bkne->bkmn", X.conj(), X)
    return X, torch.from_numpy(np.stack((M.real, M.imag), 2))


@pytest.mark.parametrize("S,J", [(5, 3), (8, 8), (12, 4)])
def test_decompose_matches_numpy(S, J):
    import tmg_ops
    HW, N = 20, 40
    kap = np.array([0.02, 0.005, 0.01])
    X, raw = _random_csd(S, N, 10 + S)
    o = tmg_ops.spod_decompose(raw, S, HW, torch.from_numpy(kap), J, 0.0)
    full = tmg_ops.spod_decompose(raw, S, HW, torch.from_numpy(kap), min(S, 8), 0.0, loo=False)
    for b in range(2):
        for k in range(3):
            sv = np.linalg.svd(math.sqrt(kap[k] / (S * HW)) * X[b, k, :S], compute_uv=False) ** 2
            np.testing.assert_allclose(o["spod_energy"][b, k].numpy(), sv[:J], rtol=1e-12, atol=0)
            np.testing.assert_allclose(float(o["spod_total"][b, k]), sv.sum(), rtol=1e-12)
            if S <= 8:
                np.testing.assert_allclose(float(full["spod_energy"][b, k].sum()), float(full["spod_total"][b, k]), rtol=1e-12)
                np.testing.assert_allclose(float(full["captured"][b, k]), 1.0, rtol=1e-12)
            W = o["weights"][b, k].numpy()                                      # [S, J]
            M = o["csd"][b, k].numpy()[:S, :S]                                  # M / HW
            np.testing.assert_allclose(W.conj().T @ M @ W, np.eye(J), atol=1e-11)
            Phi = W.T @ X[b, k, :S]                                             # [J, N], synthesised explicitly
            np.testing.assert_allclose(Phi.conj() @ Phi.T / HW, np.eye(J), atol=1e-11)
            bj = Phi.conj() @ X[b, k, S] / HW
            np.testing.assert_allclose(o["target_coef"][b, k].numpy(), bj, rtol=1e-10, atol=1e-13)
            np.testing.assert_allclose(o["target_mode_energy"][b, k].numpy(), kap[k] * np.abs(bj) ** 2, rtol=1e-10)
            ten = kap[k] * (np.abs(X[b, k, S]) ** 2).sum() / HW
            np.testing.assert_allclose(float(o["target_energy"][b, k]), ten, rtol=1e-12)
            np.testing.assert_allclose(float(o["target_captured"][b, k]), kap[k] * (np.abs(bj) ** 2).sum() / ten, rtol=1e-10)
            np.testing.assert_allclose(o["member_mode_energy"][b, k].sum(0).numpy(), S * o["spod_energy"][b, k].numpy(), rtol=1e-10)
            # leave-one-out, recomputed directly: member m on the modes of the others
            for m in range(S):
                rest = [n for n in range(S) if n != m]
                Xo = X[b, k, rest]
                _, s, vh = np.linalg.svd(Xo, full_matrices=False)               # the modes' subspaces are the right singular vectors
                Jn = min(J, S - 1)
                proj = vh[:Jn].conj() @ X[b, k, m]
                np.testing.assert_allclose(float(o["loo_captured"][b, k, m]), (np.abs(proj) ** 2).sum() / (np.abs(X[b, k, m]) ** 2).sum(),
                                           rtol=1e-9)
            assert float(o["target_captured_rank"][b, k]) == float((o["loo_captured"][b, k] < o["target_captured"][b, k]).sum())
            # the phase convention
            th = W / np.abs(W).sum(0, keepdims=True)
            top = np.abs(th).argmax(0)
            for j in range(J):
                assert th[top[j], j].imag == 0.0 and th[top[j], j].real > 0
    assert o["csd"].dtype == torch.complex128 and o["target_coef"].dtype == torch.complex128 and o["spod_energy"].dtype == torch.float64
    np.testing.assert_allclose(o["spod_noise_floor"].numpy(), 0.0)
    fl = tmg_ops.spod_decompose(raw, S, HW, torch.from_numpy(kap), J, 1000.0, loo=False)
    np.testing.assert_allclose(fl["spod_noise_floor"].numpy(), 1000.0 * 2.0 ** -24 * o["spod_total"].numpy(), rtol=1e-15)
    assert "loo_captured" not in fl and "target_captured_rank" not in fl      # loo=False: the two keys are absent


def test_decompose_degenerate_cases():
    import tmg_ops
    HW = 20
    # S = 1: one mode, the rest zero energy and NaN; the leave-one-out keys are NaN
    X, raw = _random_csd(1, 30, 3)
    o = tmg_ops.spod_decompose(raw, 1, HW, 0.02, 4, 100.0)
    assert bool((o["spod_energy"][..., 1:] == 0).all()) and bool((o["spod_energy"][..., 0] > 0).all())
    assert bool(torch.isnan(o["target_mode_energy"][..., 1:]).all()) and bool(torch.isfinite(o["target_mode_energy"][..., 0]).all())
    assert bool(torch.isnan(o["weights"][..., 1:].real).all()) and bool(torch.isnan(o["target_coef"][..., 1:].real).all())
    assert bool(torch.isnan(o["loo_captured"]).all()) and bool(torch.isnan(o["target_captured_rank"]).all())
    assert tuple(o["loo_captured"].shape) == (2, 3, 1) and not bool(o["valid"][..., 1:].any())
    np.testing.assert_allclose(o["captured"].numpy(), 1.0, rtol=1e-12)
    # S < J
    X, raw = _random_csd(3, 30, 4)
    o = tmg_ops.spod_decompose(raw, 3, HW, 0.02, 8, 100.0)
    assert tuple(o["spod_energy"].shape) == (2, 3, 8) and bool((o["spod_energy"][..., 3:] == 0).all())
    assert bool(o["valid"][..., :3].all()) and not bool(o["valid"][..., 3:].any())
    assert bool(torch.isfinite(o["target_captured"]).all()) and tuple(o["member_mode_energy"].shape) == (2, 3, 3, 8)
    # a rank-1 ensemble: the trailing modes fall under the floor and come back NaN, their energies as computed
    X, raw = _random_csd(6, 30, 5, rank=1)
    o = tmg_ops.spod_decompose(raw, 6, HW, 0.02, 4, 300.0)
    assert bool(o["valid"][..., 0].all()) and not bool(o["valid"][..., 1:].any())
    assert bool(torch.isfinite(o["spod_energy"]).all()) and bool((o["spod_energy"][..., 1:].abs() <= o["spod_noise_floor"].unsqueeze(-1)).all())
    assert bool(torch.isnan(o["target_mode_energy"][..., 1:]).all()) and bool(torch.isnan(o["weights"][..., 1:].real).all())
    lead = o["target_mode_energy"][..., 0] / o["target_energy"]
    np.testing.assert_allclose(o["target_captured"].numpy(), lead.numpy(), rtol=1e-12)   # the NaN modes are left out of the sum
    np.testing.assert_allclose(o["captured"].numpy(), 1.0, rtol=1e-9)
    with pytest.raises(ValueError, match="csd_raw"):
        tmg_ops.spod_decompose(raw, 5, HW, 0.02, 4, 1.0)
    with pytest.raises(ValueError, match="kappa"):
        tmg_ops.spod_decompose(raw, 6, HW, [0.1, 0.2], 4, 1.0)


# ---- the from-scratch reference against spod_decompose, and the yardstick ----------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e_refs():
    out = []
    for idx in range(len(K.E2E_CASES)):
        Tn, hw, Cc, B, S, u_given, window, bins, channels, J = K.E2E_CASES[idx]
        ys, u = K.e2e_inputs(idx)
        x64, x32 = K.fields(ys, u)
        bins = K.e2e_bins(idx)
        ref = K.ref_spod(x64, bins, channels, window, J)
        out.append((x64, x32, bins, ref))
    return out


def test_reference_and_decompose_agree(e2e_refs):
    import tmg_ops
    for idx, (x64, x32, bins, ref) in enumerate(e2e_refs):
        Tn, hw, Cc, B, S, u_given, window, _, channels, J = K.E2E_CASES[idx]
        HW = hw[0] * hw[1]
        M = ref["csd"] * HW
        o = tmg_ops.spod_decompose(torch.from_numpy(np.stack((M.real, M.imag), 2)), S, HW, torch.from_numpy(K.kappa_of(bins, Tn)), J, 0.0)
        np.testing.assert_allclose(o["spod_energy"].numpy(), ref["spod_energy"], rtol=1e-9, atol=1e-14 * float(ref["spod_total"].max()))
        np.testing.assert_allclose(o["spod_total"].numpy(), ref["spod_total"], rtol=1e-12)
        np.testing.assert_allclose(o["target_energy"].numpy(), ref["target_energy"], rtol=1e-12)
        # spod_total is the field mean over the channels of psd_mean at the bin (the fp64 statement of both)
        X = K.ref_coef(x64, bins, window)[:, :, :S][:, :, :, list(channels)]    # [B, NB, S, Cg, HW]
        psd = K.kappa_of(bins, Tn).reshape(1, -1, 1, 1) * (np.abs(X) ** 2).mean(2)   # [B, NB, Cg, HW]: the members' mean
        np.testing.assert_allclose(ref["spod_total"], psd.mean(-1).sum(-1), rtol=1e-12)


def test_yardstick_is_the_recorded_one(e2e_refs):
    worst = 0.0
    for idx, (x64, x32, bins, ref) in enumerate(e2e_refs):
        _, hw, _, _, _, _, window, _, channels, _ = K.E2E_CASES[idx]
        bound, e32, rel = K.csd_tolerance(ref["csd"], x64, x32, bins, channels, window)
        print("case %d: e32 %.3e = %.3e scale" % (idx, e32, rel))
        worst = max(worst, rel)
    assert 0.5 * K.E32_MEASURED <= worst <= 1.05 * K.E32_MEASURED and K.C_SCALE == 10 * K.E32_MEASURED


WRONG = [dict(conj_swapped=True), dict(unbiased=True), dict(no_kappa=True), dict(with_target=True)]


@pytest.mark.parametrize("wrong", WRONG, ids=lambda w: next(iter(w)))
def test_reference_tells_wrong_definitions_apart(e2e_refs, wrong):
    """Each wrong definition moves the reference by more than the GPU comparison allows: the csd bound for a swapped conjugation, and
    for the others the largest eigenvalue shift that csd bound admits (Weyl: ||dA||_F with dA = kappa dM / (S HW))."""
    hits = 0
    for idx, (x64, x32, bins, ref) in enumerate(e2e_refs):
        Tn, hw, Cc, B, S, u_given, window, _, channels, J = K.E2E_CASES[idx]
        if S < 2:
            continue
        bad = K.ref_spod(x64, bins, channels, window, J, **wrong)
        bound, _, _ = K.csd_tolerance(ref["csd"], x64, x32, bins, channels, window)
        if "conj_swapped" in wrong:
            assert bool((np.abs(bad["csd"] - ref["csd"]) > bound).any()), idx
        kap = K.kappa_of(bins, Tn).reshape(1, -1)
        weyl = kap / S * np.sqrt((bound[:, :, :S, :S] ** 2).sum((-2, -1)))
        moved = np.abs(bad["spod_energy"][..., 0] - ref["spod_energy"][..., 0])
        if "conj_swapped" not in wrong:
            assert bool((moved > weyl).all()), (idx, moved, weyl)
        hits += 1
    assert hits >= 4


def test_planted_reference_gap():
    """The planted structure's own reference keeps Davis-Kahan's s = 2 ||dA||_F / (lambda_0 - lambda_1) under 0.1 for the largest dA
    the csd bound admits, and finds psi_1 at bin k1."""
    p = K.PLANTED
    HW = p["hw"][0] * p["hw"][1]
    for target in ("same", "psi2_at_k1"):
        x, psi1, psi2 = K.planted(target)
        ys = K.normalised(x, None)
        x64, x32 = K.fields(ys, None)
        ref = K.ref_spod(x64, (p["k1"],), p["channels"], None, p["J"])
        bound, _, _ = K.csd_tolerance(ref["csd"], x64, x32, (p["k1"],), p["channels"], None)
        kap = K.kappa_of((p["k1"],), p["Tn"])[0]
        dA = kap / p["S"] * math.sqrt((bound[0, 0, :p["S"], :p["S"]] ** 2).sum())
        s = 2 * dA / (ref["lam_all"][0, 0, 0] - ref["lam_all"][0, 0, 1])
        print("planted %s: s = %.3e, lambda %s" % (target, s, ref["lam_all"][0, 0, :3]))
        assert s < 0.1
        assert abs((ref["modes"][0, 0, 0].conj() * psi1).sum() / HW) > 0.999
        if target == "same":
            assert ref["target_captured"][0, 0] > 0.99
        else:
            assert ref["target_captured"][0, 0] < 0.05
