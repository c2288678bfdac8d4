"""CPU-side checks of the ensemble spectral skill: the kernel entries are declared in their own header, listed apart and exported;
the signatures of the three Python layers; the plan query's values and the codes the entries return before any launch; every argument
error without a GPU; tmg_ops.xspec_outputs against its restatement (tests/xspec_cases.py), the NaN and inf rules of cutoff_k
included; the identities of the fp64 reference; and the sensitivity of the comparison the GPU test uses: every named mutation of the
reference is caught."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import common as C
import xspec_cases as K

NAMES = ["tmg_ens_xspec_plan", "tmg_ens_xspec_prep", "tmg_ens_xspec_cols", "tmg_ens_xspec_accum"]
c_i64 = ctypes.c_int64


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_xspec.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.XSPEC_EXPORTS == NAMES
    assert "xspec" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    P64, PF = ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_float)
    vp = ctypes.c_void_p
    want = {"tmg_ens_xspec_plan": [P64, P64], "tmg_ens_xspec_prep": [vp, P64, vp, vp, vp, vp, vp, vp, P64, vp],
            "tmg_ens_xspec_cols": [vp, vp, vp, vp, vp, vp, P64, PF, vp], "tmg_ens_xspec_accum": [vp] * 10 + [P64, vp]}
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.XSPEC_ARGTYPES[name] == want[name]
    assert "tmg_xspec.hip" in tmg_hip.SOURCES and "tmg_xspec.hip" in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_xspec.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_xspec\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_xspec.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    # every kernel rounds each operation on its own; no atomics, no inline assembly, nothing printed or asserted in a kernel
    assert code.count("#pragma clang fp contract(off)") == 3
    assert not re.search(r"\basm\b|printf|assert\s*\(|atomic|while\s*\(", code)
    # the spectrum files are reused unchanged: the row pass is tmg_spec_rows, the column product is spec_cols_kernel's
    spec = re.sub(r"//[^\n]*", "", open(os.path.join(tmg_hip.CSRC, "tmg_spectrum.hip")).read())
    loop = spec[spec.index("for (int k0 = 0; k0 < Hh"):spec.index("float* e = e2")]
    assert "".join(loop.split()) in "".join(code.split())


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredSpectralSkill).parameters
    assert list(sig) == old + ["window", "center", "level"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, "hann", "target", 0.5]
    init = inspect.signature(tmg_ops.EnsembleSpectralSkill.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid", "window", "center",
                          "level"]
    assert [init[n].default for n in ("u", "grid", "window", "center", "level")] == [None, (1.0, 1.0), "hann", None, 0.5]
    add = inspect.signature(tmg_ops.EnsembleSpectralSkill.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    assert issubclass(tmg_ops.EnsembleSpectralSkill, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.xspec_args).parameters) == ["C", "Hh", "Ww", "grid", "window", "level"]
    assert list(inspect.signature(tmg_ops.xspec_outputs).parameters) == list(K.RAW_KEYS) + ["S", "k", "level", "timed"]
    assert tmg_ops.XSPEC_RAW_KEYS == K.RAW_KEYS
    assert list(inspect.signature(tmg_hip.ens_xspec_plan).parameters)[:5] == ["k", "B", "Hh", "Ww", "NK"]
    for doc in (utils.modelPredSpectralSkill.__doc__, tmg_ops.EnsembleSpectralSkill.__doc__):
        for word in ("pressure or scalar coherence", "uadrature and phase", "er-member per-step", "low-fidelity input", "ixel boxes",
                     "multiples of 16", "on-finite members"):
            assert word in " ".join(doc.split()), word


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,B,Hh,Ww,NK", [(1, 1, 16, 16, 13), (3, 2, 32, 80, 40), (5, 1, 80, 16, 73), (1024, 4, 512, 512, 8192)])
def test_plan_values(k, B, Hh, Ww, NK):
    import tmg_hip
    p = tmg_hip.ens_xspec_plan(k, B, Hh, Ww, NK)
    QT = Ww // 16
    assert p["prep_grid"] == -(-2 * B * Hh * Ww // 256) and (p["cols_grid_x"], p["cols_grid_y"]) == (QT, k * B)
    assert p["cols_lds_bytes"] == 256 * Hh <= 160 * 1024 and (p["accum_grid_x"], p["accum_grid_y"]) == (-(-NK // 256), 3 * B)
    assert p["threads"] == 256 and p["f_floats"] == 2 * k * B * Hh * Ww and p["part_floats"] == 3 * k * B * QT * NK
    assert p["zt_floats"] == 2 * B * Hh * Ww and p["part_t_floats"] == B * QT * NK


def test_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    plan = (c_i64 * 11)()
    good = [3, 2, 32, 80, 40]
    assert lib.tmg_ens_xspec_plan(_i64(*good), plan) == 0
    for pos, bad in ((0, 0), (1, 0), (4, 0), (2, 0), (2, 24), (2, 528), (3, 8), (3, 40), (3, 1024)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_xspec_plan(_i64(*d), plan) == -1, (pos, bad)
    for pos, bad in ((0, 1025), (1, 65536), (1, 30000), (1, 21846), (4, 8193)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_xspec_plan(_i64(*d), plan) == -2, (pos, bad)
    assert lib.tmg_ens_xspec_plan(None, plan) == -3 and lib.tmg_ens_xspec_plan(_i64(*good), None) == -3
    assert tmg_hip.ens_xspec_plan(0, 1, 16, 16, 5, code=True)[1] == -1
    with pytest.raises(RuntimeError):
        tmg_hip.ens_xspec_plan(1, 1, 16, 20, 5)
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                                  # never dereferenced: every code comes before a launch
    k, B, Hh, Ww, NK, S, Tk = 3, 2, 32, 80, 40, 5, 4
    p = tmg_hip.ens_xspec_plan(k, B, Hh, Ww, NK)

    def prep(dims=(k, B, Hh, Ww, 3, 1, S, p["f_floats"]), y=one, yd=(3, 0), mu=one, sd=one, f=one, fsum=one):
        return lib.tmg_ens_xspec_prep(y, _i64(*yd), nul, mu, sd, nul, f, fsum, _i64(*dims), nul)

    base = [k, B, Hh, Ww, 3, 1, S, p["f_floats"]]
    for pos, bad in ((0, 0), (1, 0), (2, 20), (3, 0), (4, 1), (4, 5), (5, -1), (5, 4), (6, 0)):
        d = list(base)
        d[pos] = bad
        assert prep(tuple(d)) == -1, (pos, bad)
    assert prep(yd=(2, 0)) == -1 and prep(yd=(4, 2)) == -1 and prep(yd=(4, -1)) == -1
    assert prep((k, B, Hh, Ww, 3, 3, S, p["f_floats"])) == -1                     # the mean field is one image per case
    assert prep((k, B, Hh, Ww, 3, 1, 1025, p["f_floats"])) == -2 and prep((1025, B, Hh, Ww, 3, 1, S, 1 << 40)) == -2
    assert prep(y=nul) == -3 and prep(mu=nul) == -3 and prep(sd=nul) == -3 and prep(f=nul) == -3 and prep(fsum=nul) == -3
    assert prep((k, B, Hh, Ww, 3, 1, S, p["f_floats"] - 1)) == -4
    assert lib.tmg_ens_xspec_prep(one, _i64(3, 0), nul, one, one, nul, one, one, None, nul) == -3

    sc = (ctypes.c_float * 1)(0.5 / (Hh * Ww) ** 2)

    def cols(dims=(k * B, B, Hh, Ww, NK, 1, p["f_floats"], p["zt_floats"], p["part_floats"]), ft=one, zt=one, part=one, fl=sc):
        return lib.tmg_ens_xspec_cols(ft, one, one, one, zt, part, _i64(*dims), fl, nul)

    base = [k * B, B, Hh, Ww, NK, 1, p["f_floats"], p["zt_floats"], p["part_floats"]]
    for pos, bad in ((0, 0), (0, 5), (1, 0), (2, 8), (3, 88), (4, 0), (5, 2), (5, -1)):
        d = list(base)
        d[pos] = bad
        assert cols(tuple(d)) == -1, (pos, bad)
    assert cols((k * B, B, Hh, Ww, NK, 0, p["f_floats"], p["zt_floats"], p["part_floats"])) == -1   # the target is one image per case
    assert cols(fl=(ctypes.c_float * 1)(0.0)) == -1 and cols(fl=(ctypes.c_float * 1)(float("nan"))) == -1
    assert cols((65536, 1, Hh, Ww, NK, 1, 1 << 40, 1 << 40, 1 << 40)) == -2 and cols((k * B, B, Hh, Ww, 8193, 1, 1 << 40, 1 << 40, 1 << 40)) == -2
    assert cols(ft=nul) == -3 and cols(zt=nul) == -3 and cols(part=nul) == -3 and cols(fl=None) == -3
    for pos in (6, 7, 8):
        d = list(base)
        d[pos] -= 1
        assert cols(tuple(d)) == -4, pos

    def accum(dims=(k, B, NK, Ww // 16, S, Tk, 1, 0, 0, 0, 1), **nulls):
        a = {n: one for n in ("part", "part_t", "part_b", "step", "tpow", "sum_out", "bar_out", "tmem", "ttgt", "tbar")}
        a.update({n: nul for n in nulls})
        return lib.tmg_ens_xspec_accum(*a.values(), _i64(*dims), nul)

    base = [k, B, NK, Ww // 16, S, Tk, 1, 0, 0, 0, 1]
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 33), (4, 0), (5, 0), (6, -1), (6, Tk), (7, -1), (7, 1), (9, -1), (10, 4), (10, 3),
                     (0, 6)):
        d = list(base)
        d[pos] = bad
        assert accum(tuple(d)) == -1, (pos, bad)
    assert accum((2, B, NK, 5, S, Tk, 1, 3, 3, 0, 1)) == -1                       # the step's last chunk must say so
    assert accum((k, B, 8193, 5, S, Tk, 1, 0, 0, 0, 1)) == -2 and accum((k, 65536, NK, 5, S, Tk, 1, 0, 0, 0, 1)) == -2
    assert accum(part=0) == -3 and accum(step=0) == -3 and accum(part_t=0) == -3 and accum(tpow=0) == -3 and accum(tmem=0) == -3
    assert accum(ttgt=0) == -3
    last = (2, B, NK, 5, S, Tk, 1, 3, 3, 0, 3)
    assert accum(last, part_b=0) == -3 and accum(last, sum_out=0) == -3 and accum(last, bar_out=0) == -3 and accum(last, tbar=0) == -3
    assert lib.tmg_ens_xspec_accum(*([one] * 10), None, nul) == -3


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_device_work():
    import tmg_ops as ops
    from utils import utils
    ok = dict(C=3, Hh=32, Ww=48, grid=(0.05, 0.07), window="hann", level=0.5)
    grid, bins, k = ops.xspec_args(**ok)
    assert grid == (0.05, 0.07) and tuple(bins.shape) == (32, 48) and k.dtype == torch.float64
    bad = [dict(C=1), dict(C=5), dict(C=2.0), dict(C=True), dict(Hh=8), dict(Hh=40), dict(Ww=528), dict(Hh=32.0), dict(grid=(1.0,)),
           dict(grid=(1.0, 0.0)), dict(grid=(1.0, float("inf"))), dict(grid=(1.0, -1.0)), dict(grid=3), dict(grid=("a", 1)),
           dict(window="hamming"), dict(window=1), dict(level=0.0), dict(level=1.0), dict(level=float("nan")), dict(level="0.5"),
           dict(level=True), dict(Hh=512, Ww=16, grid=(1.0, 1e-4))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.xspec_args(**dict(ok, **kw))
    cok = dict(members=5, B=2, C=3, Hh=32, Ww=48, steps=2, device="cuda", out_mu=K.MU, out_std=K.SD)
    cbad = bad[:-1] + [dict(members=0), dict(members=1025), dict(steps=0), dict(B=0), dict(out_std=[1.0, 0.0, 1.0]), dict(out_std=[1.0]),
                       dict(out_mu=[float("nan"), 0.0]), dict(u=[[1.0, 1.0]]), dict(u=[[1.0], [1.0]]), dict(u=[[1.0, -1.0], [1.0, 1.0]]),
                       dict(center=np.zeros((2, 2, 32, 32), np.float32)), dict(center=np.zeros((1, 2, 32, 48), np.float32)),
                       dict(center=np.zeros((2, 1, 32, 48), np.float32)), dict(center=np.full((2, 2, 32, 48), np.nan, np.float32)),
                       dict(center="target")]
    for kw in cbad:
        with pytest.raises(ValueError):
            ops.EnsembleSpectralSkill(**dict(cok, **kw))
    with pytest.raises(RuntimeError, match="not a GPU"):
        ops.EnsembleSpectralSkill(**dict(cok, device="cpu"))
    with pytest.raises(ValueError):                                           # the argument error wins over the device error
        ops.EnsembleSpectralSkill(**dict(cok, device="cpu", level=2.0))
    for kw in (dict(window="hamming"), dict(level=0.0), dict(level=1.5), dict(center="mean")):
        with pytest.raises(ValueError):
            utils.modelPredSpectralSkill(None, None, None, None, **kw)
    raw = _raw_of_case(1)[0]
    a = [torch.from_numpy(raw[key]) for key in K.RAW_KEYS]
    k = K.bins(16, 16, 1.0, 1.0)[1]
    ops.xspec_outputs(*a, 3, k, 0.5, 2)
    for args in ((a, 0, k, 0.5, 2), (a, 3, k, 0.5, 0), (a, 3, k, 1.0, 2), (a, 3, k[:-1], 0.5, 2), (a, 4, k, 0.5, 2),
                 (a[:1] + [a[1][:, :1]] + a[2:], 3, k, 0.5, 2), ([a[0][0]] + a[1:], 3, k, 0.5, 2)):
        with pytest.raises(ValueError):
            ops.xspec_outputs(*args[0], *args[1:])


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _raw_of_case(idx):
    """(fp64 raw reference, fp32 yardstick, the case) of CASES[idx], computed once."""
    if idx not in _CACHE:
        c = K.make_case(idx)
        fm64, fm32 = K.fields(c["ym"], c["u"])
        ft64, ft32 = K.fields(c["yt"], c["u"])
        c.update(fm64=fm64, ft64=ft64)
        ref = K.reference(fm64, ft64, c["cen"], c["grid"], c["window"], c["t_start"])
        y32 = K.f32_raw(fm32, ft32, c["cen"], c["grid"], c["window"], c["t_start"])
        _CACHE[idx] = (ref, y32, c)
    return _CACHE[idx]


@pytest.mark.parametrize("idx", [1, 4, 8, 10])
def test_reference_identities(idx):
    ref, y32, c = _raw_of_case(idx)
    S, B, T, Hh, Ww = c["S"], c["B"], c["T"], c["H"], c["W"]
    b, k = K.bins(Hh, Ww, *c["grid"])
    NK = k.size
    PT, mem, bar = K.modal(c["fm64"], c["ft64"], c["cen"], c["window"])
    tot = float(PT.sum((-2, -1)).max())
    # D = P + P_T - 2 X, mode by mode
    assert float(np.abs(mem[2] - (mem[0] + PT[:, None] - 2 * mem[1])).max()) <= 1e-13 * tot
    assert float(np.abs(bar[2] - (bar[0] + PT - 2 * bar[1])).max()) <= 1e-13 * tot
    # the spread identity: mean_m |Z_m - Z_T|^2 - |Zbar - Z_T|^2 = mean_m |Z_m - Zbar|^2, the right side formed directly
    g = K.window2(Hh, Ww, c["window"])
    cen = 0.0 if c["cen"] is None else c["cen"].astype(np.float64)
    f = c["fm64"] - cen
    Z = np.fft.fft2(g * (f[..., 0, :, :] + 1j * f[..., 1, :, :]))
    direct = 0.5 / float(Hh * Ww) ** 2 * (np.abs(Z - Z.mean(1, keepdims=True)) ** 2).mean(1)        # [T, B, H, W]
    spread = ref["xs_sum"][:, :, 2] / S - ref["xs_mean_field"][:, :, 2]                              # [B, T, NK]
    assert float(np.abs(spread - K._shell(direct, b, NK).transpose(1, 0, 2)).max()) <= 1e-12 * tot
    # Parseval: sum_s X = 0.5 mean(g^2 (u_m u_T + v_m v_T))
    ft = c["ft64"] - cen
    phys = 0.5 * (g ** 2 * (f * ft[:, None]).sum(3)).mean((-2, -1))                                 # [T, S, B]
    assert float(np.abs(ref["xs_sum"][:, :, 1].sum(-1) - phys.sum(1).T).max()) <= 1e-12 * tot
    assert float(np.abs(ref["xs_target_power"].sum(-1) - (0.5 * (g ** 2 * (ft * ft).sum(2)).mean((-2, -1))).T).max()) <= 1e-12 * tot
    # the time sums are the sums of the steps from t_start on
    t0 = c["t_start"]
    assert np.allclose(ref["xs_time_target"], ref["xs_target_power"][:, t0:].sum(1), rtol=1e-13, atol=0)
    assert np.allclose(ref["xs_time_member"].sum(1), ref["xs_sum"][:, t0:].sum(1), rtol=1e-12, atol=1e-15 * tot)
    # the yardstick itself is close, and the band-copied members are coherent below k0 and not above
    assert not K.mismatches(y32, ref, y32)
    d = K.derived(ref, S, k, 0.5, T - t0)
    if c["window"] is None:
        assert float(np.nanmin(d["time_member_corr"][:, :, 1:c["k0"]])) > 1 - 1e-9
    assert float(np.nanmedian(np.abs(d["time_member_corr"][:, :, c["k0"] + 2:]))) < 0.5
    if idx == 10:
        empty = np.bincount(b.ravel(), minlength=NK) == 0
        assert empty.any() and np.isnan(d["spec_corr"][..., empty]).all() and np.isfinite(d["spec_corr"][..., ~empty]).all()


# ---- xspec_outputs ----------------------------------------------------------------------------------------------------------------------
def _host(raw, S, k, level, Tn):
    import tmg_ops as ops
    out = ops.xspec_outputs(*[torch.from_numpy(np.ascontiguousarray(raw[key])) for key in K.RAW_KEYS], S, torch.from_numpy(k), level, Tn)
    assert set(out) == set(K.DERIVED_KEYS) and all(v.dtype == torch.float64 and v.device.type == "cpu" for v in out.values())
    return {key: v.numpy() for key, v in out.items()}


@pytest.mark.parametrize("idx", [0, 1, 4, 8, 9, 10])
@pytest.mark.parametrize("level", [0.5, 0.9])
def test_host_outputs_equal_the_restatement(idx, level):
    ref, _, c = _raw_of_case(idx)
    k = K.bins(c["H"], c["W"], *c["grid"])[1]
    Tn = c["T"] - c["t_start"]
    raw32 = {key: v.astype(np.float32) for key, v in ref.items()}              # what the device hands over: fp32
    got, want = _host(raw32, c["S"], k, level, Tn), K.derived(raw32, c["S"], k, level, Tn)
    assert not K.derived_mismatches(got, want)
    N, S, NK = c["B"], c["S"], k.size
    assert got["spec_corr"].shape == (N, c["T"], NK) and got["time_rel_err"].shape == (N, NK) and got["time_member_corr"].shape == (N, S, NK)
    assert got["cutoff_k"].shape == (N, S + 1) and got["cutoff_k_mean"].shape == (N,) and got["xs_k"].shape == (NK,)
    assert np.array_equal(got["xs_k"], k)


def test_cutoff_rules_and_nan_rules():
    N, S, NK, Tk = 1, 3, 6, 1
    k = np.arange(NK) * 0.5
    corr = np.array([[1.0, 0.9, 0.7, 0.3, 0.1, 0.0],        # interpolated between shells 2 and 3: 1.0 + (0.7 - 0.5) / 0.4 * 0.5
                     [1.0, 0.2, 0.9, 0.9, 0.9, 0.9],        # s* = 1: k[1]
                     [1.0, 0.9, 0.8, 0.7, 0.6, 0.55]])      # never under the level: inf
    bar = np.array([1.0, np.nan, 0.9, np.nan, 0.1, 0.0])    # empty shells: between the finite shells 2 and 4
    PT = np.ones((N, Tk, NK))
    PT[..., [1, 3]] = 0.0                                   # the target has no power on shells 1 and 3 ...
    tm = np.zeros((N, S, 3, NK))
    tm[:, :, 0] = 1.0
    tm[:, :, 1] = corr
    tm[:, :, 2] = 2 - 2 * corr
    tb = np.stack([np.ones(NK), np.nan_to_num(bar), 2 - 2 * np.nan_to_num(bar)])[None]
    raw = {"xs_target_power": PT, "xs_sum": np.zeros((N, Tk, 3, NK)) + tm.sum(1)[:, None], "xs_mean_field": tb[:, None] + np.zeros((N, Tk, 1, 1)),
           "xs_time_member": tm, "xs_time_target": np.ones((N, NK)), "xs_time_mean_field": tb}
    got = _host(raw, S, k, 0.5, 1)
    assert np.allclose(got["cutoff_k"][0, :3], [1.0 + 0.2 / 0.4 * 0.5, 0.5, np.inf], rtol=1e-15)
    assert got["cutoff_len"][0, 2] == 0.0 and got["cutoff_len"][0, 1] == 2 * math.pi / 0.5
    assert np.isclose(got["cutoff_k_mean"][0], (1.25 + 0.5) / 2) and np.isclose(got["cutoff_k_std"][0], 0.375)
    # ... so the step outputs are NaN there and nowhere else
    for key in ("spec_corr", "mean_field_corr", "power_ratio", "rel_err"):
        assert np.isnan(got[key][0, 0, [1, 3]]).all() and np.isfinite(got[key][0, 0, [0, 2, 4, 5]]).all(), key
    # a time target without power on shells 1 and 3: the mean field's cut-off skips them
    raw["xs_time_target"] = PT[:, 0].copy()
    got = _host(raw, S, k, 0.5, 1)
    assert np.isnan(got["time_mean_field_corr"][0, [1, 3]]).all()
    assert np.isclose(got["cutoff_k"][0, 3], 1.0 + (0.9 - 0.5) / 0.8 * 1.0)
    assert not K.derived_mismatches(got, K.derived(raw, S, k, 0.5, 1))
    # spread_skill: 1 for mean|Z_m - T|^2 = (1 + 1 / S) spread with D_bar = spread / S ... stated directly: NaN under a negative argument
    raw["xs_mean_field"][:, :, 2] = 5.0                    # D_bar over Dm: negative spread
    got = _host(raw, S, k, 0.5, 1)
    assert (got["spread_spec"] < 0).all() and np.isnan(got["spread_skill"]).all()
    raw["xs_mean_field"][:, :, 2] = 0.0                    # D_bar == 0
    assert np.isnan(_host(raw, S, k, 0.5, 1)["spread_skill"]).all()
    # every member inf: the mean over no member is NaN
    tm[:, :, 1] = 0.9
    got = _host(dict(raw, xs_time_member=tm, xs_time_target=np.ones((N, NK))), S, k, 0.5, 1)
    assert np.isinf(got["cutoff_k"][0, :3]).all() and np.isnan(got["cutoff_k_mean"]).all() and np.isnan(got["cutoff_k_std"]).all()


def test_a_calibrated_ensemble_has_unit_spread_skill():
    """Members and target drawn from one distribution about a common signal, noise variance sigma^2 per mode: Dm = 2 sigma^2,
    D_bar = (1 + 1 / S) sigma^2, spread_spec = (1 - 1 / S) sigma^2 (the population variance), so spread_skill^2 = (S - 1) / S: near 1,
    and the closer the larger the ensemble."""
    rng = np.random.default_rng(5)
    S, B, T, Hh, Ww = 8, 1, 6, 64, 64
    sig = rng.standard_normal((T, 1, B, 2, Hh, Ww))
    fm = sig + rng.standard_normal((T, S, B, 2, Hh, Ww))
    ft = (sig + rng.standard_normal((T, 1, B, 2, Hh, Ww)))[:, 0]
    ref = K.reference(fm, ft, None, (1.0, 1.0), None, 0)
    k = K.bins(Hh, Ww, 1.0, 1.0)[1]
    d = K.derived(ref, S, k, 0.5, T)
    assert float(np.abs(d["time_spread_skill"][0, 16:40] - math.sqrt((S - 1) / S)).max()) < 0.1
    assert float(np.abs(d["time_rel_err"][0, 16:40] - 1).max()) < 0.15            # |noise_m - noise_T|^2 = 2 sigma^2 over P_T = 2 sigma^2


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate", K.MUTATIONS)
def test_named_mutations_are_caught(mutate):
    ref, y32, c = _raw_of_case(4)
    assert not K.mismatches(ref, ref, y32)
    bad = K.mismatches(K.reference(c["fm64"], c["ft64"], c["cen"], c["grid"], c["window"], c["t_start"], mutate), ref, y32)
    assert bad, mutate
    want = {"noconj": "xs_sum", "nohalf": "xs_target_power", "dsum": "xs_sum", "bar_s1": "xs_mean_field", "shift": "xs_target_power",
            "tcen": "xs_target_power"}[mutate]
    assert want in bad, (mutate, bad)


def test_the_comparison_sees_one_element_one_shape_and_one_key():
    ref, y32, _ = _raw_of_case(1)
    E = K.etot(ref)
    for key in K.RAW_KEYS:
        off = {n: v.copy() for n, v in ref.items()}
        off[key].reshape(-1)[-1] += 1e-4 * E
        assert K.mismatches(off, ref, y32) == [key]
        off[key].reshape(-1)[-1] = np.nan
        assert K.mismatches(off, ref, y32) == [key]
        assert K.mismatches({n: v for n, v in ref.items() if n != key}, ref, y32) == [key]
        assert K.mismatches(dict(ref, **{key: ref[key][..., :-1]}), ref, y32) == [key]
