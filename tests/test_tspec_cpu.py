"""CPU-side checks of the ensemble temporal power spectra: the three kernel entries are declared in a header of their own, listed
and exported; the ops / post-processing entry points exist with their signatures (the pinned ones unchanged); the argument errors come
in the documented order without a GPU; the host-built operand and G_k match an fp64 statement; the fp32 restatement of the kernels'
data flow (test_tspec_gpu.f32_psd) stays inside the GPU test's bound against fp64 at every GPU case, C_PRAW being ten times its
largest error over the case table - the evidence for the bound where there is no GPU; and the fp64 reference tells four wrong definitions apart."""
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
import test_tspec_gpu as G

NEW_SYMBOLS = ["tmg_tspec_store", "tmg_tspec_block", "tmg_tspec_finalize"]


def test_new_symbols_declared_listed_and_exported():
    import tmg_hip
    hdr = open(os.path.join(C.ROOT, "include", "tmglow_hip_tspec.h")).read()
    ret = dict((n, t) for t, n in re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", hdr))
    assert sorted(ret) == sorted(NEW_SYMBOLS) == sorted(tmg_hip.TSPEC_EXPORTS)
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NEW_SYMBOLS:
        assert ret[name] == "int", name
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64, name
        assert hasattr(lib, name), name
        assert getattr(tmg_hip.lib(), name).restype is ctypes.c_int, name
    main = open(os.path.join(C.ROOT, "include", "tmglow_hip.h")).read()
    assert main.count('#include "tmglow_hip_tspec.h"') == 1
    assert not set(NEW_SYMBOLS) & set(re.findall(r"\b(?:int|int64_t)\s+(tmg_\w+)\s*\(", main))
    assert "tmg_tspec.hip" in tmg_hip.SOURCES and "tmg_tspec.hip" in tmg_hip.NO_PACKED_F32
    assert os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_tspec.hip"))
    assert all(callable(getattr(tmg_hip, n)) for n in ("tspec_store", "tspec_block", "tspec_finalize"))


def test_entry_points_and_pinned_signatures():
    from utils import utils
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredTimeSpectra).parameters
    assert list(sig) == old + ["nfreq", "window", "dt"]
    assert [sig[n].default for n in list(sig)[4:]] == [1, 1, 1, 0, 64, 32, "hann", None]
    init = inspect.signature(tmg_ops.EnsembleTimeSpectrum.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "nfreq", "window", "dt"]
    assert [init[n].default for n in ("u", "nfreq", "window", "dt")] == [None, 32, "hann", 1.0]
    assert list(inspect.signature(tmg_ops.EnsembleTimeSpectrum.add).parameters) == ["self", "y", "m0"]
    # the four existing entries keep their parameter lists and defaults
    for f, extra in ((utils.modelPredStats, []), (utils.modelPredTurbulence, []), (utils.modelPredSpectra, ["window"]),
                     (utils.modelPredScores, [])):
        p = inspect.signature(f).parameters
        assert list(p) == old + extra, f.__name__
        assert [p[n].default for n in list(p)[4:]] == [1, 1, 1, 0, 64] + (["hann"] if extra else []), f.__name__


def _ts(members=3, B=2, Cc=3, steps=5, out_mu=None, out_std=None, u=None, nfreq=4, window="hann", dt=1.0, device="cpu"):
    import tmg_ops
    return tmg_ops.EnsembleTimeSpectrum(members, B, Cc, 4, 5, steps, device, torch.zeros(Cc) if out_mu is None else out_mu,
                                        torch.ones(Cc) if out_std is None else out_std, u=u, nfreq=nfreq, window=window, dt=dt)


# every case is wrong in the named argument AND in every later one of the documented order (C, steps, nfreq, window, dt, members,
# entries of out_mu / out_std, shape of u, device): the earliest decides the message
LATER = dict(members=0, out_std=torch.ones(1), u=torch.ones(5))


@pytest.mark.parametrize("Cc", [1, 5])
def test_bad_channel_count_raises_first(Cc):
    with pytest.raises(ValueError, match="channels"):
        _ts(Cc=Cc, steps=1, nfreq=0, window="hamming", dt=0.0, **LATER)


@pytest.mark.parametrize("steps", [1, 0, -3])
def test_bad_steps_raise_second(steps):
    with pytest.raises(ValueError, match="steps >= 2"):
        _ts(steps=steps, nfreq=0, window="hamming", dt=0.0, **LATER)


def test_bad_nfreq_raises_third():
    with pytest.raises(ValueError, match="nfreq >= 1"):
        _ts(nfreq=0, window="hamming", dt=0.0, **LATER)


def test_bad_window_raises_fourth():
    with pytest.raises(ValueError, match="window must be"):
        _ts(window="hamming", dt=0.0, **LATER)


@pytest.mark.parametrize("dt", [0.0, -1.0, float("nan"), float("inf"), "x"])
def test_bad_dt_raises_fifth(dt):
    with pytest.raises(ValueError, match="dt needs"):
        _ts(dt=dt, **LATER)


def test_bad_member_count_raises_sixth():
    with pytest.raises(ValueError, match="members"):
        _ts(**LATER)


def test_short_out_std_raises_seventh():
    with pytest.raises(ValueError, match="entries"):
        _ts(out_std=torch.ones(2), u=torch.ones(5))
    with pytest.raises(ValueError, match="entries"):
        _ts(out_mu=torch.zeros(1), u=torch.ones(5))


def test_bad_u_raises_before_the_device():
    with pytest.raises(ValueError, match="^u needs"):
        _ts(u=torch.ones(5))


@pytest.mark.parametrize("steps,nfreq,window", [(2, 1, None), (41, 32, "hann")])
def test_cpu_device_raises_last(steps, nfreq, window):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _ts(steps=steps, nfreq=nfreq, window=window, u=torch.full((2, 3), 0.5))


def _cpu_model_and_loader():
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    return m, [(x, torch.zeros(2, 3, 3, 16, 16), torch.ones(2))]


def test_model_pred_time_spectra_argument_errors_and_cpu():
    from utils import utils
    m, loader = _cpu_model_and_loader()
    log = SimpleNamespace(log=lambda *a, **k: None)
    args = SimpleNamespace(device=None)
    with pytest.raises(ValueError, match="window must be"):
        utils.modelPredTimeSpectra(args, m, loader, log, samples=2, tmax=3, window="hamming")
    with pytest.raises(ValueError, match="nfreq"):
        utils.modelPredTimeSpectra(args, m, loader, log, samples=2, tmax=3, nfreq=0)
    with pytest.raises(ValueError, match="dt must"):
        utils.modelPredTimeSpectra(args, m, loader, log, samples=2, tmax=3, dt=0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredTimeSpectra(args, m, loader, log, samples=2, tmax=3)


# ---- the host-built constants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tn,NF,window", [(5, 3, "hann"), (16, 9, None), (16, 9, "hann"), (19, 4, "hann"), (35, 18, None), (2, 2, "hann"),
                                          (41, 21, "hann"), (1000, 32, "hann")])
def test_host_operand_and_gk_match_fp64(Tn, NF, window):
    import tmg_ops
    tm, cst = tmg_ops._tspec_operand(Tn, NF, window)
    R = 2 * NF + 1
    assert tm.dtype == cst.dtype == torch.float32 and tuple(tm.shape) == (Tn, (R + 15) // 16 * 16) and tuple(cst.shape) == (3, NF)
    # the fp64 statement, with the argument NOT reduced: exp(-2 pi i k n / Tn) through complex exponentials
    g = G.hann(Tn) if window == "hann" else np.ones(Tn)
    n, k = np.arange(Tn)[:, None], np.arange(NF)[None, :]
    Z = g[:, None] * np.exp(-2j * math.pi * k * n / Tn)
    # rounding to fp32 (2^-24 relative) plus the un-reduced argument's own error (k n up to 3e4 radians: a few 1e-12)
    np.testing.assert_allclose(tm[:, :NF].double().numpy(), Z.real, rtol=0, atol=6e-8 * g.max() + 1e-10)
    np.testing.assert_allclose(tm[:, NF:2 * NF].double().numpy(), Z.imag, rtol=0, atol=6e-8 * g.max() + 1e-10)
    assert bool((tm[:, 2 * NF] == 1).all()) and bool((tm[:, R:] == 0).all())
    Gk = Z.sum(0)
    np.testing.assert_allclose(cst[0].double().numpy(), Gk.real, rtol=6e-8, atol=1e-9 * Tn)
    np.testing.assert_allclose(cst[1].double().numpy(), Gk.imag, rtol=6e-8, atol=1e-9 * Tn)
    if window == "hann" and Tn > 4:                                            # non-zero only at k = 0, 1
        assert abs(Gk[0]) > 1 and abs(Gk[1]) > 0.1 and float(cst[:2, 2:].abs().max()) == 0
    ck = np.full(NF, 2.0)
    ck[0] = 1.0
    if Tn % 2 == 0 and NF > Tn // 2:
        ck[Tn // 2] = 1.0
    np.testing.assert_allclose(cst[2].double().numpy(), ck / Tn ** 2, rtol=6e-8, atol=0)
    # the test file's own restatement of the constants is the same set of numbers
    (tm_t, G_t, ck_t), _ = G.operand32(Tn, NF, window)
    assert torch.equal(tm[:, :R], tm_t) and torch.equal(cst[2], ck_t)
    assert torch.allclose(cst[:2], G_t, rtol=2e-7, atol=0) and torch.equal(cst[:2] == 0, G_t == 0)   # (fp64 sums in another order)


# ---- the fp32 restatement against fp64 at the GPU test's inputs -------------------------------------------------------------------------
def _gpu_inputs():
    """(label, ys, u, nfreq, window) of every input the GPU test feeds the kernels."""
    for idx, c in enumerate(G.CASES):
        ys, u = G.case_inputs(idx, "cpu")
        yield "case %d" % idx, ys, u, c[1], c[9]
    ys, u, _ = G.tone_inputs("cpu")
    yield "tone", ys, u, G.TONE[0] // 2 + 1, None
    for Tn, window in G.PARSEVAL:
        yield "parseval %d" % Tn, G.parseval_inputs(Tn, "cpu"), None, Tn // 2 + 1, window


def test_fp32_restatement_stays_in_the_gpu_bound():
    """The restatement's error is inside 1e-5 |ref| + C_PRAW Praw at every input the GPU test feeds, and C_PRAW is ten times the largest
    e32 / Praw over the case table: measured 1.90e-8 with this file's BLAS; another library's summation order inside the 16-step
    products moves single roundings, so the pin allows a factor of two either way."""
    worst = 0.0
    for label, ys, u, nfreq, window in _gpu_inputs():
        x64, x32 = G.fields(ys, u)
        ref, e32, praw = G.yardstick(x64, x32, nfreq, window)
        got = G.f32_psd(x32, nfreq, window)
        for name in G.KEYS:
            err = np.abs(got[name].double().numpy() - ref[name])
            assert bool((err <= 1e-5 * np.abs(ref[name]) + G.C_PRAW * praw).all()), (label, name)
            print("%s %s: e32 = %.3e Praw" % (label, name, e32[name] / praw))
            if label.startswith("case"):
                worst = max(worst, e32[name] / praw)
    print("largest e32 / Praw over the case table: %.3e; C_PRAW = %.3e" % (worst, G.C_PRAW))
    assert 0.05 * G.C_PRAW <= worst <= 0.2 * G.C_PRAW


def test_pure_tone_statement_is_the_analytic_one():
    """The fp64 statement of the tone's fp32 series is a^2 / 2 in bin k0 and nothing elsewhere, to the input's rounding."""
    ys, u, P = G.tone_inputs("cpu")
    x64, _ = G.fields(ys, u)
    np.testing.assert_allclose(G.ref_psd(x64, G.TONE[0] // 2 + 1, None), P, rtol=0, atol=1e-7)


# ---- the reference is sensitive ---------------------------------------------------------------------------------------------------------
def _breaks(idx, **wrong):
    """True when the wrongly defined statement leaves the GPU bound around the right one at case idx."""
    Tn, nfreq, _, _, _, _, _, _, _, window, _ = G.CASES[idx]
    ys, u = G.case_inputs(idx, "cpu")
    x64, x32 = G.fields(ys, u)
    ref, e32, praw = G.yardstick(x64, x32, nfreq, window)
    bad = G.ref_stats(G.ref_psd(x64, nfreq, window, **wrong))
    return not bool((np.abs(bad["psd_mean"] - ref["psd_mean"]) <= G.bound_of(ref["psd_mean"], e32["psd_mean"], praw)).all())


def test_reference_tells_wrong_definitions_apart():
    nyq = [i for i, c in enumerate(G.CASES) if c[0] % 2 == 0 and G.n_freq(c[0], c[1]) > c[0] // 2]
    han = [i for i, c in enumerate(G.CASES) if c[9] == "hann"]
    assert nyq and han
    for i in nyq:
        assert _breaks(i, nyquist_c=2.0), "c_k = 2 at Nyquist passes at case %d" % i
    for i in han:
        assert _breaks(i, remove_mean=False), "no mean removal passes at case %d" % i
        assert _breaks(i, periodic=False), "a symmetric window passes at case %d" % i
        assert _breaks(i, shift=1), "an off-by-one in n passes at case %d" % i
