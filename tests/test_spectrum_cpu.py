"""CPU-side checks of the ensemble kinetic-energy spectra: the four kernel entries are declared, listed and exported, the ops /
post-processing entry points exist with their signatures (the pinned ones unchanged), the argument errors come in the documented order
without a GPU, and the shell map tmg_ops.spectrum_bins equals an fp64 statement written here."""
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

NEW_SYMBOLS = ["tmg_spec_rows", "tmg_spec_cols", "tmg_spec_accum", "tmg_spec_finalize"]


def test_new_symbols_declared_listed_and_exported():
    import tmg_hip
    hdr = open(os.path.join(C.ROOT, "include", "tmglow_hip.h")).read()
    ret = dict((n, t) for t, n in re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NEW_SYMBOLS:
        assert ret.get(name) == "int", name
        assert name in tmg_hip.EXPORTS, name
        assert name not in tmg_hip.RET_I64, name
        assert hasattr(lib, name), name
    assert len(tmg_hip.RET_I64) == 4
    assert "tmg_spectrum.hip" in tmg_hip.SOURCES and "tmg_spectrum.hip" in tmg_hip.NO_PACKED_F32
    assert all(callable(getattr(tmg_hip, n)) for n in ("spec_rows", "spec_cols", "spec_accum", "spec_finalize"))


def test_entry_points_and_pinned_signatures():
    from utils import utils
    import tmg_ops
    sig = inspect.signature(utils.modelPredSpectra).parameters
    assert list(sig) == ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows", "window"]
    assert [sig[n].default for n in ("samples", "stride", "tmax", "t_start", "max_rows", "window")] == [1, 1, 1, 0, 64, "hann"]
    init = inspect.signature(tmg_ops.EnsembleSpectrum.__init__).parameters
    assert list(init) == ["self", "members", "B", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid", "window"]
    assert init["u"].default is None and init["window"].default == "hann"
    assert list(inspect.signature(tmg_ops.EnsembleSpectrum.add).parameters) == ["self", "y", "m0", "time"]
    # the pinned ones keep their parameter lists
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert list(inspect.signature(utils.modelPredTurbulence).parameters) == old
    assert list(inspect.signature(tmg_ops.EnsembleStats.__init__).parameters) == [
        "self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid"]


def _spectrum(Hh=16, Ww=16, grid=(0.05, 0.07), window="hann", device="cpu"):
    import tmg_ops
    return tmg_ops.EnsembleSpectrum(2, 1, Hh, Ww, 1, device, torch.zeros(3), torch.ones(3), grid=grid, window=window)


# every case is wrong in the named argument AND in every later one of the documented order (grid, window, size, device): the earliest
# decides the message
@pytest.mark.parametrize("grid", [(0.0, 0.1), (0.1, -1.0), (float("nan"), 0.1), (0.1, float("inf")), (0.1,), (0.1, 0.1, 0.1), None])
def test_bad_grid_raises_first(grid):
    with pytest.raises(ValueError, match="grid"):
        _spectrum(Hh=20, grid=grid, window="hamming")


@pytest.mark.parametrize("window", ["hamming", "Hann", "", 1])
def test_bad_window_raises_second(window):
    with pytest.raises(ValueError, match="window"):
        _spectrum(Hh=20, window=window)


@pytest.mark.parametrize("hw", [(20, 16), (16, 8), (0, 16), (16, 528), (512, 1024), (17, 17)])
def test_bad_size_raises_third(hw):
    with pytest.raises(ValueError, match="multiple of 16"):
        _spectrum(Hh=hw[0], Ww=hw[1])


@pytest.mark.parametrize("window", ["hann", None])
def test_cpu_device_raises_last(window):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _spectrum(window=window)


def test_model_pred_spectra_on_cpu_raises():
    from nn.tmGlow import TMGlow
    from utils import utils
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    log = SimpleNamespace(log=lambda *a, **k: None)
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    loader = [(x, torch.zeros(2, 3, 2, 16, 16), torch.ones(2))]
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredSpectra(SimpleNamespace(device=None, dx=0.1, dy=0.1), m, loader, log, samples=2, tmax=2)
    with pytest.raises(ValueError, match="window"):
        utils.modelPredSpectra(SimpleNamespace(device=None, dx=0.1, dy=0.1), m, loader, log, samples=2, tmax=2, window="boxcar")


# (H, W, dx, dy, NK, smallest distance of any r + 0.5 to an integer): no exact tie decides a bin on these grids
BINS = [(16, 16, 0.05, 0.05, 12, 1.5e-2), (16, 32, 0.05, 0.07, 21, 5.1e-3), (32, 16, 0.05, 0.07, 29, 2.2e-3),
        (48, 80, 0.05, 0.07, 50, 7.4e-4)]


@pytest.mark.parametrize("Hh,Ww,dx,dy,NK,edge", BINS)
def test_spectrum_bins_match_fp64_statement(Hh, Ww, dx, dy, NK, edge):
    import tmg_ops
    Lx, Ly = Ww * dx, Hh * dy
    Lmax = max(Lx, Ly)
    r = np.empty((Hh, Ww), dtype=np.float64)
    for p in range(Hh):
        for q in range(Ww):
            ps, qs = (p if p <= Hh // 2 else p - Hh), (q if q <= Ww // 2 else q - Ww)
            r[p, q] = math.sqrt((ps * Lmax / Ly) ** 2 + (qs * Lmax / Lx) ** 2)
    ref = np.floor(r + 0.5).astype(np.int64)
    dist = float(np.abs(r + 0.5 - np.round(r + 0.5)).min())
    assert dist > 1e-6 and abs(dist / edge - 1) < 0.05, dist
    bins, k = tmg_ops.spectrum_bins(Hh, Ww, dx, dy)
    assert bins.dtype == torch.int32 and tuple(bins.shape) == (Hh, Ww)
    assert k.dtype == torch.float64 and tuple(k.shape) == (NK,)
    assert ref.max() + 1 == NK
    assert np.array_equal(bins.numpy(), ref)
    counts = np.bincount(bins.numpy().ravel(), minlength=NK)
    assert counts.min() >= 1 and counts[0] == 1 and bins[0, 0] == 0            # no empty shell; shell 0 is the mean mode alone
    np.testing.assert_allclose(k.numpy(), np.arange(NK) * 2 * math.pi / Lmax, rtol=1e-15, atol=0)


@pytest.mark.parametrize("Hh,Ww,dx,dy,NK,edge", BINS)
def test_shell_lists_cover_every_mode_once(Hh, Ww, dx, dy, NK, edge):
    """The per-tile lists the column pass sums in: each tile's 16 H modes exactly once, every list segment inside its shell."""
    import tmg_ops
    bins, _ = tmg_ops.spectrum_bins(Hh, Ww, dx, dy)
    perm, offs = tmg_ops._spectrum_lists(bins, NK)
    assert perm.dtype == torch.int32 and offs.dtype == torch.int32
    assert tuple(perm.shape) == (Ww // 16, Hh * 16) and tuple(offs.shape) == (Ww // 16, NK + 1)
    for t in range(Ww // 16):
        assert sorted(perm[t].tolist()) == list(range(Hh * 16))
        assert offs[t, 0] == 0 and offs[t, NK] == Hh * 16 and bool((offs[t, 1:] >= offs[t, :-1]).all())
        tile = bins[:, t * 16:(t + 1) * 16].reshape(-1)
        for s in range(NK):
            idx = perm[t, offs[t, s]:offs[t, s + 1]].long()
            assert bool((tile[idx] == s).all())
