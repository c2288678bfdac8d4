"""CPU-side checks of the ensemble turbulence statistics (Reynolds shear stress, turbulent kinetic energy, vorticity): the two
kernels' entries are declared, listed and exported, the ops / post-processing entry points exist with their signatures, and they
refuse to compute without a GPU or on a bad grid."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import common as C

NEW_SYMBOLS = ["tmg_ens_turb_accum", "tmg_ens_turb_finalize"]


def test_new_symbols_declared_listed_and_exported():
    import tmg_hip
    hdr = open(os.path.join(C.ROOT, "include", "tmglow_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(tmg_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in tmg_hip.EXPORTS, name
        assert hasattr(lib, name), name
    assert callable(tmg_hip.ens_turb_accum) and callable(tmg_hip.ens_turb_finalize)


def test_entry_points_exist():
    from utils import utils
    import tmg_ops
    sig = inspect.signature(utils.modelPredTurbulence).parameters
    assert list(sig) == ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    assert [sig[n].default for n in ("samples", "stride", "tmax", "t_start", "max_rows")] == [1, 1, 1, 0, 64]
    # modelPredStats keeps its parameter list: the turbulence statistics are a function of their own
    assert list(inspect.signature(utils.modelPredStats).parameters) == list(sig)
    init = inspect.signature(tmg_ops.EnsembleStats.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid"]
    assert init["grid"].default is None


def _tiny_model():
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()


def test_model_pred_turbulence_on_cpu_raises():
    from utils import utils
    m = _tiny_model()
    log = SimpleNamespace(log=lambda *a, **k: None)
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    loader = [(x, torch.zeros(2, 3, 2, 16, 16), torch.ones(2))]
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredTurbulence(SimpleNamespace(device=None, dx=0.1, dy=0.1), m, loader, log, samples=2, tmax=2)


def test_ensemble_stats_with_grid_on_cpu_raises():
    import tmg_ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        tmg_ops.EnsembleStats(2, 1, 3, 4, 4, 1, "cpu", torch.zeros(3), torch.ones(3), grid=(0.1, 0.2))


@pytest.mark.parametrize("grid", [(0.0, 0.1), (0.1, -1.0), (float("nan"), 0.1), (0.1, float("inf")), (0.1,), (0.1, 0.1, 0.1)])
def test_bad_grid_raises_value_error(grid):
    """Checked before the device, so that the message is the same with and without a GPU."""
    import tmg_ops
    with pytest.raises(ValueError, match="grid"):
        tmg_ops.EnsembleStats(2, 1, 3, 4, 4, 1, "cpu", torch.zeros(3), torch.ones(3), grid=grid)
