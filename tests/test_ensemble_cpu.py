"""CPU-side checks of the batched ensemble prediction: the keyed latent draw and the ensemble-statistics kernels are declared,
listed and exported, the model and post-processing entry points exist, and they refuse to compute without a GPU."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import common as C

NEW_SYMBOLS = ["tmg_gauss_sample_keyed", "tmg_ens_accum", "tmg_ens_time_finalize"]


def test_new_symbols_declared_listed_and_exported():
    import tmg_hip
    hdr = open(os.path.join(C.ROOT, "include", "tmglow_hip.h")).read()
    declared = set(re.findall(r"\b(?:int|int64_t)\s+(tmg_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in tmg_hip.EXPORTS, name
        assert hasattr(lib, name), name


def test_entry_points_exist():
    from nn.tmGlow import LSTMCFlowDecoder, TMGlow
    from utils import utils
    import tmg_ops
    assert callable(TMGlow.sampleEnsemble)
    assert list(inspect.signature(TMGlow.sampleEnsemble).parameters) == ["self", "x", "h_in", "members"]
    sig = inspect.signature(utils.modelPredStats).parameters
    assert list(sig) == ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    assert sig["max_rows"].default == 64 and sig["t_start"].default == 0
    assert callable(tmg_ops.latent_nonces)
    assert inspect.signature(LSTMCFlowDecoder.reverse).parameters["rows_per_key"].default is None


def _tiny_model():
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()


def test_sample_ensemble_on_cpu_raises():
    m = _tiny_model()
    x = torch.zeros(2, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.sampleEnsemble(x, None, 3)


def test_model_pred_stats_on_cpu_raises():
    from utils import utils
    m = _tiny_model()
    log = SimpleNamespace(log=lambda *a, **k: None)
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    loader = [(x, torch.zeros(2, 3, 2, 16, 16), torch.ones(2))]
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredStats(SimpleNamespace(device=None), m, loader, log, samples=2, tmax=2)


def test_ensemble_stats_on_cpu_raises():
    import tmg_ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        tmg_ops.EnsembleStats(2, 1, 3, 4, 4, 1, "cpu", torch.zeros(3), torch.ones(3))
