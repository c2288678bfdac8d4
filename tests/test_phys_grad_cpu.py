"""The gradient fixture of the physics residuals (tests/golden/phys_fields_grad.npz, recorded from the reference's
PhysConstrainedLES and TMGLowLoss in fp64) against the autograd of the fp64 oracle, and the CPU-visible parts of the
differentiable residual API.  No GPU needed."""
import numpy as np
import pytest
import torch

import common as C
from oracle import physics_oracle as PO

TAGS = ["%s.k%d%d.%s" % (case, k1, k2, s) for case in ("rag", "tiny") for k1 in (3, 5) for k2 in (3, 5) for s in ("scaled", "raw")]


def _rel_max(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def oracle_field_grads(d, tag):
    """fp64 oracle gradients of sum(gu * divergence) and sum(gp * pressure_poisson) on the fixture's inputs."""
    case, ks, sc = tag.split(".")
    k1, k2, scale = int(ks[1]), int(ks[2]), sc == "scaled"
    dx, dy, rho = (float(v) for v in d["cfg"])
    au, ap = (float(v) for v in d[tag + ".amp"])
    u, p = torch.from_numpy(d[case + ".u"]), torch.from_numpy(d[case + ".p"])
    gu, gp = torch.from_numpy(d[case + ".gu"]).double(), torch.from_numpy(d[case + ".gp"]).double()
    f32 = lambda a, t: (torch.tensor(a, dtype=torch.float32) * t).float().double().requires_grad_(True)  # noqa: E731
    ud = f32(au, u)
    (PO.divergence(ud, dx, dy, k1, scale) * gu).sum().backward()
    uq, pq = f32(ap, u), f32(ap, p)
    (PO.pressure_poisson(uq, pq, dx, dy, rho, k1, k2, scale) * gp).sum().backward()
    return {"du_div": ud.grad, "du_pres": uq.grad, "dp_pres": pq.grad}


@pytest.mark.parametrize("tag", TAGS)
def test_gradient_fixture_matches_fp64_oracle(tag):
    d = C.load_npz("phys_fields_grad.npz")
    assert float(d[tag + ".margin"]) > 1e-4       # fp32 kernels see the same clamp mask as the fp64 recording
    got = oracle_field_grads(d, tag)
    for k, v in got.items():
        ref = d[tag + "." + k]
        assert float(np.abs(ref).max()) > 0, (tag, k)
        assert _rel_max(v, ref) <= 1e-12, (tag, k, _rel_max(v, ref))


def test_gradient_fixture_covers_the_clamp_and_the_halo():
    """Partly clamped residuals (zero and non-zero gradient contributions), a multi-tile ragged field and one smaller than the
    halo of the 5x5 stencils."""
    d = C.load_npz("phys_fields_grad.npz")
    assert d["rag.u"].shape[-2:] == (17, 27) and d["tiny.u"].shape[-2:] == (4, 5)
    dx, dy, rho = (float(v) for v in d["cfg"])
    for tag in TAGS:
        case, ks, sc = tag.split(".")
        k1, k2, scale = int(ks[1]), int(ks[2]), sc == "scaled"
        au, ap = (float(v) for v in d[tag + ".amp"])
        u = torch.from_numpy(d[case + ".u"]).double()
        p = torch.from_numpy(d[case + ".p"]).double()
        for field in (PO.divergence(au * u, dx, dy, k1, scale), PO.pressure_poisson(ap * u, ap * p, dx, dy, rho, k1, k2, scale)):
            clamped = float((field.abs() >= 1).double().mean())
            assert 0.0 < clamped < 0.9, (tag, clamped)


@pytest.mark.parametrize("name", ["vpres", "vdiv"])
def test_calcV_fixture_matches_fp64_oracle(name):
    """TMGLowLoss.calcVPres / calcVDiv of the reference (value and y-gradient) against the same terms built from the oracle."""
    d = C.load_npz("phys_fields_grad.npz")
    std = torch.from_numpy(d["loss.std"]).view(1, 3, 1, 1)
    mu = torch.from_numpy(d["loss.mu"]).view(1, 3, 1, 1)
    dx, dy = (float(v) for v in d["loss.cfg"])
    y = torch.from_numpy(d["loss.y"]).double().requires_grad_(True)
    hat = std * y + mu
    if name == "vpres":
        v = torch.mean(PO.pressure_poisson(hat[:, :2], hat[:, 2:], dx, dy)[:, :, 1:-1, 1:-1] ** 2)
    else:
        v = torch.mean(PO.divergence(hat[:, :2], dx, dy)[:, :, 1:-1, 1:-1] ** 2)
    v.backward()
    ref = float(d["loss." + name])
    assert abs(v.item() - ref) <= 1e-12 * abs(ref), (v.item(), ref)
    assert _rel_max(y.grad, d["loss.dy_" + name]) <= 1e-12


def test_loss_module_exposes_the_residual_terms():
    """TMGLowLoss carries the reference's public `phys` member (3x3 stencils, the loss's dx / dy) and calcVPres / calcVDiv."""
    from types import SimpleNamespace
    from nn.trainFlowParallel import TMGLowLoss
    from pc.physicsConstrained import PhysConstrainedLES
    model = SimpleNamespace(out_std=torch.tensor([1.3, 0.7, 2.1]), out_mu=torch.tensor([0.2, -0.1, 0.4]))
    crit = TMGLowLoss(SimpleNamespace(beta=200.0, dx=0.03, dy=0.04), model)
    assert isinstance(crit.phys, PhysConstrainedLES)
    assert (crit.phys.k1, crit.phys.k2, crit.phys.dx, crit.phys.dy, crit.phys.rho) == (3, 3, 0.03, 0.04, 1.0)
    assert callable(crit.calcVPres) and callable(crit.calcVDiv)
    assert len(crit.state_dict()) == 2      # the residual module adds no parameters or buffers


def test_differentiable_residuals_still_refuse_cpu_tensors():
    """The HIP path is fp32-on-device only; with grad it raises as it does without."""
    from pc.physicsConstrained import PhysConstrainedLES
    phys = PhysConstrainedLES(0.05, 0.05, grad_kernels=[5, 3])
    u = torch.zeros(1, 2, 8, 8, requires_grad=True)
    p = torch.zeros(1, 1, 8, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="fp32 tensors on a HIP device"):
        phys.calcDivergence(u, scale=False)
    with pytest.raises(RuntimeError, match="fp32 tensors on a HIP device"):
        phys.calcPressurePoisson(u, p)
