"""Backward of the physics residuals PhysConstrainedLES.calcDivergence / calcPressurePoisson (the adjoint kernel
tmg_phys_fields_bwd) and of TMGLowLoss.calcVPres / calcVDiv.

Bounds: the HIP kernels run in fp32 against fp64 references, relative L2 <= 2e-5 and max-abs <= 2e-4 * max|ref| per gradient.
The clamp passes gradient only where -1 <= pre-clamp value <= 1, and fp32 / fp64 may decide differently for values within
rounding of +-1: the fixture's recording keeps every pre-clamp value 1e-4 away from +-1, and the large-field cases give zero
upstream weight to the few pixels within 1e-4 of +-1 (the test asserts that they are few and that the fields are partly clamped)."""
import pytest
import torch

import common as C
from oracle import physics_oracle as PO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAIRS = [(3, 3), (3, 5), (5, 3), (5, 5)]
COMBOS = [(k1, k2, s) for k1, k2 in PAIRS for s in (True, False)]


def _phys(k1, k2, dx=0.05, dy=0.0625, rho=1.3):
    from pc.physicsConstrained import PhysConstrainedLES
    return PhysConstrainedLES(dx, dy, rho=rho, grad_kernels=[k1, k2])


def _check(got, ref, what, l2=2e-5, mx=2e-4):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(ref.abs().max())
    assert scale > 0, what
    rel = float((got - ref).norm() / ref.norm())
    err = float((got - ref).abs().max())
    assert rel <= l2 and err <= mx * scale, "%s: rel-L2 %.2e, max-abs %.2e (max |ref| %.2e)" % (what, rel, err, scale)


def hip_grads(phys, u, p, gu, gp, scale):
    """d/du of sum(gu * ustar) and d/du, d/dp of sum(gp * pstar) through the module API (fp32 device tensors)."""
    ud = u.detach().clone().requires_grad_(True)
    (phys.calcDivergence(ud, scale=scale) * gu).sum().backward()
    uq, pq = u.detach().clone().requires_grad_(True), p.detach().clone().requires_grad_(True)
    (phys.calcPressurePoisson(uq, pq, scale=scale) * gp).sum().backward()
    return {"du_div": ud.grad, "du_pres": uq.grad, "dp_pres": pq.grad}


@pytest.fixture
def oracle_on_device(monkeypatch):
    """The oracle's stencils moved to the GPU, so its fp64 autograd runs there (the large cases would take minutes on the host)."""
    for name in ("_G1", "_G2", "_G1_5", "_G2_5"):
        monkeypatch.setattr(PO, name, getattr(PO, name).to(DEV))
    return PO


def _raw(u, p, dx, dy, rho, k1, k2, scale):
    """fp64 pre-clamp residuals, restated from the oracle's stencils (physics_oracle.divergence / pressure_poisson without the clamp)."""
    uw = torch.cat((u[:, :, :, :1], u, u[:, :, :, -1:]), dim=-1)
    d = PO.grad1y(uw[:, 1:2], dy, k1) + PO.grad1x(uw[:, 0:1], dx, k1)
    ddp = (PO.grad2x(p, dx, k2) + PO.grad2y(p, dy, k2)) / rho
    rhs = PO.grad1x(u[:, 0:1], dx, k1) ** 2 + 2 * PO.grad1y(u[:, 0:1], dy, k1) * PO.grad1x(u[:, 1:2], dx, k1) + PO.grad1y(u[:, 1:2], dy, k1) ** 2
    return (dx * d if scale else d), (dx * dy * (ddp + rhs) if scale else ddp + rhs)


# ---- 1. against the reference's gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rag", "tiny"])
def test_gradients_match_reference_fixture(case):
    d = C.load_npz("phys_fields_grad.npz")
    dx, dy, rho = (float(v) for v in d["cfg"])
    t = lambda k: torch.from_numpy(d[case + "." + k]).to(DEV)  # noqa: E731
    u, p, gu, gp = t("u"), t("p"), t("gu"), t("gp")
    for k1, k2, scale in COMBOS:
        tag = "%s.k%d%d.%s" % (case, k1, k2, "scaled" if scale else "raw")
        au, ap = (float(v) for v in d[tag + ".amp"])
        phys = _phys(k1, k2, dx, dy, rho)
        ud = (au * u).requires_grad_(True)
        (phys.calcDivergence(ud, scale=scale) * gu).sum().backward()
        uq, pq = (ap * u).requires_grad_(True), (ap * p).requires_grad_(True)
        (phys.calcPressurePoisson(uq, pq, scale=scale) * gp).sum().backward()
        for k, v in (("du_div", ud.grad), ("du_pres", uq.grad), ("dp_pres", pq.grad)):
            _check(v, d[tag + "." + k], tag + " " + k)


# ---- 2. against the fp64 oracle on fields of many tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("k1,k2", PAIRS)
def test_gradients_match_fp64_oracle_on_large_fields(k1, k2, oracle_on_device):
    dx, dy, rho = 2.0 / 64, 2.0 / 64 * 1.25, 1.3
    phys = _phys(k1, k2, dx, dy, rho)
    for N, Hh, Ww in ((16, 256, 256), (3, 37, 45)):
        g = torch.Generator(device=DEV).manual_seed(N * 1000 + Hh + 10 * k1 + k2)
        base_u = torch.randn(N, 2, Hh, Ww, device=DEV, generator=g)
        base_p = torch.randn(N, 1, Hh, Ww, device=DEV, generator=g)
        gu0 = torch.randn(N, 1, Hh, Ww + 2, device=DEV, generator=g)
        gp0 = torch.randn(N, 1, Hh, Ww, device=DEV, generator=g)
        for scale in (True, False):
            su, sp = (1.6, 0.6) if scale else (0.06, 5e-4)      # amplitudes that clamp part of each residual field
            u, p = su * base_u, sp * base_p
            u64, p64 = u.double(), p.double()
            raw_d, raw_p = _raw(u64, p64, dx, dy, rho, k1, k2, scale)
            near_d, near_p = ((raw_d.abs() - 1).abs() < 1e-4), ((raw_p.abs() - 1).abs() < 1e-4)
            what = "k%d%d %s %dx%dx%d" % (k1, k2, scale, N, Hh, Ww)
            for raw, near in ((raw_d, near_d), (raw_p, near_p)):
                frac = float((raw.abs() > 1).double().mean())
                assert 0.05 < frac < 0.95 and float(near.double().mean()) < 1e-3, (what, frac)
            gu, gp = gu0.masked_fill(near_d, 0.0), gp0.masked_fill(near_p, 0.0)
            for raw, near, gw in ((raw_d, near_d, gu), (raw_p, near_p, gp)):
                assert not bool(((raw.abs() - 1).abs() < 1e-4)[gw != 0].any())
            ud, uq, pq = u64.clone().requires_grad_(True), u64.clone().requires_grad_(True), p64.clone().requires_grad_(True)
            (PO.divergence(ud, dx, dy, k1, scale) * gu.double()).sum().backward()
            (PO.pressure_poisson(uq, pq, dx, dy, rho, k1, k2, scale) * gp.double()).sum().backward()
            got = hip_grads(phys, u, p, gu, gp, scale)
            _check(got["du_div"], ud.grad, what + " du_div")
            _check(got["du_pres"], uq.grad, what + " du_pres")
            _check(got["dp_pres"], pq.grad, what + " dp_pres")


# ---- 3. through the caller's slicing; each input alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("k1,k2,scale", [(3, 3, True), (5, 3, False)])
def test_gradients_reach_slices_of_one_prediction(k1, k2, scale):
    dx, dy, rho = 0.05, 0.0625, 1.3
    phys = _phys(k1, k2, dx, dy, rho)
    g = torch.Generator().manual_seed(5 + k1)
    amp = torch.tensor([1.6, 1.6, 0.6]).view(1, 3, 1, 1) if scale else torch.tensor([0.06, 0.06, 5e-4]).view(1, 3, 1, 1)
    y0 = (amp * torch.randn(4, 3, 40, 36, generator=g)).float()
    gu = torch.randn(4, 1, 40, 38, generator=g)
    gp = torch.randn(4, 1, 40, 36, generator=g)
    y = y0.to(DEV).requires_grad_(True)
    loss = (phys.calcPressurePoisson(y[:, :2], y[:, 2:], scale=scale) * gp.to(DEV)).sum() + \
           (phys.calcDivergence(y[:, :2], scale=scale) * gu.to(DEV)).sum()
    loss.backward()
    yr = y0.double().requires_grad_(True)
    ref = (PO.pressure_poisson(yr[:, :2], yr[:, 2:], dx, dy, rho, k1, k2, scale) * gp.double()).sum() + \
          (PO.divergence(yr[:, :2], dx, dy, k1, scale) * gu.double()).sum()
    ref.backward()
    _check(y.grad, yr.grad, "sliced y")
    assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
    # each input alone, the other one not requiring grad
    u, p = y0[:, :2].to(DEV), y0[:, 2:].to(DEV)
    for which in ("u", "p"):
        ua = u.clone().requires_grad_(which == "u")
        pa = p.clone().requires_grad_(which == "p")
        out = phys.calcPressurePoisson(ua, pa, scale=scale)
        assert out.grad_fn is not None
        (out * gp.to(DEV)).sum().backward()
        if which == "u":
            assert pa.grad is None
            _check(ua.grad, yr.grad[:, :2] - _div_part(y0, gu, phys, scale), "u alone")
        else:
            assert ua.grad is None
            _check(pa.grad, yr.grad[:, 2:], "p alone")


def _div_part(y0, gu, phys, scale):
    ur = y0[:, :2].double().requires_grad_(True)
    (PO.divergence(ur, phys.dx, phys.dy, phys.k1, scale) * gu.double()).sum().backward()
    return ur.grad


def test_no_grad_calls_build_no_graph():
    phys = _phys(5, 5)
    u = torch.randn(2, 2, 20, 20, device=DEV)
    p = torch.randn(2, 1, 20, 20, device=DEV)
    assert phys.calcDivergence(u).grad_fn is None and phys.calcPressurePoisson(u, p).grad_fn is None
    with torch.no_grad():
        ur = u.clone().requires_grad_(True)
        assert phys.calcDivergence(ur).grad_fn is None


# ---- 4. fast path (3x3, scaled: tmg_phys_fwd) against the generic forward -----------------------------------------------------
def test_fast_path_and_generic_path_agree():
    from pc.physicsConstrained import _ResidualFn
    phys = _phys(3, 3)
    g = torch.Generator(device=DEV).manual_seed(3)
    u = 1.6 * torch.randn(3, 2, 50, 70, device=DEV, generator=g)
    p = 0.6 * torch.randn(3, 1, 50, 70, device=DEV, generator=g)
    gu = torch.randn(3, 1, 50, 72, device=DEV, generator=g)
    gp = torch.randn(3, 1, 50, 70, device=DEV, generator=g)
    res = {}
    for fast in (True, False):
        uu, pp = u.clone().requires_grad_(True), p.clone().requires_grad_(True)
        a = _ResidualFn.apply(uu, None, phys, True, 'div', fast)
        b = _ResidualFn.apply(uu, pp, phys, True, 'pres', fast)
        ((a * gu).sum() + (b * gp).sum()).backward()
        res[fast] = (a.detach(), b.detach(), uu.grad, pp.grad)
    for x, y_, what in zip(res[True], res[False], ("ustar", "pstar", "du", "dp")):
        C.assert_field(x, y_, what, atol=1e-5, rtol=1e-5)
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3])


# ---- 5. bitwise reproducible ---------------------------------------------------------------------------------------------------
def test_backward_is_bitwise_reproducible():
    phys = _phys(5, 5)
    g = torch.Generator(device=DEV).manual_seed(9)
    u = 0.06 * torch.randn(8, 2, 128, 96, device=DEV, generator=g)
    p = 5e-4 * torch.randn(8, 1, 128, 96, device=DEV, generator=g)
    gu = torch.randn(8, 1, 128, 98, device=DEV, generator=g)
    gp = torch.randn(8, 1, 128, 96, device=DEV, generator=g)
    a = hip_grads(phys, u, p, gu, gp, False)
    b = hip_grads(phys, u, p, gu, gp, False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 6. captured in a graph: no host synchronisation ------------------------------------------------------------------------
@pytest.mark.parametrize("k1,k2,scale", [(3, 3, True), (5, 5, False)])
def test_forward_and_backward_replay_from_a_graph(k1, k2, scale):
    phys = _phys(k1, k2)
    g = torch.Generator(device=DEV).manual_seed(21)
    a = (1.6, 0.6) if scale else (0.06, 5e-4)
    u = (a[0] * torch.randn(4, 2, 64, 80, device=DEV, generator=g)).requires_grad_(True)
    p = (a[1] * torch.randn(4, 1, 64, 80, device=DEV, generator=g)).requires_grad_(True)
    gu = torch.randn(4, 1, 64, 82, device=DEV, generator=g)
    gp = torch.randn(4, 1, 64, 80, device=DEV, generator=g)

    def step():
        loss = (phys.calcDivergence(u, scale=scale) * gu).sum() + (phys.calcPressurePoisson(u, p, scale=scale) * gp).sum()
        return torch.autograd.grad(loss, [u, p])

    eager = step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])


# ---- 7. calcVPres + calcVDiv rebuild the fused trainer loss -------------------------------------------------------------------
def test_calcV_terms_rebuild_the_fused_trainer_loss():
    import math
    from types import SimpleNamespace
    from nn.trainFlowParallel import TMGLowLoss
    B, T, Hh, Ww = 2, 10, 256, 256
    g = torch.Generator(device=DEV).manual_seed(77)
    std, mu = torch.tensor([1.3, 0.7, 2.1]), torch.tensor([0.2, -0.1, 0.4])
    crit = TMGLowLoss(SimpleNamespace(beta=200.0, dx=2.0 / 64, dy=2.0 / 64), SimpleNamespace(out_std=std, out_mu=mu)).to(DEV)
    y0 = 0.02 * torch.randn(B, T, 3, Hh, Ww, device=DEV, generator=g)
    tgt = 0.02 * torch.randn(B, T, 3, Hh, Ww, device=DEV, generator=g)
    logp = 50.0 * torch.randn(B, T, device=DEV, generator=g)
    tmean = tgt.mean(1)
    trms = torch.sqrt(((tgt - tmean.unsqueeze(1)) ** 2).mean(1))
    with torch.no_grad():       # every residual well inside the clamp: both kernels take the same clamp decisions
        hat = crit.output_std * y0.view(-1, 3, Hh, Ww) + crit.output_mu
        for f in (crit.phys.calcPressurePoisson(hat[:, :2], hat[:, 2:]), crit.phys.calcDivergence(hat[:, :2])):
            assert float(f.abs().max()) < 0.999
    y1 = y0.clone().requires_grad_(True)
    fused = crit(y1, logp, tgt, tmean, trms)
    fused.backward()
    y2 = y0.clone().requires_grad_(True)
    flat = y2.view(-1, 3, Hh, Ww)
    v_pres, v_div = crit.calcVPres(flat), crit.calcVDiv(flat)
    v_l1 = torch.mean((y2 - tgt) ** 2)
    pred_rms = torch.sqrt(torch.mean((y2 - torch.mean(y2, dim=1).unsqueeze(1)) ** 2, dim=1))
    v_rms = torch.mean((pred_rms - trms) ** 2)
    rebuilt = crit.beta * (v_pres + v_div + v_l1 + v_rms) + logp.mean() / math.log(2.) / (3 * Hh * Ww)
    rebuilt.backward()
    assert abs(rebuilt.item() - fused.item()) <= 1e-5 * abs(fused.item()), (rebuilt.item(), fused.item())
    _check(y2.grad, y1.grad, "y grad", l2=1e-5, mx=1e-4)
    assert v_pres.item() > 0 and v_div.item() > 0
