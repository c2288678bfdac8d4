#!/usr/bin/env python3
"""Generate tests/golden/phys_fields_grad.npz by IMPORTING the reference (build container only).

    python tests/golden/make_phys_grad_golden.py            # needs /root/reference/tmglow

Same pattern as make_golden.py: the script drives the reference's public API (`pc.physicsConstrained.PhysConstrainedLES`,
`nn.trainFlowParallel.TMGLowLoss`) in fp64 and records inputs, outputs and input gradients.  Nothing in it is reference source.

Contents (tag = "<case>.k<k1><k2>.<scaled|raw>"; case "rag" = 1 x 17 x 27, 2 x 2 tiles of 16 x 16, the last row of tiles one pixel high; case "tiny" =
2 x 4 x 5, smaller than the halo of the 5 x 5 stencils):
  <case>.u, <case>.p, <case>.gu, <case>.gp      fp32 base fields and seeded upstream weights (gu [N,1,H,W+2], gp [N,1,H,W])
  <tag>.amp                                     (au, ap): the divergence sees fp32(au * u), the pressure residual fp32(ap * u), fp32(ap * p)
  <tag>.du_div                                  d/du of sum(gu * calcDivergence(fp32(au * u), scale))
  <tag>.du_pres, <tag>.dp_pres                  d/du, d/dp of sum(gp * calcPressurePoisson(fp32(ap * u), fp32(ap * p), scale))
  <tag>.margin                                  min over both fields of | |pre-clamp value| - 1 |   (> 1e-4: fp32 sees the same clamp mask)
  loss.y, loss.std, loss.mu, loss.cfg (dx, dy), loss.vpres, loss.vdiv, loss.dy_vpres, loss.dy_vdiv: TMGLowLoss.calcVPres / calcVDiv
The amplitudes leave part of each residual field inside the clamp and part outside (as in make_golden.phys_fields_case).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
REF = "/root/reference/tmglow"

CASES = {"rag": (1, 17, 27), "tiny": (2, 4, 5)}
DX, DY, RHO = 0.05, 0.0625, 1.3
MARGIN = 1e-4


def amplitudes(scale):
    return (50.0, 45.0) if scale else (6.0, 0.45)


def scaled(amp, t):
    """The field both sides see: the product rounded to fp32 (the HIP test forms it in fp32 too)."""
    return (torch.tensor(amp, dtype=torch.float32) * t).float()


class _NoClamp:
    """Within the block torch.clamp is the identity, so the reference returns its pre-clamp residuals."""

    def __enter__(self):
        self.orig = torch.clamp
        torch.clamp = lambda x, *a, **k: x

    def __exit__(self, *exc):
        torch.clamp = self.orig


def field_grads(rpc, k1, k2, scale, u, p, gu, gp):
    phys = rpc.PhysConstrainedLES(DX, DY, rho=RHO, grad_kernels=[k1, k2]).double()
    au, ap = amplitudes(scale)
    ud = scaled(au, u).double().requires_grad_(True)
    (phys.calcDivergence(ud, scale=scale) * gu.double()).sum().backward()
    uq = scaled(ap, u).double().requires_grad_(True)
    pq = scaled(ap, p).double().requires_grad_(True)
    (phys.calcPressurePoisson(uq, pq, scale=scale) * gp.double()).sum().backward()
    with torch.no_grad(), _NoClamp():
        raw_d = phys.calcDivergence(ud, scale=scale)
        raw_p = phys.calcPressurePoisson(uq, pq, scale=scale)
    margin = min(float(((raw_d.abs() - 1).abs()).min()), float(((raw_p.abs() - 1).abs()).min()))
    clamped = (float((raw_d.abs() > 1).double().mean()), float((raw_p.abs() > 1).double().mean()))
    return {"du_div": ud.grad.numpy(), "du_pres": uq.grad.numpy(), "dp_pres": pq.grad.numpy(), "amp": np.array([au, ap]),
            "margin": np.array(margin)}, clamped


def main():
    sys.path.insert(0, REF)
    import pc.physicsConstrained as rpc
    import nn.trainFlowParallel as tfp
    out = {"cfg": np.array([DX, DY, RHO])}
    for ci, (case, (N, Hh, Ww)) in enumerate(CASES.items()):
        # seeds are drawn until no pre-clamp value of any stencil pair / scaling lies within MARGIN of +-1
        for seed in range(100 * ci + 31, 100 * ci + 131):
            g = torch.Generator().manual_seed(seed)
            u = 0.02 * torch.randn(N, 2, Hh, Ww, generator=g)
            p = 0.01 * torch.randn(N, 1, Hh, Ww, generator=g)
            gu = torch.randn(N, 1, Hh, Ww + 2, generator=g)
            gp = torch.randn(N, 1, Hh, Ww, generator=g)
            rec = {}
            for k1 in (3, 5):
                for k2 in (3, 5):
                    for scale in (True, False):
                        tag = "%s.k%d%d.%s" % (case, k1, k2, "scaled" if scale else "raw")
                        rec[tag], clamped = field_grads(rpc, k1, k2, scale, u, p, gu, gp)
                        print("  ", tag, "seed", seed, "margin %.2e" % rec[tag]["margin"], "clamped frac div %.2f pres %.2f" % clamped)
            if min(float(r["margin"]) for r in rec.values()) > MARGIN:
                break
        else:
            raise RuntimeError("no seed keeps the pre-clamp values away from +-1")
        out.update({case + ".u": u.numpy(), case + ".p": p.numpy(), case + ".gu": gu.numpy(), case + ".gp": gp.numpy(),
                    case + ".seed": np.array(seed)})
        for tag, r in rec.items():
            out.update({tag + "." + k: v for k, v in r.items()})
    # TMGLowLoss.calcVPres / calcVDiv (trainFlowParallel.py:153-177) on normalised predictions, fp64
    g = torch.Generator().manual_seed(13)
    B, Hh, Ww, dx = 3, 10, 12, 2.0 / 64
    std = torch.tensor([1.3, 0.7, 2.1], dtype=torch.float64)
    mu = torch.tensor([0.2, -0.1, 0.4], dtype=torch.float64)
    crit = tfp.TMGLowLoss(SimpleNamespace(beta=200.0, dx=dx, dy=dx * 1.25), SimpleNamespace(module=SimpleNamespace(out_std=std, out_mu=mu)))
    crit = crit.double()
    y32 = 0.15 * torch.randn(B, 3, Hh, Ww, generator=g)
    out.update({"loss.y": y32.numpy(), "loss.std": std.numpy(), "loss.mu": mu.numpy(), "loss.cfg": np.array([dx, dx * 1.25])})
    for name in ("vpres", "vdiv"):
        y = y32.double().requires_grad_(True)
        v = crit.calcVPres(y) if name == "vpres" else crit.calcVDiv(y)
        v.backward()
        out["loss." + name] = np.array(v.item())
        out["loss.dy_" + name] = y.grad.numpy()
        print("  loss", name, v.item())
    with torch.no_grad(), _NoClamp():
        hat = std.view(1, 3, 1, 1) * y32.double() + mu.view(1, 3, 1, 1)
        raw = (crit.phys.calcPressurePoisson(hat[:, :2], hat[:, 2:]), crit.phys.calcDivergence(hat[:, :2]))
    out["loss.margin"] = np.array(min(float(((r.abs() - 1).abs()).min()) for r in raw))
    out["loss.clamped"] = np.array([float((r.abs() > 1).double().mean()) for r in raw])
    print("  loss margin %.2e clamped" % out["loss.margin"], out["loss.clamped"])
    path = os.path.join(HERE, "phys_fields_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
