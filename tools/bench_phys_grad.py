#!/usr/bin/env python3
"""Forward + backward of both physics residuals (PhysConstrainedLES.calcDivergence / calcPressurePoisson) for every stencil pair,
at a trainer-sized batch, against the same computation as a torch F.conv2d autograd chain on the GPU (GPU only).

    python tools/bench_phys_grad.py [--n 80] [--hw 256] [--iters 20] [--out FILE.json]

Times come from device events after warm-up.  Rates use the algorithmic traffic (bytes the computation must move at least once):
  adjoint kernel alone (tmg_phys_fields_bwd): read u, v, p and both upstreams, write du, dv, dp   = 32 B / pixel
  forward + backward of both residuals:      the adjoint's 32 B plus the forwards' reads of u, v, p and writes of ustar, pstar
                                              (20 B)                                                = 52 B / pixel
and are set against the 8 TB/s HBM bound of the MI355X."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-turbulence_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import tmg_hip as H  # noqa: E402
from pc.physicsConstrained import PhysConstrainedLES  # noqa: E402

HBM = 8.0e12
DX, DY, RHO = 2.0 / 64, 2.0 / 64, 1.0

# the stencils of the reference's pc/grad1Filter.py / pc/grad2Filter.py (the 5x5 second-derivative one with its last column of -1)
G1 = {3: torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]]) / 8.,
      5: torch.tensor([[1., -8., 0., 8., -1.], [2., -16., 0., 16., -2.], [3., -24., 0., 24., -3.], [2., -16., 0., 16., -2.],
                       [1., -8., 0., 8., -1.]]) / 108.}
G2 = {3: torch.tensor([[1., -2., 1.], [2., -4., 2.], [1., -2., 1.]]) / 4.,
      5: torch.tensor([[-1., 16., -30., 16., -1.], [-2., 32., -60., 32., -1.], [-3., 48., -90., 48., -1.], [-2., 32., -60., 32., -1.],
                       [-1., 16., -30., 16., -1.]]) / 108.}


class TorchChain:
    """calcDivergence / calcPressurePoisson (scaled) as zero-padded F.conv2d correlations, as the reference writes them."""

    def __init__(self, k1, k2, dev):
        self.w1, self.w2 = G1[k1].to(dev).view(1, 1, k1, k1), G2[k2].to(dev).view(1, 1, k2, k2)

    @staticmethod
    def _c(x, w):
        r = w.shape[-1] // 2
        return F.conv2d(F.pad(x, (r, r, r, r)), w)

    def div(self, u):
        u = torch.cat((u[:, :, :, :1], u, u[:, :, :, -1:]), dim=-1)
        star = self._c(u[:, 1:2], self.w1.transpose(-1, -2)) / DY + self._c(u[:, 0:1], self.w1) / DX
        return torch.clamp(DX * star, -1, 1)

    def pres(self, u, p):
        ddp = (self._c(p, self.w2) / DX ** 2 + self._c(p, self.w2.transpose(-1, -2)) / DY ** 2) / RHO
        ux, vx = self._c(u[:, 0:1], self.w1) / DX, self._c(u[:, 1:2], self.w1) / DX
        uy, vy = self._c(u[:, 0:1], self.w1.transpose(-1, -2)) / DY, self._c(u[:, 1:2], self.w1.transpose(-1, -2)) / DY
        return torch.clamp(DX * DY * (ddp + ux ** 2 + 2 * uy * vx + vy ** 2), -1, 1)


def timeit(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3    # seconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=80)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_phys_grad.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    N, S = a.n, a.hw
    g = torch.Generator(device=dev).manual_seed(0)
    u = (1.6 * torch.randn(N, 2, S, S, device=dev, generator=g)).requires_grad_(True)     # partly clamped residuals
    p = (0.6 * torch.randn(N, 1, S, S, device=dev, generator=g)).requires_grad_(True)
    gu = torch.randn(N, 1, S, S + 2, device=dev, generator=g)
    gp = torch.randn(N, 1, S, S, device=dev, generator=g)
    du, dp = torch.empty_like(u), torch.empty_like(p)
    px = N * S * S
    rows = []
    for k1 in (3, 5):
        for k2 in (3, 5):
            phys, ref = PhysConstrainedLES(DX, DY, rho=RHO, grad_kernels=[k1, k2]), TorchChain(k1, k2, dev)

            def hip_fb():
                return torch.autograd.grad([phys.calcDivergence(u), phys.calcPressurePoisson(u, p)], [u, p], [gu, gp])

            def torch_fb():
                return torch.autograd.grad([ref.div(u), ref.pres(u, p)], [u, p], [gu, gp])

            def bwd_only():
                H.phys_fields_bwd(u.detach(), p.detach(), gu, gp, du, dp, DX, DY, RHO, k1, k2, True)

            hg, tg = hip_fb(), torch_fb()
            diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(hg, tg))
            t_bwd, t_hip, t_torch = timeit(bwd_only, a.iters), timeit(hip_fb, a.iters), timeit(torch_fb, a.iters)
            row = {"k1": k1, "k2": k2, "scale": True, "N": N, "H": S, "W": S,
                   "adjoint_kernel_us": t_bwd * 1e6, "adjoint_kernel_TBps": 32 * px / t_bwd / 1e12,
                   "adjoint_kernel_share_of_hbm": 32 * px / t_bwd / HBM,
                   "hip_fwd_bwd_us": t_hip * 1e6, "hip_fwd_bwd_TBps": 52 * px / t_hip / 1e12,
                   "torch_conv2d_fwd_bwd_us": t_torch * 1e6, "speedup_vs_torch": t_torch / t_hip,
                   "max_rel_diff_vs_torch": diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"tool": "tools/bench_phys_grad.py", "device": torch.cuda.get_device_name(0), "iters": a.iters,
           "bytes_per_pixel": {"adjoint_kernel": 32, "fwd_bwd": 52}, "hbm_bound_Bps": HBM, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
