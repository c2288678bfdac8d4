"""Navier-Stokes residuals on the HIP path.  API mirror of the reference's pc/physicsConstrained.py:17-94: the stencils of
pc/grad1Filter.py and pc/grad2Filter.py (kernel_size 3 or 5, any combination) are evaluated inside the kernels, with or without the
cell-size scaling.  The trainer's loss (3x3, scaled: trainFlowParallel.py:115) runs on the fused tile kernel of tmg_phys_fwd; every
other combination on tmg_phys_fields.  Both residuals are differentiable, as the reference's F.conv2d chains are: when an input
requires grad the forward runs inside _ResidualFn, whose backward is the adjoint kernel tmg_phys_fields_bwd for every stencil pair and
scaling (the fast path included).  Without grad the calls are the plain kernel launches."""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

import tmg_hip as H


class _ResidualFn(torch.autograd.Function):
    """One residual field of `phys` ('div': calcDivergence, 'pres': calcPressurePoisson) with its adjoint.  u: [N,2,H,W] (a view is
    fine: autograd carries the gradient back through the caller's slicing), p: [N,1,H,W] or None for 'div'.  `fast` routes the forward
    through the fused tile kernel of the trainer's 3x3 / scaled case; the backward is tmg_phys_fields_bwd either way."""

    @staticmethod
    def forward(ctx, u, p_, phys, scale, which, fast):
        u = u.contiguous()
        p_ = p_.contiguous() if p_ is not None else None
        out = phys._forward(u, p_, scale, which, fast)
        ctx.save_for_backward(u, p_)
        ctx.cfg = (phys.dx, phys.dy, phys.rho, phys.k1, phys.k2, scale, which)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        u, p_ = ctx.saved_tensors
        dx, dy, rho, k1, k2, scale, which = ctx.cfg
        g = g.contiguous()
        du = torch.empty_like(u)
        dp = torch.empty_like(p_) if (which == 'pres' and ctx.needs_input_grad[1]) else None
        H.phys_fields_bwd(u, p_ if which == 'pres' else None, g if which == 'div' else None, g if which == 'pres' else None, du, dp,
                          dx, dy, rho, k1, k2, scale)
        return (du if ctx.needs_input_grad[0] else None), dp, None, None, None, None


class PhysConstrainedLES(nn.Module):
    def __init__(self, dx, dy, rho=1.0, grad_kernels=[3, 3]):
        super().__init__()
        for k in grad_kernels[:2]:
            if int(k) not in (3, 5):
                raise ValueError('kernel_size size {:d} is not supported!'.format(int(k)))      # as grad1Filter.py:57 / grad2Filter.py:49
        self.k1, self.k2 = int(grad_kernels[0]), int(grad_kernels[1])
        self.rho, self.dx, self.dy = rho, dx, dy

    def _fast(self, scale):
        return scale and self.k1 == 3 and self.k2 == 3

    def _fields(self, u, p_):
        n, _, hh, ww = u.shape
        y = torch.cat([u, p_ if p_ is not None else torch.zeros((n, 1, hh, ww), device=u.device, dtype=u.dtype)], 1).contiguous()
        pstar = torch.empty((n, 1, hh, ww), device=u.device, dtype=torch.float32)
        ustar = torch.empty((n, 1, hh, ww + 2), device=u.device, dtype=torch.float32)
        H.phys_fwd(y, None, None, (1., 1., 1.), (0., 0., 0.), self.dx, self.dy, self.rho, pstar=pstar, ustar=ustar)
        return pstar, ustar

    def _forward(self, u, p_, scale, which, fast):
        """The residual field of contiguous u [N,2,H,W] (and p [N,1,H,W] for 'pres') without autograd."""
        if fast:
            pstar, ustar = self._fields(u, p_ if which == 'pres' else None)
            return ustar if which == 'div' else pstar
        if which == 'div':
            ustar = torch.empty((u.shape[0], 1, u.shape[2], u.shape[3] + 2), device=u.device, dtype=torch.float32)
            H.phys_fields(u, None, ustar, None, self.dx, self.dy, self.rho, self.k1, self.k2, scale)
            return ustar
        pstar = torch.empty((u.shape[0], 1, u.shape[2], u.shape[3]), device=u.device, dtype=torch.float32)
        H.phys_fields(u, p_, None, pstar, self.dx, self.dy, self.rho, self.k1, self.k2, scale)
        return pstar

    def calcDivergence(self, uPred, scale=True):
        """[B,2,H,W] velocity -> [B,1,H,W+2] clamped divergence, dx-scaled when `scale` (first/last column replicated, reference :42-60)."""
        if torch.is_grad_enabled() and uPred.requires_grad:
            return _ResidualFn.apply(uPred[:, :2], None, self, scale, 'div', self._fast(scale))
        if self._fast(scale):
            return self._fields(uPred[:, :2], None)[1]
        u = uPred[:, :2].contiguous()
        ustar = torch.empty((u.shape[0], 1, u.shape[2], u.shape[3] + 2), device=u.device, dtype=torch.float32)
        H.phys_fields(u, None, ustar, None, self.dx, self.dy, self.rho, self.k1, self.k2, scale)
        return ustar

    def calcPressurePoisson(self, uPred, pPred, scale=True):
        """Residual of the pressure Poisson equation, dx*dy-scaled when `scale`, clamped to [-1,1] (reference :62-94)."""
        if torch.is_grad_enabled() and (uPred.requires_grad or pPred.requires_grad):
            return _ResidualFn.apply(uPred[:, :2], pPred, self, scale, 'pres', self._fast(scale))
        if self._fast(scale):
            return self._fields(uPred[:, :2], pPred)[0]
        u, p_ = uPred[:, :2].contiguous(), pPred.contiguous()
        pstar = torch.empty((u.shape[0], 1, u.shape[2], u.shape[3]), device=u.device, dtype=torch.float32)
        H.phys_fields(u, p_, None, pstar, self.dx, self.dy, self.rho, self.k1, self.k2, scale)
        return pstar
