"""The physics-loss kernels of tmg_physics.hip, each against a plain fp64 statement of the same operation, on every branch of their
launchers.  The tmg_hip wrappers are called directly (H.lib().tmg_* where a refusal code or a NULL argument is the point), no
autograd node or module in between.  The fp64 references use the stencils of oracle/physics_oracle.py (the project's own fp64
restatement, pinned to the recorded fixtures by test_physics_oracle.py) and nothing of tmg_hip, tmg_ops or the modules.

Setup of every case: dx = 2 / 64, dy = 1.25 dx, rho = 1.3 (the trainer passes 1: a missing / rho is invisible there),
sd = (1.3, 0.7, 2.1), mu = (0.2, -0.1, 0.4), y = amp * randn in fp32 from a seeded CPU generator.  The references take the fp32
values of these parameters (what the kernels are given), widened to fp64.

Case map (the plan of every case is computed in the test from the launcher's formula and asserted; outputs sit inside NaN guards):
  tmg_phys_fwd -> phys_fwd_kernel, grid (ceil(W / 16), ceil(H / 16), N), one 16 x 16 tile per block; + phys_div_edge_kernel
    (ceil(2 N H / 256) blocks) when ustar is given.  SHAPES (N, H, W): (5,1,40) one row | (5,40,1) one column: both replicated
    columns are the same column | (5,2,2) smallest 2-D field | (7,3,3) smallest with an interior pixel | (3,16,16) exactly one
    tile | (6,17,33) last tile one row high | (6,33,17) last tile one column wide | (3,37,45) ragged both ways | (4,48,50)
    several tiles.  On each: target given / None (sums[2] stays exactly 0), pstar x ustar given / None (all four), one call with
    sums NULL that writes only the fields.  The three sums are judged separately, both fields elementwise (the two outer columns
    of ustar, written by the edge kernel, with the same bound).  H <= 2 or W <= 2: the pressure sum is exactly 0; H <= 2: the
    divergence sum too.  Sums, not means: no count of zero is divided by.
  tmg_phys_rms -> phys_rms_kernel, min(2048, ceil(B chw / 256)) blocks: (B, T) in {(1,1), (3,2), (2,5), (2,10)} x chw = 3 H W of
    (2,2), (16,16), (37,45); loop: B = 2, T = 2, 3 x 296 x 296 (grid 2048, total % 256 != 0, threads loop); mean_out / coef_out given
    and None (sum_out checked in both); T = 1: rms == 0, coef exactly 0, the sum is sum trms^2; constant series (T = 4, value
    0.5: the fp32 mean is exact) mixed with varying ones: coef exactly 0 there (the fp64 statement defines coef = 0 at rms = 0).
  tmg_phys_bwd_dev -> phys_bwd_kernel, the same grid: every (H, W) above with N = B T, (B, T) = (3,2), (1,5), (2,3) in turn;
    BWD_CONFIGS: each of cp, cd, cl, cr as the only non-zero coefficient and all four together with unequal values; coef / mean
    None (with cr non-zero: ignored) and given; upstream None, a device scalar 0.37, a device scalar 0 (output exactly 0).
    Reference: fp64 autograd of cp/2 sum pstar_int^2 + cd/2 sum ustar_int^2 + cl/2 sum (y - t)^2 + cr/2 sum (rms - trms)^2.
  tmg_phys_fields -> phys_fields_kernel<K1, K2>, min(4096, ceil(N H (W + 2) / 256)) blocks: the four (k1, k2) pairs x scale 0 / 1
    on (2,1,1), (2,2,3), (3,4,4), (3,5,5), (3,37,45); loop (17,256,256): grid 4096, threads loop; ustar None | pstar None | pstar
    None with p None | all given; refused: pstar with p NULL -3, k1 = 7 and k2 = 4 -100, the guarded outputs stay NaN.
  tmg_phys_fields_bwd, direct, the branches the module tests cannot reach (FB_CASES): W = 1, W = 2 (a column both first and last),
    H below the stencil, gustar None, gpstar None with p None, dp None; du NULL -3; N = 0 returns 0 and writes nothing.
  Sensitivity (test_*_detects_*): the fp64 reference with one unit of work altered - the last column of the divergence padded
    with zeros instead of replicated, the interior mask moved by one row, the statistics of sample b + 1 used for sample b, rho
    left out - moves the measure to >= 10x its bound.

Clamp.  A clamped field inherits the bound of its pre-clamp value (the clamp is 1-Lipschitz), so the forward needs no care.
The backward passes gradient only where -1 <= raw <= 1; near |raw| = 1 fp32 and fp64 may decide differently and the whole
source term differs.  phys_bwd: an OUTPUT pixel is taken out of the comparison when a pre-clamp fp64 residual that enters the
loss, within its 3 x 3 stencil reach (the same after the column replication), has ||raw| - 1| < 1e-4 (the margin of
test_phys_grad_gpu.py).  Asserted per case: at most 1 % of the output pixels are taken out, and the residual under test is clamped
on 5 % .. 95 % of its pixels.  Amplitudes, measured with these fp64 formulas on the CPU on exactly the fields of the test (N = B T,
seed 1000 N + H + W): pressure alone 0.3 (36.7 .. 62.5 % of the pressure residual clamped, at most 0.27 % of the outputs taken out),
divergence alone 2.5 (37.5 .. 51.8 %, at most 0.22 %), all four 1.5 (pressure 81.7 .. 91.7 %, divergence 10.4 .. 27.3 %, at most
0.22 %; the 3 x 3 field with N = 6: 88.9 % / 13.3 %, so it keeps the common amplitude); cl / cr alone: no clamp, nothing taken out.  phys_fields_bwd: the upstream weights exist, so they are zeroed within 1e-4 of the
clamp and no output is taken out.

Error measure: share(a, ref, s, tol) of test_pointwise_kernels.py, elementwise, s_e = the magnitude of the element's own terms:
absolute values pushed through the same stencils (and, backward, through their transposes) in fp64.  u = 2^-24.  Bounds count the
roundings of each kernel's formula, worst case (a sequential K-term sum: K - 1); a K-term sum that ends in one atomic per block
gets sqrt(K) u of the sum of its |terms|.
  field values: A = |sd| |y| + |mu|, hat = sd y + mu: 2 u A (phys_fields reads u, p directly: 0).  3 x 3 stencil sums: the
    weights are powers of two (exact products), 6 non-zero terms in a first-derivative stencil, 9 in a second: 5 / 8 adds.  5 x 5:
    weight / 108 (1), the product (1), 20 / 25 non-zero terms.  e1 = hat + {5 | 21}, e2 = hat + {8 | 26}.
  TOL_D(e1) = e1 + 3: / dx, the add, * dx.  phys_fwd ustar 10 u; fields 8 u (3 x 3), 24 u (5 x 5), of S_d = sd (|G1y| A_v / dy + |G1x| A_u / dx).
  TOL_P(e1, e2) = max(e2 + 4, 2 e1 + 4) + 5: second derivatives: the squared cell size and the divide (2), their add, / rho; products
    of first derivatives: 2 (e1 + 1) + 2; three adds of the four terms, dx dy and its product (2).  phys_fwd pstar 23 u; fields
    19 / 35 / 51 / 51 u for (3,3) (3,5) (5,3) (5,5), of S_p = sp ((|G2x| A_p / dx^2 + |G2y| A_p / dy^2) / rho + X_x^2 + 2 X_y Y_x + Y_y^2).
  sums: sum_e (2 |f_e| TOL S_e + u f_e^2) + sqrt(K) u sum f_e^2, f the clamped field; L2: (5 + sqrt K) u sum (y - t)^2.
  rms: mean T u of M1 = sum_t |y_t| / T (T - 1 adds and the divide).  The deviations inherit that; to first order it cancels in
    sum_t d_t^2 (sum_t d_t = 0) but is counted in full: |d rms| <= u (T M1 + (T / 2 + 3.5) rms) =: E.  e = rms - trms: E + u |e|.
    sum: sum (2 |e| E + 3 u e^2) + sqrt(K) u sum e^2.  coef = e / (T rms): (E + u |e|) / (T rms) + |coef| (E / rms + 2 u).
  phys_bwd: sources a = c raw dx dy: TOL_P + 4 multiplies; s1..s4 = 2 a (first derivative, e1 + 1) + 1: 36 u of their |terms|; s5 = a / rho
    28 u; s6 = cd raw_d dx: TOL_D + 3 = 13 u.  Gather for u, v: source * weight / cell (1), <= 24 non-zero additions (6 + 6 from the
    pressure sources, <= 12 from the divergence taps at a replicated column), * sd, the two adds of the data terms:
    TOL_G_UV = 36 + 1 + 24 + 1 + 2 = 64 u; for p: 28 + 4 + 8 + 1 + 2 = TOL_G_P = 43 u, of the |sources| through the |transposed stencils|.
    L2 term cl (y - t): 5 u of |cl| |y - t|; rms term cr coef (y - mean): 7 u of |cr coef| (|y| + |mean|) (coef, mean rounded to fp32
    on entry).  The bound of an element is the sum of its terms' bounds.
  phys_fields_bwd: a = sp g (1), sources 2 a times a first derivative (e1 + 1) and the product: e1 + 3; gather: weight / cell and the
    product (2; 5 x 5: / 108 too, 3), 30 (3 x 3) / 100 (5 x 5) additions: du 40 u (k1 = 3) / 127 u (k1 = 5); dp: a / rho (2), the weight
    w / dx^2 + w' / dy^2 and the product (4; 5 x 5: 5), 8 / 24 additions: 14 u / 31 u.
Observed on an MI355X (largest share of each bound, from the SHARE lines of the first run of this file, every test passing as
first bounded; LAB_NOTES.md, "The physics-loss and up-sampling kernels against fp64 on every path"): phys_fwd pstar 0.0504, ustar
0.1352 (edge columns 0.1352), sum pstar^2 0.0022, sum ustar^2 0.0269, sum (y - t)^2 0.0812; phys_rms mean 0.2518, coef 0.2802, sum
0.0468; phys_bwd dy with cp / cd / cl / cr alone 0.0223 / 0.0255 / 0.2907 / 0.4943, all four 0.4093; phys_fields ustar 0.2198 (k1 = 3),
0.1100 (k1 = 5), pstar 0.0974 / 0.0421 / 0.0283 / 0.0365 for (3,3) (3,5) (5,3) (5,5); phys_fields_bwd du 0.0314 (k1 = 3), 0.0124
(k1 = 5), dp 0.0595 (k2 = 3), 0.0582 (k2 = 5).  The bounds are worst-case counts (every rounding at its largest, all with one sign),
so shares of a few percent are what a correct kernel gives; the sensitivity tests show what a wrong one gives."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import common as C  # noqa: F401  (sets sys.path)
from oracle import physics_oracle as PO
from test_pointwise_kernels import share, check, misaligned, grid_for, U, SHARES, _report_shares, REF_CPU_MAX  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F64 = torch.float64
GUARD = 64


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


DX, DY, RHO = f32(2.0 / 64), f32(1.25 * 2.0 / 64), f32(1.3)
SD, MU = (1.3, 0.7, 2.1), (0.2, -0.1, 0.4)
SD64 = torch.tensor([f32(v) for v in SD], dtype=F64).view(1, 3, 1, 1)
MU64 = torch.tensor([f32(v) for v in MU], dtype=F64).view(1, 3, 1, 1)
HAT = 2                                     # roundings of sd * y + mu


def e1_of(k, hat=0):
    return hat + (5 if k == 3 else 21)


def e2_of(k, hat=0):
    return hat + (8 if k == 3 else 26)


def tol_d(k1, hat=0):
    return (e1_of(k1, hat) + 3) * U


def tol_p(k1, k2, hat=0):
    return (max(e2_of(k2, hat) + 4, 2 * e1_of(k1, hat) + 4) + 5) * U


TOL_US, TOL_PS = tol_d(3, HAT), tol_p(3, 3, HAT)
assert abs(TOL_US - 10 * U) < 1e-20 and abs(TOL_PS - 23 * U) < 1e-20
TOL_G_UV, TOL_G_P, TOL_L, TOL_R = 64 * U, 43 * U, 5 * U, 7 * U

# (N, H, W): tiles across, tiles down, height and width of the last tile
SHAPES = [((5, 1, 40), (3, 1, 1, 8)), ((5, 40, 1), (1, 3, 8, 1)), ((5, 2, 2), (1, 1, 2, 2)), ((7, 3, 3), (1, 1, 3, 3)),
          ((3, 16, 16), (1, 1, 16, 16)), ((6, 17, 33), (3, 2, 1, 1)), ((6, 33, 17), (2, 3, 1, 1)), ((3, 37, 45), (3, 3, 5, 13)),
          ((4, 48, 50), (4, 3, 16, 2))]
SHAPE_IDS = ["%dx%dx%d" % s for s, _ in SHAPES]


def _H():
    import tmg_hip as H
    return H


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(shape, fill=NAN):
    """(buffer, view): `shape` elements of `fill` between two NaN guards."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    v = buf[GUARD:GUARD + n].view(shape)
    v.fill_(fill)
    return buf, v


def intact(g):
    return bool(torch.isnan(g[0][:GUARD]).all()) and bool(torch.isnan(g[0][-GUARD:]).all())


def untouched(g):
    return bool(torch.isnan(g[0]).all())


def tile_plan(N, Hh, Ww):
    """phys_fwd / phys_bwd / phys_fields_bwd: grid ((W + 15) / 16, (H + 15) / 16, N) and the extent of the last tile."""
    gx, gy = (Ww + 15) // 16, (Hh + 15) // 16
    return gx, gy, Hh - 16 * (gy - 1), Ww - 16 * (gx - 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 statements
# ---------------------------------------------------------------------------------------------------------------------------------
def _k(order, ksize, transpose, absolute, like):
    k = PO._stencil(order, ksize).to(like)
    k = k.t() if transpose else k
    return (k.abs() if absolute else k).reshape(1, 1, ksize, ksize)


def corr(f, order, ksize, transpose=False, absolute=False):
    """zero-padded correlation with the oracle's stencil (x direction; transpose: y direction)."""
    return F.conv2d(f, _k(order, ksize, transpose, absolute, f), padding=ksize // 2)


def adj(s, order, ksize, transpose=False):
    """the transpose of corr(., |stencil|): absolute sources through the absolute transposed stencil."""
    return F.conv_transpose2d(s, _k(order, ksize, transpose, True, s), padding=ksize // 2)


def widen(f, rep_last=True):
    last = f[..., -1:] if rep_last else torch.zeros_like(f[..., -1:])
    return torch.cat((f[..., :1], f, last), dim=-1)


def fold(gw):
    """adjoint of widen: widened column 0 falls on column 0, W + 1 on W - 1."""
    g = gw[..., 1:-1].clone()
    g[..., 0] += gw[..., 0]
    g[..., -1] += gw[..., -1]
    return g


def raws(u, v, p, k1=3, k2=3, scale=True, rho=RHO, rep_last=True, absolute=False):
    """pre-clamp (divergence [N,1,H,W+2], pressure [N,1,H,W]) of fields u, v, p [N,1,H,W]; absolute: the own-term magnitudes S_d, S_p
    of |fields| through |stencils|.  Restates physics_oracle.divergence / pressure_poisson without the clamp."""
    ab = absolute
    sd_, sp_ = (DX, DX * DY) if scale else (1.0, 1.0)
    uw, vw = widen(u, rep_last), widen(v, rep_last)
    d = sd_ * (corr(vw, 1, k1, True, ab) / DY + corr(uw, 1, k1, False, ab) / DX)
    if p is None:
        return d, None
    ux_x, ux_y = corr(u, 1, k1, False, ab) / DX, corr(u, 1, k1, True, ab) / DY
    uy_x, uy_y = corr(v, 1, k1, False, ab) / DX, corr(v, 1, k1, True, ab) / DY
    ddp = (corr(p, 2, k2, False, ab) / DX ** 2 + corr(p, 2, k2, True, ab) / DY ** 2) / rho
    return d, sp_ * (ddp + ux_x ** 2 + 2 * ux_y * uy_x + uy_y ** 2)


def adj_scale(Au, Av, wp, wd, k1=3, k2=3, scale=True):
    """|terms| of the adjoint: wp / wd = |upstream weight| x pass mask on the pressure / widened divergence grid (or None);
    returns the magnitudes of d/du, d/dv, d/dp."""
    sd_, sp_ = (DX, DX * DY) if scale else (1.0, 1.0)
    sU, sV, sP = torch.zeros_like(Au), torch.zeros_like(Au), torch.zeros_like(Au)
    if wp is not None:
        a = sp_ * wp
        Xx, Xy = corr(Au, 1, k1, False, True) / DX, corr(Au, 1, k1, True, True) / DY
        Yx, Yy = corr(Av, 1, k1, False, True) / DX, corr(Av, 1, k1, True, True) / DY
        sU = adj(2 * a * Xx, 1, k1) / DX + adj(2 * a * Yx, 1, k1, True) / DY
        sV = adj(2 * a * Xy, 1, k1) / DX + adj(2 * a * Yy, 1, k1, True) / DY
        sP = adj(a / RHO, 2, k2) / DX ** 2 + adj(a / RHO, 2, k2, True) / DY ** 2
    if wd is not None:
        a = sd_ * wd
        sU = sU + fold(adj(a, 1, k1) / DX)
        sV = sV + fold(adj(a, 1, k1, True) / DY)
    return sU, sV, sP


def interior(t, shift=0):
    """rows 1 .. H - 2 (moved by `shift`) and columns 1 .. -2 of a [N,1,H,W'] field."""
    Hh = t.shape[2]
    return t[:, :, max(0, 1 + shift):max(0, Hh - 1 + shift), 1:-1]


def int_mask(t):
    m = torch.zeros_like(t)
    interior(m).fill_(1.0)
    return m


def make_y(N, Hh, Ww, amp, extra=0):
    g = _gen(N * 1000 + Hh + Ww + extra)
    y = (amp * torch.randn(N, 3, Hh, Ww, generator=g)).float()
    t = (amp * torch.randn(N, 3, Hh, Ww, generator=g)).float()
    return y, t


def fwd_ref(y, t, **alter):
    """fp64: dict of fields, their own-term magnitudes, the three sums and their absolute bounds."""
    shift = alter.pop("shift", 0)
    y64 = y.double()
    hat = SD64 * y64 + MU64
    A = SD64.abs() * y64.abs() + MU64.abs()
    rd, rp = raws(hat[:, 0:1], hat[:, 1:2], hat[:, 2:3], **alter)
    Sd, Sp = raws(A[:, 0:1], A[:, 1:2], A[:, 2:3], absolute=True)
    us, ps = rd.clamp(-1, 1), rp.clamp(-1, 1)
    ui, pi, Sdi, Spi = interior(us, shift), interior(ps, shift), interior(Sd, shift), interior(Sp, shift)
    sums = [float((pi ** 2).sum()), float((ui ** 2).sum()), float(((y64 - t.double()) ** 2).sum())]
    bounds = [float((2 * pi.abs() * TOL_PS * Spi + U * pi ** 2).sum()) + math.sqrt(max(pi.numel(), 1)) * U * sums[0],
              float((2 * ui.abs() * TOL_US * Sdi + U * ui ** 2).sum()) + math.sqrt(max(ui.numel(), 1)) * U * sums[1],
              (5 + math.sqrt(y.numel())) * U * sums[2]]
    return dict(us=us, ps=ps, Sd=Sd, Sp=Sp, rd=rd, rp=rp, sums=sums, bounds=bounds)


def check_abs(a, ref, bound, what, case=""):
    """|a - ref| <= bound (an absolute bound worked out for this value), through the common measure."""
    check(torch.as_tensor(a, dtype=F64).reshape(-1), torch.as_tensor(ref, dtype=F64).reshape(-1),
          torch.as_tensor(bound, dtype=F64).reshape(-1) / U, U, what, case)


def share_abs(a, ref, bound):
    return share(torch.as_tensor(a, dtype=F64).reshape(-1), torch.as_tensor(ref, dtype=F64).reshape(-1),
                 torch.as_tensor(bound, dtype=F64).reshape(-1) / U, U)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. phys_fwd
# ---------------------------------------------------------------------------------------------------------------------------------
def run_fwd(y, t, want_sums=True, want_p=True, want_u=True):
    N, _, Hh, Ww = y.shape
    H = _H()
    yd, td = y.to(DEV), (t.to(DEV) if t is not None else None)
    gs = guarded((3,), 0.0)
    gp, gu = guarded((N, 1, Hh, Ww)), guarded((N, 1, Hh, Ww + 2))
    if want_sums:
        H.phys_fwd(yd, td, gs[1], SD, MU, DX, DY, RHO, pstar=gp[1] if want_p else None, ustar=gu[1] if want_u else None)
    else:
        rc = H.lib().tmg_phys_fwd(H._ptr(yd), H._ptr(td), H._ptr(None), H._ptr(gp[1] if want_p else None), H._ptr(gu[1] if want_u else None),
                                  H._i64(N, Hh, Ww), H._flts(list(SD) + list(MU) + [DX, DY, RHO]), H._stream())
        assert rc == 0
    torch.cuda.synchronize()
    assert intact(gs) and intact(gp) and intact(gu)
    if not want_p:
        assert untouched(gp)
    if not want_u:
        assert untouched(gu)
    return gs[1].cpu().double(), gp[1].cpu(), gu[1].cpu()


@pytest.mark.parametrize("shape,plan", SHAPES, ids=SHAPE_IDS)
def test_phys_fwd(shape, plan):
    N, Hh, Ww = shape
    assert tile_plan(N, Hh, Ww) == plan, (shape, tile_plan(N, Hh, Ww))
    assert (2 * N * Hh + 255) // 256 >= 1                      # phys_div_edge_kernel's grid, one thread per edge pixel
    y, t = make_y(N, Hh, Ww, 1.5)
    r = fwd_ref(y, t)
    what = SHAPE_IDS[SHAPES.index((shape, plan))]
    for has_t in (True, False):
        for want_p in (True, False):
            for want_u in (True, False):
                sums, ps, us = run_fwd(y, t if has_t else None, True, want_p, want_u)
                check_abs(sums[0], r["sums"][0], r["bounds"][0], "phys fwd sum pstar^2", what)
                check_abs(sums[1], r["sums"][1], r["bounds"][1], "phys fwd sum ustar^2", what)
                if has_t:
                    check_abs(sums[2], r["sums"][2], r["bounds"][2], "phys fwd sum (y-t)^2", what)
                else:
                    assert float(sums[2]) == 0.0, what
                if Hh <= 2 or Ww <= 2:
                    assert float(sums[0]) == 0.0 and r["sums"][0] == 0.0, what
                if Hh <= 2:
                    assert float(sums[1]) == 0.0 and r["sums"][1] == 0.0, what
                if want_p:
                    check(ps, r["ps"], r["Sp"], TOL_PS, "phys fwd pstar", what)
                if want_u:
                    check(us[..., 1:-1], r["us"][..., 1:-1], r["Sd"][..., 1:-1], TOL_US, "phys fwd ustar", what)
                    check(us[..., [0, -1]], r["us"][..., [0, -1]], r["Sd"][..., [0, -1]], TOL_US, "phys fwd ustar edge columns", what)
    # sums NULL: only the fields are written
    sums, ps, us = run_fwd(y, t, False, True, True)
    assert bool((sums == 0).all()), what
    check(ps, r["ps"], r["Sp"], TOL_PS, "phys fwd pstar", what)
    check(us, r["us"], r["Sd"], TOL_US, "phys fwd ustar", what)
    if min(Hh, Ww) >= 16:
        for raw in (r["rd"], r["rp"]):
            frac = float((raw.abs() > 1).double().mean())
            assert 0.05 < frac < 0.95, (what, frac)            # neither field is all clamp nor free of it


def test_phys_fwd_detects_altered_reference():
    """the divergence's last column zero-padded instead of replicated; the interior mask moved by one row; rho left out."""
    N, Hh, Ww = 6, 17, 33
    y, t = make_y(N, Hh, Ww, 0.4)
    sums, ps, us = run_fwd(y, t)
    good = fwd_ref(y, t)
    assert share(us, good["us"], good["Sd"], TOL_US) <= 1 and share(ps, good["ps"], good["Sp"], TOL_PS) <= 1
    r = fwd_ref(y, t, rep_last=False)
    assert share(us, r["us"], r["Sd"], TOL_US) >= 10
    assert share_abs(sums[1], r["sums"][1], r["bounds"][1]) >= 10
    r = fwd_ref(y, t, shift=1)
    assert share_abs(sums[0], r["sums"][0], r["bounds"][0]) >= 10 and share_abs(sums[1], r["sums"][1], r["bounds"][1]) >= 10
    r = fwd_ref(y, t, rho=1.0)
    assert share(ps, r["ps"], r["Sp"], TOL_PS) >= 10 and share_abs(sums[0], r["sums"][0], r["bounds"][0]) >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. phys_rms
# ---------------------------------------------------------------------------------------------------------------------------------
def rms_ref(y, trms, roll=0):
    """fp64: mean, rms, coef (0 at rms = 0), the sum and the bounds of each."""
    y64 = y.double()
    T = y.shape[1]
    m = y64.mean(1)
    rms = ((y64 - m.unsqueeze(1)) ** 2).mean(1).sqrt()
    if roll:
        m, rms = m.roll(-roll, 0), rms.roll(-roll, 0)
    e = rms - trms.to(rms.device).double()
    pos = rms > 0
    safe = torch.where(pos, rms, torch.ones_like(rms))
    coef = torch.where(pos, e / (T * safe), torch.zeros_like(e))
    M1 = y64.abs().mean(1)
    if roll:
        M1 = M1.roll(-roll, 0)
    E = torch.where(pos, U * (T * M1 + (T / 2 + 3.5) * rms), torch.zeros_like(rms))       # rms == 0 (T = 1, constant series): exact
    total = float((e ** 2).sum())
    b_sum = float((2 * e.abs() * E + 3 * U * e ** 2).sum()) + math.sqrt(e.numel()) * U * total
    b_coef = torch.where(pos, (E + U * e.abs()) / (T * safe) + coef.abs() * (E / safe + 2 * U), torch.zeros_like(e))
    return dict(mean=m, M1=M1, rms=rms, coef=coef, sum=total, b_sum=b_sum, b_coef=b_coef, T=T)


def run_rms(y, trms, with_stats):
    H = _H()
    B, T = y.shape[:2]
    chw = y[0, 0].numel()
    gm, gc = guarded((B,) + tuple(y.shape[2:])), guarded((B,) + tuple(y.shape[2:]))
    gs = guarded((1,), 0.0)
    H.phys_rms(y.to(DEV) if not y.is_cuda else y, trms.to(DEV), gm[1] if with_stats else None, gc[1] if with_stats else None, gs[1])
    torch.cuda.synchronize()
    assert intact(gm) and intact(gc) and intact(gs)
    if not with_stats:
        assert untouched(gm) and untouched(gc)
    return gm[1], gc[1], float(gs[1].double().cpu())


def rms_plan(B, chw):
    total = B * chw
    blocks = min(2048, (total + 255) // 256)
    return blocks, total > blocks * 256


@pytest.mark.parametrize("B,T", [(1, 1), (3, 2), (2, 5), (2, 10)])
@pytest.mark.parametrize("hw", [(2, 2), (16, 16), (37, 45)])
def test_phys_rms(B, T, hw):
    Hh, Ww = hw
    g = _gen(B * 100 + T * 10 + Hh)
    y = torch.randn(B, T, 3, Hh, Ww, generator=g)
    trms = torch.randn(B, 3, Hh, Ww, generator=g).abs()
    blocks, loops = rms_plan(B, 3 * Hh * Ww)
    assert blocks < 2048 and not loops
    r = rms_ref(y, trms)
    what = "B%d T%d %dx%d" % (B, T, Hh, Ww)
    for with_stats in (True, False):
        m, c, s = run_rms(y, trms, with_stats)
        check_abs(s, r["sum"], r["b_sum"], "phys rms sum", what)
        if with_stats:
            check(m, r["mean"], r["M1"], T * U, "phys rms mean", what)
            check_abs(c.cpu(), r["coef"], r["b_coef"], "phys rms coef", what)
            if T == 1:
                assert bool((c == 0).all()) and torch.equal(m.cpu(), y[:, 0]), what
    if T == 1:
        assert bool((r["rms"] == 0).all()) and r["sum"] == float((trms.double() ** 2).sum())


def test_phys_rms_loops_over_the_2048_block_cap():
    B, T, Hh, Ww = 2, 2, 296, 296
    chw = 3 * Hh * Ww
    blocks, loops = rms_plan(B, chw)
    assert blocks == 2048 and loops and B * chw > 2048 * 256 and (B * chw) % 256 != 0
    g = torch.Generator(device=DEV).manual_seed(31)
    y = torch.randn(B, T, 3, Hh, Ww, generator=g, device=DEV)
    trms = torch.randn(B, 3, Hh, Ww, generator=g, device=DEV).abs()
    r = rms_ref(y, trms)                                    # more than REF_CPU_MAX elements: the same fp64 formulas on the device
    assert B * chw > REF_CPU_MAX
    m, c, s = run_rms(y, trms, True)
    check_abs(s, r["sum"], r["b_sum"], "phys rms sum", "loop")
    check(m, r["mean"], r["M1"], T * U, "phys rms mean", "loop")
    check_abs(c, r["coef"], r["b_coef"], "phys rms coef", "loop")
    check_abs(run_rms(y, trms, False)[2], r["sum"], r["b_sum"], "phys rms sum", "loop, no statistics")


def test_phys_rms_constant_series_have_coef_zero():
    """T = 4, value 0.5 (the fp32 mean is exact) at every third pixel, varying series at the others."""
    B, T, Hh, Ww = 2, 4, 16, 16
    g = _gen(77)
    y = torch.randn(B, T, 3, Hh, Ww, generator=g)
    const = (torch.arange(3 * Hh * Ww).view(3, Hh, Ww) % 3 == 0)
    y[:, :, const] = 0.5
    trms = torch.randn(B, 3, Hh, Ww, generator=g).abs()
    r = rms_ref(y, trms)
    assert bool((r["rms"][:, const] == 0).all()) and bool((r["rms"][:, ~const] > 0).all())
    m, c, s = run_rms(y, trms, True)
    assert bool((c[:, const.to(DEV)] == 0).all()) and bool((m[:, const.to(DEV)] == 0.5).all())
    check_abs(c.cpu(), r["coef"], r["b_coef"], "phys rms coef", "const")
    check(m, r["mean"], r["M1"], T * U, "phys rms mean", "const")
    check_abs(s, r["sum"], r["b_sum"], "phys rms sum", "const")


def test_phys_rms_detects_the_next_samples_statistics():
    B, T, Hh, Ww = 3, 2, 16, 16
    g = _gen(78)
    y = torch.randn(B, T, 3, Hh, Ww, generator=g)
    trms = torch.randn(B, 3, Hh, Ww, generator=g).abs()
    m, c, s = run_rms(y, trms, True)
    r = rms_ref(y, trms, roll=1)
    assert share(m, r["mean"], r["M1"], T * U) >= 10
    assert share_abs(c.cpu(), r["coef"], r["b_coef"]) >= 10 and share_abs(s, r["sum"], r["b_sum"]) >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. phys_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
CP, CD, CL, CR = f32(0.7), f32(1.9), f32(0.45), f32(1.3)
UP = f32(0.37)
# (id, (cp, cd, cl, cr), amp (None: by shape), coef / mean given, upstream, residual under test)
BWD_CONFIGS = [
    ("cp", (CP, 0, 0, 0), 0.3, False, None, "p"),
    ("cd", (0, CD, 0, 0), 2.5, False, UP, "d"),
    ("cl", (0, 0, CL, CR), 1.0, False, None, ""),           # cr non-zero with coef NULL: the rms term is skipped
    ("cr", (0, 0, 0, CR), 1.0, True, UP, ""),
    ("all", (CP, CD, CL, CR), None, True, None, "pd"),
    ("all_up0", (CP, CD, CL, CR), None, True, 0.0, ""),
]
BT = [(3, 2), (1, 5), (2, 3)]


def amp_all(Hh, Ww):
    return 1.5


def bwd_ref(y, t, trms, B, T, co, coef_given, up, rho=RHO, rep_last=True, shift=0, stat_roll=0):
    """fp64 autograd of cp/2 sum pstar_int^2 + cd/2 sum ustar_int^2 + cl/2 sum (y - t)^2 + cr/2 sum (rms - trms)^2, times up;
    with it the per-element absolute bound, the near-clamp exclusion mask, the clamped shares and fp32 mean / coef."""
    cp, cd, cl, cr = (float(up if up is not None else 1.0) * c for c in co)
    N, _, Hh, Ww = y.shape
    yv = y.double().requires_grad_(True)
    hat = SD64 * yv + MU64
    rd, rp = raws(hat[:, 0:1], hat[:, 1:2], hat[:, 2:3], rho=rho, rep_last=rep_last)
    loss = cp / 2 * (interior(rp.clamp(-1, 1), shift) ** 2).sum() + cd / 2 * (interior(rd.clamp(-1, 1), shift) ** 2).sum() \
        + cl / 2 * ((yv - t.double()) ** 2).sum()
    y5 = yv.view(B, T, 3, Hh, Ww)
    m = y5.mean(1)
    rms = ((y5 - m.unsqueeze(1)) ** 2).mean(1).sqrt()
    coef = ((rms - trms.double()) / (T * rms)).detach()
    if coef_given:
        loss = loss + cr / 2 * ((rms - trms.double()) ** 2).sum()
    loss.backward()
    ref = yv.grad
    y64, m = y.double(), m.detach()
    if stat_roll:
        term = lambda cf, mn: (cr * cf.unsqueeze(1) * (y64.view(B, T, 3, Hh, Ww) - mn.unsqueeze(1))).reshape(N, 3, Hh, Ww)  # noqa: E731
        ref = ref - term(coef, m) + term(coef.roll(-stat_roll, 0), m.roll(-stat_roll, 0))
    rd, rp = rd.detach(), rp.detach()
    # |terms|
    A = SD64.abs() * y64.abs() + MU64.abs()
    Sd, Sp = raws(A[:, 0:1], A[:, 1:2], A[:, 2:3], absolute=True)
    wp = abs(cp) * Sp * int_mask(rp) * ((rp >= -1) & (rp <= 1))
    wd = abs(cd) * Sd * int_mask(rd) * ((rd >= -1) & (rd <= 1))
    sU, sV, sP = adj_scale(A[:, 0:1], A[:, 1:2], wp, wd)
    s_phys = torch.cat((sU, sV, sP), 1) * SD64.abs()
    bound = torch.cat((TOL_G_UV * s_phys[:, :2], TOL_G_P * s_phys[:, 2:]), 1) + TOL_L * abs(cl) * (y64 - t.double()).abs()
    if coef_given:
        bound = bound + TOL_R * abs(cr) * (coef.abs().unsqueeze(1) * (y64.view(B, T, 3, Hh, Ww).abs() + m.abs().unsqueeze(1))).reshape(N, 3, Hh, Ww)
    # output pixels within the 3 x 3 reach of a residual of the loss that is within 1e-4 of the clamp
    near = torch.zeros(N, 1, Hh, Ww, dtype=F64)
    if cp != 0:
        near = torch.maximum(near, (((rp.abs() - 1).abs() < 1e-4) * int_mask(rp)).double())
    if cd != 0:
        near = torch.maximum(near, (((rd.abs() - 1).abs() < 1e-4) * int_mask(rd)).double()[..., 1:-1])
    out = F.max_pool2d(near, 3, stride=1, padding=1) > 0
    keep = (~out).expand(N, 3, Hh, Ww)
    clamped = dict(p=float((rp.abs() > 1).double().mean()), d=float((rd.abs() > 1).double().mean()))
    return dict(ref=ref, bound=bound, keep=keep, out_share=float(out.double().mean()), clamped=clamped, mean=m.float(), coef=coef.float())


def run_bwd(y, t, mean, coef, T, co, up):
    H = _H()
    gd = guarded(tuple(y.shape))
    upd = torch.tensor([up], device=DEV, dtype=torch.float32) if up is not None else None
    H.phys_bwd(y.to(DEV), t.to(DEV), mean.to(DEV) if mean is not None else None, coef.to(DEV) if coef is not None else None, gd[1], T,
               SD, MU, DX, DY, RHO, co[0], co[1], co[2], co[3], upstream=upd)
    torch.cuda.synchronize()
    assert intact(gd)
    return gd[1].cpu()


def bwd_inputs(Hh, Ww, B, T, amp):
    y, t = make_y(B * T, Hh, Ww, amp)
    trms = (amp * torch.randn(B, 3, Hh, Ww, generator=_gen(B + T + Hh))).abs().float()
    return y, t, trms


def bwd_case_checks(r, under_test, what):
    """both clamp conditions (asserted, not only met)"""
    assert r["out_share"] <= 0.01, (what, r["out_share"])
    for k in under_test:
        assert 0.05 <= r["clamped"][k] <= 0.95, (what, k, r["clamped"][k])


@pytest.mark.parametrize("shape,plan", SHAPES, ids=SHAPE_IDS)
def test_phys_bwd(shape, plan):
    _, Hh, Ww = shape
    B, T = BT[SHAPES.index((shape, plan)) % 3]
    assert tile_plan(B * T, Hh, Ww)[:2] == plan[:2] and tile_plan(B * T, Hh, Ww)[2:] == plan[2:]
    for name, co, amp, coef_given, up, under_test in BWD_CONFIGS:
        what = "%dx%d B%d T%d %s" % (Hh, Ww, B, T, name)
        y, t, trms = bwd_inputs(Hh, Ww, B, T, amp if amp is not None else amp_all(Hh, Ww))
        r = bwd_ref(y, t, trms, B, T, co, coef_given, up)
        bwd_case_checks(r, under_test, what)
        if not under_test:
            assert bool(r["keep"].all()) or name == "all_up0"
        got = run_bwd(y, t, r["mean"] if coef_given else None, r["coef"] if coef_given else None, T, co, up)
        if up == 0.0:
            assert bool((got == 0).all()), what
            continue
        k = r["keep"]
        check_abs(got[k], r["ref"][k], r["bound"][k], "phys bwd dy (%s)" % name, what)
        if name == "cp" and (Hh <= 2 or Ww <= 2):
            assert bool((got == 0).all()), what                     # empty interior: no pressure term at all
        if name == "cd" and Hh <= 2:
            assert bool((got == 0).all()), what


def test_phys_bwd_detects_altered_reference():
    """each alteration of the fp64 reference on the case it belongs to: >= 10x the bound."""
    Hh, Ww, B, T = 17, 33, 3, 2
    for name, alter in (("cd", dict(rep_last=False)), ("cd", dict(shift=1)), ("cp", dict(shift=1)), ("cp", dict(rho=1.0)),
                        ("cr", dict(stat_roll=1)), ("all", dict(stat_roll=1)), ("all", dict(rep_last=False))):
        _, co, amp, coef_given, up, _ = [c for c in BWD_CONFIGS if c[0] == name][0]
        y, t, trms = bwd_inputs(Hh, Ww, B, T, amp if amp is not None else amp_all(Hh, Ww))
        good = bwd_ref(y, t, trms, B, T, co, coef_given, up)
        got = run_bwd(y, t, good["mean"] if coef_given else None, good["coef"] if coef_given else None, T, co, up)
        r = bwd_ref(y, t, trms, B, T, co, coef_given, up, **alter)
        k = good["keep"] & r["keep"]
        assert share_abs(got[k], good["ref"][k], good["bound"][k]) <= 1, (name, alter)
        assert share_abs(got[k], r["ref"][k], r["bound"][k]) >= 10, (name, alter)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. phys_fields
# ---------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(3, 3), (3, 5), (5, 3), (5, 5)]
FIELD_SHAPES = [(2, 1, 1), (2, 2, 3), (3, 4, 4), (3, 5, 5), (3, 37, 45)]


def fields_plan(N, Hh, Ww):
    total = N * Hh * (Ww + 2)
    blocks = min(4096, max(1, (total + 255) // 256))
    return blocks, total > blocks * 256


def field_inputs(N, Hh, Ww, scale, dev="cpu", seed=0):
    g = torch.Generator(device=dev).manual_seed(N * 1000 + Hh + Ww + seed)
    au, ap = (1.6, 0.6) if scale else (0.06, 5e-4)             # amplitudes that clamp part of each residual field
    u = au * torch.randn(N, 2, Hh, Ww, generator=g, device=dev)
    p = ap * torch.randn(N, 1, Hh, Ww, generator=g, device=dev)
    return u, p


def fields_ref(u, p, k1, k2, scale, **alter):
    u64, p64 = u.double(), p.double()
    rd, rp = raws(u64[:, 0:1], u64[:, 1:2], p64, k1, k2, scale, **alter)
    Sd, Sp = raws(u64[:, 0:1].abs(), u64[:, 1:2].abs(), p64.abs(), k1, k2, scale, absolute=True)
    return rd, rp, Sd, Sp


def run_fields(u, p, k1, k2, scale, want_u=True, want_p=True, give_p=True):
    H = _H()
    N, _, Hh, Ww = u.shape
    gu, gp = guarded((N, 1, Hh, Ww + 2)), guarded((N, 1, Hh, Ww))
    H.phys_fields(u.to(DEV), p.to(DEV) if give_p else None, gu[1] if want_u else None, gp[1] if want_p else None, DX, DY, RHO, k1, k2, scale)
    torch.cuda.synchronize()
    assert intact(gu) and intact(gp)
    assert want_u or untouched(gu)
    assert want_p or untouched(gp)
    return gu[1], gp[1]


@pytest.mark.parametrize("scale", [True, False], ids=["scaled", "raw"])
@pytest.mark.parametrize("k1,k2", PAIRS)
def test_phys_fields(k1, k2, scale):
    for N, Hh, Ww in FIELD_SHAPES:
        blocks, loops = fields_plan(N, Hh, Ww)
        assert blocks < 4096 and not loops
        u, p = field_inputs(N, Hh, Ww, scale)
        rd, rp, Sd, Sp = fields_ref(u, p, k1, k2, scale)
        what = "k%d%d %s %dx%dx%d" % (k1, k2, scale, N, Hh, Ww)
        if (Hh, Ww) == (37, 45):
            for raw in (rd, rp):
                assert 0.05 < float((raw.abs() > 1).double().mean()) < 0.95, what
        # all given | ustar None | pstar None | pstar None with p None
        for want_u, want_p, give_p in ((True, True, True), (False, True, True), (True, False, True), (True, False, False)):
            us, ps = run_fields(u, p, k1, k2, scale, want_u, want_p, give_p)
            if want_u:
                check(us, rd.clamp(-1, 1), Sd, tol_d(k1), "phys fields ustar k1=%d" % k1, what)
            if want_p:
                check(ps, rp.clamp(-1, 1), Sp, tol_p(k1, k2), "phys fields pstar k%d%d" % (k1, k2), what)


@pytest.mark.parametrize("k1,k2,scale", [(3, 3, True), (5, 5, False)])
def test_phys_fields_loops_over_the_4096_block_cap(k1, k2, scale):
    N, Hh, Ww = 17, 256, 256
    blocks, loops = fields_plan(N, Hh, Ww)
    assert blocks == 4096 and loops and N * Hh * (Ww + 2) > 4096 * 256 > REF_CPU_MAX
    u, p = field_inputs(N, Hh, Ww, scale, dev=DEV)
    rd, rp, Sd, Sp = fields_ref(u, p, k1, k2, scale)        # the same fp64 formulas on the device
    for raw in (rd, rp):
        assert 0.05 < float((raw.abs() > 1).double().mean()) < 0.95
    us, ps = run_fields(u, p, k1, k2, scale)
    check(us, rd.clamp(-1, 1), Sd, tol_d(k1), "phys fields ustar k1=%d" % k1, "loop")
    check(ps, rp.clamp(-1, 1), Sp, tol_p(k1, k2), "phys fields pstar k%d%d" % (k1, k2), "loop")


def test_phys_fields_refusals_write_nothing():
    H = _H()
    N, Hh, Ww = 3, 5, 5
    u, p = (t.to(DEV) for t in field_inputs(N, Hh, Ww, True))
    fl = H._flts([DX, DY, RHO])
    for k1, k2, give_p, code in ((3, 3, False, -3), (7, 3, True, -100), (3, 4, True, -100), (7, 4, False, -100)):
        gu, gp = guarded((N, 1, Hh, Ww + 2)), guarded((N, 1, Hh, Ww))
        rc = H.lib().tmg_phys_fields(H._ptr(u), H._ptr(p if give_p else None), H._ptr(gu[1]), H._ptr(gp[1]), H._i64(N, Hh, Ww, k1, k2, 1), fl,
                                     H._stream())
        torch.cuda.synchronize()
        assert rc == code, (k1, k2, give_p, rc)
        assert untouched(gu) and untouched(gp), (k1, k2, give_p)
    with pytest.raises(ValueError):
        H.phys_fields(u, p, None, guarded((N, 1, Hh, Ww))[1], DX, DY, RHO, 7, 3, True)


def test_phys_fields_detects_altered_reference():
    """rho left out; the last column of the divergence zero-padded instead of replicated."""
    N, Hh, Ww = 3, 37, 45
    for k1, k2, scale in ((3, 3, True), (5, 5, False)):
        u, p = field_inputs(N, Hh, Ww, scale)
        us, ps = run_fields(u, p, k1, k2, scale)
        rd, rp, Sd, Sp = fields_ref(u, p, k1, k2, scale, rho=1.0)
        assert share(ps, rp.clamp(-1, 1), Sp, tol_p(k1, k2)) >= 10
        rd, rp, Sd, Sp = fields_ref(u, p, k1, k2, scale, rep_last=False)
        assert share(us, rd.clamp(-1, 1), Sd, tol_d(k1)) >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. phys_fields_bwd, the branches the module tests cannot reach
# ---------------------------------------------------------------------------------------------------------------------------------
def tol_fb_du(k1):
    return (e1_of(k1) + 3 + (2 if k1 == 3 else 3) + (30 if k1 == 3 else 100)) * U


def tol_fb_dp(k2):
    return (2 + (4 if k2 == 3 else 5) + (8 if k2 == 3 else 24)) * U


assert abs(tol_fb_du(3) - 40 * U) < 1e-20 and abs(tol_fb_du(5) - 127 * U) < 1e-20
assert abs(tol_fb_dp(3) - 14 * U) < 1e-20 and abs(tol_fb_dp(5) - 31 * U) < 1e-20
# (id, (N, H, W), k1, k2, scale, gustar given, gpstar given, p given, dp given)
FB_CASES = [
    ("w1_k33", (3, 9, 1), 3, 3, True, True, True, True, True),
    ("w1_k55", (2, 7, 1), 5, 5, False, True, True, True, True),
    ("w2_k53", (3, 9, 2), 5, 3, True, True, True, True, True),
    ("w2_k35", (3, 18, 2), 3, 5, False, True, True, True, True),
    ("h2_k55", (2, 2, 9), 5, 5, True, True, True, True, True),
    ("h1w1_k55", (2, 1, 1), 5, 5, True, True, True, True, True),
    ("no_gus", (3, 20, 19), 3, 5, True, False, True, True, True),
    ("no_gps_no_p", (3, 20, 19), 5, 5, False, True, False, False, True),
    ("no_dp", (3, 20, 19), 5, 3, True, True, True, True, False),
    ("no_gps_no_p_no_dp", (3, 17, 33), 3, 3, True, True, False, False, False),
]


def fb_inputs(case):
    name, (N, Hh, Ww), k1, k2, scale, has_gu, has_gp, has_p, has_dp = case
    u, p = field_inputs(N, Hh, Ww, scale, seed=7)
    g = _gen(N + Hh + Ww + k1)
    gu = torch.randn(N, 1, Hh, Ww + 2, generator=g)
    gp = torch.randn(N, 1, Hh, Ww, generator=g)
    rd, rp = raws(u.double()[:, 0:1], u.double()[:, 1:2], p.double(), k1, k2, scale)
    gu = gu.masked_fill((rd.abs() - 1).abs() < 1e-4, 0.0)       # no upstream weight where fp32 and fp64 may clamp differently
    gp = gp.masked_fill((rp.abs() - 1).abs() < 1e-4, 0.0)
    return u, p, gu, gp, rd, rp


def fb_ref(u, p, gu, gp, rd, rp, k1, k2, scale, **alter):
    """fp64 autograd of sum(gu * ustar) + sum(gp * pstar) and the |terms| of du, dp."""
    u64, p64 = u.double().requires_grad_(True), p.double().requires_grad_(True)
    d, q = raws(u64[:, 0:1], u64[:, 1:2], p64, k1, k2, scale, **alter)
    loss = p64.sum() * 0
    if gu is not None:
        loss = loss + (gu.double() * d.clamp(-1, 1)).sum()
    if gp is not None:
        loss = loss + (gp.double() * q.clamp(-1, 1)).sum()
    loss.backward()
    wp = gp.double().abs() * ((rp >= -1) & (rp <= 1)) if gp is not None else None
    wd = gu.double().abs() * ((rd >= -1) & (rd <= 1)) if gu is not None else None
    sU, sV, sP = adj_scale(u.double()[:, 0:1].abs(), u.double()[:, 1:2].abs(), wp, wd, k1, k2, scale)
    return u64.grad, p64.grad, torch.cat((sU, sV), 1), sP


def run_fb(u, p, gu, gp, k1, k2, scale, has_dp):
    H = _H()
    N, _, Hh, Ww = u.shape
    gdu, gdp = guarded((N, 2, Hh, Ww)), guarded((N, 1, Hh, Ww))
    dv = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    H.phys_fields_bwd(u.to(DEV), dv(p), dv(gu), dv(gp), gdu[1], gdp[1] if has_dp else None, DX, DY, RHO, k1, k2, scale)
    torch.cuda.synchronize()
    assert intact(gdu) and intact(gdp)
    assert has_dp or untouched(gdp)
    return gdu[1].cpu(), gdp[1].cpu()


@pytest.mark.parametrize("case", FB_CASES, ids=[c[0] for c in FB_CASES])
def test_phys_fields_bwd_direct(case):
    name, (N, Hh, Ww), k1, k2, scale, has_gu, has_gp, has_p, has_dp = case
    assert tile_plan(N, Hh, Ww)[:2] == ((Ww + 15) // 16, (Hh + 15) // 16)
    u, p, gu, gp, rd, rp = fb_inputs(case)
    gu_, gp_ = (gu if has_gu else None), (gp if has_gp else None)
    du_r, dp_r, s_du, s_dp = fb_ref(u, p, gu_, gp_, rd, rp, k1, k2, scale)
    du, dp = run_fb(u, p if has_p else None, gu_, gp_, k1, k2, scale, has_dp)
    check(du, du_r, s_du, tol_fb_du(k1), "phys fields_bwd du k1=%d" % k1, name)
    if has_dp:
        if has_gp:
            check(dp, dp_r, s_dp, tol_fb_dp(k2), "phys fields_bwd dp k2=%d" % k2, name)
        else:
            assert bool((dp == 0).all()), name                      # no pressure upstream: dp is written, as zeros


def test_phys_fields_bwd_refusal_and_empty_batch():
    H = _H()
    N, Hh, Ww = 3, 9, 7
    u, p = (t.to(DEV) for t in field_inputs(N, Hh, Ww, True))
    gu, gp = torch.randn(N, 1, Hh, Ww + 2, device=DEV), torch.randn(N, 1, Hh, Ww, device=DEV)
    fl = H._flts([DX, DY, RHO])
    gdu, gdp = guarded((N, 2, Hh, Ww)), guarded((N, 1, Hh, Ww))
    call = lambda du, n, pp=p: H.lib().tmg_phys_fields_bwd(H._ptr(u), H._ptr(pp), H._ptr(gu), H._ptr(gp), H._ptr(du), H._ptr(gdp[1]),  # noqa: E731
                                                           H._i64(n, Hh, Ww, 3, 3, 1), fl, H._stream())
    assert call(None, N) == -3                                      # du NULL
    assert call(gdu[1], N, None) == -3                              # gpstar given with p NULL
    assert call(gdu[1], 0) == 0                                     # N = 0: nothing to do, nothing launched
    torch.cuda.synchronize()
    assert untouched(gdu) and untouched(gdp)


def test_phys_fields_bwd_detects_altered_reference():
    """on the one-column field: the last column of the divergence zero-padded instead of replicated; rho left out."""
    case = FB_CASES[0]
    name, (N, Hh, Ww), k1, k2, scale = case[:5]
    u, p, gu, gp, rd, rp = fb_inputs(case)
    du, dp = run_fb(u, p, gu, gp, k1, k2, scale, True)
    du_r, dp_r, s_du, s_dp = fb_ref(u, p, gu, gp, rd, rp, k1, k2, scale)
    assert share(du, du_r, s_du, tol_fb_du(k1)) <= 1 and share(dp, dp_r, s_dp, tol_fb_dp(k2)) <= 1
    du_a = fb_ref(u, p, gu, gp, rd, rp, k1, k2, scale, rep_last=False)[0]
    assert share(du, du_a, s_du, tol_fb_du(k1)) >= 10
    dp_a = fb_ref(u, p, gu, gp, rd, rp, k1, k2, scale, rho=1.0)[1]
    assert share(dp, dp_a, s_dp, tol_fb_dp(k2)) >= 10
