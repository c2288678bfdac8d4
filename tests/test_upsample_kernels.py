"""The bilinear up-sampling kernels of tmg_pointwise.hip (align_corners = True, dense NHWC) against fp64 on every path of their two
launchers.  H.upsample_fwd(src, dst) / H.upsample_bwd(dout, din) are called directly (no autograd node in between); every output
sits between NaN guards that must stay NaN, and the plan of every case (kernel, grid, whether threads loop) is computed in the
test from the launcher's formula and asserted.

Case map (UPS_CASES; (hi, wi) -> (ho, wo), C channels; "mis" = a tensor whose pointer is 4 bytes past a 16-byte boundary):
  tmg_upsample_fwd -> upsample_fwd4_kernel (C % 4 == 0 and 16-byte pointers) else upsample_fwd_kernel; grid_for(work items).
  tmg_upsample_bwd -> upsample_bwd4_kernel (C % 4 == 0, 16-byte pointers and win_ok: 2 (ho - 1) <= 5 (hi - 1) + 2 on both axes,
    hi > 1, wi > 1) else upsample_bwd_kernel (the general gather).
    channels      c4 c8 c32 -> float4 kernels; c1 c3 c6 -> scalar; C = 8 with the low-res tensor (mis_lo), the high-res tensor
                  (mis_hi) or both (mis_both) misaligned -> scalar, forward and backward.
    win_ok edge   w2_4 (2,2)->(4,4) window | w2_5 (2,2)->(5,5) gather | w3_7 window | w3_8 gather | w5_12 window | w5_13 gather |
                  w53_127 (5,3)->(12,7) window on both axes | w53_128 (5,3)->(12,8) gather, one axis over.
    further       ident (6,5)->(6,5) (window) | x3 (4,5)->(12,15) (gather) | r == 0: r0_row (1,6)->(2,12), r0_col (6,1)->(12,2),
                  r0_11_22 (1,1)->(2,2), r0_11_11 (1,1)->(1,1) (hi == 1 or wi == 1: always the gather) | large coordinates on a thin
                  map: thin4 (2,600)->(4,1200) C = 4 (float4, window), thin3 the same with C = 3.
    caps          capf4 1 x (192,192)->(384,384) x 32: forward float4 items 1 179 648 > 4096 * 256, grid 4096, threads loop |
                  capb4 1 x (260,256)->(520,512) x 64: backward float4 items 1 064 960 > 4096 * 256 | caps 1 x (600,600)->(1200,1200)
                  x 3: scalar forward (4 320 000 elements) and scalar backward (1 080 000) both over the cap.
    B in {1, 3} spread over the cases.
  test_fwd4_and_scalar_on_the_same_values: the same values through an aligned and a misaligned tensor.  The source called the two
    kernels bit-identical; on the device they are one or two ulp apart, so the comment was corrected and each is held to bound 1.
  Sensitivity: the reference's last output row taken from row hi - 2 alone (its y1 term lost); one input column's gradient
    missing its outermost candidate output: each >= 10x the bound.

References (neither uses library code).
  1. Primary.  The operation as it DEFINES its source coordinate, in fp32: r = fl32((hi - 1) / (ho - 1)) (0 when ho == 1),
     s = fl32(r o), i0 = min(int(s), hi - 1), i1 = min(i0 + 1, hi - 1), f = s - i0 (exact: s and i0 lie within a factor of 2 or
     i0 = 0), computed in numpy float32 and widened: Wy [ho, hi], Wx [wo, wi] with weights 1 - f and f (exact in fp64).  Forward
     Wy x Wx^T per image and channel in fp64, backward its transpose.  s_e = the same product with |x| (all weights >= 0).
       TOL_FWD = 6 u: every term w_y w_x v passes 1 - fx, the product with v, the inner add, 1 - fy, the outer product, the
         outer add: 6 roundings of 2^-24 at most (an fma saves some).
       TOL_BWD = 12 u: 1 - fy, 1 - fx, wy wx, the product with dout: 4 u; the K <= 64 term sum (<= 8 candidates per axis in the
         window kernel; <= 2 / r + 1 <= 7 per axis for the gather cases here, 2 x 12 for r == 0) sqrt(64) u = 8 u of sum |terms|.
  2. Independent.  fp64 F.interpolate(mode="bilinear", align_corners=True) and its autograd, whose coordinate o (hi - 1) / (ho - 1)
     is exact to fp64.  The kernel's s carries two fp32 roundings (the division, the product): |ds| <= 2 u (hi - 1) per axis.  The
     interpolant is continuous and piecewise linear in s, with slope |v[i + 1] - v[i]| in the cell, so a forward value moves by at most
     |ds_y| Dy + |ds_x| Dx, Dy / Dx the largest neighbour difference (along y / x) over the cells on either side of the output's
     own (rows y0 - 1 .. y0 + 1, columns x0 - 1 .. x0 + 2 for Dy, transposed for Dx: a superset, so an upper bound) - also when s
     lands on the other side of an integer, where int(s) differs but the value does not jump.  Backward: every hat weight moves
     by at most |ds| (slope 1), the product wy wx by at most |ds_y| + |ds_x|, only for outputs within one input step of the input
     (closed interval): (|ds_y| + |ds_x|) sum of |dout| over those.  This term is ADDED to bound 1; on thin4 / thin3
     (2 u 599 per x) it dominates, everywhere else bound 1 does.
Observed on an MI355X (largest share of each bound; LAB_NOTES.md, "The physics-loss and up-sampling kernels against fp64 on every
path"): forward 0.3127 of bound 1 and 0.5675 of bound 2, backward 0.2642 and 0.2278.  On the FIRST run 22 cases missed bound 1 (forward
up to 8995x on caps, backward up to 151x, growing with the coordinate: thin, cap) while all met bound 2: the compiler had contracted
s - i0 into fma(r, o, -i0), so the fraction came from the UNROUNDED product and the integer part from the rounded one, each kernel
with its own choice.  No plan assertion and no bound was touched: the kernels now take the coordinate from upsample_coord
(contraction off) and every case passes.  The bit-for-bit comparison of the float4 and the scalar forward failed by one or two ulp
(1.2e-7 .. 2.4e-7) before and after that fix: the claim in the source was wrong and is corrected there (see the test above)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import common as C  # noqa: F401  (sets sys.path)
from test_pointwise_kernels import share, check, misaligned, grid_for, U, SHARES, _report_shares, REF_CPU_MAX  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
F32 = np.float32
F64 = torch.float64
GUARD = 64                      # fp32 elements of NaN on either side of an output (256 bytes: keeps the alignment)
TOL_FWD = 6 * U
TOL_BWD = (4 + math.sqrt(64)) * U
CAP = 4096 * 256


def _H():
    import tmg_hip as H
    return H


def guarded(shape, mis=False):
    """(buffer, view): a NaN view of `shape` between NaN guards, 16-byte aligned or (mis) 4 bytes past that."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 4,), NAN, device=DEV)
    off = GUARD + (1 if mis else 0)
    v = buf[off:off + n].view(shape)
    assert v.data_ptr() % 16 == (4 if mis else 0) and v.is_contiguous()
    return buf, v, off, n


def intact(g):
    buf, _, off, n = g
    return bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all())


# (id, B, (hi, wi), (ho, wo), C, low-res misaligned, high-res misaligned, forward kernel, backward kernel, fwd loops, bwd loops)
UPS_CASES = [
    ("c4", 1, (5, 7), (10, 14), 4, False, False, "fwd4", "bwd4", False, False),
    ("c8", 3, (5, 7), (10, 14), 8, False, False, "fwd4", "bwd4", False, False),
    ("c32", 1, (3, 4), (6, 8), 32, False, False, "fwd4", "bwd4", False, False),
    ("c1", 3, (5, 7), (10, 14), 1, False, False, "fwd", "bwd", False, False),
    ("c3", 1, (5, 7), (10, 14), 3, False, False, "fwd", "bwd", False, False),
    ("c6", 3, (5, 7), (10, 14), 6, False, False, "fwd", "bwd", False, False),
    ("mis_lo", 3, (5, 7), (10, 14), 8, True, False, "fwd", "bwd", False, False),
    ("mis_hi", 1, (5, 7), (10, 14), 8, False, True, "fwd", "bwd", False, False),
    ("mis_both", 3, (5, 7), (10, 14), 8, True, True, "fwd", "bwd", False, False),
    ("w2_4", 1, (2, 2), (4, 4), 4, False, False, "fwd4", "bwd4", False, False),
    ("w2_5", 3, (2, 2), (5, 5), 4, False, False, "fwd4", "bwd", False, False),
    ("w3_7", 3, (3, 3), (7, 7), 4, False, False, "fwd4", "bwd4", False, False),
    ("w3_8", 1, (3, 3), (8, 8), 4, False, False, "fwd4", "bwd", False, False),
    ("w5_12", 1, (5, 5), (12, 12), 8, False, False, "fwd4", "bwd4", False, False),
    ("w5_13", 3, (5, 5), (13, 13), 8, False, False, "fwd4", "bwd", False, False),
    ("w53_127", 3, (5, 3), (12, 7), 4, False, False, "fwd4", "bwd4", False, False),
    ("w53_128", 1, (5, 3), (12, 8), 4, False, False, "fwd4", "bwd", False, False),
    ("ident", 3, (6, 5), (6, 5), 4, False, False, "fwd4", "bwd4", False, False),
    ("x3", 1, (4, 5), (12, 15), 4, False, False, "fwd4", "bwd", False, False),
    ("r0_row", 3, (1, 6), (2, 12), 4, False, False, "fwd4", "bwd", False, False),
    ("r0_col", 1, (6, 1), (12, 2), 4, False, False, "fwd4", "bwd", False, False),
    ("r0_11_22", 3, (1, 1), (2, 2), 4, False, False, "fwd4", "bwd", False, False),
    ("r0_11_11", 1, (1, 1), (1, 1), 8, False, False, "fwd4", "bwd", False, False),
    ("thin4", 1, (2, 600), (4, 1200), 4, False, False, "fwd4", "bwd4", False, False),
    ("thin3", 3, (2, 600), (4, 1200), 3, False, False, "fwd", "bwd", False, False),
    ("capf4", 1, (192, 192), (384, 384), 32, False, False, "fwd4", "bwd4", True, False),
    ("capb4", 1, (260, 256), (520, 512), 64, False, False, "fwd4", "bwd4", True, True),
    ("caps", 1, (600, 600), (1200, 1200), 3, False, False, "fwd", "bwd", True, True),
]
IDS = [c[0] for c in UPS_CASES]
BY_ID = {c[0]: c for c in UPS_CASES}


def plan_fwd(src, dst):
    """tmg_upsample_fwd: (kernel, grid, threads loop)."""
    B, hi, wi, Cn = src.shape
    _, ho, wo, _ = dst.shape
    total = B * ho * wo * Cn
    vec = Cn % 4 == 0 and total // 4 < 2 ** 31 and (src.data_ptr() | dst.data_ptr()) % 16 == 0
    items = total // 4 if vec else total
    g = grid_for(items)
    return ("fwd4" if vec else "fwd"), g, items > g * 256


def plan_bwd(dout, din):
    """tmg_upsample_bwd: (kernel, grid, threads loop)."""
    B, hi, wi, Cn = din.shape
    _, ho, wo, _ = dout.shape
    total = B * hi * wi * Cn
    win_ok = (ho - 1) * 2 <= (hi - 1) * 5 + 2 and (wo - 1) * 2 <= (wi - 1) * 5 + 2 and hi > 1 and wi > 1
    vec = Cn % 4 == 0 and win_ok and B * ho * wo * Cn // 4 < 2 ** 31 and (dout.data_ptr() | din.data_ptr()) % 16 == 0
    items = total // 4 if vec else total
    g = grid_for(items)
    return ("bwd4" if vec else "bwd"), g, items > g * 256


def axis(n_in, n_out):
    """One axis of the operation as it defines it in fp32: W [n_out, n_in] (fp64 values of the fp32 weights), i0, and the exact
    coordinate in fp64."""
    o = np.arange(n_out)
    r = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    s = (r * o.astype(F32)).astype(F32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    f = (s - i0.astype(F32)).astype(F32).astype(np.float64)
    W = np.zeros((n_out, n_in))
    W[o, i0] = 1.0 - f
    W[o, i1] += f
    exact = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else np.zeros(n_out)
    return W, i0, exact


def _dev(numel):
    return "cpu" if numel <= REF_CPU_MAX else DEV


def fwd_refs(x, ho, wo):
    """x: fp32 CPU [B, hi, wi, C].  (primary, its |terms|, independent, coordinate term), fp64."""
    B, hi, wi, Cn = x.shape
    dev = _dev(B * ho * wo * Cn)
    x64 = x.to(dev).double()
    (Wy, y0, _), (Wx, x0, _) = axis(hi, ho), axis(wi, wo)
    ty, tx = torch.from_numpy(Wy).to(dev), torch.from_numpy(Wx).to(dev)
    up = lambda v: torch.einsum("yi,bijc,xj->byxc", ty, v, tx)  # noqa: E731
    ref, s = up(x64), up(x64.abs())
    ind = F.interpolate(x64.permute(0, 3, 1, 2), size=(ho, wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    # coordinate term: |ds_y| Dy + |ds_x| Dx over the cells around the output's own
    y0t, x0t = torch.from_numpy(y0).to(dev), torch.from_numpy(x0).to(dev)
    coord = torch.zeros_like(ref)
    if hi > 1:
        gy = (x64[:, 1:] - x64[:, :-1]).abs()                       # [B, hi - 1, wi, C]
        Dy = torch.zeros_like(ref)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1, 2):
                Dy = torch.maximum(Dy, gy[:, (y0t + di).clamp(0, hi - 2)][:, :, (x0t + dj).clamp(0, wi - 1)])
        coord += 2 * U * (hi - 1) * Dy
    if wi > 1:
        gx = (x64[:, :, 1:] - x64[:, :, :-1]).abs()                 # [B, hi, wi - 1, C]
        Dx = torch.zeros_like(ref)
        for di in (-1, 0, 1, 2):
            for dj in (-1, 0, 1):
                Dx = torch.maximum(Dx, gx[:, (y0t + di).clamp(0, hi - 1)][:, :, (x0t + dj).clamp(0, wi - 2)])
        coord += 2 * U * (wi - 1) * Dx
    return ref, s, ind, coord


def bwd_refs(d, hi, wi, Wy=None, Wx=None):
    """d: fp32 CPU [B, ho, wo, C].  (primary, its |terms|, independent, coordinate term), fp64."""
    B, ho, wo, Cn = d.shape
    dev = _dev(B * ho * wo * Cn)
    d64 = d.to(dev).double()
    (Wy0, _, ey), (Wx0, _, ex) = axis(hi, ho), axis(wi, wo)
    ty = torch.from_numpy(Wy0 if Wy is None else Wy).to(dev)
    tx = torch.from_numpy(Wx0 if Wx is None else Wx).to(dev)
    down = lambda v, a, b: torch.einsum("yi,byxc,xj->bijc", a, v, b)  # noqa: E731
    ref, s = down(d64, ty, tx), down(d64.abs(), ty, tx)
    xr = torch.zeros(B, Cn, hi, wi, dtype=F64, device=dev, requires_grad=True)
    yr = F.interpolate(xr, size=(ho, wo), mode="bilinear", align_corners=True)
    (yr * d64.permute(0, 3, 1, 2)).sum().backward()
    ind = xr.grad.permute(0, 2, 3, 1)
    Ay = torch.from_numpy((np.abs(ey[:, None] - np.arange(hi)[None]) <= 1.0 + 1e-9).astype(np.float64)).to(dev)
    Ax = torch.from_numpy((np.abs(ex[:, None] - np.arange(wi)[None]) <= 1.0 + 1e-9).astype(np.float64)).to(dev)
    coord = 2 * U * ((hi - 1) + (wi - 1)) * down(d64.abs(), Ay, Ax)
    return ref, s, ind, coord


def _tensors(case, seed_off=0):
    name, B, (hi, wi), (ho, wo), Cn, mlo, mhi = case[:7]
    g = torch.Generator().manual_seed(4000 + 7 * hi + wi + 13 * Cn + B + seed_off)
    x = torch.randn(B, hi, wi, Cn, generator=g)
    d = torch.randn(B, ho, wo, Cn, generator=g)
    return x, d


def _place(t, mis):
    t = t.to(DEV)
    if mis:
        return misaligned(t)
    assert t.data_ptr() % 16 == 0
    return t


def run_fwd(case):
    name, B, (hi, wi), (ho, wo), Cn, mlo, mhi, kf, kb, lf, lb = case
    x, _ = _tensors(case)
    src = _place(x, mlo)
    gd = guarded((B, ho, wo, Cn), mhi)
    kern, grid, loops = plan_fwd(src, gd[1])
    assert (kern, loops) == (kf, lf) and (grid == 4096) == lf, (name, kern, grid, loops)
    _H().upsample_fwd(src, gd[1])
    torch.cuda.synchronize()
    assert intact(gd), name
    assert torch.equal(src.cpu(), x), name
    return x, gd[1]


def run_bwd(case):
    name, B, (hi, wi), (ho, wo), Cn, mlo, mhi, kf, kb, lf, lb = case
    _, d = _tensors(case)
    dout = _place(d, mhi)
    gd = guarded((B, hi, wi, Cn), mlo)
    kern, grid, loops = plan_bwd(dout, gd[1])
    assert (kern, loops) == (kb, lb) and (grid == 4096) == lb, (name, kern, grid, loops)
    _H().upsample_bwd(dout, gd[1])
    torch.cuda.synchronize()
    assert intact(gd), name
    return d, gd[1]


def test_case_table_covers_every_path():
    """(a CPU-side statement about the table itself, kept with the GPU cases it describes)"""
    assert {c[7] for c in UPS_CASES} == {"fwd", "fwd4"} and {c[8] for c in UPS_CASES} == {"bwd", "bwd4"}
    assert any(c[9] and c[7] == k for c in UPS_CASES for k in ("fwd4",)) and any(c[9] and c[7] == "fwd" for c in UPS_CASES)
    assert any(c[10] and c[8] == "bwd4" for c in UPS_CASES) and any(c[10] and c[8] == "bwd" for c in UPS_CASES)
    assert {c[1] for c in UPS_CASES} == {1, 3}
    for name, B, (hi, wi), (ho, wo), Cn, mlo, mhi, kf, kb, lf, lb in UPS_CASES:
        if lf:
            assert B * ho * wo * (Cn // 4 if kf == "fwd4" else Cn) > CAP, name
        if lb:
            assert B * hi * wi * (Cn // 4 if kb == "bwd4" else Cn) > CAP, name


@pytest.mark.parametrize("case", UPS_CASES, ids=IDS)
def test_upsample_forward(case):
    name, (ho, wo) = case[0], case[3]
    x, y = run_fwd(case)
    ref, s, ind, coord = fwd_refs(x, ho, wo)
    check(y, ref, s, TOL_FWD, "ups fwd (fp32-coordinate ref)", name)
    check(y, ind, s + coord / TOL_FWD, TOL_FWD, "ups fwd (interpolate ref)", name)
    if case[2] == case[3]:
        assert torch.equal(y.cpu(), x), name                        # identity: weights 1 and 0


@pytest.mark.parametrize("case", UPS_CASES, ids=IDS)
def test_upsample_backward(case):
    name, (hi, wi) = case[0], case[2]
    d, din = run_bwd(case)
    ref, s, ind, coord = bwd_refs(d, hi, wi)
    check(din, ref, s, TOL_BWD, "ups bwd (fp32-coordinate ref)", name)
    check(din, ind, s + coord / TOL_BWD, TOL_BWD, "ups bwd (interpolate ref)", name)


@pytest.mark.parametrize("name", ["c8", "w3_8", "thin4", "r0_row"])
def test_fwd4_and_scalar_on_the_same_values(name):
    """The same values through upsample_fwd4_kernel (aligned) and upsample_fwd_kernel (misaligned).  The source used to call the
    two bit-identical; on an MI355X they are one or two ulp apart (1.2e-7 .. 2.4e-7 on unit data, with the coordinate pinned
    or not: the compiler contracts the two kernels' expressions into different fma chains), so the comment was corrected and each
    kernel is held to the fp64 bound, on identical values; their difference is then within the two bounds together."""
    case = BY_ID[name]
    _, B, (hi, wi), (ho, wo), Cn = case[:5]
    assert Cn % 4 == 0
    x, _ = _tensors(case, seed_off=1)
    ref, s, _, _ = fwd_refs(x, ho, wo)
    out = {}
    for mis in (False, True):
        src = _place(x, mis)
        gd = guarded((B, ho, wo, Cn), mis)
        assert plan_fwd(src, gd[1])[0] == ("fwd" if mis else "fwd4")
        _H().upsample_fwd(src, gd[1])
        torch.cuda.synchronize()
        assert intact(gd)
        out[mis] = gd[1].cpu()
        check(out[mis], ref, s, TOL_FWD, "ups fwd (fp32-coordinate ref)", name + (" scalar" if mis else " float4"))
    print("fwd4 vs scalar %s: max |diff| %.3e, bit-identical %s" % (name, float((out[False] - out[True]).abs().max()),
                                                                     torch.equal(out[False], out[True])))
    assert share(out[False], out[True].double(), s.cpu(), 2 * TOL_FWD) <= 1, name


def test_forward_detects_a_last_row_from_y0_only():
    """The reference whose last output row is row y0 = hi - 2 alone (the y1 = hi - 1 term, which carries the whole weight there,
    lost): float4 and scalar kernel."""
    for name in ("c8", "c3"):
        case = BY_ID[name]
        (hi, wi), (ho, wo) = case[2], case[3]
        x, y = run_fwd(case)
        ref, s, _, _ = fwd_refs(x, ho, wo)
        Wx = torch.from_numpy(axis(wi, wo)[0])
        ref[:, ho - 1] = torch.einsum("bjc,xj->bxc", x.double()[:, hi - 2], Wx)
        assert share(y, ref, s, TOL_FWD) >= 10, name


def test_backward_detects_a_missing_outermost_candidate():
    """The reference in which ONE input column lost the outermost output column that touches it: window and gather kernel."""
    for name in ("c8", "w5_13", "c3"):
        case = BY_ID[name]
        (hi, wi), (ho, wo) = case[2], case[3]
        d, din = run_bwd(case)
        Wx = axis(wi, wo)[0]
        outer = [int(np.nonzero(Wx[:, j])[0].max()) for j in range(wi)]
        ix = int(np.argmax([Wx[outer[j], j] if outer[j] < wo - 1 else 0.0 for j in range(wi)]))
        assert Wx[outer[ix], ix] >= 0.1
        Wx[outer[ix], ix] = 0.0
        ref, s, _, _ = bwd_refs(d, hi, wi, Wx=Wx)
        full = bwd_refs(d, hi, wi)[0]
        assert torch.equal(ref[:, :, :ix], full[:, :, :ix]) and torch.equal(ref[:, :, ix + 1:], full[:, :, ix + 1:])
        assert share(din, ref, s, TOL_BWD) >= 10, name
