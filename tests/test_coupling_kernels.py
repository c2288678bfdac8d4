"""The fused coupling kernels of the narrow flow levels, and the coupling + mix kernels of the 64- / 128-channel levels, each against
a plain fp64 torch-autograd restatement of the SAME operation, at the shapes, layouts and launch plans where tile kernels go wrong.

Entry points called directly (every one compared with fp64):
  tmg_coupling_fwd         (ctypes, one interleaved [B,H,W,C] tensor)       cpl_fwd_kernel<CT, K4>
  tmg_coupling_fwd_halves  (tmg_hip.coupling_fwd: pairs of halves, slices)  cpl_fwd_kernel<CT, K4>
  tmg_coupling_bwd         (ctypes, interleaved, generative form)           cpl_bwd_kernel<CT, MT, KS, PERM>
  tmg_coupling_bwd_halves  (tmg_hip.coupling_bwd, generative and density)   cpl_bwd_kernel<CT, MT, KS, PERM>
  tmg_dense2_bwd           (tmg_hip.dense2_bwd)                             dense2_bwd_lean_kernel<NQ, TWL>, dense2_bwd_kernel<WG>
  tmg_mix_f32_affine_fwd   (tmg_hip.mix_affine_fwd)                         mix32_kernel<4, 2, 1>, mix32_kernel<8, 1, 1>
  tmg_mix_f32_affine_bwd   (tmg_hip.mix_affine_bwd)                         mix32_kernel<4, 2, 2>, mix32_kernel<8, 1, 2>

The reference layer (tmg_coupling.hip, file header and the comment above CplBP), t = relu(x1 | d1, d2), hc = the conditioning
map's share of the zero conv (before bias and scale), osc = exp(clamp(kappa, -4, ln 4)):
  hh = (conv3x3_valid(pad_replicate(t)) + hc + bz) osc             oracle.tmglow_oracle.zero_conv
  shift = hh[0::2], r = hh[1::2], sg = 2 softsign(r)
  generative (reverse = 1): y2 = x2 e^{-sg} - shift; density (reverse = 0): y2 = (x2 + shift) e^{sg}   oracle affine_apply
  logdet[b] += sum sg;  out = Wm [x1; y2] + bm  (Wm = bm = None: out = [x1 | y2])
Backward contract (the loss is L = <dout, out> + <g, logdet>; checked against the per-op chain at tmg_ops.py:1395-1405, which
feeds affine_bwd's dhh through conv_fwd + conv_rep_border_fix into G0 / GD and only then through dense2_bwd):
  dtin1 = dL/dx1 through the mix ALONE (the pass-through share; dense2_bwd adds the coupling network's share)
  dtin2 = dL/dx2;  DH = osc dL/dhh (= dL/d(conv + hc + bz), channel pairs (shift_j, r_j))
  G0 = dL/dt[:ch], GD = (dL/dt[ch], dL/dt[ch + 1], 0, 0): gradients w.r.t. the RECTIFIED zero-conv input, i.e. BEFORE the ReLU
  mask; tmg_dense2_bwd applies the masks [x1 > 0], [d1 > 0], [d2 > 0] (its header formulas).
  Density form (fwd=True): no mix in front (dtin1 = dout1), x2 is the coupling OUTPUT half y2.

Case map (CU = torch.cuda.get_device_properties(0).multi_processor_count; the launch plans are computed in the test from the
launchers' formulas and asserted, not hard-coded):
  cpl_fwd instantiations: C = 8 (<1,2>) FWD_CASES f8a (rev 1) f8b (rev 0); C = 16 (<1,3>) f16a (1) f16b (0); C = 24 (<2,4>)
    f24a (0) f24b (1); C = 32 (<2,5>) f32a (1) f32b (0).
  cpl_bwd instantiations: C = 8 <1,1,2,PERM> b8a, <1,1,2> (density) b8b; C = 16 <1,1,4,PERM> b16a, <1,1,4> b16b; C = 24 <2,1,6>
    b24a (generative) b24b (density); C = 32 <2,2,8> b32a (generative) b32b (density).
  Optional operands: Wm/bm None f8b f16b f24b f32b, given elsewhere; y2save None f16a f32b, given elsewhere; g None b16a b24b,
    given elsewhere (and mix bwd m64g0).
  Layouts: interleaved through the ctypes entries f8a f24a f32b b8a b24a; halves f8b f16b f24b b8b b16b b32a and the metric
    shapes; channel-slice views with pixel stride > C (x, out, dout, dtin, x2 and always hc = Hc[..., C:2C], DH = stash[..., C:2C])
    f16a f32a b16a b24b b32b plan8.
  Geometry: H, W not multiples of 16 f16a f24a f24b f32b b16a b24a b24b b32b; W < 16 f16a f32b b16a b32b; H = W = 1 (replicate
    adjoint folds the ring and the corners onto the pixel itself) f8a f16b b8a b16b; exactly one tile per image f8b f32a b8b b32a;
    an odd tile count per image f24a b24a (3) and the plan cases (25).
  Launch plans, per kernel (test_cpl_fwd_launch_plans / test_cpl_bwd_launch_plans): B chosen from CU so that per_blk >= 2 with a
    ragged last block, grid >= 16 with grid % 8 != 0 (uneven XCD remap) and >= 64 tiles, and a block's tile run crossing an image
    boundary (log-det flush, tile -> image index); plus the metric shapes once per direction: B = 64, 128 x 128, C = 16 and
    B = 64, 64 x 64, C = 32.  The child process (test_launch_plans_in_a_fresh_process, TMG_CPL_GRID=5 TMG_D2_BLOCKS=3) forces
    runs of 4 - 6 tiles per block with image changes inside one block.
  tmg_dense2_bwd: lean kernel (the level node's call: inputs (x1, D), add0 = the output itself or a separate tensor, split2 / gap2,
    dd_of with the compact pair and the dd_quad slot) NQ = 2 at ch = 4, 8, NQ = 4 at ch = 12, 16; TW_log2 = 3 (W <= 8),
    4 (9 <= W <= 16), 5 (W > 16): D2_LEAN_CASES; general kernel with dW1 / dW2 (WG = true) and without (WG = false: two gradient
    segments), one case with several tiles per block (B from the 512 / nchunks formula): D2_GENERAL_CASES.
  mix32 AFF: forward at the envelope edge (C = 64: ppi 32 accepted, 48 declined; C = 128: 16 accepted, 24 declined), backward at
    ppi = 15 and 33 (not multiples of 16) with g given, and one with g None.
  Declined shapes (test_declined_shapes_write_nothing): C = 12, C = 40, C = 20 (C/2 % 4 != 0), a pixel stride % 4 != 0, a data
    pointer 4 bytes off 16-byte alignment, on every entry point with an envelope; outputs stay NaN, logdet unchanged.
  Sensitivity (test_*_detects_a_wrong_tile): the fp64 reference with the upstream gradient (dout, g) zeroed on one 16 x 16 tile -
    the last tile of the last image and a tile of a middle image - moves every checked output's error measure by >= 10x its
    tolerance; forward kernels the same with the input of one tile perturbed.

Error measure: err(a, ref) = max|a - ref| / max(1, max|ref|) (test_hip_ops._close), NaN = infinite; the log-det image by image:
|ld_b - ref_b| / max(1, |ld0_b| + sum_image |sg|).  Bounds, with u = 2^-24 = 6e-8 the fp32 unit roundoff and K the length of an
fp32 accumulation (rounding errors of a K-term sum grow like sqrt(K) u of the sum of the |terms|, at most K u):
  TOL_OUT = 1e-5 (out, y2): the zero conv sums K = 9 (ch + 2) + 2 <= 164 products (sqrt(K) u = 8e-7 of |terms|, which stay within a
    few times the output scale), the mix C <= 32 more; __expf / __frcp_rn add ~1 ulp each and |dy2/dr| <= 2 |y2| doubles the conv's
    error in y2.  TOL_R = 5e-6 (r): the conv alone.
  TOL_BWD = 1e-5 (dtin, DH, G0, GD, dto1, dhh): Wm^T dout (C terms), three ~1 ulp transcendentals and a squared rcp, then G's
    9 C-term contraction of DH.  TOL_D2 = 1e-5 (dense2 outputs, dd1, dd2, and dW1 / dW2, which accumulate up to 3e5 pixels:
    per-thread partial sums, one atomic per block).
  TOL_LD = 5e-6 of the image's sum |sg|: each sg carries the ~1e-6 relative error of r and one rcp, the wave sums and atomics
    add log2(N) u.
Measured on an MI355X: at most 8.5 % of these bounds (GD 8e-7, r 4e-7, dW2 5e-7, logdet 8e-8 relative).
A dropped or repeated tile moves a measure by O(1e-2 .. 1): three orders or more above every bound."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import common as C  # noqa: F401  (sets sys.path)
from oracle import tmglow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TOL_OUT, TOL_R, TOL_BWD, TOL_D2, TOL_LD = 1e-5, 5e-6, 1e-5, 1e-5, 5e-6
CC = 4                      # conditioning columns of wz between x1 and (d1, d2): wz_d1col = ch + CC, as the level node's ch + Cc
REF_CPU_MAX_PIX = 16384     # fp64 references of larger cases run on the device


# ---------------------------------------------------------------------------------------------------------------------------------
# launch plans (the launchers' formulas; tmg_coupling.hip launch_cpl_fwd / launch_cpl_bwd, tmg_pointwise.hip tmg_dense2_bwd)
# ---------------------------------------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cpl_gcap(C_, kind):
    if os.environ.get("TMG_CPL_GRID"):
        return int(os.environ["TMG_CPL_GRID"])
    return ((3 if C_ <= 16 else 2) if kind == "fwd" else (4 if C_ <= 16 else 2)) * _cus()


def _xcd_block(b, G):
    """tmg_common.h tmg_xcd_block: logical id of physical block b."""
    if G < 16:
        return b
    qn, rn, x = G >> 3, G & 7, b & 7
    return x * qn + min(x, rn) + (b >> 3)


def cpl_plan(ntiles, tpi, gcap):
    per = -(-ntiles // gcap)
    grid = -(-ntiles // per)
    logical = sorted(_xcd_block(b, grid) for b in range(grid))
    assert logical == list(range(grid)), "the XCD remap must be a permutation of the blocks"
    runs = [(l * per, min(l * per + per, ntiles)) for l in range(grid)]
    return dict(per=per, grid=grid, ntiles=ntiles, ragged=runs[-1][1] - runs[-1][0] < per,
                xcd_uneven=grid >= 16 and grid % 8 != 0, cross=any(t0 // tpi != (t1 - 1) // tpi for t0, t1 in runs if t1 > t0))


def _plan_batch(tpi, gcap):
    """Smallest batch whose plan has per_blk >= 2, a ragged last block, grid >= 16 with grid % 8 != 0, >= 64 tiles and a block run
    that crosses an image boundary."""
    for B in range(1, 4096):
        p = cpl_plan(B * tpi, tpi, gcap)
        if p["per"] >= 2 and p["ragged"] and p["xcd_uneven"] and p["ntiles"] >= 64 and p["cross"]:
            return B, p
    raise AssertionError("no batch reaches the plan conditions (tpi %d, gcap %d)" % (tpi, gcap))


def _tiles16(Hh, Ww):
    return -(-Hh // 16) * -(-Ww // 16)


def _d2_blocks(with_wg):
    e = int(os.environ.get("TMG_D2_BLOCKS", "0") or 0)
    return e if e > 0 else (512 if with_wg else 1024)


def _d2_twl(Ww):
    l = 0
    while (1 << l) < Ww:
        l += 1
    return min(max(l, 3), 5)


def d2_plan(B, Hh, Ww, cin_total, ch, lean, with_wg):
    """Blocks and tiles of tmg_dense2_bwd: (TW_log2, NQ or None, blocks along x, tiles)."""
    twl = _d2_twl(Ww)
    TW, TH = 1 << twl, 256 >> twl
    ntiles = B * -(-Hh // TH) * -(-Ww // TW)
    if lean:
        nq = ch // 4
        NQ = 2 if nq <= 2 else 4
        nch = -(-nq // NQ)
    else:
        NQ = None
        cpad = (cin_total + 3) & ~3
        kch = min(cpad, 28)
        nch = -(-cpad // kch)
    g = max(1, _d2_blocks(with_wg) // nch)
    per = -(-ntiles // g)
    return dict(twl=twl, NQ=NQ, grid=-(-ntiles // per), ntiles=ntiles)


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _H():
    import tmg_hip as H
    return H


def _err(a, ref):
    a, ref = a.detach().double().to(ref.device), ref.detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.numel() == 0:
        return 0.0
    d = (a - ref).abs()
    if bool(torch.isnan(d).any()):
        return math.inf
    return float(d.max()) / max(1.0, float(ref.abs().max()))


def _ld_err(ld, ref, scale):
    d = (ld.detach().double().cpu() - ref.detach().double().cpu()).abs() / scale.clamp(min=1.0)
    d[torch.isnan(d)] = math.inf
    return d


def _ref_dev(npix):
    return "cpu" if npix <= REF_CPU_MAX_PIX else DEV


def _nchw(t, rd):
    return t.detach().to(rd, torch.float64).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _osc(kappa):
    return torch.exp(torch.clamp(kappa, -4.0, O.LOG4))


class Buf:
    """An NHWC activation in one of the kernels' layouts: "inter" (one contiguous tensor), "halves" (a pair of [.., C/2] tensors),
    "slice" (channels 4 .. 4 + C of a wider tensor: pixel stride C + 8).  Filled with `init`, or NaN (an output); the channels of a
    slice's parent outside the view are NaN and must stay so."""

    def __init__(self, shape, layout, init=None):
        B, Hh, Ww, Cn = shape
        self.layout, self.C = layout, Cn
        if layout == "slice":
            self.base = torch.full((B, Hh, Ww, Cn + 8), NAN, device=DEV)
            self.arg = self.base[..., 4:4 + Cn]
        elif layout == "halves":
            self.arg = (torch.full((B, Hh, Ww, Cn // 2), NAN, device=DEV), torch.full((B, Hh, Ww, Cn // 2), NAN, device=DEV))
        else:
            self.arg = torch.full(shape, NAN, device=DEV)
        if init is not None:
            if layout == "halves":
                self.arg[0].copy_(init[..., :Cn // 2])
                self.arg[1].copy_(init[..., Cn // 2:])
            else:
                self.arg.copy_(init)

    def value(self):
        return torch.cat(self.arg, 3) if self.layout == "halves" else self.arg

    def half(self, k):
        """View of channel half k (a tensor of its own in the halves layout)."""
        if self.layout == "halves":
            return self.arg[k]
        ch = self.C // 2
        return self.arg[..., k * ch:(k + 1) * ch]

    def outside_intact(self):
        if self.layout != "slice":
            return True
        return bool(torch.isnan(self.base[..., :4]).all()) and bool(torch.isnan(self.base[..., 4 + self.C:]).all())


def _stash(B, Hh, Ww, C_):
    """[B,H,W,3C] NaN stash and its channel slice k = 1 (as the level node's Hc[..., k C:(k + 1) C] / DH)."""
    base = torch.full((B, Hh, Ww, 3 * C_), NAN, device=DEV)
    return base, base[..., C_:2 * C_]


def _stash_intact(base, C_):
    return bool(torch.isnan(base[..., :C_]).all()) and bool(torch.isnan(base[..., 2 * C_:]).all())


def _tile_mask(B, Hh, Ww, where, rd):
    """1 everywhere except one 16 x 16 tile: the last tile of the last image ("last") or the first tile of a middle image ("mid")."""
    M = torch.ones(B, 1, Hh, Ww, dtype=torch.float64, device=rd)
    if where == "last":
        b, y0, x0 = B - 1, 16 * ((Hh - 1) // 16), 16 * ((Ww - 1) // 16)
    else:
        b, y0, x0 = B // 2, 0, 0
    M[b, :, y0:y0 + 16, x0:x0 + 16] = 0.0
    return M, b


# ---------------------------------------------------------------------------------------------------------------------------------
# coupling layer: inputs, fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------------
def cpl_inputs(C_, B, Hh, Ww, seed):
    g = torch.Generator().manual_seed(seed)
    ch = C_ // 2
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    D = torch.zeros(B, Hh, Ww, 4)
    D[..., :2] = rnd(B, Hh, Ww, 2)
    return dict(
        x=rnd(B, Hh, Ww, C_), D=D, hc=rnd(B, Hh, Ww, C_) * 0.5,
        wz=rnd(C_, ch + CC + 2, 3, 3) * 0.12, bz=rnd(C_) * 0.1, kappa=torch.tensor([0.25]),
        Wm=torch.eye(C_) + rnd(C_, C_) * (0.3 / math.sqrt(C_)), bm=rnd(C_) * 0.1,
        ld0=rnd(B) * 5.0, dout=rnd(B, Hh, Ww, C_), g=rnd(B))


def cpl_ref(inp, reverse, mix, rd, x_delta=None):
    """fp64 restatement of one coupling layer; returns the leaves and intermediates needed by the backward reference."""
    C_ = inp["x"].shape[3]
    ch = C_ // 2
    x = _nchw(inp["x"], rd)
    if x_delta is not None:
        x = x + _nchw(x_delta, rd)
    D = _nchw(inp["D"], rd)
    x1m = x[:, :ch].clone().requires_grad_(True)
    x2 = x[:, ch:].clone().requires_grad_(True)
    t = F.relu(torch.cat([x[:, :ch], D[:, :2]], 1)).detach().requires_grad_(True)
    d1c = ch + CC
    wz = inp["wz"].to(rd, torch.float64)
    kappa = inp["kappa"].to(rd, torch.float64)
    P = {"z.conv.weight": torch.cat([wz[:, :ch], wz[:, d1c:d1c + 2]], 1), "z.conv.bias": inp["bz"].to(rd, torch.float64), "z.scale": kappa}
    osc = _osc(kappa)
    hh = O.zero_conv(P, "z.", t) + _nchw(inp["hc"], rd) * osc
    y2, ld = O.affine_apply(hh, x2, reverse)
    sg = 2.0 * F.softsign(hh[:, 1::2])
    y = torch.cat([x1m, y2], 1)
    if mix:
        out = torch.einsum("oc,bchw->bohw", inp["Wm"].to(rd, torch.float64), y) + inp["bm"].to(rd, torch.float64).view(1, -1, 1, 1)
    else:
        out = y
    return dict(x1m=x1m, x2=x2, t=t, hh=hh, y2=y2, ld=ld, sg=sg, out=out, osc=osc)


def cpl_bwd_ref(inp, dens, with_g, rd, M=None):
    """fp64 gradients of L = <dout, out> + <g, logdet> (M: per-pixel weights of both upstream terms) in the kernel's contract."""
    R = cpl_ref(inp, reverse=not dens, mix=not dens, rd=rd)
    B = inp["x"].shape[0]
    ch = inp["x"].shape[3] // 2
    M = torch.ones(1, 1, 1, 1, dtype=torch.float64, device=rd) if M is None else M
    L = (_nchw(inp["dout"], rd) * M * R["out"]).sum()
    if with_g:
        L = L + (inp["g"].to(rd, torch.float64).view(B, 1, 1, 1) * M * R["sg"]).sum()
    dx1, dx2, dt, dhh = torch.autograd.grad(L, [R["x1m"], R["x2"], R["t"], R["hh"]])
    GD = torch.cat([dt[:, ch:], torch.zeros_like(dt[:, ch:])], 1)
    ref = dict(dtin=_nhwc(torch.cat([dx1, dx2], 1)), DH=_nhwc(dhh * R["osc"]), G0=_nhwc(dt[:, :ch]), GD=_nhwc(GD))
    fwd = dict(r=_nhwc(R["hh"][:, 1::2]).detach(), y2=_nhwc(R["y2"]).detach())
    return ref, fwd


# ---------------------------------------------------------------------------------------------------------------------------------
# coupling forward
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_cpl_fwd(inp_dev, x_arg, out_arg, rsave, y2save, logdet, reverse, mix, via):
    """One forward launch; x_arg / out_arg as Buf.arg.  Returns True when launched, False when declined."""
    H = _H()
    C_ = inp_dev["wz"].shape[0]
    d1c = C_ // 2 + CC
    Wm, bm = (inp_dev["Wm"], inp_dev["bm"]) if mix else (None, None)
    if via == "ctypes":      # tmg_coupling_fwd: one interleaved tensor each, dims as the binding builds them
        x, out, hc = x_arg, out_arg, inp_dev["hcv"]
        dims = H._i64(x.shape[0], x.shape[1], x.shape[2], C_, 1 if reverse else 0, H.seg(x)[1], H.seg(out)[1], H.seg(hc)[1],
                      inp_dev["wz"].shape[1], d1c)
        rc = H.lib().tmg_coupling_fwd(H._ptr(x), H._ptr(out), H._ptr(rsave), H._ptr(y2save), H._ptr(inp_dev["D"]), H._ptr(hc),
                                      H._ptr(inp_dev["wz"]), H._ptr(inp_dev["bz"]), H._ptr(inp_dev["kappa"]), H._ptr(Wm), H._ptr(bm),
                                      H._ptr(logdet), dims, H._stream())
        assert rc in (0, -100), rc
        return rc == 0
    return H.coupling_fwd(x_arg, out_arg, rsave, y2save, inp_dev["D"], inp_dev["hcv"], inp_dev["wz"], inp_dev["bz"], inp_dev["kappa"],
                          Wm, bm, logdet, reverse, d1c)


def _to_dev(inp):
    d = {k: v.to(DEV) for k, v in inp.items()}
    B, Hh, Ww, C_ = inp["x"].shape
    d["Hc"], d["hcv"] = _stash(B, Hh, Ww, C_)
    d["hcv"].copy_(d["hc"])
    return d


def check_cpl_fwd(C_, reverse, B, Hh, Ww, layout, mix, with_y2, seed):
    inp = cpl_inputs(C_, B, Hh, Ww, seed)
    dv = _to_dev(inp)
    ch = C_ // 2
    xb = Buf((B, Hh, Ww, C_), layout, dv["x"])
    ob = Buf((B, Hh, Ww, C_), layout)
    rsave = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    y2save = torch.full((B, Hh, Ww, ch), NAN, device=DEV) if with_y2 else None
    logdet = dv["ld0"].clone()
    assert launch_cpl_fwd(dv, xb.arg, ob.arg, rsave, y2save, logdet, reverse, mix, "ctypes" if layout == "inter" else "bind")
    torch.cuda.synchronize()
    rd = _ref_dev(B * Hh * Ww)
    with torch.no_grad():
        R = cpl_ref(inp, reverse, mix, rd)
    errs = dict(out=_err(ob.value(), _nhwc(R["out"])) / TOL_OUT, r=_err(rsave, _nhwc(R["hh"][:, 1::2])) / TOL_R)
    if with_y2:
        errs["y2"] = _err(y2save, _nhwc(R["y2"])) / TOL_OUT
    scale = (inp["ld0"].abs().double() + R["sg"].abs().sum((1, 2, 3)).cpu())
    lde = _ld_err(logdet, inp["ld0"].double() + R["ld"].cpu(), scale)
    errs["logdet"] = float(lde.max()) / TOL_LD
    print("cpl_fwd C=%d rev=%d %dx%dx%d %s mix=%d y2=%d: err / tol %s" % (C_, reverse, B, Hh, Ww, layout, mix, with_y2,
                                                                       {k: "%.2e" % v for k, v in errs.items()}))
    assert xb.outside_intact() and ob.outside_intact() and _stash_intact(dv["Hc"], C_), "wrote outside a channel-slice view"
    for k, v in errs.items():
        assert v <= 1.0, "cpl_fwd %s: err %.3e x tol (per image: %s)" % (k, v, (lde / TOL_LD).tolist()[:8] if k == "logdet" else "")


# (name, C, reverse, B, H, W, layout, mix, y2save)
FWD_CASES = [
    ("f8a", 8, 1, 2, 1, 1, "inter", True, True),
    ("f8b", 8, 0, 3, 16, 16, "halves", False, True),
    ("f16a", 16, 1, 2, 20, 13, "slice", True, False),
    ("f16b", 16, 0, 2, 1, 1, "halves", False, True),
    ("f24a", 24, 0, 2, 5, 40, "inter", True, True),
    ("f24b", 24, 1, 3, 33, 17, "halves", False, True),
    ("f32a", 32, 1, 2, 16, 16, "slice", True, True),
    ("f32b", 32, 0, 2, 9, 7, "inter", False, False),
]


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_cpl_fwd_matches_fp64(case):
    check_cpl_fwd(*case[1:], seed=sum(map(ord, case[0])))


@pytest.mark.parametrize("C_,layout", [(8, "slice"), (32, "halves")])
def test_cpl_fwd_launch_plans(C_, layout):
    """per_blk >= 2 with a ragged last block, grid >= 16 and % 8 != 0, >= 64 tiles, runs across image boundaries: 80 x 80 images
    (25 tiles each), the batch derived from the CU count."""
    B, p = _plan_batch(25, _cpl_gcap(C_, "fwd"))
    print("cpl_fwd plan C=%d: B=%d %s" % (C_, B, p))
    check_cpl_fwd(C_, 1, B, 80, 80, layout, True, True, seed=C_ + 1)


@pytest.mark.parametrize("C_,hw", [(16, (128, 128)), (32, (64, 64))])
def test_cpl_fwd_metric_shapes(C_, hw):
    check_cpl_fwd(C_, 1, 64, hw[0], hw[1], "halves", True, True, seed=C_ + 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# coupling backward
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_cpl_bwd(dv, dout_arg, x2_arg, r, g, DH, dtin_arg, G0, GD, dens, via):
    H = _H()
    C_ = dv["wz"].shape[0]
    d1c = C_ // 2 + CC
    if via == "ctypes":      # tmg_coupling_bwd: interleaved dout / layer input / dtin, generative form
        assert not dens
        x, dout, dtin = x2_arg, dout_arg, dtin_arg
        dims = H._i64(dout.shape[0], dout.shape[1], dout.shape[2], C_, H.seg(dout)[1], H.seg(x)[1], H.seg(DH)[1], H.seg(dtin)[1],
                      dv["wz"].shape[1], d1c)
        rc = H.lib().tmg_coupling_bwd(H._ptr(dout), H._ptr(x), H._ptr(r), H._ptr(g), H._ptr(dv["Wm"]), H._ptr(dv["wz"]),
                                      H._ptr(dv["kappa"]), H._ptr(DH), H._ptr(dtin), H._ptr(G0), H._ptr(GD), dims, H._stream())
        assert rc in (0, -100), rc
        return rc == 0
    return H.coupling_bwd(dout_arg, x2_arg, r, g, dv["Wm"], dv["wz"], dv["kappa"], DH, dtin_arg, G0, GD, d1c, fwd=dens)


def check_cpl_bwd(C_, dens, B, Hh, Ww, layout, with_g, seed):
    inp = cpl_inputs(C_, B, Hh, Ww, seed)
    dv = _to_dev(inp)
    ch = C_ // 2
    rd = _ref_dev(B * Hh * Ww)
    ref, fw = cpl_bwd_ref(inp, dens, with_g, rd)
    db = Buf((B, Hh, Ww, C_), layout, dv["dout"])
    # the second half read by the kernel: the layer input's (generative) or the coupling output's (density), in the same layout
    src = dv["x"].clone()
    if dens:
        src[..., ch:] = fw["y2"].float().to(DEV)
    xb = Buf((B, Hh, Ww, C_), layout, src)
    x2_arg = xb.arg if layout == "inter" else xb.half(1)
    r = fw["r"].float().to(DEV).contiguous()
    DHb, DH = _stash(B, Hh, Ww, C_)
    tb = Buf((B, Hh, Ww, C_), layout)
    G0 = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    GD = torch.full((B, Hh, Ww, 4), NAN, device=DEV)
    g = dv["g"] if with_g else None
    assert launch_cpl_bwd(dv, db.arg, x2_arg, r, g, DH, tb.arg, G0, GD, dens, "ctypes" if layout == "inter" else "bind")
    torch.cuda.synchronize()
    got = dict(dtin=tb.value(), DH=DH, G0=G0, GD=GD)
    errs = {k: _err(got[k], ref[k]) / TOL_BWD for k in ref}
    print("cpl_bwd C=%d dens=%d %dx%dx%d %s g=%d: err / tol %s" % (C_, dens, B, Hh, Ww, layout, with_g,
                                                                 {k: "%.2e" % v for k, v in errs.items()}))
    assert db.outside_intact() and xb.outside_intact() and tb.outside_intact() and _stash_intact(DHb, C_), "wrote outside a view"
    for k, v in errs.items():
        assert v <= 1.0, "cpl_bwd %s: err %.3e x tol" % (k, v)


# (name, C, density, B, H, W, layout, g)
BWD_CASES = [
    ("b8a", 8, False, 2, 1, 1, "inter", True),
    ("b8b", 8, True, 3, 16, 16, "halves", True),
    ("b16a", 16, False, 2, 20, 13, "slice", False),
    ("b16b", 16, True, 2, 1, 1, "halves", True),
    ("b24a", 24, False, 2, 5, 40, "inter", True),
    ("b24b", 24, True, 3, 33, 17, "slice", False),
    ("b32a", 32, False, 2, 16, 16, "halves", True),
    ("b32b", 32, True, 2, 9, 7, "slice", True),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_cpl_bwd_matches_fp64(case):
    check_cpl_bwd(*case[1:], seed=sum(map(ord, case[0])))


@pytest.mark.parametrize("C_,dens,layout", [(8, False, "slice"), (32, False, "halves"), (16, True, "halves")])
def test_cpl_bwd_launch_plans(C_, dens, layout):
    B, p = _plan_batch(25, _cpl_gcap(C_, "bwd"))
    print("cpl_bwd plan C=%d: B=%d %s" % (C_, B, p))
    check_cpl_bwd(C_, dens, B, 80, 80, layout, True, seed=C_ + 3)


@pytest.mark.parametrize("C_,hw", [(16, (128, 128)), (32, (64, 64))])
def test_cpl_bwd_metric_shapes(C_, hw):
    check_cpl_bwd(C_, False, 64, hw[0], hw[1], "halves", True, seed=C_ + 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# tmg_dense2_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def d2_ref(t0, D, G0, GD, W1, W2, rd, M=None):
    """fp64 backward of the two growth-1 layers (denseBlock.py:135-152 via oracle dense2_nonorm's structure) at given d1, d2:
    L = <G0, relu(t0)> + <GD0, relu(d1)> + <GD1, relu(d2)> with d1 = conv(relu(t0), W1) + c1, d2 = conv(relu([t0, d1]), W2) + c2
    and c1, c2 the constants that make d1, d2 equal D's channels 0, 1.  Returns dL/dt0, dL/dd1, dL/dd2, dL/dW1, dL/dW2."""
    t0 = _nchw(t0, rd).requires_grad_(True)
    D = _nchw(D, rd)
    W1 = W1.to(rd, torch.float64).requires_grad_(True)
    W2 = W2.to(rd, torch.float64).requires_grad_(True)
    M = torch.ones(1, 1, 1, 1, dtype=torch.float64, device=rd) if M is None else M
    c1 = F.conv2d(F.relu(t0), W1, padding=1)
    d1 = c1 + (D[:, 0:1] - c1).detach()
    c2 = F.conv2d(F.relu(torch.cat([t0, d1], 1)), W2, padding=1)
    d2 = c2 + (D[:, 1:2] - c2).detach()
    G0, GD = _nchw(G0, rd) * M, _nchw(GD, rd) * M
    L = (G0 * F.relu(t0)).sum() + (GD[:, 0:1] * F.relu(d1)).sum() + (GD[:, 1:2] * F.relu(d2)).sum()
    gt, g1, g2, gw1, gw2 = torch.autograd.grad(L, [t0, d1, d2, W1, W2])
    return _nhwc(gt), _nhwc(g1), _nhwc(g2), gw1, gw2


def d2_inputs(ch, cc, B, Hh, Ww, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    D = torch.zeros(B, Hh, Ww, 4)
    D[..., :2] = rnd(B, Hh, Ww, 2)
    GD = torch.zeros(B, Hh, Ww, 4)
    GD[..., :2] = rnd(B, Hh, Ww, 2)
    return dict(x1=rnd(B, Hh, Ww, ch), cond=rnd(B, Hh, Ww, cc), D=D, GD=GD, G0=rnd(B, Hh, Ww, ch + cc), add0=rnd(B, Hh, Ww, ch),
                w1=rnd(1, ch + cc, 3, 3) * 0.3, w2=rnd(1, ch + cc + 1, 3, 3) * 0.3, dW1=rnd(1, ch + cc, 3, 3), dW2=rnd(1, ch + cc + 1, 3, 3))


def check_d2_lean(ch, B, Hh, Ww, inplace, dd_quad, seed):
    """The level node's call (tmg_ops.py:1346 / 1368 / 1404): inputs (x1 = tin[..., :ch], D), G0 [.., ch], out = dtin[..., :ch],
    add0 (the output itself or a tensor of its own), w2 rows split2 = ch / gap2 = Cc, dd1 / dd2 = the layer's pair of the compact
    stash (dd_quad: the last layer's (dd1, dd2, 0, 0) slot)."""
    H = _H()
    cc = CC
    inp = d2_inputs(ch, cc, B, Hh, Ww, seed)
    p = d2_plan(B, Hh, Ww, ch + 4, ch, True, False)
    tin = torch.full((B, Hh, Ww, 2 * ch), NAN, device=DEV)
    tin[..., :ch] = inp["x1"].to(DEV)
    x1 = tin[..., :ch]
    D, GD = inp["D"].to(DEV), inp["GD"].to(DEV)
    G0 = inp["G0"][..., :ch].contiguous().to(DEV)
    dtin = torch.full((B, Hh, Ww, 2 * ch), NAN, device=DEV)
    dt1 = dtin[..., :ch]
    if inplace:
        dt1.copy_(inp["add0"])
        add0 = dt1
    else:
        add0 = inp["add0"].to(DEV)
    NLp = 4
    DD = torch.full((B, Hh, Ww, 2 * NLp), NAN, device=DEV)
    k = NLp - 2 if dd_quad else 1       # (the quad slot of the last real layer: channels 2k .. 2k + 3, 16-byte aligned)
    H.dense2_bwd([x1, D], inp["w1"].to(DEV), inp["w2"].to(DEV), None, None, GD, D, [G0], [dt1], ch, add0=add0, rows1=ch, rows2=ch + 1,
                 split2=ch, gap2=cc, dd1=DD[..., 2 * k:2 * k + 1], dd2=DD[..., 2 * k + 1:2 * k + 2], dd_quad=dd_quad)
    torch.cuda.synchronize()
    rd = _ref_dev(B * Hh * Ww)
    W2 = torch.cat([inp["w2"][:, :ch], inp["w2"][:, ch + cc:ch + cc + 1]], 1)
    gt, g1, g2, _, _ = d2_ref(inp["x1"], inp["D"], inp["G0"][..., :ch], inp["GD"], inp["w1"][:, :ch], W2, rd)
    errs = dict(out=_err(dt1, gt + inp["add0"].to(rd, torch.float64)) / TOL_D2, dd1=_err(DD[..., 2 * k:2 * k + 1], g1) / TOL_D2,
                dd2=_err(DD[..., 2 * k + 1:2 * k + 2], g2) / TOL_D2)
    print("dense2 lean ch=%d %dx%dx%d plan %s: err / tol %s" % (ch, B, Hh, Ww, p, {kk: "%.2e" % v for kk, v in errs.items()}))
    assert bool(torch.isnan(dtin[..., ch:]).all()), "wrote past the output view"
    if dd_quad:
        assert bool((DD[..., 2 * k + 2:2 * k + 4] == 0).all()), "the dd_quad slot's channels 2, 3 must be zero"
        assert bool(torch.isnan(DD[..., :2 * k]).all())
    else:
        assert bool(torch.isnan(DD[..., :2 * k]).all()) and bool(torch.isnan(DD[..., 2 * k + 2:]).all()), "wrote outside the dd pair"
    for kk, v in errs.items():
        assert v <= 1.0, "dense2 lean %s: err %.3e x tol" % (kk, v)
    return p


# (ch, B, H, W, add0 in place, dd_quad): NQ = 2 at ch 4, 8; 4 at ch 12, 16; TW_log2 3 / 4 / 5 at W <= 8 / <= 16 / > 16
D2_LEAN_CASES = [
    (4, 3, 9, 7, True, False),
    (8, 2, 20, 16, False, True),
    (8, 2, 6, 33, True, False),
    (12, 2, 1, 1, False, False),
    (12, 2, 17, 40, True, True),
    (16, 3, 13, 13, False, False),
    (16, 2, 40, 5, True, False),
    (4, 2, 24, 24, False, True),
]


@pytest.mark.parametrize("case", D2_LEAN_CASES)
def test_dense2_bwd_lean_matches_fp64(case):
    check_d2_lean(*case, seed=sum(case[:4]))


def test_dense2_bwd_lean_reaches_every_instantiation():
    seen = set()
    for ch, B, Hh, Ww, _, _ in D2_LEAN_CASES:
        p = d2_plan(B, Hh, Ww, ch + 4, ch, True, False)
        seen.add((p["NQ"], p["twl"]))
    assert seen == {(n, t) for n in (2, 4) for t in (3, 4, 5)}, sorted(seen)


def check_d2_general(ch, B, Hh, Ww, with_wg, seed, need_loop=False):
    """Inputs (x1, cond, D), two gradient / output segments (never the lean kernel), add0 on segment 0, dd1 / dd2 into a stash,
    dW1 / dW2 accumulated onto nonzero values (with_wg) or not requested."""
    H = _H()
    cc = CC
    inp = d2_inputs(ch, cc, B, Hh, Ww, seed)
    cin = ch + cc
    p = d2_plan(B, Hh, Ww, cin + 4, ch, False, with_wg)
    if need_loop:
        assert p["ntiles"] > p["grid"], p
    dv = {k: v.to(DEV) for k, v in inp.items()}
    o1 = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    o2 = torch.full((B, Hh, Ww, cc), NAN, device=DEV)
    g0 = [dv["G0"][..., :ch].contiguous(), dv["G0"][..., ch:].contiguous()]
    DD = torch.full((B, Hh, Ww, 4), NAN, device=DEV)
    dW1 = dv["dW1"].clone() if with_wg else None
    dW2 = dv["dW2"].clone() if with_wg else None
    H.dense2_bwd([dv["x1"], dv["cond"], dv["D"]], dv["w1"], dv["w2"], dW1, dW2, dv["GD"], dv["D"], g0, [o1, o2], cin, add0=dv["add0"],
                 rows1=cin, rows2=cin + 1, dd1=DD[..., 1:2], dd2=DD[..., 2:3])
    torch.cuda.synchronize()
    rd = _ref_dev(B * Hh * Ww)
    t0 = torch.cat([inp["x1"], inp["cond"]], 3)
    gt, g1, g2, gw1, gw2 = d2_ref(t0, inp["D"], inp["G0"], inp["GD"], inp["w1"], inp["w2"], rd)
    errs = dict(out0=_err(o1, gt[..., :ch] + inp["add0"].to(rd, torch.float64)), out1=_err(o2, gt[..., ch:]),
                dd1=_err(DD[..., 1:2], g1), dd2=_err(DD[..., 2:3], g2))
    if with_wg:
        errs.update(dW1=_err(dW1, gw1 + inp["dW1"].to(rd, torch.float64)), dW2=_err(dW2, gw2 + inp["dW2"].to(rd, torch.float64)))
    errs = {k: v / TOL_D2 for k, v in errs.items()}
    print("dense2 general ch=%d %dx%dx%d wg=%d plan %s: err / tol %s" % (ch, B, Hh, Ww, with_wg, p, {k: "%.2e" % v for k, v in errs.items()}))
    assert bool(torch.isnan(DD[..., 0]).all()) and bool(torch.isnan(DD[..., 3]).all()), "wrote outside the dd pair"
    for k, v in errs.items():
        assert v <= 1.0, "dense2 general %s: err %.3e x tol" % (k, v)


@pytest.mark.parametrize("ch,B,Hh,Ww,with_wg", [(8, 2, 9, 7, True), (16, 2, 20, 13, False), (4, 3, 1, 1, True), (12, 2, 17, 40, True)])
def test_dense2_bwd_general_matches_fp64(ch, B, Hh, Ww, with_wg):
    check_d2_general(ch, B, Hh, Ww, with_wg, seed=ch + B + Hh)


def test_dense2_bwd_general_blocks_loop_over_tiles():
    """dW1 / dW2 in the kernel (512 blocks / channel chunks): a batch of 128 x 128 images with about twice as many tiles as blocks."""
    ch = 8
    tpi = d2_plan(1, 128, 128, ch + CC + 4, ch, False, True)["ntiles"]
    B = 2 * _d2_blocks(True) // tpi + 1
    check_d2_general(ch, B, 128, 128, True, seed=5, need_loop=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# mix32 with the affine coupling (64- / 128-channel levels)
# ---------------------------------------------------------------------------------------------------------------------------------
def mix_inputs(C_, B, Hh, Ww, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=rnd(B, Hh, Ww, C_), hh=rnd(B, Hh, Ww, C_), W=torch.eye(C_) + rnd(C_, C_) * (0.3 / math.sqrt(C_)), bias=rnd(C_) * 0.1,
                ld0=rnd(B) * 5.0, dy=rnd(B, Hh, Ww, C_), g=rnd(B), kappa=torch.tensor([0.25]))


def mix_fwd_ref(inp, rd, x_delta=None):
    ch = inp["x"].shape[3] // 2
    x = _nchw(inp["x"], rd)
    if x_delta is not None:
        x = x + _nchw(x_delta, rd)
    hh = _nchw(inp["hh"], rd)
    y2, ld = O.affine_apply(hh, x[:, ch:], True)
    y = torch.einsum("oc,bchw->bohw", inp["W"].to(rd, torch.float64), torch.cat([x[:, :ch], y2], 1)) + inp["bias"].to(rd, torch.float64).view(1, -1, 1, 1)
    sg = 2.0 * F.softsign(hh[:, 1::2])
    return dict(y=_nhwc(y), r=_nhwc(hh[:, 1::2]), y2=_nhwc(y2), ld=ld, sgabs=sg.abs().sum((1, 2, 3)))


def check_mix_fwd(C_, B, Hh, Ww, seed, expect):
    H = _H()
    inp = mix_inputs(C_, B, Hh, Ww, seed)
    dv = {k: v.to(DEV) for k, v in inp.items()}
    ch = C_ // 2
    y = torch.full((B, Hh, Ww, C_), NAN, device=DEV)
    r = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    y2 = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    logdet = dv["ld0"].clone()
    ok = H.mix_affine_fwd(dv["x"], dv["hh"], dv["W"], dv["bias"], y, r, y2, logdet)
    torch.cuda.synchronize()
    assert ok == expect, (C_, Hh * Ww, ok)
    if not ok:
        assert bool(torch.isnan(y).all() and torch.isnan(r).all() and torch.isnan(y2).all()), "a declined launch wrote"
        assert torch.equal(logdet, dv["ld0"])
        return
    R = mix_fwd_ref(inp, _ref_dev(B * Hh * Ww))
    lde = _ld_err(logdet, inp["ld0"].double() + R["ld"].cpu(), inp["ld0"].abs().double() + R["sgabs"].cpu())
    errs = dict(y=_err(y, R["y"]) / TOL_OUT, r=_err(r, R["r"]) / TOL_R, y2=_err(y2, R["y2"]) / TOL_OUT, logdet=float(lde.max()) / TOL_LD)
    print("mix_affine_fwd C=%d %dx%dx%d: err / tol %s" % (C_, B, Hh, Ww, {k: "%.2e" % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v <= 1.0, "mix_affine_fwd %s: err %.3e x tol" % (k, v)


@pytest.mark.parametrize("C_,hw,accepted", [(64, (4, 8), True), (64, (6, 8), False), (128, (4, 4), True), (128, (4, 6), False),
                                           (64, (16, 16), True), (128, (8, 8), True)])
def test_mix_affine_fwd_envelope_edge(C_, hw, accepted):
    """ppi = pixels per image must be a multiple of the wave's pixel group: 32 at C = 64, 16 at C = 128."""
    check_mix_fwd(C_, 5, hw[0], hw[1], seed=C_ + hw[0] * hw[1], expect=accepted)


def mix_bwd_ref(inp, with_g, rd, M=None):
    ch = inp["x"].shape[3] // 2
    B = inp["x"].shape[0]
    x = _nchw(inp["x"], rd)
    x1m = x[:, :ch].clone().requires_grad_(True)
    x2 = x[:, ch:].clone().requires_grad_(True)
    hh = _nchw(inp["hh"], rd).clone().requires_grad_(True)
    y2, _ = O.affine_apply(hh, x2, True)
    y = torch.einsum("oc,bchw->bohw", inp["W"].to(rd, torch.float64), torch.cat([x1m, y2], 1))
    M = torch.ones(1, 1, 1, 1, dtype=torch.float64, device=rd) if M is None else M
    L = (_nchw(inp["dy"], rd) * M * y).sum()
    if with_g:
        L = L + (inp["g"].to(rd, torch.float64).view(B, 1, 1, 1) * M * 2.0 * F.softsign(hh[:, 1::2])).sum()
    d1, d2, dh = torch.autograd.grad(L, [x1m, x2, hh])
    return dict(dto1=_nhwc(d1), dtin2=_nhwc(d2), dhh=_nhwc(dh * _osc(inp["kappa"].to(rd, torch.float64))))


def check_mix_bwd(C_, B, Hh, Ww, with_g, seed):
    """The level node's call (tmg_ops.py:1386): t2 = tin[..., ch:], dtin2 = dtin[..., ch:], dhh = the stash slice."""
    H = _H()
    inp = mix_inputs(C_, B, Hh, Ww, seed)
    dv = {k: v.to(DEV) for k, v in inp.items()}
    ch = C_ // 2
    r = dv["hh"][..., 1::2].contiguous()
    dto1 = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    dtin = torch.full((B, Hh, Ww, C_), NAN, device=DEV)
    DHb, dhh = _stash(B, Hh, Ww, C_)
    assert H.mix_affine_bwd(dv["dy"], dv["W"], r, dv["x"][..., ch:], dv["g"] if with_g else None, dv["kappa"], dto1, dtin[..., ch:], dhh)
    torch.cuda.synchronize()
    ref = mix_bwd_ref(inp, with_g, _ref_dev(B * Hh * Ww))
    errs = dict(dto1=_err(dto1, ref["dto1"]), dtin2=_err(dtin[..., ch:], ref["dtin2"]), dhh=_err(dhh, ref["dhh"]))
    errs = {k: v / TOL_BWD for k, v in errs.items()}
    print("mix_affine_bwd C=%d %dx%dx%d g=%d: err / tol %s" % (C_, B, Hh, Ww, with_g, {k: "%.2e" % v for k, v in errs.items()}))
    assert bool(torch.isnan(dtin[..., :ch]).all()) and _stash_intact(DHb, C_), "wrote outside a view"
    for k, v in errs.items():
        assert v <= 1.0, "mix_affine_bwd %s: err %.3e x tol" % (k, v)


@pytest.mark.parametrize("C_,B,hw,with_g", [(64, 7, (3, 5), True), (128, 5, (3, 11), True), (64, 3, (1, 33), False), (128, 4, (16, 16), True)],
                         ids=["m64g15", "m128g33", "m64g0", "m128big"])
def test_mix_affine_bwd_per_pixel_image_index(C_, B, hw, with_g):
    """ppi 15 / 33 are not multiples of a 16-pixel group: groups straddle images and g is read per pixel (g[px / ppi])."""
    check_mix_bwd(C_, B, hw[0], hw[1], with_g, seed=C_ + B)


# ---------------------------------------------------------------------------------------------------------------------------------
# declined shapes write nothing
# ---------------------------------------------------------------------------------------------------------------------------------
def _odd_view(base_shape, kind):
    """A [.., C] view whose pixel stride is not a multiple of 4 ("stride") or whose data pointer is 4 bytes off alignment ("align")."""
    B, Hh, Ww, C_ = base_shape
    if kind == "stride":
        return torch.randn(B, Hh, Ww, C_ + 2, device=DEV)[..., :C_]
    return torch.randn(B, Hh, Ww, C_ + 4, device=DEV)[..., 1:1 + C_]


DECLINED = [("C12", 12, None), ("C40", 40, None), ("C20", 20, None), ("stride", 16, "stride"), ("align", 16, "align")]


@pytest.mark.parametrize("case", DECLINED, ids=[c[0] for c in DECLINED])
def test_declined_shapes_write_nothing(case):
    """Outside the envelope every entry point returns -100 (the bindings: False) and writes nothing: the NaN-poisoned outputs stay
    NaN and the log-det is unchanged."""
    H = _H()
    _, C_, odd = case
    B, Hh, Ww = 2, 9, 11
    ch = C_ // 2
    inp = cpl_inputs(C_, B, Hh, Ww, 3)
    dv = _to_dev(inp)
    shp = (B, Hh, Ww, C_)
    x = _odd_view(shp, odd) if odd else dv["x"]
    dout = _odd_view(shp, odd) if odd else dv["dout"]
    r_any = torch.full((B, Hh, Ww, ch), 0.5, device=DEV)

    def fresh():
        return dict(out=torch.full(shp, NAN, device=DEV), r=torch.full((B, Hh, Ww, ch), NAN, device=DEV),
                    y2=torch.full((B, Hh, Ww, ch), NAN, device=DEV), G0=torch.full((B, Hh, Ww, ch), NAN, device=DEV),
                    GD=torch.full((B, Hh, Ww, 4), NAN, device=DEV), dtin=torch.full(shp, NAN, device=DEV), ld=dv["ld0"].clone(),
                    DH=_stash(B, Hh, Ww, C_))

    def nothing_written(o):
        torch.cuda.synchronize()
        for k in ("out", "r", "y2", "G0", "GD", "dtin"):
            assert bool(torch.isnan(o[k]).all()), "%s: %s written by a declined launch" % (case[0], k)
        assert bool(torch.isnan(o["DH"][0]).all()), "%s: DH written" % case[0]
        assert torch.equal(o["ld"], dv["ld0"]), "%s: logdet changed" % case[0]

    for via in ("bind", "ctypes"):
        for mix in (True, False):
            o = fresh()
            assert not launch_cpl_fwd(dv, x, o["out"], o["r"], o["y2"], o["ld"], True, mix, via)
            nothing_written(o)
        o = fresh()
        assert not launch_cpl_bwd(dv, dout, x if via == "ctypes" else x[..., ch:], r_any, dv["g"], o["DH"][1], o["dtin"], o["G0"],
                                  o["GD"], False, via)
        nothing_written(o)
    o = fresh()
    assert not launch_cpl_bwd(dv, dout, x[..., ch:], r_any, dv["g"], o["DH"][1], o["dtin"], o["G0"], o["GD"], True, "bind")
    nothing_written(o)
    # the mix kernels: C outside {64, 128}, or C = 64 with the odd view
    Cm = 64 if odd else C_
    mi = {k: v.to(DEV) for k, v in mix_inputs(Cm, B, 4, 8, 4).items()}
    xm = _odd_view((B, 4, 8, Cm), odd) if odd else mi["x"]
    dym = _odd_view((B, 4, 8, Cm), odd) if odd else mi["dy"]
    chm = Cm // 2
    y, r, y2 = (torch.full((B, 4, 8, c), NAN, device=DEV) for c in (Cm, chm, chm))
    ld = mi["ld0"].clone()
    assert not H.mix_affine_fwd(xm, mi["hh"], mi["W"], mi["bias"], y, r, y2, ld)
    dto1 = torch.full((B, 4, 8, chm), NAN, device=DEV)
    dtin = torch.full((B, 4, 8, Cm), NAN, device=DEV)
    dhh = torch.full((B, 4, 8, Cm), NAN, device=DEV)
    assert not H.mix_affine_bwd(dym, mi["W"], mi["hh"][..., 1::2].contiguous(), mi["x"][..., chm:], mi["g"], mi["kappa"], dto1,
                                dtin[..., chm:], dhh)
    torch.cuda.synchronize()
    for t in (y, r, y2, dto1, dtin, dhh):
        assert bool(torch.isnan(t).all()), "%s: a declined mix launch wrote" % case[0]
    assert torch.equal(ld, mi["ld0"])


# ---------------------------------------------------------------------------------------------------------------------------------
# every test can fail: a wrong tile moves the error measure far past the bound (reference only)
# ---------------------------------------------------------------------------------------------------------------------------------
SENS_HW = (40, 37)      # 3 x 3 tiles per image, the last one ragged
SENS_B = 3


@pytest.mark.parametrize("C_,dens", [(8, False), (16, True), (32, False)])
def test_cpl_bwd_detects_a_wrong_tile(C_, dens):
    inp = cpl_inputs(C_, SENS_B, SENS_HW[0], SENS_HW[1], 7)
    base, _ = cpl_bwd_ref(inp, dens, True, "cpu")
    for where in ("last", "mid"):
        M, _ = _tile_mask(SENS_B, SENS_HW[0], SENS_HW[1], where, "cpu")
        moved, _ = cpl_bwd_ref(inp, dens, True, "cpu", M=M)
        for k in base:
            e = _err(moved[k], base[k]) / TOL_BWD
            assert e >= 10.0, "cpl_bwd C=%d %s tile: %s moves only %.2e x tol" % (C_, where, k, e)


@pytest.mark.parametrize("C_,reverse", [(8, 1), (24, 0)])
def test_cpl_fwd_detects_a_wrong_tile(C_, reverse):
    inp = cpl_inputs(C_, SENS_B, SENS_HW[0], SENS_HW[1], 8)
    with torch.no_grad():
        base = cpl_ref(inp, reverse, True, "cpu")
        for where in ("last", "mid"):
            M, b = _tile_mask(SENS_B, SENS_HW[0], SENS_HW[1], where, "cpu")
            delta = 1.5 * (1.0 - _nhwc(M).float()) * torch.ones(1, 1, 1, C_)
            moved = cpl_ref(inp, reverse, True, "cpu", x_delta=delta)
            assert _err(_nhwc(moved["out"]), _nhwc(base["out"])) / TOL_OUT >= 10.0
            assert _err(_nhwc(moved["y2"]), _nhwc(base["y2"])) / TOL_OUT >= 10.0
            assert _err(_nhwc(moved["hh"][:, 1::2]), _nhwc(base["hh"][:, 1::2])) / TOL_R >= 10.0
            scale = inp["ld0"].abs().double() + base["sg"].abs().sum((1, 2, 3))
            assert float(_ld_err(moved["ld"], base["ld"], scale)[b]) / TOL_LD >= 10.0, where


def test_dense2_bwd_detects_a_wrong_tile():
    ch, B, Hh, Ww = 8, SENS_B, SENS_HW[0], SENS_HW[1]
    inp = d2_inputs(ch, CC, B, Hh, Ww, 9)
    t0 = torch.cat([inp["x1"], inp["cond"]], 3)
    base = d2_ref(t0, inp["D"], inp["G0"], inp["GD"], inp["w1"], inp["w2"], "cpu")
    for where in ("last", "mid"):
        M, _ = _tile_mask(B, Hh, Ww, where, "cpu")
        moved = d2_ref(t0, inp["D"], inp["G0"], inp["GD"], inp["w1"], inp["w2"], "cpu", M=M)
        for name, a, b in zip(("dx", "dd1", "dd2", "dW1", "dW2"), moved, base):
            assert _err(a, b) / TOL_D2 >= 10.0, (where, name)


def test_mix_affine_detects_a_wrong_tile():
    C_, B, Hh, Ww = 64, SENS_B, 20, 24
    inp = mix_inputs(C_, B, Hh, Ww, 10)
    base = mix_bwd_ref(inp, True, "cpu")
    with torch.no_grad():
        fb = mix_fwd_ref(inp, "cpu")
    for where in ("last", "mid"):
        M, b = _tile_mask(B, Hh, Ww, where, "cpu")
        moved = mix_bwd_ref(inp, True, "cpu", M=M)
        for k in base:
            assert _err(moved[k], base[k]) / TOL_BWD >= 10.0, (where, k)
        with torch.no_grad():
            fm = mix_fwd_ref(inp, "cpu", x_delta=1.5 * (1.0 - _nhwc(M).float()) * torch.ones(1, 1, 1, C_))
        for k, tol in (("y", TOL_OUT), ("y2", TOL_OUT)):
            assert _err(fm[k], fb[k]) / tol >= 10.0, (where, k)
        # (the mix forward reads r from hh: a wrong tile of x moves y / y2 only, and the log-det of a wrong tile of hh)
        hh2 = dict(inp, hh=inp["hh"] + 1.5 * (1.0 - _nhwc(M).float()))
        with torch.no_grad():
            fh = mix_fwd_ref(hh2, "cpu")
        assert float(_ld_err(fh["ld"], fb["ld"], inp["ld0"].abs().double() + fb["sgabs"])[b]) / TOL_LD >= 10.0, where


# ---------------------------------------------------------------------------------------------------------------------------------
# launch-plan invariance: TMG_CPL_GRID / TMG_D2_BLOCKS are read once per process, so a fresh child process runs these
# ---------------------------------------------------------------------------------------------------------------------------------
def run_forced_plan_cases():
    """Run in the child with TMG_CPL_GRID=5 TMG_D2_BLOCKS=3: 5-block coupling grids (long tile runs, image changes inside a block),
    3 dense2 blocks (grid-stride loops over all tiles)."""
    assert os.environ.get("TMG_CPL_GRID") == "5" and os.environ.get("TMG_D2_BLOCKS") == "3"
    tpi = _tiles16(20, 40)
    for C_, B in ((8, 3), (32, 4)):
        for kind in ("fwd", "bwd"):
            p = cpl_plan(B * tpi, tpi, _cpl_gcap(C_, kind))
            assert p["per"] >= 3 and p["cross"] and p["grid"] <= 5, p
    check_cpl_fwd(8, 1, 3, 20, 40, "slice", True, True, seed=31)
    check_cpl_fwd(32, 0, 4, 20, 40, "halves", False, True, seed=32)
    check_cpl_bwd(8, False, 3, 20, 40, "inter", True, seed=33)
    check_cpl_bwd(32, False, 4, 20, 40, "halves", True, seed=34)
    check_cpl_bwd(16, True, 3, 20, 40, "slice", True, seed=35)
    assert d2_plan(3, 20, 40, 16 + 4, 16, True, False)["grid"] <= 3
    check_d2_lean(16, 3, 20, 40, True, False, seed=36)
    check_d2_lean(4, 4, 17, 7, False, True, seed=37)
    check_d2_general(8, 3, 20, 40, True, seed=38, need_loop=True)


def test_launch_plans_in_a_fresh_process():
    env = dict(os.environ, TMG_CPL_GRID="5", TMG_D2_BLOCKS="3")
    worker = os.path.join(C.ROOT, "tests", "coupling_plan_worker.py")
    r = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "forced launch plans: ok" in r.stdout
