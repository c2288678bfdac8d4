"""The bandwidth-bound kernels of tmg_pointwise.hip / tmg_glue.hip, each against a plain fp64 torch restatement of the SAME operation,
on every kernel their launchers can dispatch to and at every cap / loop condition of their launch plans.  The tmg_hip wrappers are
called directly (no autograd node in between).

Case map (the plan of every case is computed in the test from the launcher's formula and asserted):
  tmg_affine_apply / _pass -> affine_apply_kernel, three read paths (AFF_FWD; expect = vec4 | pair | single):
    vec4 (Ch % 4 == 0, strides % 4 == 0, 16-byte pointers): f4 f8 f20 (c4n = 5) f20d cap4; x2 / y2 = second half of a [B,H,W,2Ch]
      buffer, hh = channels 4.. of a buffer with pixel stride 2Ch + 8.  pair (scalar loop, hh read as float2): s1 s3 s6 s6d caps, and
      the Ch % 4 == 0 shapes pushed off the float4 path by a view: off2 (hh at a 2-channel offset), xstr (x2 / y2 pixel stride
      Ch + 2).  single (scalar loop, hh read float by float: pointer or stride odd): hodd8 hodd6 (odd channel offset), hstr4 hstr3
      (odd pixel stride).  Grid cap gx = 64 with every thread looping: cap4 (float4, 64 x 64, Ch = 68) caps (scalar, Ch = 17).
      reverse 0 / 1, x1 -> y1 pass-through and rsave given / None, B in {1, 3}, 7 x 9 and 33 x 31 pixels: spread over the cases.
  tmg_affine_bwd_scaled -> affine_bwd_kernel (AFF_BWD): dhh written as float2 (dense, slice) or float by float (dodd: odd offset,
      dstr: odd stride); g None / given; kappa None / inside / below / above the clamp; loop: B = 2, 128 x 128, Ch = 36
      (npix Ch > 4096 * 256, the grid_for cap).
  tmg_lstm_pointwise_fwd / _bwd -> fwd4 / bwd4 (R in {4, 8, 32}; c_prev None, dense, offset-4 view) and the scalar kernels
      (R in {1, 6}; R = 8 with an offset-2 c_prev view); dh / dc_in / dc_prev None and given; loop cases above 4096 * 256 quads
      (R = 4) and elements (R = 1).  test_lstm_vec_equals_scalar: same values through both kernels, bit-identical.
  tmg_gauss_fwd -> gauss_fwd_kernel: blocks per image min(ceil(per / 256), clamp(ceil(2048 / B), 4, 256)): cap 256 and threads
      looping (B = 1, 512 x 512, Ch = 5), cap 4 with one block per image (B = 704, 2 x 2, Ch = 3), cap 21 with a ragged last block
      (B = 100, 25 x 25, Ch = 8); tmg_gauss_bwd -> gauss_bwd_kernel: grid_for loop on the first of these.  Modes 0 / 1, clip_mean
      0 / 1, Ch in {1, 5, 8}, all operands slice views, zout None (mode 0), dzin / dzout / g None and given, logp non-zero on entry.
  tmg_chan_reduce (modes 0, 1), tmg_chan_moments, tmg_bn_finalize, tmg_bn_finalize64, tmg_bn_bwd_apply (BN_CASES): C = 1 (256 lanes),
      3 (85 lanes, one idle thread), 12 (21 lanes), 100 (2 lanes, 56 idle threads), 129 (one lane), 256 (one lane, the 1024-block
      cap: 193 x 191 pixels; bn_bwd_apply loops there: npix C > 4096 * 256); every case runs more than one block and the valid
      pixels of the last four-pixel iteration are 1 (C = 1, 3, 100, 129), 2 (C = 3, 100) and 3 (C = 12, 256).  C = 257: refused
      (-2, the wrapper raises).  n = 1: the max(n - 1, 1) branch.  Cancellation: means 1e3, unit spread, 320 x 320 pixels.
  tmg_masked_add -> masked_add4_kernel (n in {4, 8}; loop above 4096 * 256 quads) and masked_add_kernel (n in {3, 6}; n = 8 at a
      2-channel offset; loop above 4096 * 256 elements): every None / given combination of src, ref, add and accumulate.
  tmg_dkappa: one block (nw = 100, 2048), two (2049), the 64-block cap with threads looping (150 000); tmg_vec_sum (one block of
      256 threads): 1, 255, 256 values, and 257, 1000 where they loop; tmg_spread2 (glue_grid, one quad per thread): even and odd
      grids, C4 in {1, 3}, dense and slice dy, 1 to 4 blocks, the 4096-block cap with threads looping (1026 x 2048 grid), C = 6 declined.
  tmg_checker -> checker4_kernel (C = 8 dense and as an offset-4 view; loop) and checker_kernel (offset-2 view, C = 3, loop).
  Sensitivity (test_*_detects_*): the fp64 reference with one unit of work altered - the last quad of the last image, the last
      pixel of a middle image, one lane's pixels of one channel - moves the measure to >= 10x its bound.

Error measure (elementwise; the global max|err| / max|ref| forgives any error on a small element):
  share(a, ref, s, tol) = max_e |a_e - ref_e| / (tol (|ref_e| + s_e) + 2^-126),  NaN = infinite;  a check passes when share <= 1.
s_e is the magnitude of the element's own terms (sum of |terms| for a reduction).  Two departures from the plain measure
|a - ref| <= tol (|ref| + s), both stated here because they are the test's own: (1) the denominator carries a floor of 2^-126, the
smallest normal fp32 number: gates of -90 give sigmoids of 1e-39, below it, which fp32 holds as 0, an error of the number format
and not of the kernel (the LSTM checks scale the floor by the sigmoid's cofactor; everywhere else it only keeps 0 / 0 from being
NaN); (2) the fp64 references are plain torch formulas on the CPU, except in the cases of more than REF_CPU_MAX elements (the loop
and cap cases), where the same fp64 formulas run through torch on the device to keep the test to a few seconds: still no code of
the library.  u = 2^-24.  Bounds count the roundings of the kernel's formula; the error of a device transcendental is not derived
here: the same fp32 formula was evaluated by CPU torch against fp64 on 2e6 points (expf 1.04 u,
tanhf 1.06 u, 1 / (1 + expf(-x)) 2.5 u, rsqrt 1.5 u, relative) and FOUR times that is allowed, device libm may differ by a couple of
ulp: EXP = 4.2 u, TANH = 4.3 u, SIG = 10 u, RSQ = 6 u.  A K-term fp32 sum (per-thread partial sums, one atomic per block) is allowed
sqrt(K) u of the sum of the |terms|.
  TOL_AFF  = 10.2 u: sg = 2 r / (1 + |r|) carries 2 roundings, |sg| <= 2, so e^{sg} 4 u; + EXP + the add and the multiply.
  TOL_AFFB = 20.4 u: dr = osc dsg / den^2: e^{-sg} (4 u + EXP), 3 roundings in dsg, 3 in den^2, the divide, osc (EXP + 1).
  TOL_LD(K) = (2 + sqrt K) u of |ld0| + sum |sg|.
  TOL_LSTM_F = 17.3 u: c = gf cp + gi gg (SIG + TANH + 3 roundings), h = go tanh(c) measured against |go| (|tanh c| + |c| + s_c) with
    SIG + TANH + 1 more: TOL_LSTM_H = 32.6 u.  TOL_LSTM_B = 51.9 u: up to three sigmoids and three tanh in one product
    (3 SIG + 3 TANH) + 9 roundings; s carries the terms of 1 - gi, 1 - tc^2 (which cancel for saturated gates) at their full size.
  TOL_GAUSS = 7.2 u (e, z: EXP + 3), TOL_GAUSS_B = 14.4 u (2 EXP + 6), TOL_LP(K) = (2 TOL_GAUSS + 4 u) + sqrt(K) u of |lp0| + the
    sum of 0.5 (ln 2 pi + 2 |lsd| + E^2), E the |terms| of e.
  TOL_RED(K) = (8 + sqrt K) u of the sum of |terms| (mode 0: |x| + |off|, squared for s1; mode 1: |du|, |du| (|x| + |mean|) rstd).
  fp64 moments: (2 + sqrt K) 2^-53 of sum |x|, sum x^2.  bn_finalize64: mean 2 u, var 2 u RELATIVE TO THE VARIANCE ITSELF (0.5 u
    rounding + the fp64 sums' sqrt(K) 2^-53 (m^2 + v) / v <= 0.6 u at K = 1e5, m = 1e3, v = 1), rstd 8 u (+ eps, RSQ), a 9 u,
    bsh 12 u of |beta| + |mean a|.  The fp32 two-pass path gets TOL_RED(K) of its sums' |terms| (documented bound), not this one.
  running statistics: 9 u (+ the statistic's own bound) of the two terms.  bn_bwd_apply: (12 + sqrt K) u of
    gamma rstd (|g| + sum|du| / n + (|x| + |mean|) rstd sum|du xhat| / n).
  dkappa, vec_sum: (1 + sqrt K) u of the sum of |terms|.  masked_add, spread2, checker, rsave, y1: exact.
Observed on an MI355X (largest share of each bound, from the SHARE lines of a run of the whole GPU suite, every test of this file
passing; LAB_NOTES.md, "The bandwidth-bound kernels against fp64 on every dispatch path"): affine y2 0.2278, logdet 0.0357,
affine_bwd gin 0.1971, dhh 0.2669; lstm c_next 0.1335, h_next 0.0673, gate gradients 0.0564, dc_prev 0.0576; gauss zout 0.1990,
logp 0.0545, dzout 0.1973, dhz 0.2161; chan_reduce sum 0.0438, sum sq 0.0592, centred sum 0.0246, centred sq 0.0495, bn-relu sum du
0.0285, sum du xhat 0.0314; chan_moments sum 0.0000, sum sq 0.2357; bn_finalize mean 0.0395, var 0.0531, rstd 0.0395, a 0.0425, bsh
0.0227, running_mean 0.0280, running_var 0.0189; bn_finalize64 mean 0.4808, var 0.4959, rstd 0.1972, a 0.2240, bsh 0.1292,
running_mean 0.1062, running_var 0.0812, under cancellation mean 0.2001, var 0.4840, rstd 0.1246 (the fp32 two-pass variance there:
0.0000 of its own bound, 0.6636 of the 2 u bound it is not held to); n = 1: rstd 0.1149, running_mean 0.0790, running_var 0.0526;
bn_bwd_apply dx 0.0562 / 0.0510 (accumulate 0 / 1); dkappa 0.0139, vec_sum 0.0139.  The whole file has run on a device since the
first version of this text (which ended at test_lstm_vec_equals_scalar): that test and everything after it pass."""
import math

import pytest
import torch
import torch.nn.functional as F

import common as C  # noqa: F401  (sets sys.path)
from oracle import tmglow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
U = 2.0 ** -24
TINY = 2.0 ** -126
EXP, TANH, SIG, RSQ = 4.2 * U, 4.3 * U, 10 * U, 6 * U      # 4x the CPU fp32 error of the same formula (docstring)
TOL_AFF = 6 * U + EXP
TOL_AFFB = 12 * U + 2 * EXP
TOL_LSTM_F, TOL_LSTM_H, TOL_LSTM_B = SIG + TANH + 3 * U, 2 * (SIG + TANH) + 4 * U, 3 * (SIG + TANH) + 9 * U
TOL_GAUSS, TOL_GAUSS_B = EXP + 3 * U, 2 * EXP + 6 * U
LOG4 = math.log(4.0)
LOG2PI = math.log(2 * math.pi)
SPLIT_LIMITS = (-2.0, math.log(5.0), -2.0, math.log(5.0))
TOP_LIMITS = (0.0, 0.0, -10.0, math.log(5.0))
REF_CPU_MAX = 400000        # fp64 references of larger cases run on the device
SHARES = {}


def tol_sum(K, base=1.0):
    return (base + math.sqrt(K)) * U


def _H():
    import tmg_hip as H
    return H


@pytest.fixture(scope="module", autouse=True)
def _report_shares():
    yield
    for k in sorted(SHARES):
        print("SHARE %-28s %.4f" % (k, SHARES[k]))


def share(a, ref, s, tol, what=None, floor=TINY):
    """max |a - ref| / (tol (|ref| + s) + floor); NaN counts as infinite."""
    ref = ref.detach().double()
    a = a.detach().double().to(ref.device)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    if a.numel() == 0:
        return 0.0
    s = torch.as_tensor(s, dtype=torch.float64, device=ref.device)
    q = (a - ref).abs() / (tol * (ref.abs() + s) + floor)
    v = math.inf if bool(torch.isnan(q).any()) else float(q.max())
    if what is not None:
        SHARES[what] = max(SHARES.get(what, 0.0), v)
    return v


def check(a, ref, s, tol, what, case="", floor=TINY):
    v = share(a, ref, s, tol, what, floor)
    assert v <= 1.0, "%s %s: %.3g of its bound (tol %.2e)" % (what, case, v, tol)


def grid_for(n, cap=4096):
    return min(cap, max(1, -(-n // 256)))


def _rd(numel):
    return "cpu" if numel <= REF_CPU_MAX else DEV


def view(B, Hh, Ww, Cn, off=0, extra=0, init=None):
    """Channels off .. off + Cn of a NaN [B,H,W,off + Cn + extra] buffer: (buffer, view).  The buffer outside the view must stay NaN."""
    base = torch.full((B, Hh, Ww, off + Cn + extra), NAN, device=DEV)
    v = base[..., off:off + Cn]
    if init is not None:
        v.copy_(init.to(DEV))
    return base, v


def intact(base, off, Cn):
    return bool(torch.isnan(base[..., :off]).all()) and bool(torch.isnan(base[..., off + Cn:]).all())


def misaligned(t):
    """A contiguous copy of t whose data pointer is 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _stride(t):
    return _H().seg(t)[1]


def _al(ts, m):
    return all(t is None or t.data_ptr() % m == 0 for t in ts)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. affine forward
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, B, H, W, Ch, reverse, pass-through, rsave, x layout, hh (offset, extra), expected path, gx capped)
AFF_FWD = [
    ("f4", 1, 7, 9, 4, 0, True, True, "half", (4, 4), "vec4", False),
    ("f8", 3, 7, 9, 8, 1, False, True, "half", (4, 4), "vec4", False),
    ("f20", 3, 33, 31, 20, 0, True, False, "half", (4, 4), "vec4", False),
    ("f20d", 1, 7, 9, 20, 1, True, True, "dense", (0, 0), "vec4", False),
    ("s1", 3, 7, 9, 1, 0, False, True, "dense", (0, 0), "pair", False),
    ("s3", 1, 33, 31, 3, 1, True, True, "half", (4, 4), "pair", False),
    ("s6", 3, 7, 9, 6, 0, True, False, "half", (4, 4), "pair", False),
    ("s6d", 3, 7, 9, 6, 1, False, True, "dense", (0, 0), "pair", False),
    ("off2", 3, 7, 9, 8, 0, True, True, "half", (2, 2), "pair", False),
    ("xstr", 3, 7, 9, 8, 1, True, True, "stride2", (0, 0), "pair", False),
    ("hodd8", 3, 7, 9, 8, 0, True, True, "half", (1, 3), "single", False),
    ("hodd6", 1, 33, 31, 6, 1, False, True, "half", (3, 1), "single", False),
    ("hstr4", 3, 7, 9, 4, 1, False, True, "dense", (0, 3), "single", False),
    ("hstr3", 3, 7, 9, 3, 0, True, False, "half", (0, 1), "single", False),
    ("cap4", 1, 64, 64, 68, 0, True, True, "half", (4, 4), "vec4", True),
    ("caps", 1, 64, 64, 17, 1, False, True, "dense", (0, 0), "pair", True),
]


def aff_fwd_plan(hh, x2, y2, rsave, x1, y1, Ch, ppi):
    """tmg_affine_apply_pass: (read path, gx, work items per image)."""
    vec = Ch % 4 == 0 and all(_stride(t) % 4 == 0 for t in (hh, x2, y2)) and _al((hh, x2, y2, rsave), 16)
    if x1 is not None and (_stride(x1) % 4 or _stride(y1) % 4 or not _al((x1, y1), 16)):
        vec = False
    pair = _stride(hh) % 2 == 0 and _al((hh,), 8)
    per = ppi * (Ch // 4 if vec else Ch)
    return ("vec4" if vec else "pair" if pair else "single"), min(64, max(1, -(-per // 1024))), per


def _xy_layout(B, Hh, Ww, Ch, lay, x_init, pas):
    """x1, x2 (inputs) and y1, y2 (NaN outputs) with the buffers and (offset, n) to check for stray writes."""
    if lay == "half":
        xb = x_init.to(DEV).contiguous()
        yb = torch.full((B, Hh, Ww, 2 * Ch), NAN, device=DEV)
        return xb[..., :Ch], xb[..., Ch:], yb[..., :Ch], yb[..., Ch:], [(yb, 0 if pas else Ch, 2 * Ch if pas else Ch)]
    if lay == "dense":
        x1, x2 = x_init[..., :Ch].contiguous().to(DEV), x_init[..., Ch:].contiguous().to(DEV)
        return x1, x2, torch.full_like(x1, NAN), torch.full_like(x2, NAN), []
    assert lay == "stride2"
    _, x1 = view(B, Hh, Ww, Ch, 0, 2, x_init[..., :Ch])
    _, x2 = view(B, Hh, Ww, Ch, 0, 2, x_init[..., Ch:])
    b1, y1 = view(B, Hh, Ww, Ch, 0, 2)
    b2, y2 = view(B, Hh, Ww, Ch, 0, 2)
    return x1, x2, y1, y2, [(b2, 0, Ch)] + ([(b1, 0, Ch)] if pas else [])


def aff_ref(hh, x2, reverse):
    """fp64: y2, its own-term scale, sg."""
    hh, x2 = hh.double(), x2.double()
    sh, r = hh[..., 0::2], hh[..., 1::2]
    sg = 2 * r / (1 + r.abs())
    if reverse:
        return x2 * torch.exp(-sg) - sh, x2.abs() * torch.exp(-sg) + sh.abs(), sg
    return (x2 + sh) * torch.exp(sg), (x2.abs() + sh.abs()) * torch.exp(sg), sg


def _aff_fwd_run(case):
    name, B, Hh, Ww, Ch, rev, pas, rs, xlay, (hoff, hextra), expect, capped = case
    H = _H()
    g = _gen(100 + Ch + Hh + rev)
    hh0 = 1.5 * torch.randn(B, Hh, Ww, 2 * Ch, generator=g)
    x0 = torch.randn(B, Hh, Ww, 2 * Ch, generator=g)
    ld0 = torch.randn(B, generator=g) * 3 + 1.0
    hb, hh = view(B, Hh, Ww, 2 * Ch, hoff, hextra, hh0)
    x1, x2, y1, y2, guards = _xy_layout(B, Hh, Ww, Ch, xlay, x0, pas)
    rsave = torch.full((B, Hh, Ww, Ch), NAN, device=DEV) if rs else None
    ld = ld0.to(DEV)
    path, gx, per = aff_fwd_plan(hh, x2, y2, rsave, x1 if pas else None, y1 if pas else None, Ch, Hh * Ww)
    assert path == expect, (name, path)
    assert (gx == 64 and per > 64 * 1024) if capped else (gx < 64), (name, gx, per)
    H.affine_apply(hh, x2, y2, rsave, ld, rev, x1=x1 if pas else None, y1=y1 if pas else None)
    torch.cuda.synchronize()
    return dict(hh0=hh0, x0=x0, ld0=ld0, y2=y2, y1=y1, x1=x1, rsave=rsave, ld=ld, guards=guards, hb=hb)


@pytest.mark.parametrize("case", AFF_FWD, ids=[c[0] for c in AFF_FWD])
def test_affine_forward(case):
    name, B, Hh, Ww, Ch, rev, pas, rs = case[:8]
    t = _aff_fwd_run(case)
    yr, s, sg = aff_ref(t["hh0"], t["x0"][..., Ch:], rev)
    check(t["y2"].cpu(), yr, s, TOL_AFF, "affine y2", name)
    K = Hh * Ww * Ch
    check(t["ld"].cpu(), t["ld0"].double() + sg.sum((1, 2, 3)), t["ld0"].double().abs() + sg.abs().sum((1, 2, 3)), tol_sum(K, 2), "affine logdet", name)
    if rs:
        assert torch.equal(t["rsave"].cpu(), t["hh0"][..., 1::2]), name
    if pas:
        assert torch.equal(t["y1"].cpu(), t["x0"][..., :Ch]), name
    else:
        assert bool(torch.isnan(t["y1"]).all()), name
    for base, off, n in t["guards"]:
        assert intact(base, off, n), name


def test_affine_forward_detects_a_wrong_quad():
    """The reference with the last quad of the last image (float4 path) / the last pixel of a middle image (scalar path) altered."""
    for case, where in ((AFF_FWD[1], "last quad"), (AFF_FWD[6], "mid pixel")):
        name, B, Hh, Ww, Ch, rev = case[:6]
        t = _aff_fwd_run(case)
        x2 = t["x0"][..., Ch:].clone()
        hh = t["hh0"].clone()
        b, c0 = (B - 1, Ch - 4) if where == "last quad" else (1, 0)
        x2[b, Hh - 1, Ww - 1, c0:] = 0
        sg_true = aff_ref(hh, x2, rev)[2][b, Hh - 1, Ww - 1, c0:].sum()
        hh[b, Hh - 1, Ww - 1, 2 * c0:] = -8.0 if float(sg_true) > 0 else 8.0       # the unit's log-det share with the other sign
        yr, s, sg = aff_ref(hh, x2, rev)
        assert share(t["y2"].cpu(), yr, s, TOL_AFF) >= 10, name
        K = Hh * Ww * Ch
        ldr, lds = t["ld0"].double() + sg.sum((1, 2, 3)), t["ld0"].double().abs() + sg.abs().sum((1, 2, 3))
        assert share(t["ld"].cpu()[b], ldr[b], lds[b], tol_sum(K, 2)) >= 10, name


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. affine backward
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, B, H, W, Ch, reverse, g, kappa, dhh (offset, extra), float2 stores, grid capped)
AFF_BWD = [
    ("b4", 1, 7, 9, 4, 0, True, None, (0, 0), True, False),
    ("b8", 3, 7, 9, 8, 1, False, 0.3, (4, 4), True, False),
    ("b20", 3, 33, 31, 20, 0, True, -5.0, (4, 4), True, False),
    ("b1", 3, 7, 9, 1, 1, True, 2.0, (0, 0), True, False),
    ("b3", 1, 33, 31, 3, 0, False, None, (4, 4), True, False),
    ("b6", 3, 7, 9, 6, 1, True, 0.3, (2, 2), True, False),
    ("dodd8", 3, 7, 9, 8, 1, True, 0.3, (1, 3), False, False),
    ("dodd6", 1, 33, 31, 6, 0, True, None, (3, 1), False, False),
    ("dstr4", 3, 7, 9, 4, 0, False, 2.0, (0, 3), False, False),
    ("dstr3", 3, 7, 9, 3, 1, True, -5.0, (0, 1), False, False),
    ("b68", 1, 64, 64, 68, 0, True, 0.3, (4, 4), True, False),
    ("loop", 2, 128, 128, 36, 1, True, 0.3, (0, 0), True, True),
]


def aff_bwd_ref(go, yv, r, g, kappa, reverse):
    """fp64 restatement: gin, dhh (interleaved) and the own-term scale of dhh."""
    go, yv, r = go.double(), yv.double(), r.double()
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # kappa and the clamp limits are fp32 values
    hsc = math.exp(min(max(f32(kappa), -4.0), f32(LOG4))) if kappa is not None else 1.0   # out_scale_of, stated independently
    den = 1 + r.abs()
    sg = 2 * r / den
    gb = g.double().view(-1, 1, 1, 1) if g is not None else torch.zeros(1, dtype=torch.float64, device=go.device)
    if reverse:
        inv = torch.exp(-sg)
        gi, da = go * inv, -go
        dsg, sd = -2 * go * yv * inv + 2 * gb, 2 * (go * yv).abs() * inv + 2 * gb.abs()
    else:
        gi = go * torch.exp(sg)
        da = gi
        dsg, sd = 2 * go * yv + 2 * gb, 2 * (go * yv).abs() + 2 * gb.abs()
    dhh = torch.stack((da * hsc, hsc * dsg / den ** 2), -1).flatten(-2)
    sdh = torch.stack((torch.zeros_like(sd), hsc * sd / den ** 2), -1).flatten(-2)
    return gi, dhh, sdh


def _aff_bwd_run(case):
    name, B, Hh, Ww, Ch, rev, has_g, kappa, (doff, dextra), pair, capped = case
    H = _H()
    g_ = _gen(200 + Ch + Hh + rev)
    dy0 = torch.randn(B, Hh, Ww, 2 * Ch, generator=g_)
    y0 = torch.randn(B, Hh, Ww, 2 * Ch, generator=g_)
    r0 = 1.5 * torch.randn(B, Hh, Ww, Ch, generator=g_)
    gv = torch.randn(B, generator=g_) if has_g else None
    dy, yb = dy0.to(DEV), y0.to(DEV)
    dx = torch.full((B, Hh, Ww, 2 * Ch), NAN, device=DEV)
    db, dhh = view(B, Hh, Ww, 2 * Ch, doff, dextra)
    kd = torch.tensor([kappa], device=DEV) if kappa is not None else None
    assert (_stride(dhh) % 2 == 0 and dhh.data_ptr() % 8 == 0) == pair, name
    assert (grid_for(B * Hh * Ww * Ch) == 4096 and B * Hh * Ww * Ch > 4096 * 256) == capped, name
    H.affine_bwd(dy[..., Ch:], yb[..., Ch:], r0.to(DEV), gv.to(DEV) if has_g else None, dx[..., Ch:], dhh, rev, kappa=kd)
    torch.cuda.synchronize()
    return dict(dy0=dy0, y0=y0, r0=r0, g=gv, dx=dx, dhh=dhh, db=db)


@pytest.mark.parametrize("case", AFF_BWD, ids=[c[0] for c in AFF_BWD])
def test_affine_backward(case):
    name, B, Hh, Ww, Ch, rev, has_g, kappa, (doff, dextra) = case[:9]
    t = _aff_bwd_run(case)
    rd = _rd(B * Hh * Ww * Ch)
    gi, dhh, sdh = aff_bwd_ref(t["dy0"][..., Ch:].to(rd), t["y0"][..., Ch:].to(rd), t["r0"].to(rd), t["g"].to(rd) if has_g else None, kappa, rev)
    check(t["dx"][..., Ch:].to(rd), gi, 0.0, TOL_AFFB, "affine_bwd gin", name)
    check(t["dhh"].to(rd), dhh, sdh, TOL_AFFB, "affine_bwd dhh", name)
    assert bool(torch.isnan(t["dx"][..., :Ch]).all()) and intact(t["db"], doff, 2 * Ch), name


def test_affine_backward_detects_a_wrong_pixel():
    for case in (AFF_BWD[1], AFF_BWD[6]):           # float2 stores / float-by-float stores
        name, B, Hh, Ww, Ch, rev, has_g, kappa = case[:8]
        t = _aff_bwd_run(case)
        dy = t["dy0"][..., Ch:].clone()
        dy[1, Hh - 1, Ww - 1, :] = 0                # the last pixel of the middle image
        gi, dhh, sdh = aff_bwd_ref(dy, t["y0"][..., Ch:], t["r0"], t["g"] if has_g else None, kappa, rev)
        assert share(t["dx"][..., Ch:].cpu(), gi, 0.0, TOL_AFFB) >= 10, name
        assert share(t["dhh"].cpu(), dhh, sdh, TOL_AFFB) >= 10, name


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ConvLSTM pointwise
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, (B, H, W), R, c_prev: None | dense | off4 | off2, dh, dc_in, dc_prev, float4 kernel, grid capped)
LSTM_CASES = [
    ("v4", (1, 7, 9), 4, "dense", True, True, True, True, False),
    ("v8n", (3, 7, 9), 8, None, True, False, True, True, False),
    ("v8o4", (3, 7, 9), 8, "off4", False, True, True, True, False),
    ("v32", (1, 5, 3), 32, "off4", True, True, False, True, False),
    ("s1", (3, 7, 9), 1, "dense", True, True, True, False, False),
    ("s6", (3, 7, 9), 6, "off2", True, False, False, False, False),
    ("s6n", (1, 5, 3), 6, None, False, True, True, False, False),
    ("s8o2", (3, 7, 9), 8, "off2", True, True, True, False, False),
    ("vloop", (1, 1025, 1024), 4, "dense", True, True, True, True, True),
    ("sloop", (1, 1025, 1024), 1, "dense", True, None, True, False, True),
]


def _lstm_data(shape, R, seed):
    B, Hh, Ww = shape
    g = _gen(seed)
    gates = 2 * torch.randn(B, Hh, Ww, 4 * R, generator=g)
    flat = gates.view(-1)
    for k, v in enumerate((30.0, -30.0, 90.0, -90.0)):      # saturating pre-activations, spread over the four gates
        flat[k + 1::23 + 4 * k] = v
    cp = torch.randn(B, Hh, Ww, R, generator=g)
    dh = torch.randn(B, Hh, Ww, R, generator=g)
    dc = torch.randn(B, Hh, Ww, R, generator=g)
    return gates, cp, dh, dc


def lstm_vec(R, npix, c_prev, others):
    return R % 4 == 0 and (c_prev is None or _stride(c_prev) % 4 == 0) and npix * (R // 4) < 2 ** 31 and _al([c_prev] + list(others), 16)


def lstm_fwd_ref(gates, cp):
    """fp64: c_next, h_next, their own-term scales, and their underflow floors: a sigmoid below 2^-126 (gate -90) is 0 in fp32, an
    ABSOLUTE error of up to 2^-126 that reaches the result times the sigmoid's cofactor."""
    a = gates.double()
    R = a.shape[-1] // 4
    gi, gf, go, gg = torch.sigmoid(a[..., :R]), torch.sigmoid(a[..., R:2 * R]), torch.sigmoid(a[..., 2 * R:3 * R]), torch.tanh(a[..., 3 * R:])
    cp = cp.double() if cp is not None else torch.zeros_like(gi)
    cn = gf * cp + gi * gg
    sc = (gf * cp).abs() + (gi * gg).abs()
    fc = TINY * (1 + cp.abs() + gg.abs())
    return cn, sc, go * torch.tanh(cn), go * (torch.tanh(cn).abs() + cn.abs() + sc), fc, fc + TINY


def lstm_bwd_ref(gates, cp, cnx, dh, dci):
    """fp64 of lstm_bwd1 with the scales of its differences at full size: (values, scales) for r0..r3 (as [.., 4R]) and dc_prev, and
    the underflow floors (TINY times the scale with every sigmoid replaced by 1, see lstm_fwd_ref)."""
    a = gates.double()
    R = a.shape[-1] // 4
    gi, gf, go, gg = torch.sigmoid(a[..., :R]), torch.sigmoid(a[..., R:2 * R]), torch.sigmoid(a[..., 2 * R:3 * R]), torch.tanh(a[..., 3 * R:])
    z = torch.zeros_like(gi)
    cp = cp.double() if cp is not None else z
    dhv = dh.double() if dh is not None else z
    dci = dci.double() if dci is not None else z
    tc = torch.tanh(cnx.double())
    dc = dci + dhv * go * (1 - tc * tc)
    sdc = dci.abs() + (dhv * go).abs() * (1 + tc * tc)
    val = torch.cat((dc * gg * gi * (1 - gi), dc * cp * gf * (1 - gf), dhv * tc * go * (1 - go), dc * gi * (1 - gg * gg)), -1)
    sc = torch.cat((sdc * (gg * gi).abs() * (1 + gi), sdc * (cp * gf).abs() * (1 + gf), (dhv * tc * go).abs() * (1 + go),
                    sdc * gi * (1 + gg * gg)), -1)
    sd1 = dci.abs() + dhv.abs() * (1 + tc * tc)
    fl = TINY * (1 + torch.cat((2 * sd1 * gg.abs(), 2 * sd1 * cp.abs(), 2 * (dhv * tc).abs(), sd1 * (1 + gg * gg)), -1))
    return val, sc, dc * gf, sdc * gf, fl, TINY * (1 + sd1)


def _lstm_cprev(kind, shape, R, cp0):
    if kind is None:
        return None, None
    off = {"dense": 0, "off4": 4, "off2": 2}[kind]
    return view(shape[0], shape[1], shape[2], R, off, off, cp0)


@pytest.mark.parametrize("case", LSTM_CASES, ids=[c[0] for c in LSTM_CASES])
def test_lstm_pointwise(case):
    name, shape, R, ckind, has_dh, has_dci, has_dcp, vec, capped = case
    H = _H()
    B, Hh, Ww = shape
    npix = B * Hh * Ww
    gates0, cp0, dh0, dc0 = _lstm_data(shape, R, 300 + R + Hh)
    rd = _rd(npix * 4 * R)
    gates = gates0.to(DEV)
    cb, cprev = _lstm_cprev(ckind, shape, R, cp0)
    cn = torch.full((B, Hh, Ww, R), NAN, device=DEV)
    hn = torch.full((B, Hh, Ww, R), NAN, device=DEV)
    assert lstm_vec(R, npix, cprev, (gates, cn, hn)) == vec, name
    work = npix * (R // 4 if vec else R)
    assert (grid_for(work) == 4096 and work > 4096 * 256) == capped, name
    H.lstm_pointwise_fwd(gates, cprev, cn, hn)
    torch.cuda.synchronize()
    assert torch.equal(gates.cpu(), gates0), "the forward leaves the pre-activations as they are"
    cpr = cp0.to(rd) if ckind is not None else None
    cr, sc, hr, sh, fc, fh = lstm_fwd_ref(gates0.to(rd), cpr)
    assert bool(torch.isfinite(cn).all()) and bool(torch.isfinite(hn).all()), name
    check(cn.to(rd), cr, sc, TOL_LSTM_F, "lstm c_next", name, fc)
    check(hn.to(rd), hr, sh, TOL_LSTM_H, "lstm h_next", name, fh)
    # backward on the kernel's own c_next (the reference takes the same fp32 values)
    dh = dh0.to(DEV) if has_dh else None
    dci = dc0.to(DEV) if has_dci else None
    dcp = torch.full((B, Hh, Ww, R), NAN, device=DEV) if has_dcp else None
    assert lstm_vec(R, npix, cprev, (gates, cn, dh, dci, dcp)) == vec, name
    H.lstm_pointwise_bwd(gates, cprev, cn, dh, dci, dcp)
    torch.cuda.synchronize()
    val, sv, dpr, sp, fv, fp = lstm_bwd_ref(gates0.to(rd), cpr, cn.to(rd), dh0.to(rd) if has_dh else None, dc0.to(rd) if has_dci else None)
    assert bool(torch.isfinite(gates).all()), name
    check(gates.to(rd), val, sv, TOL_LSTM_B, "lstm gate gradients", name, fv)
    if has_dcp:
        check(dcp.to(rd), dpr, sp, TOL_LSTM_B, "lstm dc_prev", name, fp)
    if cb is not None and ckind != "dense":
        off = {"off4": 4, "off2": 2}[ckind]
        assert torch.equal(cb[..., off:off + R].cpu(), cp0) and intact(cb, off, R), name


@pytest.mark.parametrize("R", [4, 8, 32])
def test_lstm_vec_equals_scalar(R):
    """fwd4 / bwd4 against the scalar kernels on the same values: bit-identical.  The scalar kernel is forced by one operand
    (h_next, c_next) placed 4 bytes past a 16-byte boundary, everything else as in the float4 call."""
    H = _H()
    shape = (3, 7, 9)
    npix = 3 * 7 * 9
    gates0, cp0, dh0, dc0 = _lstm_data(shape, R, 400 + R)
    outs = []
    for scalar in (False, True):
        gates, cp, dh, dci = gates0.to(DEV), cp0.to(DEV), dh0.to(DEV), dc0.to(DEV)
        cn = torch.full((3, 7, 9, R), NAN, device=DEV)
        hn = torch.full((3, 7, 9, R), NAN, device=DEV)
        if scalar:
            hn = misaligned(hn)
        assert lstm_vec(R, npix, cp, (gates, cn, hn)) == (not scalar)
        H.lstm_pointwise_fwd(gates, cp, cn, hn)
        cnb = misaligned(cn) if scalar else cn
        dcp = torch.full((3, 7, 9, R), NAN, device=DEV)
        assert lstm_vec(R, npix, cp, (gates, cnb, dh, dci, dcp)) == (not scalar)
        H.lstm_pointwise_bwd(gates, cp, cnb, dh, dci, dcp)
        torch.cuda.synchronize()
        outs.append((cn.cpu(), hn.cpu(), gates.cpu(), dcp.cpu()))
    for a, b, what in zip(outs[0], outs[1], ("c_next", "h_next", "gate gradients", "dc_prev")):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b), what


def test_lstm_detects_a_wrong_quad():
    case = LSTM_CASES[1]
    name, shape, R = case[:3]
    H = _H()
    B, Hh, Ww = shape
    gates0, cp0, dh0, dc0 = _lstm_data(shape, R, 300 + R + Hh)
    gates = gates0.to(DEV)
    cn = torch.full((B, Hh, Ww, R), NAN, device=DEV)
    hn = torch.full((B, Hh, Ww, R), NAN, device=DEV)
    H.lstm_pointwise_fwd(gates, None, cn, hn)
    dcp = torch.full((B, Hh, Ww, R), NAN, device=DEV)
    H.lstm_pointwise_bwd(gates, None, cn, dh0.to(DEV), None, dcp)
    torch.cuda.synchronize()
    alt = gates0.clone()
    alt[B - 1, Hh - 1, Ww - 1, 3 * R + R - 4:] += 0.5       # the g gate of the last quad of the last pixel
    alt[B - 1, Hh - 1, Ww - 1, 2 * R + R - 4:3 * R] -= 0.5  # and its o gate
    cr, sc, hr, sh = lstm_fwd_ref(alt, None)[:4]
    assert share(cn.cpu(), cr, sc, TOL_LSTM_F) >= 10 and share(hn.cpu(), hr, sh, TOL_LSTM_H) >= 10
    dha = dh0.clone()
    dha[B - 1, Hh - 1, Ww - 1, R - 4:] = 0
    val, sv, dpr, sp = lstm_bwd_ref(gates0, None, cn.cpu(), dha, None)[:4]
    assert share(gates.cpu(), val, sv, TOL_LSTM_B) >= 10 and share(dcp.cpu(), dpr, sp, TOL_LSTM_B) >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. diagonal Gaussian
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, B, H, W, Ch, mode, clip_mean, zout given, dzin, dzout, g, expected (cap, gx), bwd grid capped)
GAUSS_CASES = [
    ("m0c1", 3, 7, 9, 5, 0, 1, True, True, True, True, None, False),
    ("m0c0", 3, 7, 9, 8, 0, 0, False, False, True, True, None, False),
    ("m0ch1", 3, 7, 9, 1, 0, 1, True, False, False, False, None, False),
    ("m1c1", 3, 7, 9, 8, 1, 1, True, True, False, True, None, False),
    ("m1c0", 3, 7, 9, 5, 1, 0, True, True, False, False, None, False),
    ("m1ch1", 1, 7, 9, 1, 1, 1, True, False, False, True, None, False),
    ("cap256", 1, 512, 512, 5, 0, 1, True, True, True, True, (256, 256), True),
    ("cap4", 704, 2, 2, 3, 1, 1, True, True, False, True, (4, 1), False),
    ("ragged", 100, 25, 25, 8, 0, 1, True, False, True, True, (21, 20), False),
]


def gauss_plan(B, per):
    cap = min(256, max(4, -(-2048 // B)))
    return cap, max(1, min(cap, -(-per // 256)))


def _three_way(shape, lo, hi, g):
    """Values clearly below lo, clearly above hi and clearly inside (margin 0.1), a third each."""
    u = torch.rand(shape, generator=g)
    k = torch.randint(0, 3, shape, generator=g)
    inside = lo + 0.1 + u * (hi - lo - 0.2)
    return torch.where(k == 0, lo - 0.1 - 2 * u, torch.where(k == 1, hi + 0.1 + 2 * u, inside))


def _gauss_data(B, Hh, Ww, Ch, clip, seed):
    g = _gen(seed)
    lim = SPLIT_LIMITS if clip else TOP_LIMITS
    shape = (B, Hh, Ww, Ch)
    mraw = _three_way(shape, lim[0], lim[1], g) if clip else torch.randn(shape, generator=g)
    sraw = _three_way(shape, max(lim[2], -3.0) if not clip else lim[2], lim[3], g)
    if not clip:    # TOP_LIMITS: log-std clamp at -10; a few values clearly below it as well
        sraw.view(-1)[::7] = -10.1 - torch.rand(sraw.view(-1)[::7].shape, generator=g)
    hz = torch.cat((mraw, sraw), 3)
    return hz, torch.randn(shape, generator=g), torch.randn(shape, generator=g), torch.randn(B, generator=g), 2 * torch.randn(B, generator=g) + 1, lim


def gauss_ref(hz, v, dzin, g, mode, clip, lim):
    """fp64: forward value (eps or z), its scale, per-element log-prob terms and their scale, and the backward outputs with scales."""
    l32 = [float(torch.tensor(x, dtype=torch.float32)) for x in lim]      # the launcher receives the limits as floats
    hz, v = hz.double(), v.double()
    Ch = v.shape[-1]
    mraw, sraw = hz[..., :Ch], hz[..., Ch:]
    mean = mraw.clamp(l32[0], l32[1]) if clip else mraw
    mpass = ((mraw > l32[0]) & (mraw < l32[1])) if clip else torch.ones_like(mraw, dtype=torch.bool)
    lsd = sraw.clamp(l32[2], l32[3])
    spass = (sraw > l32[2]) & (sraw < l32[3])
    gb = g.double().view(-1, 1, 1, 1) if g is not None else torch.zeros(1, dtype=torch.float64, device=v.device)
    dzi = dzin.double() if dzin is not None else torch.zeros_like(v)
    if mode == 0:
        il = torch.exp(-lsd)
        e, E = (v - mean) * il, (v.abs() + mean.abs()) * il
        out, so = e, E
        term, sterm = -0.5 * (LOG2PI + 2 * lsd + e * e), 0.5 * (LOG2PI + 2 * lsd.abs() + E * E)
        dmean, sdm = gb * e * il, gb.abs() * E * il
        dlsd, sdl = gb * (e * e - 1), gb.abs() * (E * E + 1)
        dz, sdz = -gb * e * il + dzi, gb.abs() * E * il + dzi.abs()
    else:
        out, so = mean + torch.exp(lsd) * v, mean.abs() + torch.exp(lsd) * v.abs()
        term, sterm = -0.5 * (LOG2PI + 2 * lsd + v * v), 0.5 * (LOG2PI + 2 * lsd.abs() + v * v)
        dmean, sdm = dzi, torch.zeros_like(v)
        dlsd, sdl = dzi * torch.exp(lsd) * v - gb, (dzi * v).abs() * torch.exp(lsd) + gb.abs()
        dz, sdz = None, None
    z = torch.zeros_like(v)
    dhz = torch.cat((torch.where(mpass, dmean, z), torch.where(spass, dlsd, z)), -1)
    sdh = torch.cat((sdm + z, sdl + z), -1)
    return out, so, term.sum((1, 2, 3)), sterm.sum((1, 2, 3)), dz, sdz, dhz, sdh


def _gauss_run(case):
    name, B, Hh, Ww, Ch, mode, clip, has_zout, has_dzin, has_dzout, has_g, plan, bcap = case
    H = _H()
    hz0, v0, dz0, g0, lp0, lim = _gauss_data(B, Hh, Ww, Ch, clip, 500 + Ch + B)
    _, hz = view(B, Hh, Ww, 2 * Ch, 3, 5, hz0)
    _, zin = view(B, Hh, Ww, Ch, 1, 2, v0)
    zb, zout = view(B, Hh, Ww, Ch, 2, 1) if has_zout else (None, None)
    lp = lp0.to(DEV)
    if plan is not None:
        assert gauss_plan(B, Hh * Ww * Ch) == plan, (name, gauss_plan(B, Hh * Ww * Ch))
        if name == "cap256":
            assert Hh * Ww * Ch > 256 * 256                                    # every thread loops
        if name == "ragged":
            assert 4 < plan[0] < 256 and (Hh * Ww * Ch) % 256 != 0
    H.gauss_fwd(hz, zin, zout, lp, mode, clip, lim)
    _, dzin = view(B, Hh, Ww, Ch, 2, 2, dz0) if has_dzin else (None, None)
    dzb, dzout = view(B, Hh, Ww, Ch, 1, 1) if has_dzout else (None, None)
    dhb, dhz = view(B, Hh, Ww, 2 * Ch, 3, 2)
    work = B * Hh * Ww * Ch
    assert (grid_for(work) == 4096 and work > 4096 * 256) == bcap, name
    H.gauss_bwd(hz, zin, dzin, g0.to(DEV) if has_g else None, dzout, dhz, mode, clip, lim)
    torch.cuda.synchronize()
    return dict(hz0=hz0, v0=v0, dz0=dz0 if has_dzin else None, g0=g0 if has_g else None, lp0=lp0, lim=lim, zb=zb, zout=zout, lp=lp,
                dzb=dzb, dzout=dzout, dhb=dhb, dhz=dhz)


def _gauss_check(case, t, hz, v, dz, g, must_fail=False):
    name, B, Hh, Ww, Ch, mode, clip, has_zout, has_dzin, has_dzout, has_g = case[:11]
    rd = _rd(B * Hh * Ww * Ch)
    mv = lambda x: x.to(rd) if x is not None else None
    out, so, lpt, slp, dzr, sdz, dhr, sdh = gauss_ref(mv(hz), mv(v), mv(dz), mv(g), mode, clip, t["lim"])
    K = Hh * Ww * Ch
    tol_lp = 2 * TOL_GAUSS + 4 * U + math.sqrt(K) * U
    lp0 = t["lp0"].double().to(rd)
    res = []
    if has_zout:
        res.append(("gauss zout", t["zout"].to(rd), out, so, TOL_GAUSS))
    res.append(("gauss logp", t["lp"].to(rd), lp0 + lpt, lp0.abs() + slp, tol_lp))
    if mode == 0 and has_dzout:
        res.append(("gauss dzout", t["dzout"].to(rd), dzr, sdz, TOL_GAUSS_B))
    res.append(("gauss dhz", t["dhz"].to(rd), dhr, sdh, TOL_GAUSS_B))
    if must_fail:
        return {w: share(a, r, s, tol) for w, a, r, s, tol in res}
    for w, a, r, s, tol in res:
        check(a, r, s, tol, w, name)


@pytest.mark.parametrize("case", GAUSS_CASES, ids=[c[0] for c in GAUSS_CASES])
def test_gauss(case):
    name, B, Hh, Ww, Ch = case[:5]
    t = _gauss_run(case)
    _gauss_check(case, t, t["hz0"], t["v0"], t["dz0"], t["g0"])
    if t["zb"] is not None:
        assert intact(t["zb"], 2, Ch), name
    if t["dzb"] is not None:
        assert intact(t["dzb"], 1, Ch), name
    assert intact(t["dhb"], 3, 2 * Ch), name
    if case[5] == 1 or not case[9]:
        assert t["dzout"] is None or bool(torch.isnan(t["dzout"]).all()), "mode 1 writes no dzout"


def test_gauss_detects_a_wrong_pixel():
    for case in (GAUSS_CASES[0], GAUSS_CASES[3]):
        name, B, Hh, Ww, Ch, mode = case[:6]
        t = _gauss_run(case)
        v = t["v0"].clone()
        v[1, Hh - 1, Ww - 1, :] += 1.0          # the last pixel of the middle image
        sh = _gauss_check(case, t, t["hz0"], v, t["dz0"], t["g0"], must_fail=True)
        for w in ("gauss zout", "gauss logp", "gauss dhz"):
            assert sh[w] >= 10, (name, w, sh[w])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. channel reductions and the BatchNorm pieces
# ---------------------------------------------------------------------------------------------------------------------------------
# (C, B, H, W, tails wanted among the lanes' last four-pixel iterations, block cap reached)
BN_CASES = [
    (1, 3, 61, 47, {1}, False),
    (3, 2, 67, 41, {1, 2}, False),
    (12, 3, 29, 23, {3}, False),
    (100, 2, 19, 17, {1, 2}, False),
    (129, 1, 13, 11, {1}, False),
    (256, 1, 193, 191, {3}, True),
]
EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
MOM32 = float(torch.tensor(MOM, dtype=torch.float32))


def chan_plan(npix, Cn):
    """tmg_chan_reduce / tmg_chan_moments: (lanes, blocks, {valid pixels of a lane's last four-pixel iteration})."""
    lanes = max(1, 256 // Cn)
    blocks = max(1, min(1024, -(-(-(-npix // lanes)) // 32)))
    step = blocks * lanes
    cnts = {-(-(npix - L) // step) for L in range(min(step, npix))}
    return lanes, blocks, {c % 4 for c in cnts}


def _bn_data(Cn, B, Hh, Ww, seed, mean_scale=1.0, spread=2.0):
    g = _gen(seed)
    x = torch.randn(B, Hh, Ww, Cn, generator=g) * spread + mean_scale * (0.5 + torch.rand(Cn, generator=g))
    gamma, beta = 1 + 0.3 * torch.randn(Cn, generator=g), 0.2 * torch.randn(Cn, generator=g)
    gy = torch.randn(B, Hh, Ww, Cn, generator=g)
    rm0, rv0 = torch.randn(Cn, generator=g), 0.5 + torch.rand(Cn, generator=g)
    # no ReLU pre-activation close enough to zero for fp32 and fp64 to disagree about its sign (nudging moves the statistics: repeat)
    for _ in range(4):
        st = bn_stats(x, gamma, beta)
        u = x.double() * st["a"] + st["bsh"]
        near = u.abs() < 1e-5 * ((x.double() * st["a"]).abs() + st["bsh"].abs())
        if not bool(near.any()):
            break
        x = torch.where(near, x + 0.03 * spread, x)
    assert not bool(near.any())
    return x, gamma, beta, gy, rm0, rv0


def bn_stats(x, gamma, beta):
    """fp64 batch statistics of an NHWC tensor and the folded affine (bn_finalize_kernel's five rows)."""
    xd = x.double().flatten(0, 2)
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    rstd = 1 / torch.sqrt(var + EPS32)
    a = gamma.double().to(x.device) * rstd
    return dict(mean=mean, var=var, rstd=rstd, a=a, bsh=beta.double().to(x.device) - mean * a, n=xd.shape[0], absx=xd.abs().sum(0), sq=(xd * xd).sum(0))


def _run_stats_ref(st, rm0, rv0, n):
    """nn.BatchNorm2d's update, stated: unbiased variance n / (n - 1); n = 1 (which nn.BatchNorm2d refuses) takes max(n - 1, 1)."""
    rm = rm0.double() * (1 - MOM32) + MOM32 * st["mean"].cpu()
    vterm = MOM32 * st["var"].cpu() * (n / max(n - 1, 1))
    return rm, rm0.double().abs() * (1 - MOM32) + MOM32 * st["mean"].cpu().abs(), rv0.double() * (1 - MOM32) + vterm, rv0.double() * (1 - MOM32) + vterm


@pytest.mark.parametrize("case", BN_CASES, ids=["C%d" % c[0] for c in BN_CASES])
def test_chan_reduce_and_batchnorm(case):
    Cn, B, Hh, Ww, tails, capped = case
    H = _H()
    n = B * Hh * Ww
    lanes, blocks, got_tails = chan_plan(n, Cn)
    assert blocks > 1 and tails <= got_tails and (blocks == 1024 and -(-n // lanes) > 32 * 1024) == capped, (lanes, blocks, got_tails)
    assert lanes == (256 // Cn if Cn <= 256 else 1) and (lanes * Cn < 256) == (Cn in (3, 12, 100, 129))
    x0, gamma, beta, gy0, rm0, rv0 = _bn_data(Cn, B, Hh, Ww, 600 + Cn)
    rd = _rd(n * Cn)
    xb, x = view(B, Hh, Ww, Cn, 3, 5, x0)
    gb_, gy = view(B, Hh, Ww, Cn, 4, 4, gy0)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    st = bn_stats(x0.to(rd), gamma, beta)
    cpu = lambda t: t.detach().cpu()
    tag = "C%d" % Cn
    # ---- chan_reduce mode 0, plain sums; the sums accumulate onto what s0 / s1 hold
    init = torch.arange(Cn, dtype=torch.float32) * 0.25 + 1
    s0, s1 = init.to(DEV), (2 * init).to(DEV)
    H.chan_reduce(x, None, None, None, None, None, s0, s1, 0)
    xd = x0.to(rd).double().flatten(0, 2)
    check(cpu(s0), init.double() + cpu(xd.sum(0)), init.double() + cpu(st["absx"]), tol_sum(n, 8), "chan_reduce sum", tag)
    check(cpu(s1), 2 * init.double() + cpu(st["sq"]), 2 * init.double() + cpu(st["sq"]), tol_sum(n, 8), "chan_reduce sum sq", tag)
    # ---- centred second pass: v0 = channel sums, divisor n
    sums = torch.zeros(Cn, device=DEV)
    sq = torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, None, None, None, None, None, sums, sq, 0)
    c0, c1 = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, None, sums, None, None, None, c0, c1, 0, divisor=n)
    off = sums.double().to(rd) / n                                     # the offset the kernel was given, in fp64
    dd, sd = xd - off, xd.abs() + off.abs()
    check(cpu(c0), cpu(dd.sum(0)), cpu(sd.sum(0)), tol_sum(n, 8), "chan_reduce centred sum", tag)
    check(cpu(c1), cpu((dd * dd).sum(0)), cpu((sd * sd).sum(0)), tol_sum(n, 8), "chan_reduce centred sq", tag)
    # ---- fp32 two-pass statistics -> bn_finalize
    out32 = torch.full((5, Cn), NAN, device=DEV)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    H.bn_finalize(sums, c1, gd, bd, rm, rv, out32, n, EPS, MOM)
    tr = tol_sum(n, 8)
    mean, var, rstd, a, bsh = (cpu(st[k]) for k in ("mean", "var", "rstd", "a", "bsh"))
    s_mean, s_var = cpu(st["absx"]) / n, cpu((sd * sd).sum(0)) / n
    s_rstd = 0.5 * rstd * s_var / (var + EPS32)
    gam, bet = gamma.double(), beta.double()
    check(cpu(out32[0]), mean, s_mean, tr + U, "bn_finalize mean", tag)
    check(cpu(out32[1]), var, s_var, tr + U, "bn_finalize var", tag)
    check(cpu(out32[2]), rstd, s_rstd, tr + 8 * U, "bn_finalize rstd", tag)
    check(cpu(out32[3]), a, gam.abs() * s_rstd, tr + 9 * U, "bn_finalize a", tag)
    check(cpu(out32[4]), bsh, bet.abs() + (mean * a).abs() + a.abs() * s_mean + mean.abs() * gam.abs() * s_rstd, tr + 12 * U, "bn_finalize bsh", tag)
    rmr, srm, rvr, srv = _run_stats_ref(st, rm0, rv0, n)
    check(cpu(rm), rmr, srm + MOM32 * s_mean, tr + 9 * U, "bn_finalize running_mean", tag)
    check(cpu(rv), rvr, srv + MOM32 * s_var * n / (n - 1), tr + 9 * U, "bn_finalize running_var", tag)
    # ---- one-pass fp64 moments -> bn_finalize64, running statistics and the counter against nn.BatchNorm2d in fp64
    acc = torch.zeros(2 * Cn, dtype=torch.float64, device=DEV)
    H.chan_moments(x, acc)
    t64 = (2 + math.sqrt(n)) * 2.0 ** -53
    check(cpu(acc[:Cn]), cpu(xd.sum(0)), cpu(st["absx"]), t64, "chan_moments sum", tag)
    check(cpu(acc[Cn:]), cpu(st["sq"]), 0.0, t64, "chan_moments sum sq", tag)
    out = torch.full((5, Cn), NAN, device=DEV)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    cnt = torch.tensor(41, dtype=torch.int64, device=DEV)
    H.bn_finalize64(acc, gd, bd, rm, rv, out, n, EPS, MOM, counter=cnt)
    check(cpu(out[0]), mean, 0.0, 2 * U, "bn_finalize64 mean", tag)
    check(cpu(out[1]), var, 0.0, 2 * U, "bn_finalize64 var", tag)
    check(cpu(out[2]), rstd, 0.0, 8 * U, "bn_finalize64 rstd", tag)
    check(cpu(out[3]), a, 0.0, 9 * U, "bn_finalize64 a", tag)
    check(cpu(out[4]), bsh, bet.abs() + (mean * a).abs(), 12 * U, "bn_finalize64 bsh", tag)
    bn = torch.nn.BatchNorm2d(Cn, eps=EPS32, momentum=MOM32).double().to(rd)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
        bn.num_batches_tracked.fill_(41)
    bn.train()
    xg = x0.to(rd).double().permute(0, 3, 1, 2).requires_grad_(True)
    yref = F.relu(bn(xg))
    check(cpu(rm), cpu(bn.running_mean), srm, 9 * U, "bn_finalize64 running_mean", tag)
    check(cpu(rv), cpu(bn.running_var), srv, 9 * U, "bn_finalize64 running_var", tag)
    assert int(cnt) == int(bn.num_batches_tracked) == 42
    # ---- chan_reduce mode 1 and bn_bwd_apply against fp64 autograd of relu(batch_norm(x))
    (yref * gy0.to(rd).double().permute(0, 3, 1, 2)).sum().backward()
    dxr = xg.grad.permute(0, 2, 3, 1)
    m0, m1 = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, gy, out[3], out[4], out[0], out[2], m0, m1, 1)
    stx = {k: st[k] for k in ("mean", "rstd", "a", "bsh")}
    du_abs = (gy0.to(rd).double().flatten(0, 2) * ((xd * stx["a"] + stx["bsh"]) > 0)).abs()
    xh_abs = (xd.abs() + stx["mean"].abs()) * stx["rstd"]
    S0, S1 = cpu(du_abs.sum(0)), cpu((du_abs * xh_abs).sum(0))
    check(cpu(m0), cpu(bn.bias.grad), S0, tol_sum(n, 8), "chan_reduce bn-relu sum du", tag)
    check(cpu(m1), cpu(bn.weight.grad), S1, tol_sum(n, 8) + 12 * U, "chan_reduce bn-relu sum du xhat", tag)
    s_dx = (gam.abs().to(rd) * stx["rstd"] * (gy0.to(rd).double().flatten(0, 2).abs() + S0.to(rd) / n + xh_abs * S1.to(rd) / n)).view(B, Hh, Ww, Cn)
    assert (grid_for(n * Cn) == 4096 and n * Cn > 4096 * 256) == capped, tag     # bn_bwd_apply: grid_for(npix C), threads loop at C = 256
    for accumulate in (0, 1):
        d0 = torch.randn(B, Hh, Ww, Cn, generator=_gen(7))
        db, dx = view(B, Hh, Ww, Cn, 2, 3, d0 if accumulate else None)
        H.bn_bwd_apply(x, gy, out[3], out[4], out[0], out[2], gd, m0, m1, dx, accumulate, divisor=n)
        torch.cuda.synchronize()
        ref = dxr + d0.to(rd).double() if accumulate else dxr
        check(dx.to(rd), ref, s_dx + (d0.to(rd).double().abs() if accumulate else 0.0), tol_sum(n, 12), "bn_bwd_apply dx (accumulate %d)" % accumulate, tag)
        assert intact(db, 2, Cn), tag
    assert intact(xb, 3, Cn) and intact(gb_, 4, Cn)


def test_chan_reduce_refuses_more_than_256_channels():
    H = _H()
    x = torch.randn(1, 2, 3, 257, device=DEV)
    s0, s1 = torch.zeros(257, device=DEV), torch.zeros(257, device=DEV)
    with pytest.raises(RuntimeError):
        H.chan_reduce(x, None, None, None, None, None, s0, s1, 0)
    with pytest.raises(RuntimeError):
        H.chan_moments(x, torch.zeros(2 * 257, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    assert not bool(s0.any()) and not bool(s1.any())


def test_batchnorm_running_stats_of_one_sample():
    """n = 1: nn.BatchNorm2d refuses a single value per channel; the kernels follow its formula with max(n - 1, 1): the batch
    variance is 0 and the running variance decays by (1 - momentum)."""
    H = _H()
    Cn = 5
    g = _gen(11)
    x0 = torch.randn(1, 1, 1, Cn, generator=g)
    gamma, beta, rm0, rv0 = (1 + 0.3 * torch.randn(Cn, generator=g), torch.randn(Cn, generator=g), torch.randn(Cn, generator=g),
                             0.5 + torch.rand(Cn, generator=g))
    st = bn_stats(x0, gamma, beta)
    assert float(st["var"].abs().max()) == 0.0
    rmr, srm, rvr, srv = _run_stats_ref(st, rm0, rv0, 1)
    x = x0.to(DEV)
    for path in ("fp64", "fp32"):
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        out = torch.full((5, Cn), NAN, device=DEV)
        if path == "fp64":
            acc = torch.zeros(2 * Cn, dtype=torch.float64, device=DEV)
            H.chan_moments(x, acc)
            cnt = torch.tensor(0, dtype=torch.int64, device=DEV)
            H.bn_finalize64(acc, gamma.to(DEV), beta.to(DEV), rm, rv, out, 1, EPS, MOM, counter=cnt)
            assert int(cnt) == 1
        else:
            s0, s1, c0, c1 = (torch.zeros(Cn, device=DEV) for _ in range(4))
            H.chan_reduce(x, None, None, None, None, None, s0, s1, 0)
            H.chan_reduce(x, None, s0, None, None, None, c0, c1, 0, divisor=1)
            H.bn_finalize(s0, c1, gamma.to(DEV), beta.to(DEV), rm, rv, out, 1, EPS, MOM)
        check(rm.cpu(), rmr, srm, 9 * U, "bn running_mean (n = 1)", path)
        check(rv.cpu(), rvr, srv, 9 * U, "bn running_var (n = 1)", path)
        check(out[0].cpu(), st["mean"], 0.0, 2 * U, "bn mean (n = 1)", path)
        check(out[1].cpu(), st["var"], 0.0, 2 * U, "bn var (n = 1)", path)
        check(out[2].cpu(), st["rstd"], 0.0, 8 * U, "bn rstd (n = 1)", path)


def test_batchnorm_moments_do_not_cancel():
    """Channel means of 1e3 with unit spread over 102 400 pixels: the variance of the fp64-moments path meets the bound of the benign
    cases (2 u of the variance itself).  The fp32 two-pass path is held to its own bound (TOL_RED of its sums' |terms|) and its
    share of the 2 u bound is recorded, not asserted."""
    H = _H()
    Cn, B, Hh, Ww = 3, 1, 320, 320
    n = B * Hh * Ww
    g = _gen(13)
    x0 = torch.randn(B, Hh, Ww, Cn, generator=g) + torch.tensor([1000.0, -1000.0, 1003.0])
    gamma, beta = torch.ones(Cn), torch.zeros(Cn)
    st = bn_stats(x0, gamma, beta)
    assert n > 1e5 and float((st["var"] - 1).abs().max()) < 0.02
    _, x = view(B, Hh, Ww, Cn, 3, 2, x0)
    acc = torch.zeros(2 * Cn, dtype=torch.float64, device=DEV)
    H.chan_moments(x, acc)
    out = torch.full((5, Cn), NAN, device=DEV)
    H.bn_finalize64(acc, gamma.to(DEV), beta.to(DEV), None, None, out, n, EPS, MOM)
    check(out[0].cpu(), st["mean"], 0.0, 2 * U, "bn_finalize64 mean (cancellation)")
    check(out[1].cpu(), st["var"], 0.0, 2 * U, "bn_finalize64 var (cancellation)")
    check(out[2].cpu(), st["rstd"], 0.0, 8 * U, "bn_finalize64 rstd (cancellation)")
    s0, s1, c0, c1 = (torch.zeros(Cn, device=DEV) for _ in range(4))
    H.chan_reduce(x, None, None, None, None, None, s0, s1, 0)
    H.chan_reduce(x, None, s0, None, None, None, c0, c1, 0, divisor=n)
    out32 = torch.full((5, Cn), NAN, device=DEV)
    H.bn_finalize(s0, c1, gamma.to(DEV), beta.to(DEV), None, None, out32, n, EPS, MOM)
    xd = x0.double().flatten(0, 2)
    off = s0.double().cpu() / n
    s_var = ((xd.abs() + off.abs()) ** 2).sum(0) / n
    check(out32[1].cpu(), st["var"], s_var, tol_sum(n, 8) + U, "bn_finalize var, fp32 two-pass (cancellation)")
    share(out32[1].cpu(), st["var"], 0.0, 2 * U, "fp32 two-pass var against the 2 u bound (recorded)")


def test_chan_reduce_detects_a_dropped_lane():
    """The reference without the pixels one lane of one block reads, for one channel."""
    H = _H()
    Cn, B, Hh, Ww = BN_CASES[2][:4]
    n = B * Hh * Ww
    lanes, blocks, _ = chan_plan(n, Cn)
    x0, gamma, beta, gy0, _, _ = _bn_data(Cn, B, Hh, Ww, 600 + Cn)
    _, x = view(B, Hh, Ww, Cn, 3, 5, x0)
    _, gy = view(B, Hh, Ww, Cn, 4, 4, gy0)
    s0, s1 = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, None, None, None, None, None, s0, s1, 0)
    acc = torch.zeros(2 * Cn, dtype=torch.float64, device=DEV)
    H.chan_moments(x, acc)
    st = bn_stats(x0, gamma, beta)
    f32 = lambda k: st[k].float().to(DEV)
    m0, m1 = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, gy, f32("a"), f32("bsh"), f32("mean"), f32("rstd"), m0, m1, 1)
    torch.cuda.synchronize()
    xd, gd = x0.double().flatten(0, 2), gy0.double().flatten(0, 2)
    keep = torch.ones(n, Cn, dtype=torch.float64)
    keep[(blocks - 1) * lanes + lanes - 1::blocks * lanes, Cn - 1] = 0       # the last lane of the last block, last channel
    assert 4 <= int((keep == 0).sum()) < n // 8
    du = gd * ((xd * st["a"] + st["bsh"]) > 0)
    xh = (xd - st["mean"]) * st["rstd"]
    t = tol_sum(n, 8)
    assert share(s0.cpu(), (xd * keep).sum(0), xd.abs().sum(0), t) >= 10
    assert share(s1.cpu(), (xd * xd * keep).sum(0), (xd * xd).sum(0), t) >= 10
    assert share(acc[:Cn].cpu(), (xd * keep).sum(0), xd.abs().sum(0), (2 + math.sqrt(n)) * 2.0 ** -53) >= 10
    assert share(m0.cpu(), (du * keep).sum(0), du.abs().sum(0), t) >= 10
    assert share(m1.cpu(), (du * xh * keep).sum(0), (du.abs() * (xd.abs() + st["mean"].abs()) * st["rstd"]).sum(0), t + 12 * U) >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. masked add
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, B, H, W, n, (offset, extra) of every view, float4 kernel, grid capped)
MADD_CASES = [
    ("v4", 3, 5, 7, 4, (0, 0), True, False),
    ("v8", 3, 5, 7, 8, (4, 4), True, False),
    ("s3", 3, 5, 7, 3, (0, 0), False, False),
    ("s6", 3, 5, 7, 6, (4, 4), False, False),
    ("s8o2", 3, 5, 7, 8, (2, 2), False, False),
    ("vloop", 1, 1025, 1024, 4, (0, 0), True, True),
    ("sloop", 1, 350, 1000, 3, (0, 0), False, True),
]


@pytest.mark.parametrize("case", MADD_CASES, ids=[c[0] for c in MADD_CASES])
def test_masked_add(case):
    name, B, Hh, Ww, n, (off, extra), vec, capped = case
    H = _H()
    g = _gen(700 + n)
    shape = (B, Hh, Ww, n)
    src0, add0, dst0 = (torch.randn(shape, generator=g) for _ in range(3))
    ref0 = torch.randn(shape, generator=g)
    ref0.view(-1)[::5] = 0.0
    ref0.view(-1)[2::7] = -0.0
    combos = [(s, r, a, acc) for s in (0, 1) for r in (0, 1) for a in (0, 1) for acc in (0, 1)]
    if capped:
        combos = [(1, 1, 1, 1)]
    for hs, hr, ha, acc in combos:
        _, src = view(B, Hh, Ww, n, off, extra, src0) if hs else (None, None)
        _, ref = view(B, Hh, Ww, n, off, extra, ref0) if hr else (None, None)
        _, add = view(B, Hh, Ww, n, off, extra, add0) if ha else (None, None)
        db, dst = view(B, Hh, Ww, n, off, extra, dst0)
        ops = [t for t in (src, ref, add, dst) if t is not None]
        is_vec = n % 4 == 0 and all(_stride(t) % 4 == 0 for t in ops) and _al(ops, 16) and B * Hh * Ww * (n // 4) < 2 ** 31
        assert is_vec == vec, name
        work = B * Hh * Ww * (n // 4 if vec else n)
        assert (grid_for(work) == 4096 and work > 4096 * 256) == capped, name
        H.masked_add(dst, src=src, ref=ref, add=add, accumulate=bool(acc))
        torch.cuda.synchronize()
        v = src0.clone() if hs else torch.zeros(shape)
        if hr:
            v = torch.where(ref0 > 0, v, torch.zeros(shape))
        if ha:
            v = v + add0
        want = dst0 + v if acc else v
        assert torch.equal(dst.cpu(), want), (name, hs, hr, ha, acc)
        assert intact(db, off, n), name


def test_masked_add_detects_a_wrong_quad():
    H = _H()
    g = _gen(9)
    shape = (3, 5, 7, 8)
    src0, ref0 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    dst = torch.full(shape, NAN, device=DEV)
    H.masked_add(dst, src=src0.to(DEV), ref=ref0.to(DEV))
    ref0[2, 4, 6, 4:] = ref0[2, 4, 6, 4:].abs() * -1 - 1    # the reference masks the last quad: the exact comparison must fail
    src0[2, 4, 6, 4:] += 1
    assert not torch.equal(dst.cpu(), torch.where(ref0 > 0, src0, torch.zeros(shape)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. dkappa, vec_sum, spread2
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw,blocks", [(100, 1), (2048, 1), (2049, 2), (150000, 64)])
def test_dkappa(nw, blocks):
    """dk += <w, dw> + <b, db> for kappa inside [-4, ln 4] (Conv2dZeros: h = e^kappa (W x + b) is homogeneous of degree one in
    (W, b)); outside the clamp the gradient is zero and dk stays what it was."""
    H = _H()
    assert min(64, max(1, -(-nw // 2048))) == blocks and (blocks < 64 or nw > 64 * 2048)
    g = _gen(800 + nw)
    w, dw = torch.randn(nw, generator=g), torch.randn(nw, generator=g)
    b, db = torch.randn(37, generator=g), torch.randn(37, generator=g)
    for has_b in (True, False):
        tot = (w.double() * dw.double()).sum() + ((b.double() * db.double()).sum() if has_b else 0.0)
        sab = (w.double() * dw.double()).abs().sum() + ((b.double() * db.double()).abs().sum() if has_b else 0.0)
        for kappa, inside in ((0.3, True), (-4.0, True), (-4.5, False), (1.5, False)):
            for dk0 in (0.0, 2.5):
                dk = torch.tensor([dk0], device=DEV)
                H.dkappa(w.to(DEV), dw.to(DEV), b.to(DEV) if has_b else None, db.to(DEV) if has_b else None, torch.tensor([kappa], device=DEV), dk)
                torch.cuda.synchronize()
                if inside:
                    check(dk.cpu(), (dk0 + tot).view(1), abs(dk0) + sab, tol_sum(nw + 37, 1), "dkappa", "nw %d" % nw)
                else:
                    assert float(dk) == dk0, (nw, kappa, dk0)
    if nw == 2049:      # sensitivity: the reference without the one element the second block reads
        dk = torch.zeros(1, device=DEV)
        H.dkappa(w.to(DEV), dw.to(DEV), None, None, torch.tensor([0.0], device=DEV), dk)
        alt = (w.double() * dw.double())[:2048].sum() + 3.0
        assert share(dk.cpu(), alt.view(1), (w.double() * dw.double()).abs().sum(), tol_sum(nw, 1)) >= 10


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_vec_sum(n):
    """out[0] = sum_b g[b]: the gradient of a one-element log-det term broadcast over the batch (tmg_ops.SumTermsFn.backward)."""
    H = _H()
    assert (-(-n // 256) > 1) == (n in (257, 1000))     # one block of 256 threads, whatever n: they loop above 256 values
    gv = torch.randn(n, generator=_gen(900 + n)) + 0.5
    out = torch.full((1,), NAN, device=DEV)
    H.vec_sum(gv.to(DEV), out)
    torch.cuda.synchronize()
    check(out.cpu(), gv.double().sum().view(1), gv.double().abs().sum(), tol_sum(n, 1), "vec_sum", "n %d" % n)
    if n >= 255:        # sensitivity: the reference without the last value
        assert share(out.cpu(), gv.double()[:-1].sum().view(1) - gv.double()[-1].abs() - 1.0, gv.double().abs().sum(), tol_sum(n, 1)) >= 10


@pytest.mark.parametrize("case", [(2, 3, 5, 4, 0, "dense", 1), (2, 3, 5, 12, 1, "dense", 2), (1, 7, 3, 4, 1, "slice", 1), (2, 5, 7, 12, 0, "slice", 4),
                                  (1, 513, 1024, 4, 0, "dense", 4096)],
                         ids=["even_c4", "odd_c12", "odd_c4_slice", "even_c12_slice", "loop"])
def test_spread2(case):
    """up[b, y, x] = dy[b, y / 2, x / 2] for even y and x, zero elsewhere (the operand of the stride-2 input gradient,
    tmg_ops.ConvFn.backward: up.zero_(); up[:, ::2, ::2] = dy); the grid is 2h x 2w or, odd, (2h - 1) x (2w - 1)."""
    B, h, w, Cn, odd, lay, blocks = case
    H = _H()
    Hh, Ww = 2 * h - odd, 2 * w - odd
    quads = B * Hh * Ww * (Cn // 4)
    assert grid_for(quads) == blocks and (blocks < 4096 or quads > 4096 * 256)      # glue_grid = grid_for; at the cap the threads loop
    dy0 = torch.randn(B, h, w, Cn, generator=_gen(1000 + Cn + h))
    _, dy = view(B, h, w, Cn, 4, 4, dy0) if lay == "slice" else (None, dy0.to(DEV))
    up = torch.full((B, Hh, Ww, Cn), NAN, device=DEV)
    assert H.spread2(dy, up) is True
    torch.cuda.synchronize()
    want = torch.zeros(B, Hh, Ww, Cn)
    want[:, ::2, ::2] = dy0
    assert torch.equal(up.cpu(), want)
    want[B - 1, 2 * (h - 1), 2 * (w - 1), Cn - 4:] += 1          # sensitivity: the last quad
    assert not torch.equal(up.cpu(), want)


def test_spread2_declines_channels_not_a_multiple_of_four():
    H = _H()
    up = torch.full((1, 4, 4, 6), NAN, device=DEV)
    assert H.spread2(torch.randn(1, 2, 2, 6, device=DEV), up) is False
    torch.cuda.synchronize()
    assert bool(torch.isnan(up).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. checker squeeze / un-squeeze
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, B, h, w, C, (offset, extra) of both views, float4 kernel, grid capped)
CHECKER_CASES = [
    ("v8", 2, 3, 5, 8, (0, 0), True, False),
    ("v8o4", 2, 3, 5, 8, (4, 4), True, False),
    ("s8o2", 2, 3, 5, 8, (2, 2), False, False),
    ("s3", 2, 3, 5, 3, (0, 0), False, False),
    ("s5o1", 1, 4, 3, 5, (1, 2), False, False),
    ("vloop", 1, 256, 260, 16, (0, 0), True, True),
    ("sloop", 1, 300, 300, 3, (0, 0), False, True),
]


@pytest.mark.parametrize("to_small", [1, 0])
@pytest.mark.parametrize("case", CHECKER_CASES, ids=[c[0] for c in CHECKER_CASES])
def test_checker(case, to_small):
    name, B, h, w, Cn, (off, extra), vec, capped = case
    H = _H()
    g = _gen(1100 + Cn + h)
    if to_small:
        src0 = torch.randn(B, 2 * h, 2 * w, Cn, generator=g)
        want = O.checker_squeeze(src0.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        _, src = view(B, 2 * h, 2 * w, Cn, off, extra, src0)
        db, dst = view(B, h, w, 4 * Cn, off, extra)
    else:
        src0 = torch.randn(B, h, w, 4 * Cn, generator=g)
        want = O.checker_unsqueeze(src0.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
        _, src = view(B, h, w, 4 * Cn, off, extra, src0)
        db, dst = view(B, 2 * h, 2 * w, Cn, off, extra)
    total = B * h * w * 4 * Cn
    is_vec = Cn % 4 == 0 and _stride(src) % 4 == 0 and _stride(dst) % 4 == 0 and _al((src, dst), 16) and total // 4 < 2 ** 31
    assert is_vec == vec, name
    work = total // 4 if vec else total
    assert (grid_for(work) == 4096 and work > 4096 * 256) == capped, name
    H.checker(src, dst, to_small)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want.contiguous()), name
    assert intact(db, off, dst.shape[3]), name
    alt = want.clone()
    alt[B - 1, -1, -1, -1] += 1                  # sensitivity of the exact comparison: the last element
    assert not torch.equal(dst.cpu(), alt)
