"""Case tables, the float32 mirror of the state, the int64 reference, the fp64 direct sums, the fp64 reference by direct definition, the
fp64 host restatement of the finalize formulas and the counted rounding bounds of the ensemble energy flux (csrc/tmg_flux.hip,
tmg_ops.EnsembleFlux), shared by tests/test_flux_cpu.py (no device) and tests/test_flux_gpu.py.

Rows are the S members plus the target as row S.  a [B, 2] is the fp32 table the kernel is handed, kk [L, 2] the fp32 flux factors,
x the raw normalised rows at the TIMED steps.  For a width w: r = w // 2, N = w^2; a pixel is valid when r + 1 <= h <= H - 2 - r and
the same in w.

THE ORDER of the state (stated once here, once in the kernel's header comment), every operation a float32 operation of its own:
  f_c = fl(a_c x_c), c = 0, 1 (u, v)
  Sg_u, Sg_v, Sg_uu, Sg_uv, Sg_vv: the box sums of f_u, f_v, fl(f_u f_u), fl(f_u f_v), fl(f_v f_v), a row pass (along W) and then a column
  pass (along H, of the row sums), both from the centre outwards:  s_0 = g[0],  s_j = fl(fl(s_{j-1} + g[-j]) + g[+j]),  j = 1 .. r
  Q_uu = fl(fl(N Sg_uu) - fl(Sg_u Sg_u)),  Q_uv = fl(fl(N Sg_uv) - fl(Sg_u Sg_v)),  Q_vv = fl(fl(N Sg_vv) - fl(Sg_v Sg_v))
  Sx g = fl(fl(fl(g[h-1,w+1] - g[h-1,w-1]) + fl(2 fl(g[h,w+1] - g[h,w-1]))) + fl(g[h+1,w+1] - g[h+1,w-1]))      (tests/budget_cases.py)
  Sy g = fl(fl(fl(g[h+1,w-1] - g[h-1,w-1]) + fl(2 fl(g[h+1,w] - g[h-1,w]))) + fl(g[h+1,w+1] - g[h-1,w+1]))      on the box sums
  A = fl(fl(Q_uu Sx Sg_u) + fl(Q_uv Sx Sg_v)),  B = fl(fl(Q_uv Sy Sg_u) + fl(Q_vv Sy Sg_v)),  Pi_s = -fl(fl(A kk_x) + fl(B kk_y))
  terms 0: A, 1: B, 2: fl(Pi_s Pi_s), 3: [Pi_s < 0], 4..6: Q_uu, Q_uv, Q_vv
  raw[row, b, l, q, p] = the first timed step's term, then fl(raw + term) per timed step, in step order; valid pixels only.

The reference by direct definition (fp64, per row) uses the FULL physical velocity U_c = a_c x_c + u0 out_mu_c (the kernel leaves
out_mu out: tau and the gradients of bar(U) are invariant to it, which the comparison shows), box MEANS by plain slicing,
tau_ij = bar(U_i U_j) - bar(U_i) bar(U_j), d/dx = Sx / (8 dx), d/dy = Sy / (8 dy) on bar(U), Pi = -(tau_uu dx bar U + tau_uv (dy bar U +
dx bar V) + tau_vv dy bar V) at every timed step, then the time mean, the temporal std, the fraction of steps with Pi < 0 and the time
mean of tau.  It never goes through Q, A or B.  The direct sums are the fp64 values of the 7 un-normalised terms from f = a x.  The
host restatement applies the finalize formulas to a given state in fp64:
  Pi = -((raw_0 k_x + raw_1 k_y) / T);  tstd = sqrt(max(raw_2 / T - Pi^2, 0));  back = raw_3 / T;  tau = raw_4..6 / ((N N) T)

The bounds (u = 2^-24, e = 2^-53); k counts the roundings the test's own inputs carry per value of f, in units of u (0 for the
state tests, whose reference starts from the same fp32 x and a).
  f carries 1 + k roundings.  A box sum passes each term through at most 2 (w - 1) additions (w - 1 per pass), so against the box sum
  of magnitudes Sa:  Sg_u: 2 w - 1 + k;  Sg_uu (two factors and the product, 3 + 2 k): 2 w + 1 + 2 k.
  Q: N Sg_uu carries 2 w + 2 + 2 k on N Sa_uu, Sg_u Sg_u 2 (2 w - 1 + k) + 1 on Sa_u Sa_u, the subtraction 1 on both, + 1 for all
  second-order terms:   c_Q = 4 w + 1 + 2 k   against  MQ = N Sa_|uu| + Sa_|u| Sa_|u|
  Sx Sg_u: each box sum passes one subtraction and at most two additions (the doubling is exact): 2 w + 2 + k against GS = the stencil
  of Sa with every subtraction an addition.  A: the product Q Sx carries c_Q + (2 w + 2 + k) + 1 and the sum 1:
                        c_A = 6 w + 5 + 3 k  (+ 1 second order = 6 w + 6 + 3 k)  against  MA = MQ_uu GSx_u + MQ_uv GSx_v
  Pi_s: the factor kk, the product and the sum:  c_P = c_A + 3  against  MP = MA k_x + MB k_y;   Pi_s^2: 2 c_P + 1 against MP^2.
  The count [Pi_s < 0] can differ from the reference's only at a step where |Pi_s| <= c_P u MP: by at most the number of such steps.
  raw: T - 1 additions of the time sum on top:   |raw - ref| <= (T - 1 + c) u sum_t M.
  fields, same raw (device against the host restatement): the longest fp64 chain is the variance (11 roundings a side): C_FIN = 24,
  |got - ref| <= u |ref| + C_FIN e mag, mag the formula on magnitudes; the Welford mean and std over S members and the square roots as
  tests/budget_cases.py bounds them (c = (C_FIN + 4 S) e; sqrt moves by min(sqrt(dq), dq / value)); a curve over n pixels (C_FIN + n) e.
  fields, against the definition: the state's bounds above carried through the (linear) finalize formulas, the variance through
  dq = ((T + 2 c_P) u sum MP^2) / T + 2 |Pi|_mag dPi, plus C_DEF e times the same magnitudes formed from |U| (the definition's own fp64
  roundings with out_mu inside: a box of N <= 1089 terms summed plainly, C_DEF = 4 * 1089 + 64).
The counts come from the arithmetic above, never from what the kernel gives; the tests print the share of the bound they reach."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
E53 = 2.0 ** -53
F32 = np.float32
Q = 7
C_FIN = 24
C_DEF = 4 * 1089 + 64
FIELD_KEYS = ("flux_mean", "flux_std", "target_flux", "flux_tstd_mean", "target_flux_tstd", "backscatter_mean", "backscatter_std",
              "target_backscatter", "sgs_mean", "sgs_std", "target_sgs", "flux_curve", "sgs_energy_curve")
NEW_KEYS = FIELD_KEYS + ("member_flux", "flux_widths", "flux_lengths")
DEFAULT_WIDTHS = (3, 5, 9, 17, 33)

# ---- case tables ------------------------------------------------------------------------------------------------------------------------
CHUNKINGS = {1: [(1,)], 3: [(3,), (1, 2)], 5: [(5,), (2, 2, 1), (1,) * 5]}     # tests/budget_cases.py's
ALL8 = (3, 5, 7, 9, 11, 13, 15, 17)
# (S, B, (H, W), widths, padded, T timed steps); one untimed step comes first; padded: the rows are channel slices of a wider
# NaN-filled buffer.  5x5: one valid pixel; 35x38 with 33: the largest width on the smallest field that holds it (1 x 4 valid pixels);
# 9x11: narrower than a tile, small LDS; 37x70 (2 x 3 tiles, ragged in both directions) and 70x36 (3 x 1 tiles, the valid region of
# width 3 exactly one tile wide): the halo of 9 crossing the tile borders, LDS over 64 KB; 21x40: all 8 widths.
CASES = [
    (1, 1, (5, 5), (3,), False, 1), (3, 2, (9, 11), (3, 5), True, 2), (5, 1, (35, 38), (3, 33), False, 2),
    (5, 2, (37, 70), (3, 9, 17), False, 2), (3, 1, (70, 36), (3, 9, 17), True, 3), (5, 1, (21, 40), ALL8, True, 2),
    (1, 2, (9, 11), (5,), False, 7),
]
MAX_CASE = (1024, 1, (5, 6), (3,), False, 2)                                  # chunks (1024,) and (64,) * 16
SD = [1.7, 0.6, 2.5]
MU = [0.4, -0.1, 0.25]
GRID = (0.5, 0.25)                                                           # dx != dy
GRID_INT = (0.125, 0.125)                                                    # 8 dx = 1: kx = ky = 1 / N^3


def factors(widths, grid):
    """k64 [L, 2]: 1 / (8 dx N^3), 1 / (8 dy N^3), as tmg_ops.flux_factors forms them (fp64); the kernel is handed k64.astype(fp32)."""
    return np.array([[1.0 / ((8.0 * float(d)) * float((w * w) ** 3)) for d in grid] for w in widths], dtype=np.float64)


def valid_mask(w, hw):
    r = w // 2
    m = np.zeros(hw, dtype=bool)
    m[r + 1:hw[0] - 1 - r, r + 1:hw[1] - 1 - r] = True
    return m


@functools.lru_cache(maxsize=None)
def int_inputs(S, B, hw, T, seed, amp):
    """Integer data -> xs [T + 1, S + 1, B, 3, H, W] float32 (row S: the target; step 0 untimed), |x| <= amp."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, (T + 1, S + 1, B, 3) + tuple(hw), generator=g).float().numpy()


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, hw, T, seed):
    """Smooth shear plus Gaussian rows -> (xs [T + 1, S + 1, B, 3, H, W] float32, sd [3], mu [3], u [B, 3])."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    hh = torch.arange(Hh).view(Hh, 1) / 7.0
    ww = torch.arange(Ww).view(1, Ww) / 5.0
    base = torch.stack([torch.sin(hh) + 0.3 * torch.cos(ww), 0.5 * torch.cos(hh + ww), hh * ww * 0])
    xs = base[None, None, None] + 0.8 * torch.randn(T + 1, S + 1, B, 3, Hh, Ww, generator=g)
    u = 0.5 + torch.rand(B, 3, generator=g)
    return xs.numpy().astype(F32), np.array(SD, F32), np.array(MU, F32), u.numpy().astype(F32)


def scales(sd, u, B):
    """a [B, 2]: u out_std in fp64 from the fp32 factors, rounded to fp32 once (what the kernel is handed)."""
    a = np.broadcast_to(np.asarray(sd, F32).astype(np.float64)[:2], (B, 2)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, -1)[:, :2]
    return a.astype(F32)


def offset(mu, u, B):
    """u0 out_mu [B, 2] fp64: what the physical velocity holds beside a x."""
    uu = np.ones((B, 2)) if u is None else np.asarray(u, F32).astype(np.float64).reshape(B, -1)[:, :2]
    return uu * np.asarray(mu, F32).astype(np.float64).reshape(-1)[:2][None]


# ---- the arithmetic, held once; every function keeps the dtype it is given ---------------------------------------------------------------
def _box(g, r):
    """THE ORDER's box sums: g [..., H, W] -> [..., H - 2 r, W - 2 r], the row pass and then the column pass from the centre outwards."""
    Ww = g.shape[-1]
    s = g[..., r:Ww - r]
    for j in range(1, r + 1):
        s = (s + g[..., r - j:Ww - r - j]) + g[..., r + j:Ww - r + j]
    Hh = s.shape[-2]
    t = s[..., r:Hh - r, :]
    for j in range(1, r + 1):
        t = (t + s[..., r - j:Hh - r - j, :]) + s[..., r + j:Hh - r + j, :]
    return t


def _boxmean(g, r):
    """The box MEAN by plain slicing (the definition's): g [..., H, W] -> [..., H - 2 r, W - 2 r]."""
    Hh, Ww = g.shape[-2:]
    w = 2 * r + 1
    tot = 0.0
    for i in range(w):
        for j in range(w):
            tot = tot + g[..., i:Hh - 2 * r + i, j:Ww - 2 * r + j]
    return tot / float(w * w)


def _stencils(G, mag=False):
    """(Sx G, Sy G) on the interior of G [..., h, w] -> [..., h - 2, w - 2], in THE ORDER; mag: every subtraction an addition."""
    h, w = G.shape[-2:]
    c = lambda i, j: G[..., 1 + i:h - 1 + i, 1 + j:w - 1 + j]                 # noqa: E731
    if mag:
        return (((c(-1, 1) + c(-1, -1)) + 2 * (c(0, 1) + c(0, -1))) + (c(1, 1) + c(1, -1)),
                ((c(1, -1) + c(-1, -1)) + 2 * (c(1, 0) + c(-1, 0))) + (c(1, 1) + c(-1, 1)))
    return (((c(-1, 1) - c(-1, -1)) + 2 * (c(0, 1) - c(0, -1))) + (c(1, 1) - c(1, -1)),
            ((c(1, -1) - c(-1, -1)) + 2 * (c(1, 0) - c(-1, 0))) + (c(1, 1) - c(-1, 1)))


def _ctr(g):
    return g[..., 1:-1, 1:-1]


def terms(fu, fv, w, kx=None, ky=None, mag=False):
    """The un-normalised quantities of one width in THE ORDER, in the dtype of fu, fv [..., H, W] -> (A, B, Pi_s, Q_uu, Q_uv, Q_vv) on
    the valid region [..., H - 2 r - 2, W - 2 r - 2] (Pi_s None without kx, ky: the int64 reference).  mag: fu, fv are magnitudes and
    every subtraction is an addition: (MA, MB, MP, MQ_uu, MQ_uv, MQ_vv)."""
    r = w // 2
    N = fu.dtype.type(w * w)
    su, sv, suu, suv, svv = [_box(g, r) for g in (fu, fv, fu * fu, fu * fv, fv * fv)]
    cu, cv = _ctr(su), _ctr(sv)
    if mag:
        quu, quv, qvv = N * _ctr(suu) + cu * cu, N * _ctr(suv) + cu * cv, N * _ctr(svv) + cv * cv
    else:
        quu, quv, qvv = N * _ctr(suu) - cu * cu, N * _ctr(suv) - cu * cv, N * _ctr(svv) - cv * cv
    (sxu, syu), (sxv, syv) = _stencils(su, mag), _stencils(sv, mag)
    A, B = quu * sxu + quv * sxv, quv * syu + qvv * syv
    pi = None
    if kx is not None:
        pi = A * kx + B * ky
        pi = pi if mag else -pi
    return A, B, pi, quu, quv, qvv


def _embed(v, w, hw, fill=np.nan):
    """A valid-region array [..., H - 2 r - 2, W - 2 r - 2] -> the whole field, `fill` outside."""
    r = w // 2
    out = np.full(v.shape[:-2] + tuple(hw), fill, dtype=v.dtype)
    out[..., r + 1:hw[0] - 1 - r, r + 1:hw[1] - 1 - r] = v
    return out


# ---- 1: the float32 mirror and the int64 reference ---------------------------------------------------------------------------------------
def mirror_terms(x, a, widths, kk):
    """One step's 7 terms per width in float32.  x [R, B, C, H, W], a [B, 2], kk [L, 2] float32 -> [R, B, L, 7, H, W] float32, NaN at
    the invalid pixels."""
    x, a, kk = np.asarray(x), np.asarray(a), np.asarray(kk)
    assert x.dtype == F32 and a.dtype == F32 and kk.dtype == F32
    hw = x.shape[-2:]
    fu, fv = a[None, :, 0, None, None] * x[:, :, 0], a[None, :, 1, None, None] * x[:, :, 1]
    out = []
    for l, w in enumerate(widths):
        A, B, pi, quu, quv, qvv = terms(fu, fv, w, kk[l, 0], kk[l, 1])
        t = np.stack([A, B, pi * pi, (pi < 0).astype(F32), quu, quv, qvv], axis=2)
        assert t.dtype == F32
        out.append(_embed(t, w, hw))
    return np.stack(out, axis=2)


def mirror(xs, a, widths, kk, timed):
    """The state after every step: xs [steps, R, B, C, H, W] -> list of [R, B, L, 7, HW] float32 (None before the first timed step)."""
    raw, snaps = None, []
    for t in range(xs.shape[0]):
        if t in timed:
            term = mirror_terms(xs[t], a, widths, kk)
            raw = term if raw is None else raw + term
            assert raw.dtype == F32
        snaps.append(None if raw is None else raw.reshape(raw.shape[:4] + (-1,)).copy())
    return snaps


def int_reference(xs, widths, timed, planes):
    """Integer data, a = 1, 8 dx = 8 dy = 1: the sums of A, B, [A + B > 0] (the sign of Pi_s, exact while |A|, |B| < 2^23) and Q in
    int64 -> [R, B, L, 7, HW] int64 (plane 2 is not an integer: left 0).  planes: "Q" asserts the maxima of the Q planes only (any
    width, |x| <= 2, T <= 3), "AB" those of every plane (widths <= 5, |x| <= 1, T <= 8)."""
    x = np.asarray(xs)[list(timed)].astype(np.int64)
    hw = x.shape[-2:]
    out = []
    for w in widths:
        A, B, _, quu, quv, qvv = terms(x[:, :, :, 0], x[:, :, :, 1], w)
        assert max(np.abs(v).max() for v in (quu, quv, qvv)) * len(timed) < 2 ** 24
        r = w // 2
        assert (w * w) * _box(x[:, :, :, 0] ** 2, r).max() < 2 ** 24          # N Sg_uu itself is exact
        if planes == "AB":
            assert max(np.abs(A).max(), np.abs(B).max()) < 2 ** 23 and max(np.abs(A).max(), np.abs(B).max()) * len(timed) < 2 ** 24
        t = np.stack([A.sum(0), B.sum(0), 0 * A.sum(0), (A + B > 0).sum(0), quu.sum(0), quv.sum(0), qvv.sum(0)], axis=2)
        out.append(_embed(t, w, hw, fill=0))
    out = np.stack(out, axis=2)
    assert out.dtype == np.int64
    return out.reshape(out.shape[:4] + (-1,))


# ---- 2: the fp64 references -------------------------------------------------------------------------------------------------------------
def counts(w, k=0):
    """(c_Q, c_A, c_P) of the module docstring for a width w and k input roundings."""
    cA = 6 * w + 6 + 3 * k
    return 4 * w + 1 + 2 * k, cA, cA + 3


def direct(xs, a, widths, k64, timed, k=0, absf=None):
    """The fp64 direct sums of the 7 un-normalised terms from f = a x, their magnitude sums and the bound of the state.
    xs [steps, R, B, C, H, W], a [B, 2] fp32, k64 [L, 2] -> dict: sums, bound [R, B, L, 7, HW] (NaN at invalid pixels; plane 3's bound
    counts the steps whose sign is uncertain), mags: per width (sum MA, sum MB, sum MP^2, sum MQ x 3, sum MP) [R, B, L, 7, HW], T.
    absf = (|f_u|, |f_v|) [T, R, B, H, W] overrides the magnitudes of f (the physical velocity's, or inputs that are themselves
    uncertain by k u absf)."""
    x = np.asarray(xs, dtype=np.float64)[list(timed)]
    T = x.shape[0]
    hw = x.shape[-2:]
    a64 = np.asarray(a, dtype=np.float64)
    fu, fv = a64[None, None, :, 0, None, None] * x[:, :, :, 0], a64[None, None, :, 1, None, None] * x[:, :, :, 1]
    au, av = (np.abs(fu), np.abs(fv)) if absf is None else absf
    sums, bound, mags = [], [], []
    for l, w in enumerate(widths):
        kx, ky = float(k64[l, 0]), float(k64[l, 1])
        A, B, pi, quu, quv, qvv = terms(fu, fv, w, kx, ky)
        MA, MB, MP, mqa, mqb, mqc = terms(au, av, w, kx, ky, mag=True)
        cQ, cA, cP = counts(w, k)
        unsure = (np.abs(pi) <= cP * U24 * MP).sum(0).astype(np.float64)
        sums.append(_embed(np.stack([A.sum(0), B.sum(0), (pi * pi).sum(0), (pi < 0).sum(0).astype(np.float64), quu.sum(0), quv.sum(0),
                                     qvv.sum(0)], axis=2), w, hw))
        bound.append(_embed(np.stack([(T - 1 + cA) * U24 * MA.sum(0), (T - 1 + cA) * U24 * MB.sum(0), (T + 2 * cP) * U24 * (MP * MP).sum(0),
                                      unsure, (T - 1 + cQ) * U24 * mqa.sum(0), (T - 1 + cQ) * U24 * mqb.sum(0), (T - 1 + cQ) * U24 * mqc.sum(0)],
                                     axis=2), w, hw))
        mags.append(_embed(np.stack([MA.sum(0), MB.sum(0), (MP * MP).sum(0), MP.sum(0), mqa.sum(0), mqb.sum(0), mqc.sum(0)], axis=2), w, hw))
    flat = lambda v: np.stack(v, axis=2).reshape(v[0].shape[:2] + (len(widths), Q, -1))   # noqa: E731
    return {"sums": flat(sums), "bound": flat(bound), "mags": flat(mags), "T": T}


def definition(xs, a, off, widths, grid, timed, mut=None):
    """The reference by direct definition (module docstring).  xs [steps, R, B, C, H, W], a [B, 2] (fp32 table), off [B, 2] fp64 = u0
    out_mu -> dict of per-row fields: flux, tstd, back [R, B, L, H, W], sgs [R, B, L, 3, H, W], NaN at the invalid pixels.  mut: one
    deliberate mistake (the sensitivity test)."""
    x = np.asarray(xs, dtype=np.float64)[list(timed)]
    hw = x.shape[-2:]
    a64 = np.asarray(a, dtype=np.float64)
    U = a64[None, None, :, 0, None, None] * x[:, :, :, 0] + off[None, None, :, 0, None, None]
    V = a64[None, None, :, 1, None, None] * x[:, :, :, 1] + off[None, None, :, 1, None, None]
    dx, dy = (float(grid[1]), float(grid[0])) if mut == "dxdy" else (float(grid[0]), float(grid[1]))
    out = {"flux": [], "tstd": [], "back": [], "sgs": []}
    for w in widths:
        r = w // 2
        bm = lambda g: _boxmean(np.roll(g, 1, -1) if mut == "shift" else g, r)   # noqa: E731  ("shift": the box off by one pixel)
        bu, bv = bm(U), bm(V)
        tuu, tuv, tvv = bm(U * U) - bu * bu, bm(U * V) - bu * bv, bm(V * V) - bv * bv
        if mut == "nonorm":                                                  # the division by N^2 left out (of the box means' products)
            tuu, tuv, tvv = [t * float(w * w) ** 2 for t in (tuu, tuv, tvv)]
        (sxu, syu), (sxv, syv) = _stencils(bu), _stencils(bv)
        dxu, dyu, dxv, dyv = sxu / (8.0 * dx), syu / (8.0 * dy), sxv / (8.0 * dx), syv / (8.0 * dy)
        cross = _ctr(tuv) * (dyu if mut == "uv" else dyu + dxv)               # "uv": tau_uv counted once too few
        pi = -((_ctr(tuu) * dxu + cross) + _ctr(tvv) * dyv)
        if mut == "sign":
            pi = -pi
        out["flux"].append(_embed(pi.mean(0), w, hw))
        out["tstd"].append(_embed(pi.std(0), w, hw))
        out["back"].append(_embed((pi < 0).mean(0), w, hw))
        out["sgs"].append(_embed(np.stack([_ctr(tuu).mean(0), _ctr(tuv).mean(0), _ctr(tvv).mean(0)], axis=2), w, hw))
    return {key: np.stack(v, axis=2) for key, v in out.items()}


def restate(raw, T, widths, k64, hw, mag=False):
    """The finalize formulas in fp64 on a state raw [R, B, L, 7, HW] -> dict of per-row fields as definition() gives them.  mag: the
    same formulas on magnitudes with every subtraction an addition (tstd: the variance's magnitude)."""
    r = np.asarray(raw, dtype=np.float64).reshape(raw.shape[:4] + tuple(hw))
    if mag:
        r = np.abs(r)
    T = float(T)
    out = {"flux": [], "tstd": [], "back": [], "sgs": []}
    for l, w in enumerate(widths):
        kx, ky, Nn = float(k64[l, 0]), float(k64[l, 1]), float(w * w)
        pi = (r[:, :, l, 0] * kx + r[:, :, l, 1] * ky) / T
        pi = pi if mag else -pi
        var = r[:, :, l, 2] / T + pi * pi if mag else r[:, :, l, 2] / T - pi * pi
        out["flux"].append(pi)
        out["tstd"].append(var if mag else np.sqrt(np.where(var < 0, 0.0, var)))
        out["back"].append(r[:, :, l, 3] / T)
        out["sgs"].append(np.stack([r[:, :, l, 4 + i] / ((Nn * Nn) * T) for i in range(3)], axis=2))
    return {key: np.stack(v, axis=2) for key, v in out.items()}


def curves(rows, widths, hw):
    """Per-row fields -> (flux_curve, sgs_energy_curve) [B, R, L] fp64: the mean over each width's valid region."""
    fc, ec = [], []
    for l, w in enumerate(widths):
        m = valid_mask(w, hw)
        fc.append(rows["flux"][:, :, l][..., m].mean(-1))
        ec.append((0.5 * (rows["sgs"][:, :, l, 0] + rows["sgs"][:, :, l, 2]))[..., m].mean(-1))
    return np.stack(fc, axis=-1).transpose(1, 0, 2), np.stack(ec, axis=-1).transpose(1, 0, 2)


# ---- 3: the bounds ----------------------------------------------------------------------------------------------------------------------
def _share(err, bound, what):
    assert np.array_equal(np.isnan(err), np.isnan(bound)), "%s: NaN pattern" % what
    fin = np.isfinite(bound)
    share = float(np.where(err[fin] > 0, err[fin] / np.maximum(bound[fin], 1e-300), 0.0).max()) if fin.any() else 0.0
    assert share <= 1.0, "%s: off by %.3g of its bound" % (what, share)
    return share


def check_raw(raw, ref, what, planes=range(Q)):
    """raw [R, B, L, 7, HW] float32 (NaN where never written) inside its counted bound of the fp64 direct sums; NaN exactly at the
    invalid pixels -> the worst share reached."""
    assert raw.dtype == F32 and raw.shape == ref["sums"].shape, what
    worst = 0.0
    for q in planes:
        worst = max(worst, _share(np.abs(raw[:, :, :, q].astype(np.float64) - ref["sums"][:, :, :, q]), ref["bound"][:, :, :, q],
                                  "%s plane %d" % (what, q)))
    return worst


def same_raw_bounds(raw, T, widths, k64, hw):
    """The absolute bounds (without the output's u |ref|) of the restatement against the device on the same raw: C_FIN e mag, the
    temporal std through the square root's two inequalities -> dict as restate()."""
    mg = restate(raw, T, widths, k64, hw, mag=True)
    ref = restate(raw, T, widths, k64, hw)
    b = {key: C_FIN * E53 * v for key, v in mg.items()}
    dq = b["tstd"]
    with np.errstate(divide="ignore", invalid="ignore"):
        b["tstd"] = np.minimum(np.sqrt(dq), np.where(ref["tstd"] > 0, dq / np.maximum(ref["tstd"], 1e-300), np.inf))
    return b, mg


def definition_bounds(ref, dmag, rows, T, widths, k64, hw):
    """The absolute bounds of the published fields against the definition `rows`: ref = direct() of the kernel's f (the state's bounds
    and magnitudes), dmag = direct() with the magnitudes of the physical velocity (the definition's own roundings) -> dict."""
    shape = ref["bound"].shape[:3] + tuple(hw)
    bd = lambda q: ref["bound"][:, :, :, q].reshape(shape)                    # noqa: E731
    mg = lambda d, q: d["mags"][:, :, :, q].reshape(shape)                    # noqa: E731
    T = float(T)
    b = {"flux": [], "tstd": [], "back": [], "sgs": []}
    for l, w in enumerate(widths):
        kx, ky, Nn = float(k64[l, 0]), float(k64[l, 1]), float(w * w)
        own = C_DEF * E53 * (mg(dmag, 0)[:, :, l] * kx + mg(dmag, 1)[:, :, l] * ky) / T
        dpi = (bd(0)[:, :, l] * kx + bd(1)[:, :, l] * ky) / T + own
        pimag = (mg(ref, 0)[:, :, l] * kx + mg(ref, 1)[:, :, l] * ky) / T
        dq = bd(2)[:, :, l] / T + 2.0 * pimag * dpi + dpi * dpi + C_DEF * E53 * mg(dmag, 2)[:, :, l] / T
        with np.errstate(divide="ignore", invalid="ignore"):
            ts = rows["tstd"][:, :, l]
            b["tstd"].append(np.minimum(np.sqrt(dq), np.where(ts > 0, dq / np.maximum(ts, 1e-300), np.inf)))
        b["flux"].append(dpi)
        # a step of the definition's counts differently only where its own Pi is within the bound of zero: direct()'s count of the
        # unsure steps (the definition's own roundings are far inside it)
        b["back"].append(bd(3)[:, :, l] / T)
        b["sgs"].append(np.stack([(bd(4 + i)[:, :, l] + C_DEF * E53 * mg(dmag, 4 + i)[:, :, l]) / ((Nn * Nn) * T) for i in range(3)], axis=2))
    return {key: np.stack(v, axis=2) for key, v in b.items()}


def field_mags(ref, T, widths, k64, hw):
    """The operand magnitudes of the published fields from direct()'s magnitude sums (the count's magnitude is T) -> dict as restate()."""
    m = ref["mags"].copy()
    m[:, :, :, 3] = np.where(np.isnan(m[:, :, :, 3]), np.nan, float(T))
    return restate(m, T, widths, k64, hw, mag=True)


def check_fields(got, rows, bnd, mags, S, widths, hw, what, per_member=True):
    """The published fields `got` (numpy, fp32) against the per-row reference `rows` with the per-row absolute bounds `bnd` and the
    operand magnitudes `mags` (restate(mag=True)): |got - ref| <= u |ref| + bnd (+ Welford's (C_FIN + 4 S) e mag for a mean or a std
    over the members, the std's variance through the square root's two inequalities as tests/budget_cases.py); NaN exactly at the
    invalid pixels of each width -> the worst share reached."""
    worst = 0.0
    cw = (C_FIN + 4 * S) * E53
    names = {"flux": ("flux_mean", "flux_std", "target_flux"), "tstd": ("flux_tstd_mean", None, "target_flux_tstd"),
             "back": ("backscatter_mean", "backscatter_std", "target_backscatter"), "sgs": ("sgs_mean", "sgs_std", "target_sgs")}
    for key, (nm, ns, nt) in names.items():
        r, b, m = rows[key], bnd[key], mags[key]
        if key == "tstd":
            m = np.sqrt(m)                                                   # (restate(mag=True) gives the variance's magnitude)
        mmax, bmax = m[:-1].max(0), b[:-1].max(0)
        ref = r[:-1].mean(0)
        g = got[nm].astype(np.float64)
        assert got[nm].dtype == F32 and g.shape == ref.shape, (what, nm, g.shape, ref.shape)
        worst = max(worst, _share(np.abs(g - ref), U24 * np.abs(ref) + bmax + cw * mmax, "%s %s" % (what, nm)))
        ref = r[-1]
        worst = max(worst, _share(np.abs(got[nt].astype(np.float64) - ref), U24 * np.abs(ref) + b[-1], "%s %s" % (what, nt)))
        if ns is not None:
            ref = r[:-1].std(0)
            with np.errstate(divide="ignore", invalid="ignore"):
                dq = 2.0 * cw * mmax * mmax
                bstd = np.where(np.isnan(ref), np.nan, np.minimum(np.sqrt(dq), np.where(ref > 0, dq / np.maximum(ref, 1e-300), np.inf)))
            worst = max(worst, _share(np.abs(got[ns].astype(np.float64) - ref), U24 * np.abs(ref) + bmax + cw * mmax + bstd, "%s %s" % (what, ns)))
    if per_member and "member_flux" in got:
        ref = np.moveaxis(rows["flux"][:-1], 0, 1)
        worst = max(worst, _share(np.abs(got["member_flux"].astype(np.float64) - ref), U24 * np.abs(ref) + np.moveaxis(bnd["flux"][:-1], 0, 1),
                                  "%s member_flux" % what))
    # the curves: the mean over the valid region moves by at most the mean of the bounds; n additions in fp64
    fc, ec = curves(rows, widths, hw)
    bf, be = curves(bnd, widths, hw)                                          # (|d(uu + vv) / 2| <= (b_uu + b_vv) / 2)
    mf, me = curves(mags, widths, hw)
    npx = np.array([valid_mask(w, hw).sum() for w in widths], dtype=np.float64)
    for name, ref, b, m in (("flux_curve", fc, bf, mf), ("sgs_energy_curve", ec, be, me)):
        g = got[name].astype(np.float64)
        assert got[name].dtype == F32 and g.shape == ref.shape, (what, name, g.shape, ref.shape)
        worst = max(worst, _share(np.abs(g - ref), U24 * np.abs(ref) + b + (C_FIN + npx) * E53 * m, "%s %s" % (what, name)))
    for l, w in enumerate(widths):
        m = valid_mask(w, hw)
        for name in FIELD_KEYS[:11] + (("member_flux",) if "member_flux" in got else ()):
            v = np.moveaxis(got[name], 2 if name == "member_flux" else 1, 0)[l]
            assert np.isnan(v[..., ~m]).all() and np.isfinite(v[..., m]).all(), "%s %s: the NaN pattern of width %d" % (what, name, w)
    return worst


# ---- the cases' references, computed once per case ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_refs(i):
    """Case i of the table: inputs, tables, the mirror's snapshots, the direct sums and the definition."""
    S, B, hw, widths, padded, T = CASES[i]
    xs, sd, mu, u = real_inputs(S, B, hw, T, 100 + i)
    a, off, k64, timed = scales(sd, u, B), offset(mu, u, B), factors(widths, GRID), range(1, T + 1)
    U = [np.abs(a.astype(np.float64)[None, None, :, c, None, None] * xs[1:, :, :, c].astype(np.float64) + off[None, None, :, c, None, None])
         for c in (0, 1)]
    return dict(S=S, B=B, hw=hw, widths=widths, T=T, xs=xs, a=a, off=off, k64=k64, timed=timed,
                snaps=mirror(xs, a, widths, k64.astype(F32), timed), ref=direct(xs, a, widths, k64, timed),
                dmag=direct(xs, a, widths, k64, timed, absf=tuple(U)), rows=definition(xs, a, off, widths, GRID, timed))


def check_against_definition(c, got, rows, what):
    bnd = definition_bounds(c["ref"], c["dmag"], rows, c["T"], c["widths"], c["k64"], c["hw"])
    mags = field_mags(c["ref"], c["T"], c["widths"], c["k64"], c["hw"])
    return check_fields(got, rows, bnd, mags, c["S"], c["widths"], c["hw"], what)


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
KAT_T, KAT_HW, KAT_GRID, KAT_WIDTHS = 3, (37, 39), (0.5, 0.25), (3, 9, 33)
KAT_U = np.array([[1.25, 1.25, 1.5625]], F32)
KAT_MU = np.array([0.4, -0.1, 0.25], F32)
KAT_K = 1                                                                    # the pad of the known answers: x is the analytic row rounded once


def kat_tables():
    sd = np.array(SD, F32)
    return scales(sd, KAT_U, 1), sd, KAT_MU, KAT_U


def _kat_rows(Uf, Vf, S):
    """Physical fields [H, W] -> xs [T + 1, S + 1, 1, 3, H, W] fp32 normalised rows, row r scaled by (1 + r / 4) through its
    amplitude (the caller's want follows); constant in time; the untimed step holds other values."""
    a, sd, mu, u = kat_tables()
    off = offset(mu, u, 1)
    amp = 1.0 + 0.25 * np.arange(S + 1)
    phys = np.zeros((KAT_T + 1, S + 1, 1, 3) + KAT_HW)
    phys[1:, :, 0, 0] = amp[None, :, None, None] * Uf[None, None]
    phys[1:, :, 0, 1] = amp[None, :, None, None] * Vf[None, None]
    phys[0] = 3.0
    x = phys.copy()
    x[:, :, :, 0] = (phys[:, :, :, 0] - off[0, 0]) / a.astype(np.float64)[0, 0]
    x[:, :, :, 1] = (phys[:, :, :, 1] - off[0, 1]) / a.astype(np.float64)[0, 1]
    return x.astype(F32), amp


def kat_strain(S=2):
    """Pure strain u = alpha x, v = -alpha y (x = w dx, y = h dy) -> (xs, want dict of per-row fields [R, 1, L, ...] on the whole field):
    tau_uu = alpha^2 dx^2 (w^2 - 1) / 12, tau_vv the same with dy, tau_uv = 0, Pi = -alpha^3 (w^2 - 1) (dx^2 - dy^2) / 12, backscatter 0
    or 1 by that sign, temporal std 0."""
    dx, dy = KAT_GRID
    al0 = 0.3
    xx = np.ones((KAT_HW[0], 1)) * (np.arange(KAT_HW[1]) * dx)[None]
    yy = (np.arange(KAT_HW[0]) * dy)[:, None] * np.ones((1, KAT_HW[1]))
    xs, amp = _kat_rows(al0 * xx, -al0 * yy, S)
    al = al0 * amp
    want = {"flux": [], "tstd": [], "back": [], "sgs": []}
    one = np.ones((S + 1, 1) + KAT_HW)
    for w in KAT_WIDTHS:
        c = (w * w - 1) / 12.0
        pi = -(al ** 3) * c * (dx * dx - dy * dy)
        want["flux"].append(pi[:, None, None, None] * one)
        want["tstd"].append(0.0 * one)
        want["back"].append((pi < 0).astype(np.float64)[:, None, None, None] * one)
        want["sgs"].append(np.stack([(al ** 2 * dx * dx * c)[:, None, None, None] * one, 0.0 * one, (al ** 2 * dy * dy * c)[:, None, None, None] * one],
                                    axis=2))
    return xs, {key: np.stack(v, axis=2) for key, v in want.items()}


def kat_ramp(S=2):
    """Diagonal ramp u = v = g (i + j) in pixel indices -> (xs, want): all three tau = g^2 (w^2 - 1) / 6,
    Pi = -g^3 (w^2 - 1) (1 / dx + 1 / dy) / 3 < 0: backscatter 1, temporal std 0."""
    dx, dy = KAT_GRID
    g0 = 0.05
    ij = np.arange(KAT_HW[0])[:, None] + np.arange(KAT_HW[1])[None].astype(np.float64)
    xs, amp = _kat_rows(g0 * ij, g0 * ij, S)
    g = g0 * amp
    want = {"flux": [], "tstd": [], "back": [], "sgs": []}
    one = np.ones((S + 1, 1) + KAT_HW)
    for w in KAT_WIDTHS:
        c = float(w * w - 1)
        want["flux"].append((-(g ** 3) * c * (1.0 / dx + 1.0 / dy) / 3.0)[:, None, None, None] * one)
        want["tstd"].append(0.0 * one)
        want["back"].append(one.copy())
        want["sgs"].append(np.stack([(g ** 2 * c / 6.0)[:, None, None, None] * one] * 3, axis=2))
    return xs, {key: np.stack(v, axis=2) for key, v in want.items()}


def check_known(rows, want, bnd, widths, hw, what, keys=("flux", "tstd", "back", "sgs")):
    """Per-row fields against the analytic values inside u |want| + bnd, on every width's valid region -> the worst share."""
    worst = 0.0
    for key in keys:
        for l, w in enumerate(widths):
            m = valid_mask(w, hw)
            r, v, b = rows[key][:, :, l][..., m], want[key][:, :, l][..., m], bnd[key][:, :, l][..., m]
            worst = max(worst, _share(np.abs(r - v), U24 * np.abs(v) + b, "%s %s width %d" % (what, key, w)))
    return worst
