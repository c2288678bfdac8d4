"""Case tables, the float32 mirror of the raw state, the fp64 reference by direct definition, the fp64 host restatement of the shift
formulas and the counted rounding bounds of the ensemble TKE budget (csrc/tmg_budget.hip, tmg_ops.EnsembleBudget), shared by
tests/test_budget_cpu.py (no device) and tests/test_budget_gpu.py.

Rows are the S members plus the target as row S.  a [B, 3] and m [B, 3, H, W] are the fp32 tables the kernel is handed, x the raw
normalised rows at the TIMED steps.

THE ORDER of the raw state (stated once here, once in the kernel's header comment), every operation a float32 operation of its own:
  d_c = fl(a_c fl(x_c - m_c)), c = 0, 1, 2 (u, v, p);  f = 0 outside the field
  Sx f = fl(fl(fl(f[h-1,w+1] - f[h-1,w-1]) + fl(2 fl(f[h,w+1] - f[h,w-1]))) + fl(f[h+1,w+1] - f[h+1,w-1]))
  Sy f = fl(fl(fl(f[h+1,w-1] - f[h-1,w-1]) + fl(2 fl(f[h+1,w] - f[h-1,w]))) + fl(f[h+1,w+1] - f[h-1,w+1]))
  terms 0..2: d_u, d_v, d_p;  3..5: fl(d_u d_u), fl(d_u d_v), fl(d_v d_v);  6..9: fl(fl(d_u d_u) d_u), fl(fl(d_u d_u) d_v),
  fl(fl(d_u d_v) d_v), fl(fl(d_v d_v) d_v);  10, 11: fl(d_p d_u), fl(d_p d_v);  12: fl(fl(Sx d_u Sx d_u) + fl(Sx d_v Sx d_v));  13: with Sy
  raw[row, b, q, p] = the first timed step's term, then fl(raw + term) per timed step, in step order.

The reference by direct definition (fp64, per row): d = a (x - m) exactly, u' = d - mean_t d formed explicitly at every timed step,
the products, triple products and squared stencil outputs of u' averaged over time, U = M + mean_t d_u, derivatives by slicing.  It
never goes through shifted raw sums.  The host restatement applies the kernel's shift formulas to a given raw state in fp64.  Both
hand their moments to assemble(), which holds the seven term formulas once:
  conv = -(U dx k + V dy k);  prod = -(uu dx U + uv (dy U + dx V) + vv dy V);  turb = -(dx (uuu + uvv) + dy (uuv + vvv)) / 2;
  pres = -(dx pu + dy pv) / rho;  visc = nu ((k[h,w+1] - 2 k + k[h,w-1]) / dx^2 + (k[h+1,w] - 2 k + k[h-1,w]) / dy^2);
  diss = -nu (gx / (64 dx^2) + gy / (64 dy^2));  resid = the sum of the six;  dx f = Sx f / (8 dx), dy f = Sy f / (8 dy)
NaN on the one-pixel frame.

The bounds (u = 2^-24, e = 2^-53).
  raw: an element after T timed steps has had T - 1 fp32 additions (the first step stores), each of relative error u on a partial sum
  of at most sum_t |term|, and every term carries its own roundings c_q, counted from one term:
    planes 0..2    d: the subtraction and the multiplication                                   2, + 1 for all second-order terms: C_LIN = 3
    planes 3..5, 10, 11   two factors d (2 each) and the product                                5, + 1:  C_PROD = 6
    planes 6..9    three factors d (2 each) and two products                                    8, + 1:  C_TRIPLE = 9
    planes 12, 13  with G = sum |weight| |d| over the stencil (weights 1, 2, 1): every d carries 2 roundings and passes one
                   subtraction and at most two additions (the doubling is exact), so |fl(S) - S| <= 5 u G; the square of a value of
                   magnitude <= G moves by 2 * 5 u G^2, its own rounding adds 1, the sum of the two squares 1:   12, + 1:  C_GRAD = 13
                   against the magnitude G_u^2 + G_v^2
    |raw - ref| <= (T - 1 + c_q) u sum_t |term|_q
  terms, same raw (device against the host restatement): both sides evaluate the same fp64 formula from the same raw.  The longest
  chain is resid through turb: raw / T (1), 3 D e (2), the difference (1), 2 D^3 (3), the sum (1), uuu + uvv (1), the stencil's five
  additions and its weights (6), the division (1), the sum of the two derivatives (1), five additions of resid (5): 22 roundings on
  each side, C_TERM = 48 >= 2 * 22 + second order.  mag is the same formula evaluated on magnitudes with every subtraction turned into
  an addition:          |got - ref| <= u |ref| + C_TERM e mag                                     (u: the output's rounding to fp32)
  The Welford mean over S members adds 4 roundings per member: c = (C_TERM + 4 S) e against max_members mag.  A std moves by at most
  what its values move by (the population std is 1-Lipschitz in the largest change of a value): c mag; and the variance q that Welford
  sums is itself off by dq = 2 c mag^2, which moves sqrt(q) by at most min(sqrt(dq), dq / std), since |sqrt(a) - sqrt(b)| <=
  |a - b| / sqrt(b) and <= sqrt|a - b|.
  terms, against the definition: every raw element is within eps = (T - 1 + C_GRAD) u of its magnitude sum A_q, every term is a
  polynomial of degree <= 3 in the raw elements, so it moves by at most ((1 + eps)^3 - 1) mag(A) <= 3.1 eps mag(A), with mag(A) the
  restatement on the magnitude sums; `pad` widens |d| by what the test's own inputs are uncertain by (in units of u), and two more
  roundings cover the tables a and m:     |got - ref| <= u |ref| + 3.1 (T + C_GRAD + 1) u mag(A) + C_TERM e mag(A)
The counts come from the arithmetic above, never from what the kernel gives; the tests print the share of the bound they reach.
Real test data stays in the normal fp32 range (|d| between 1e-6 and 1e2), so that no subnormal enters the mirror."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
E53 = 2.0 ** -53
C_LIN, C_PROD, C_TRIPLE, C_GRAD = 3, 6, 9, 13
C_RAW = np.array([C_LIN] * 3 + [C_PROD] * 3 + [C_TRIPLE] * 4 + [C_PROD] * 2 + [C_GRAD] * 2, dtype=np.float64)
C_TERM = 48
F32 = np.float32
Q = 14
TERMS = ("conv", "prod", "turb", "pres", "visc", "diss", "resid")
FIELD_KEYS = ("budget_mean", "budget_std", "target_budget", "stress_mean", "stress_std", "target_stress")
NEW_KEYS = FIELD_KEYS + ("member_budget", "budget_terms")

# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# H x W: 3x3 (one interior pixel); 5x7 (ragged, one scalar block); 4x260 (W % 4 == 0: the 16-byte path, 1040 pixels: two blocks of
# 1024) and 3x515 (scalar path, 1545 pixels: seven blocks of 256, rows that cross the blocks and are no multiple of 4).
HWS = [(3, 3), (5, 7), (4, 260), (3, 515)]
CHUNKINGS = {1: [(1,)], 3: [(3,), (1, 2)], 5: [(5,), (2, 2, 1), (1,) * 5]}
# (S, B, (H, W), padded, T timed steps); one untimed step comes first; padded: the rows are channel slices of a wider NaN-filled buffer
CASES = [
    (1, 1, HWS[0], False, 1), (3, 2, HWS[1], True, 2), (5, 1, HWS[2], False, 7), (5, 2, HWS[3], False, 2), (5, 1, HWS[3], True, 7),
    (3, 2, HWS[2], True, 1), (1, 2, HWS[1], False, 7), (3, 1, HWS[0], True, 2),
]
MAX_CASE = (1024, 1, (3, 4), False, 2)                                       # chunks (1024,) and (64,) * 16
SD = [1.7, 0.6, 2.5]
MU = [0.4, -0.1, 0.25]
FL = (0.5, 0.25, 0.01, 1.3)                                                  # dx != dy
FL_NU0 = (0.25, 0.5, 0.0, 1.0)


def fl_of(i):
    """The flow constants of case i: every third case runs with nu = 0."""
    return FL_NU0 if i % 3 == 2 else FL


@functools.lru_cache(maxsize=None)
def int_inputs(S, B, hw, T, seed):
    """Integer data -> (xs [T + 1, S + 1, B, 3, H, W] (row S: the target; step 0 untimed), m [B, 3, H, W]) float32; x in -3..3, m in
    -1..1, a = 1: |d| <= 4, |S d| <= 32, a term at most 2048 and T <= 8 steps keep every sum under 2^15: exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(-3, 4, (T + 1, S + 1, B, 3) + tuple(hw), generator=g)
    m = torch.randint(-1, 2, (B, 3) + tuple(hw), generator=g)
    return xs.float().numpy(), m.float().numpy()


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, hw, T, seed):
    """Gaussian rows about a smooth mean -> (xs [T + 1, S + 1, B, 3, H, W], m [B, 3, H, W] float32, sd [3], mu [3], u [B, 3])."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    m = 0.3 + 0.5 * torch.randn(B, 3, Hh, Ww, generator=g)
    xs = m[None, None] + 0.8 * torch.randn(T + 1, S + 1, B, 3, Hh, Ww, generator=g) + 0.2 * torch.randn(1, S + 1, B, 3, 1, 1, generator=g)
    u = 0.5 + torch.rand(B, 3, generator=g)
    return xs.numpy().astype(F32), m.numpy().astype(F32), np.array(SD, F32), np.array(MU, F32), u.numpy().astype(F32)


def scales(sd, u, B):
    """a [B, 3]: u out_std in fp64 from the fp32 factors, rounded to fp32 once (what the kernel is handed)."""
    a = np.broadcast_to(np.asarray(sd, F32).astype(np.float64), (B, 3)).copy()
    if u is not None:
        a = a * np.asarray(u, F32).astype(np.float64).reshape(B, 3)
    return a.astype(F32)


def phys_mean(a, m, u, mu):
    """M [B, 2, H, W] = a m + u out_mu in fp64 from the fp32 tables (m None: 0)."""
    B = a.shape[0]
    uu = np.ones((B, 3)) if u is None else np.asarray(u, F32).astype(np.float64).reshape(B, 3)
    M = (uu * np.asarray(mu, F32).astype(np.float64).reshape(1, 3))[:, :, None, None]
    if m is not None:
        M = M + a.astype(np.float64)[:, :, None, None] * np.asarray(m, F32).astype(np.float64)
    return np.ascontiguousarray(np.broadcast_to(M, (B, 3) + M.shape[2:])[:, :2])


# ---- 1: the float32 mirror --------------------------------------------------------------------------------------------------------------
def _win(f):
    """f [..., H, W] -> c(i, j) = f[h + i, w + j] with zeros outside the field."""
    Hh, Ww = f.shape[-2:]
    fp = np.pad(f, [(0, 0)] * (f.ndim - 2) + [(1, 1), (1, 1)])
    return lambda i, j: fp[..., 1 + i:1 + i + Hh, 1 + j:1 + j + Ww]


def _sx32(f):
    c, two = _win(f), F32(2)
    return ((c(-1, 1) - c(-1, -1)) + two * (c(0, 1) - c(0, -1))) + (c(1, 1) - c(1, -1))


def _sy32(f):
    c, two = _win(f), F32(2)
    return ((c(1, -1) - c(-1, -1)) + two * (c(1, 0) - c(-1, 0))) + (c(1, 1) - c(-1, 1))


def mirror_terms(x, a, m):
    """One step's 14 terms in float32, in THE ORDER of the module docstring.  x [R, B, 3, H, W], a [B, 3], m [B, 3, H, W] or None, all
    float32 -> [R, B, 14, H, W] float32."""
    x, a = np.asarray(x), np.asarray(a)
    assert x.dtype == F32 and a.dtype == F32 and (m is None or m.dtype == F32)
    t = x - (np.zeros_like(x[0]) if m is None else m)[None]
    d = a[None, :, :, None, None] * t
    du, dv, dp = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    uu, uv, vv = du * du, du * dv, dv * dv
    sxu, sxv, syu, syv = _sx32(du), _sx32(dv), _sy32(du), _sy32(dv)
    out = np.stack([du, dv, dp, uu, uv, vv, uu * du, uu * dv, uv * dv, vv * dv, dp * du, dp * dv,
                    sxu * sxu + sxv * sxv, syu * syu + syv * syv], axis=2)
    assert out.dtype == F32
    return out


def mirror(xs, a, m, timed):
    """The raw state after every step: xs [steps, R, B, 3, H, W] -> list of [R, B, 14, HW] float32 (None before the first timed step)."""
    raw, snaps = None, []
    for t in range(xs.shape[0]):
        if t in timed:
            term = mirror_terms(xs[t], a, m)
            raw = term if raw is None else raw + term
            assert raw.dtype == F32
        snaps.append(None if raw is None else raw.reshape(raw.shape[:3] + (-1,)).copy())
    return snaps


def int_reference(xs, m, timed):
    """Integer data, a = 1: the 14 sums in int64, summed directly -> [R, B, 14, HW] int64."""
    x = np.asarray(xs)[list(timed)].astype(np.int64)
    d = x - np.asarray(m).astype(np.int64)[None, None]
    du, dv, dp = d[:, :, :, 0], d[:, :, :, 1], d[:, :, :, 2]

    def st(f, horizontal):
        c = _win(f)
        if horizontal:
            return (c(-1, 1) - c(-1, -1)) + 2 * (c(0, 1) - c(0, -1)) + (c(1, 1) - c(1, -1))
        return (c(1, -1) - c(-1, -1)) + 2 * (c(1, 0) - c(-1, 0)) + (c(1, 1) - c(-1, 1))

    q = [du, dv, dp, du * du, du * dv, dv * dv, du ** 3, du * du * dv, du * dv * dv, dv ** 3, dp * du, dp * dv,
         st(du, True) ** 2 + st(dv, True) ** 2, st(du, False) ** 2 + st(dv, False) ** 2]
    out = np.stack([v.sum(0) for v in q], axis=2)
    assert out.dtype == np.int64 and np.abs(out).max() < 2 ** 24
    return out.reshape(out.shape[:3] + (-1,))


# ---- 2: the formulas, held once ----------------------------------------------------------------------------------------------------------
def _stencils(mag, mut=None):
    """(Sx, Sy) on the interior: f [..., H, W] -> [..., H - 2, W - 2]; mag: on magnitudes, every subtraction an addition."""
    sg = 1.0 if mag else -1.0

    def c(f, i, j):
        Hh, Ww = f.shape[-2:]
        return f[..., 1 + i:Hh - 1 + i, 1 + j:Ww - 1 + j]

    def sx(f):
        return ((c(f, -1, 1) + sg * c(f, -1, -1)) + 2.0 * (c(f, 0, 1) + sg * c(f, 0, -1))) + (c(f, 1, 1) + sg * c(f, 1, -1))

    def sy(f):
        return ((c(f, 1, -1) + sg * c(f, -1, -1)) + 2.0 * (c(f, 1, 0) + sg * c(f, -1, 0))) + (c(f, 1, 1) + sg * c(f, -1, 1))

    return (sx, sx if mut == "sy" else sy, c)


def assemble(mo, U, V, fl, mag=False, mut=None):
    """The seven terms from the central moments mo (dict of [..., H, W]; gx, gy on the interior [..., H - 2, W - 2]) and the mean
    velocity U, V [..., H, W] -> [..., 7, H, W] fp64, NaN on the frame.  mag: the same formulas on magnitudes, every subtraction an
    addition (the operand sums of the bounds).  mut: one deliberate mistake (the sensitivity test)."""
    dx, dy, nu, rho = [float(v) for v in fl]
    if mut == "dxdy":
        dx, dy = dy, dx
    sx, sy, c = _stencils(mag, mut)
    lead, sg = (1.0, 1.0) if mag else (-1.0, -1.0)
    ddx, ddy = (lambda f: sx(f) / (8.0 * dx)), (lambda f: sy(f) / (8.0 * dy))
    k = 0.5 * (mo["uu"] + mo["vv"])
    ctr = lambda f: c(f, 0, 0)                                                # noqa: E731
    uuv, uvv = (mo["uvv"], mo["uuv"]) if mut == "uuv" else (mo["uuv"], mo["uvv"])
    t = {}
    t["conv"] = lead * (ctr(U) * ddx(k) + ctr(V) * ddy(k))
    t["prod"] = lead * ((ctr(mo["uu"]) * ddx(U) + ctr(mo["uv"]) * (ddy(U) + ddx(V))) + ctr(mo["vv"]) * ddy(V))
    t["turb"] = lead * (1.0 if mut == "half" else 0.5) * (ddx(mo["uuu"] + uvv) + ddy(uuv + mo["vvv"]))
    t["pres"] = lead * ((ddx(mo["pu"]) + ddy(mo["pv"])) / rho)
    t["visc"] = nu * (((c(k, 0, 1) + sg * 2.0 * ctr(k)) + c(k, 0, -1)) / (dx * dx) + ((c(k, 1, 0) + sg * 2.0 * ctr(k)) + c(k, -1, 0)) / (dy * dy))
    t["diss"] = lead * (nu * (mo["gx"] / (64.0 * (dx * dx)) + mo["gy"] / (64.0 * (dy * dy))))
    if mut is not None and mut.startswith("sign:"):
        t[mut[5:]] = -t[mut[5:]]
    t["resid"] = ((((t["conv"] + t["prod"]) + t["turb"]) + t["pres"]) + t["visc"]) + t["diss"]
    out = np.full(U.shape[:-2] + (7,) + U.shape[-2:], np.nan)
    out[..., 1:-1, 1:-1] = np.stack([t[n] for n in TERMS], axis=-3)
    return out


def definition(xs, a, m, timed, M, fl, mut=None, pad=None):
    """The reference by direct definition.  xs [steps, R, B, 3, H, W], a [B, 3], m [B, 3, H, W] or None (fp32 tables), M [B, 2, H, W]
    fp64 -> dict: terms [R, B, 7, H, W], stress [R, B, 3, H, W] (uu, uv, vv), sums / mags [R, B, 14, HW] the fp64 direct sums of
    the 14 quantities and of their magnitudes (planes 12, 13 through G = sum |weight| |d|), T.  pad [T, R, B, 3, H, W] (optional)
    widens |d| in the magnitudes by pad * |.|-units the caller's inputs are uncertain by."""
    x = np.asarray(xs, dtype=np.float64)[list(timed)]
    T = x.shape[0]
    a64 = np.asarray(a, dtype=np.float64)[None, None, :, :, None, None]
    d = a64 * (x - (0.0 if m is None else np.asarray(m, dtype=np.float64)[None, None]))
    sx, sy, _ = _stencils(False)
    du, dv, dp = d[:, :, :, 0], d[:, :, :, 1], d[:, :, :, 2]                  # [T, R, B, H, W]
    D = d.mean(0)                                                            # [R, B, 3, H, W]
    f = d - D[None]                                                          # u' formed explicitly at every step
    fu, fv, fp = f[:, :, :, 0], f[:, :, :, 1], f[:, :, :, 2]
    av = lambda v: v.mean(0)                                                 # noqa: E731
    mo = {"uu": av(fu * fu), "uv": av(fu * fv), "vv": av(fv * fv), "uuu": av(fu * fu * fu), "uuv": av(fu * fu * fv),
          "uvv": av(fu * fv * fv), "vvv": av(fv * fv * fv), "pu": av(fp * fu), "pv": av(fp * fv)}
    gu, gv = (du, dv) if mut == "gx" else (fu, fv)                           # "gx": the mean-gradient correction left out
    mo["gx"] = av(sx(gu) ** 2 + sx(gv) ** 2)
    mo["gy"] = av(sy(fu) ** 2 + sy(fv) ** 2)
    U, V = M[None, :, 0] + D[:, :, 0], M[None, :, 1] + D[:, :, 1]
    out = {"terms": assemble(mo, U, V, fl, mut=mut), "stress": np.stack([mo["uu"], mo["uv"], mo["vv"]], axis=2), "T": T}
    # the direct fp64 sums of the 14 quantities, with zero padding as the kernel reads it, and of their magnitudes
    ad = np.abs(d) + (0.0 if pad is None else np.asarray(pad, dtype=np.float64))
    au, avv, ap = ad[:, :, :, 0], ad[:, :, :, 1], ad[:, :, :, 2]

    def full(fn, v):
        """An interior stencil on the zero-padded field -> the whole field."""
        return fn(np.pad(v, [(0, 0)] * (v.ndim - 2) + [(1, 1), (1, 1)]))

    sxm, sym, _ = _stencils(True)
    q = [du, dv, dp, du * du, du * dv, dv * dv, du * du * du, du * du * dv, du * dv * dv, dv * dv * dv, dp * du, dp * dv,
         full(sx, du) ** 2 + full(sx, dv) ** 2, full(sy, du) ** 2 + full(sy, dv) ** 2]
    qa = [au, avv, ap, au * au, au * avv, avv * avv, au * au * au, au * au * avv, au * avv * avv, avv * avv * avv, ap * au, ap * avv,
          full(sxm, au) ** 2 + full(sxm, avv) ** 2, full(sym, au) ** 2 + full(sym, avv) ** 2]
    R, B = d.shape[1], d.shape[2]
    out["sums"] = np.stack([v.sum(0) for v in q], axis=2).reshape(R, B, Q, -1)
    out["mags"] = np.stack([v.sum(0) for v in qa], axis=2).reshape(R, B, Q, -1)
    return out


def restate(raw, T, M, fl, hw, mag=False):
    """The kernel's shift formulas in fp64 on a raw state.  raw [R, B, 14, HW] (mag: magnitude sums, M's magnitude, every subtraction
    an addition) -> (terms [R, B, 7, H, W], stress [R, B, 3, H, W])."""
    r = np.asarray(raw, dtype=np.float64).reshape(raw.shape[:3] + tuple(hw))
    M = np.asarray(M, dtype=np.float64)
    if mag:
        r, M = np.abs(r), np.abs(M)
    sg = 1.0 if mag else -1.0
    e = [r[:, :, i] / float(T) for i in range(Q)]
    Du, Dv, Dp = e[0], e[1], e[2]
    mo = {"uu": e[3] + sg * Du * Du, "uv": e[4] + sg * Du * Dv, "vv": e[5] + sg * Dv * Dv,
          "uuu": (e[6] + sg * 3.0 * Du * e[3]) + 2.0 * Du * Du * Du,
          "uuv": ((e[7] + sg * 2.0 * Du * e[4]) + sg * Dv * e[3]) + 2.0 * Du * Du * Dv,
          "uvv": ((e[8] + sg * 2.0 * Dv * e[4]) + sg * Du * e[5]) + 2.0 * Du * Dv * Dv,
          "vvv": (e[9] + sg * 3.0 * Dv * e[5]) + 2.0 * Dv * Dv * Dv,
          "pu": e[10] + sg * Dp * Du, "pv": e[11] + sg * Dp * Dv}
    sx, sy, c = _stencils(mag)
    mo["gx"] = (c(e[12], 0, 0) + sg * sx(Du) ** 2) + sg * sx(Dv) ** 2
    mo["gy"] = (c(e[13], 0, 0) + sg * sy(Du) ** 2) + sg * sy(Dv) ** 2
    U, V = M[None, :, 0] + Du, M[None, :, 1] + Dv
    return assemble(mo, U, V, fl, mag=mag), np.stack([mo["uu"], mo["uv"], mo["vv"]], axis=2)


def outputs_from_rows(terms, stress):
    """Per-row terms [S + 1, B, 7, H, W] and stresses [S + 1, B, 3, H, W] -> the dict of the published fields (fp64): the mean and
    the population std over the members (rows 0 .. S - 1), the target's (row S), member_budget [B, S, 7, H, W]."""
    return {"budget_mean": terms[:-1].mean(0), "budget_std": terms[:-1].std(0), "target_budget": terms[-1],
            "stress_mean": stress[:-1].mean(0), "stress_std": stress[:-1].std(0), "target_stress": stress[-1],
            "member_budget": np.ascontiguousarray(np.moveaxis(terms[:-1], 0, 1))}


# ---- 3: the bounds ----------------------------------------------------------------------------------------------------------------------
def raw_bound(ref):
    """(T - 1 + c_q) u sum_t |term|_q for every element of raw [R, B, 14, HW]."""
    return (ref["T"] - 1 + C_RAW).reshape(1, 1, Q, 1) * U24 * ref["mags"]


def check_raw(raw, ref, what):
    """raw inside its counted bound of the fp64 direct sums -> the worst share reached."""
    assert raw.dtype == F32 and raw.shape == ref["sums"].shape and np.isfinite(raw).all(), what
    err, bound = np.abs(raw.astype(np.float64) - ref["sums"]), raw_bound(ref)
    share = float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())
    assert share <= 1.0, "%s: raw is off by %.3g of its bound" % (what, share)
    return share


def _share(err, bound, what):
    assert np.array_equal(np.isnan(err), np.isnan(bound)), "%s: NaN pattern" % what
    fin = np.isfinite(bound)
    share = float(np.where(err[fin] > 0, err[fin] / np.maximum(bound[fin], 1e-300), 0.0).max()) if fin.any() else 0.0
    assert share <= 1.0, "%s: off by %.3g of its bound" % (what, share)
    return share


def check_fields(got, rows, mags, S, what, rel=0.0, per_member=True):
    """The published fields `got` (numpy, fp32) against the per-row reference rows = (terms, stress) with the operand magnitudes
    mags = (terms, stress) of restate(mag=True): |got - ref| <= u |ref| + (rel + (C_TERM + 4 S) e) mag, the std through the square
    root's two inequalities (module docstring); NaN exactly on the frame of the terms -> the worst share reached."""
    ref = outputs_from_rows(*rows)
    mg = outputs_from_rows(*mags)
    c = rel + (C_TERM + 4 * S) * E53
    worst = 0.0
    for base, key in (("budget", 0), ("stress", 1)):
        mmax = mags[key][:-1].max(0)                                         # over the members
        for name, mag in ((base + "_mean", mmax), ("target_" + base, mags[key][-1])):
            g = got[name].astype(np.float64)
            assert got[name].dtype == F32 and g.shape == ref[name].shape, (what, name, g.shape)
            worst = max(worst, _share(np.abs(g - ref[name]), U24 * np.abs(ref[name]) + c * mag, "%s %s" % (what, name)))
        name = base + "_std"
        g, r = got[name].astype(np.float64), ref[name]
        lin = c * mmax                                                       # the members' values move by at most lin: std is 1-Lipschitz
        with np.errstate(divide="ignore", invalid="ignore"):
            dq = 2.0 * (C_TERM + 4 * S) * E53 * mmax * mmax                  # Welford's own roundings of the variance
            bstd = np.where(np.isnan(r), np.nan, np.minimum(np.sqrt(dq), np.where(r > 0, dq / np.maximum(r, 1e-300), np.inf)))
        worst = max(worst, _share(np.abs(g - r), U24 * np.abs(r) + lin + bstd, "%s %s" % (what, name)))
    if per_member and "member_budget" in got:
        g = got["member_budget"].astype(np.float64)
        worst = max(worst, _share(np.abs(g - ref["member_budget"]), U24 * np.abs(ref["member_budget"]) + c * mg["member_budget"],
                                  "%s member_budget" % what))
    frame = np.ones(got["budget_mean"].shape[-2:], dtype=bool)
    frame[1:-1, 1:-1] = False
    for name in ("budget_mean", "budget_std", "target_budget") + (("member_budget",) if "member_budget" in got else ()):
        assert np.isnan(got[name][..., frame]).all() and np.isfinite(got[name][..., ~frame]).all(), "%s %s: the NaN frame" % (what, name)
    for name in ("stress_mean", "stress_std", "target_stress"):
        assert np.isfinite(got[name]).all(), "%s %s" % (what, name)
    return worst


def rel_definition(T):
    """The relative weight of mag(A) in the bound against the definition: 3.1 (T + C_GRAD + 1) u."""
    return 3.1 * (T + C_GRAD + 1) * U24


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
KAT_T, KAT_HW, KAT_FL = 8, (6, 9), (0.5, 0.25, 0.02, 1.3)
KAT_U = np.array([[1.25, 1.25, 1.5625]], F32)


def kat_tables():
    """-> (a [1, 3] fp32, sd, mu, u): out_mu = 0, so that the physical value of a normalised x is a x."""
    sd, mu = np.array(SD, F32), np.zeros(3, F32)
    return scales(sd, KAT_U, 1), sd, mu, KAT_U


def kat_shear(S=3):
    """A uniform mean shear U = s y with spatially uniform fluctuations u' = alpha_r cos(theta_t), v' = beta_r cos(theta_t) over one
    whole period of KAT_T steps (one untimed step first).  -> (xs [T + 1, S + 1, 1, 3, H, W] fp32, m fp32, want [S + 1, 1, 7, H, W]): prod =
    -alpha beta s / 2, every other term 0."""
    a, _, _, _ = kat_tables()
    Hh, Ww = KAT_HW
    s = 0.7
    yy = (np.arange(Hh, dtype=np.float64) * KAT_FL[1])[:, None] * np.ones((1, Ww))
    th = 2 * np.pi * np.arange(KAT_T) / KAT_T
    al, be = 0.5 + 0.25 * np.arange(S + 1), 0.8 - 0.1 * np.arange(S + 1)
    phys = np.zeros((KAT_T + 1, S + 1, 1, 3, Hh, Ww))
    phys[1:, :, 0, 0] = (s * yy)[None, None] + al[None, :, None, None] * np.cos(th)[:, None, None, None]
    phys[1:, :, 0, 1] = be[None, :, None, None] * np.cos(th)[:, None, None, None]
    phys[0] = 3.0                                                            # the untimed step: never read
    mean = np.zeros((1, 3, Hh, Ww))
    mean[0, 0] = s * yy
    a64 = a.astype(np.float64)[None, None, :, :, None, None]
    want = np.zeros((S + 1, 1, 7, Hh, Ww))
    want[:, 0, 1] = (-al * be * s / 2)[:, None, None]
    want[:, 0, 6] = want[:, 0, 1]
    return (phys / a64).astype(F32), (mean / a64[0, 0]).astype(F32), want


def kat_wave(S=2):
    """u' = alpha_r cos(theta_t) sin(kappa x), v' = 0, no mean flow.  -> (xs, m, want [S + 1, 1, 7, H, W]): diss = -nu alpha^2 kd^2
    cos^2(kappa x) / 2 with kd = sin(kappa dx) / dx the stencil's own wavenumber; visc = nu times the second difference of
    k = alpha^2 sin^2(kappa x) / 4; every other term 0 (resid = visc + diss)."""
    a, _, _, _ = kat_tables()
    Hh, Ww = KAT_HW
    dx, dy, nu, _ = KAT_FL
    kap = 1.1
    xx = np.ones((Hh, 1)) * (np.arange(Ww, dtype=np.float64) * dx)[None]
    th = 2 * np.pi * np.arange(KAT_T) / KAT_T
    al = 0.6 + 0.3 * np.arange(S + 1)
    phys = np.zeros((KAT_T + 1, S + 1, 1, 3, Hh, Ww))
    phys[1:, :, 0, 0] = al[None, :, None, None] * np.cos(th)[:, None, None, None] * np.sin(kap * xx)[None, None]
    phys[0] = -2.0
    a64 = a.astype(np.float64)[None, None, :, :, None, None]
    kd = np.sin(kap * dx) / dx
    kf = lambda x: np.sin(kap * x) ** 2 / 4                                  # noqa: E731
    want = np.zeros((S + 1, 1, 7, Hh, Ww))
    want[:, 0, 5] = -nu * (al ** 2)[:, None, None] * kd * kd * (np.cos(kap * xx) ** 2)[None] / 2
    want[:, 0, 4] = nu * (al ** 2)[:, None, None] * ((kf(xx + dx) - 2 * kf(xx) + kf(xx - dx)) / (dx * dx))[None]
    want[:, 0, 6] = want[:, 0, 4] + want[:, 0, 5]
    return (phys / a64).astype(F32), np.zeros((1, 3, Hh, Ww), F32), want


def kat_pad(xs, m, a):
    """What a known-answer field is uncertain by, in units of u: the fed row and the mean plane are the analytic ones rounded to
    fp32, so d = a (x - m) is off by at most u a (|x| + |m|) -> pad [T, R, B, 3, H, W] for definition(pad=...) over the timed steps
    1 .. T."""
    a64 = a.astype(np.float64)[None, None, :, :, None, None]
    return a64 * (np.abs(xs[1:].astype(np.float64)) + np.abs(m.astype(np.float64))[None, None])


def check_known(terms, want, magt, T, what, rel_extra=0.0):
    """Per-row terms [R, B, 7, H, W] against the analytic values inside u |want| + (rel_definition(T) + rel_extra) mag(A) + C_TERM e mag(A)."""
    inner = (slice(None),) * 3 + (slice(1, -1), slice(1, -1))
    err = np.abs(terms[inner] - want[inner])
    bound = U24 * np.abs(want[inner]) + (rel_definition(T) + rel_extra + C_TERM * E53) * magt[inner]
    return _share(err, bound, what)
