"""Case tables, the float32 mirror of the state, the same scheme in fp64, the int64 reference on integer data, the fp64 host
restatement of the finalize formulas and the counted rounding bounds of the ensemble's Lagrangian transport (csrc/tmg_lagr.hip,
tmg_ops.EnsembleTransport), shared by tests/test_transport_cpu.py (no device) and tests/test_transport_gpu.py.

Rows are the S members plus the target as row S.  a, o [B, 2] are the fp32 tables the kernel is handed, x the raw normalised rows.
THE DEFINITIONS are stated once in include/tmglow_hip_lagr.h; scheme() below follows them operation by operation, in the float
type it is handed: float32 is the mirror (the same bits as the device), float64 the reference scheme.  lattice = (Gh, Gw, oy, ox, sy,
sx); particle p = i Gw + j sits on pixel (oy + i sy, ox + j sx); positions are (px, py) = (w, h).

The integer reference.  On spatially uniform integer velocities the bilinear value is the velocity itself and, for n = substeps a
power of two, every operation of the scheme is exact in fp32.  int_reference() carries the positions as int64 numerators over
D = 2 n^2: with v0, v1 the velocities of the previous and of the current timed step, n k1 = n v0 + j (v1 - v0), n k2 = n v0 +
(j + 1) (v1 - v0), the predictor adds 2 n k1 and the corrector n k1 + n k2 to the numerator.

The bound of the mirror against the fp64 scheme (u = 2^-24), per coordinate.  X bounds |px|, |py| (max(H, W)), Vm bounds
|a y| + |o| over the case's rows, G is the largest bilinear slope of the case's converted planes: the largest difference of two
horizontally adjacent values plus the largest of two vertically adjacent ones, a Lipschitz constant of the interpolated velocity in
the maximum norm, h = 1 / n.  One velocity evaluation in fp32 at the fp32 position differs from the fp64 one at the fp64 position by
at most G delta + C_K u Vm, C_K = 26, counted:
  the conversion fl(fl(a y) + o)                                            2 roundings of at most Vm
  fx, fy (one subtraction each), felt through a slope of at most 2 Vm       2 * 2
  a bilinear value: (difference, product, sum) for the row, then for the column: 6 roundings of at most 2 Vm       12
                    => 18 per time level, and the two levels enter with weights that sum to 1                      18
  the interpolation in time: difference, product, sum, of at most 2 Vm      6
  s_j rounded to fp32, times |v1 - v0| <= 2 Vm                              2
With rho = C_K u Vm a Heun step takes an error delta to
  delta* = delta (1 + hG) + h rho + 2 u h Vm + u X                (h rounded, the product, the sum)
  delta' = delta + (h / 2) (G delta + rho + G delta* + rho) + 3 u h Vm + u X      (k1 + k2, hh rounded, the product; the sum)
         = delta (1 + hG + (hG)^2 / 2) + u [X (1 + hG / 2) + h Vm (C_K (1 + hG / 2) + 3 + hG)]
and delta = 0 at the seeds, which are integers.  position_bound() evaluates this recursion; the fp64 scheme's own roundings
(2^-53) are covered by counting fx and fy, which are exact.  For that comparison the inputs keep, in the fp64 scheme, every
particle at least 2^-10 pixel (far more than any bound here) from the frame at every substep, so both schemes have every particle
alive; bound_case() builds such inputs and the CPU file asserts the property.

The bounds of the finalize outputs against restate() on the same state (e = 2^-53): both sides evaluate the same fp64 formulas, so
every + - * is the same IEEE operation; the counts bound the operations a library may round differently (division, sqrt, log: 2 e
each, generously) and, conservatively, every other one as well:
  X = px dx (1); F = (X1 - X2) / den: the difference (1, of magnitude |X1| + |X2|), den (2), the division (2): C_F = 7 relative to
  Fm = (|X1| + |X2|) / den;  a square moves by 2 C_F and is rounded (1), the sum of two (1): C11, C12, C22 within C_C = 16 of their
  magnitude sums;  tr / 2 (1), hd (2), hd^2 + C12^2 (2 (C_C + 2) + 2), the sqrt halves the relative error (+ 2), lam (1):
  C_LAM = 40 relative to lam_mag (the formula on magnitudes);  ln lam moves by C_LAM e lam_mag / lam and its own 2 e |ln lam|, the
  division by 2 T_int adds 2 e:  |ftle err| <= e (C_LAM lam_mag / lam + 4 |ln lam|) / (2 T_int)
  disp = (px - px0) d: C_DISP = 2;  res_time = counter step_dt: 1;  the distance sqrt(ex^2 + ey^2): ex within 2 e (|X| + |XT|):
  |dist err| <= e (4 (|X| + |XT| + |Y| + |YT|) + 4 dist)
  Welford over S members adds 4 roundings per member of the largest magnitude; a std moves by what its values move by and by
  min(sqrt(dq), dq / std), dq the change of the variance (budget_cases.check_fields has the same form).
The counts come from the arithmetic above, never from what the kernel gives."""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
E53 = 2.0 ** -53
F32 = np.float32
C_K = 26
C_LAM = 40
FRAME_MARGIN = 2.0 ** -10

# ---- case tables ------------------------------------------------------------------------------------------------------------------------
# H x W and the seeds' stride: 3x3 stride 1 (every pixel a seed, the frame included); 5x7 stride (2, 3) (the lattice does not divide
# the field); 4x260 (W % 4 == 0: the 16-byte store path; 1040 pixels: two store blocks of 1024; 2 x 130 = 260 particles: two advect
# blocks) and 3x515 stride (1, 1) (scalar store path, 1545 pixels: seven store blocks; 1545 particles: seven advect blocks).
FIELDS = [((3, 3), (1, 1)), ((5, 7), (2, 3)), ((4, 260), (2, 2)), ((3, 515), (1, 1))]
CHUNKINGS = {1: [(1,)], 3: [(3,), (1, 2)], 5: [(5,), (2, 2, 1), (1,) * 5]}
# (S, B, field, padded, substeps, Tn timed steps); one untimed step comes first; padded: the rows are channel slices of a wider
# NaN-filled buffer
CASES = [
    (1, 1, 0, False, 1, 3), (3, 2, 1, True, 3, 3), (5, 1, 2, False, 1, 4), (5, 2, 3, False, 3, 3), (5, 1, 3, True, 1, 3),
    (3, 2, 2, True, 3, 3), (1, 2, 1, False, 1, 4), (3, 1, 0, True, 3, 3),
]
MAX_CASE = (1024, 1, ((3, 4), (1, 1)), False, 2, 3)                          # chunks (1024,) and (64,) * 16
# the finalize formulas want lattices with many interior nodes as well: (S, B, field, stride, padded, substeps, Tn)
WIDE_CASE = (5, 2, (12, 20), (2, 2), False, 2, 4)
SD = [1.7, 0.6, 2.5]
MU = [0.4, -0.1, 0.25]
GRID = (0.5, 0.25)                                                           # dx != dy
STEP_DT = 0.75


def lattice_of(hw, stride, origin=None):
    """Every pixel (oy + i sy, ox + j sx) inside the field -> (Gh, Gw, oy, ox, sy, sx); origin None: (sy // 2, sx // 2)."""
    sy, sx = stride
    oy, ox = (sy // 2, sx // 2) if origin is None else origin
    return ((hw[0] - 1 - oy) // sy + 1, (hw[1] - 1 - ox) // sx + 1, oy, ox, sy, sx)


def inner_lattice(hw, stride):
    """The lattice from (1, 1) on without the seeds on the last row and column: no seed on the frame."""
    sy, sx = stride
    return ((hw[0] - 3) // sy + 1, (hw[1] - 3) // sx + 1, 1, 1, sy, sx)


def boxes_of(hw):
    """Two boxes: the field's upper-left quarter (at least one pixel) and one single pixel row."""
    Hh, Ww = hw
    return ((0, max(0, Hh // 2 - 1), 0, max(0, Ww // 2 - 1)), (Hh - 1, Hh - 1, 0, Ww - 1))


def tables(sd, mu, u, B, grid=GRID, step_dt=STEP_DT):
    """a, o [B, 2] fp32: ((u out_std) step_dt) / d and ((u out_mu) step_dt) / d in fp64 from the fp32 factors, rounded once."""
    d = np.array(grid, np.float64).reshape(1, 2)
    uu = np.ones((B, 2)) if u is None else np.asarray(u, F32).astype(np.float64).reshape(B, -1)[:, :2]
    a = ((uu * np.asarray(sd, F32).astype(np.float64)[:2].reshape(1, 2)) * float(step_dt)) / d
    o = ((uu * np.asarray(mu, F32).astype(np.float64)[:2].reshape(1, 2)) * float(step_dt)) / d
    return a.astype(F32), o.astype(F32)


@functools.lru_cache(maxsize=None)
def real_inputs(S, B, hw, steps, seed, amp=0.4):
    """Smooth drift plus noise -> (xs [steps, S + 1, B, 3, H, W] fp32, sd, mu, u [B, 3]): velocities of the order of amp pixels per
    kept step once converted with tables(), so that some particles leave the field and most do not."""
    g = torch.Generator().manual_seed(seed)
    Hh, Ww = hw
    a, o = tables(SD, MU, None, 1)
    base = torch.randn(steps, S + 1, B, 3, 1, 1, generator=g) + 0.6 * torch.randn(steps, S + 1, B, 3, Hh, Ww, generator=g)
    u = 0.75 + 0.5 * torch.rand(B, 3, generator=g)
    phys = amp * base.double().numpy()                                       # wanted pixels per kept step (before u)
    xs = np.zeros_like(phys)
    xs[:, :, :, :2] = (phys[:, :, :, :2] - o.astype(np.float64).reshape(1, 1, 1, 2, 1, 1)) / a.astype(np.float64).reshape(1, 1, 1, 2, 1, 1)
    xs[:, :, :, 2] = phys[:, :, :, 2]
    return xs.astype(F32), np.array(SD, F32), np.array(MU, F32), u.numpy().astype(F32)


@functools.lru_cache(maxsize=None)
def int_velocities(S, B, steps, seed, vmax=2):
    """One integer velocity vector (u, v) per step, row and case -> [steps, S + 1, B, 2] int64, different for every member and
    case."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-vmax, vmax + 1, (steps, S + 1, B, 2), generator=g).numpy().astype(np.int64)
    v[:, :, :, 0] += (np.arange(S + 1) % 3 - 1)[None, :, None]
    v[:, :, :, 1] += (np.arange(B) % 2)[None, None, :]
    return v


def uniform_fields(vel, hw, C=3):
    """vel [steps, R, B, 2] -> xs [steps, R, B, C, H, W] fp32: spatially uniform velocity, the other channels 7."""
    xs = np.full(vel.shape[:3] + (C,) + tuple(hw), 7.0, F32)
    xs[:, :, :, :2] = vel.astype(F32)[..., None, None]
    return xs


# ---- 1: the scheme, in float32 (the mirror) or float64 ---------------------------------------------------------------------------------
def convert(x, a, o, dt):
    """x [R, B, C, H, W] -> the velocity planes [R, B, 2, H, W]: fl(fl(a y) + o) in dt (the tables are fp32 values either way)."""
    a, o = np.asarray(a, F32).astype(dt), np.asarray(o, F32).astype(dt)
    with np.errstate(invalid="ignore", over="ignore"):                       # (a test feeds one non-finite or huge value)
        out = a[None, :, :, None, None] * np.asarray(x, F32)[:, :, :2].astype(dt) + o[None, :, :, None, None]
    assert out.dtype == dt
    return out


def _inside(px, py, hw, mut):
    with np.errstate(invalid="ignore"):
        if mut == "exclusive":
            return (px >= 0) & (px < hw[1] - 1) & (py >= 0) & (py < hw[0] - 1)
        return (px >= 0) & (px <= hw[1] - 1) & (py >= 0) & (py <= hw[0] - 1)


def _bilinear(f, px, py, mut):
    """f [R, B, 2, H, W], inside positions px, py [R, B, P] -> [R, B, 2, P] in f's type, every operation on its own."""
    dt = f.dtype.type
    Hh, Ww = f.shape[-2:]
    j0 = np.minimum(np.floor(px).astype(np.int64), Ww - 2)
    i0 = np.minimum(np.floor(py).astype(np.int64), Hh - 2)
    fx, fy = px - j0.astype(dt), py - i0.astype(dt)
    if mut == "fxfy":
        fx, fy = fy, fx
    ff = f.reshape(f.shape[:3] + (Hh * Ww,))
    q = (i0 * Ww + j0)[:, :, None, :]
    take = lambda k: np.take_along_axis(ff, np.broadcast_to(q + k, ff.shape[:3] + (q.shape[-1],)), axis=-1)   # noqa: E731
    f00, f01, f10, f11 = take(0), take(1), take(Ww), take(Ww + 1)
    fx, fy = fx[:, :, None, :], fy[:, :, None, :]
    top = f00 + fx * (f01 - f00)
    bot = f10 + fx * (f11 - f10)
    out = top + fy * (bot - top)
    assert out.dtype == f.dtype
    return out


def _velocity(prev, cur, px, py, s, act, mut):
    """V(s) at the positions of the active particles (the others are evaluated at pixel (0, 0) and never used)."""
    zx, zy = np.where(act, px, px.dtype.type(0)), np.where(act, py, py.dtype.type(0))
    with np.errstate(invalid="ignore", over="ignore"):
        v0, v1 = _bilinear(prev, zx, zy, mut), _bilinear(cur, zx, zy, mut)
        k = v0 + s * (v1 - v0)
    return k[:, :, 0], k[:, :, 1]


def _in_boxes(px, py, boxes):
    out = np.zeros(px.shape[:2] + (len(boxes),) + px.shape[2:], dtype=bool)
    for r, (h0, h1, w0, w1) in enumerate(boxes):
        out[:, :, r] = (py >= h0) & (py <= h1) & (px >= w0) & (px <= w1)
    return out


def scheme(xs, a, o, lattice, boxes, n, timed, dt=F32, mut=None, trace=None, margin=None, probe=None):
    """The state after every step.  xs [steps, R, B, C, H, W] fp32 -> list over the steps of None (before the first timed step) or
    dict(pos [R, B, 2, P] dt, exit [R, B, P] int32, res [R, B, nb, P] int32).  dt = float32: the mirror.  mut: one deliberate
    mistake (store_first, no_h, fxfy, exclusive).  trace (a list): receives the smallest distance to the frame of every predictor
    and corrector position of an active particle, once per substep and kind.  margin (an array [R, B, P], +inf): receives per particle
    the smallest such distance (negative for the position that killed it).  probe (a list): receives per substep (act, px, py, act2,
    xa, ya), the positions at which k1 and k2 were evaluated and for which particles."""
    xs = np.asarray(xs)
    assert xs.dtype == F32
    steps, R, B = xs.shape[:3]
    hw = xs.shape[-2:]
    Gh, Gw, oy, ox, sy, sx = lattice
    P = Gh * Gw
    if dt is F32:
        sj = [F32(j / n) for j in range(n + 1)]
        h, hh = F32(1.0 / n), F32(0.5 / n)
    else:
        sj = [dt(j) / dt(n) for j in range(n + 1)]
        h, hh = dt(1.0) / dt(n), dt(0.5) / dt(n)
    st, prev, snaps, t_before = None, None, [], 0
    for t in range(steps):
        if t in timed:
            cur = convert(xs[t], a, o, dt)
            if st is None:
                ii, jj = np.divmod(np.arange(P), Gw)
                px0, py0 = (ox + jj * sx).astype(dt), (oy + ii * sy).astype(dt)
                pos = np.broadcast_to(np.stack([px0, py0])[None, None], (R, B, 2, P)).copy()
                st = dict(pos=pos, exit=np.full((R, B, P), -1, np.int32),
                          res=_in_boxes(pos[:, :, 0], pos[:, :, 1], boxes).astype(np.int32))
            else:
                pv = cur if mut == "store_first" else prev
                px, py = st["pos"][:, :, 0].copy(), st["pos"][:, :, 1].copy()
                alive = st["exit"] < 0
                dead = np.zeros_like(alive)
                for j in range(n):
                    act = alive & ~dead
                    k1u, k1v = _velocity(pv, cur, px, py, sj[j], act, mut)
                    with np.errstate(invalid="ignore", over="ignore"):
                        hp = dt(1) if mut == "no_h" else h
                        xa, ya = px + hp * k1u, py + hp * k1v
                    ins = _inside(xa, ya, hw, mut)
                    dead |= act & ~ins
                    act2 = act & ins
                    k2u, k2v = _velocity(pv, cur, xa, ya, sj[j + 1], act2, mut)
                    with np.errstate(invalid="ignore", over="ignore"):
                        xn, yn = px + hh * (k1u + k2u), py + hh * (k1v + k2v)
                    ins2 = _inside(xn, yn, hw, mut)
                    dead |= act2 & ~ins2
                    ok = act2 & ins2
                    if trace is not None:
                        for m_, qx, qy in ((act, xa, ya), (act2, xn, yn)):
                            with np.errstate(invalid="ignore"):
                                dist = np.minimum(np.minimum(qx, hw[1] - 1 - qx), np.minimum(qy, hw[0] - 1 - qy))
                            if m_.any():
                                trace.append(float(np.nan_to_num(dist[m_], nan=-np.inf).min()))
                    if margin is not None:
                        for m_, qx, qy in ((act, xa, ya), (act2, xn, yn)):
                            with np.errstate(invalid="ignore"):
                                dist = np.minimum(np.minimum(qx, hw[1] - 1 - qx), np.minimum(qy, hw[0] - 1 - qy))
                            margin[...] = np.where(m_, np.minimum(margin, np.nan_to_num(dist, nan=-np.inf)), margin)
                    if probe is not None:
                        probe.append((act.copy(), px.copy(), py.copy(), act2.copy(), xa.copy(), ya.copy()))
                    px, py = np.where(ok, xn, px), np.where(ok, yn, py)
                    assert px.dtype == dt and py.dtype == dt
                st["pos"] = np.stack([px, py], axis=2)
                st["exit"] = np.where(dead, np.int32(t_before - 1), st["exit"]).astype(np.int32)
                st["res"] = st["res"] + (_in_boxes(px, py, boxes) & (alive & ~dead)[:, :, None]).astype(np.int32)
            prev = cur
            t_before += 1
        snaps.append(None if st is None else {k: v.copy() for k, v in st.items()})
    return snaps


def mirror(xs, a, o, lattice, boxes, n, timed, mut=None):
    return scheme(xs, a, o, lattice, boxes, n, timed, F32, mut)


def int_reference(vel, hw, lattice, boxes, n, timed):
    """Uniform integer velocities vel [steps, R, B, 2] int64 (a = 1, o = 0) -> dict(pos [R, B, 2, P] float64, exactly X / D, exit,
    res) after the last step, in int64 numerators over D = 2 n^2 (module docstring)."""
    vel = np.asarray(vel, dtype=np.int64)
    steps, R, B = vel.shape[:3]
    Gh, Gw, oy, ox, sy, sx = lattice
    P, D = Gh * Gw, 2 * n * n
    ii, jj = np.divmod(np.arange(P, dtype=np.int64), Gw)
    X = np.broadcast_to(((ox + jj * sx) * D)[None, None], (R, B, P)).copy()
    Y = np.broadcast_to(((oy + ii * sy) * D)[None, None], (R, B, P)).copy()
    ex = np.full((R, B, P), -1, np.int64)
    wmax, hmax = (hw[1] - 1) * D, (hw[0] - 1) * D
    inside = lambda x, y: (x >= 0) & (x <= wmax) & (y >= 0) & (y <= hmax)     # noqa: E731

    def count(alive):
        out = np.zeros((R, B, len(boxes), P), np.int64)
        for r, (h0, h1, w0, w1) in enumerate(boxes):
            out[:, :, r] = alive & (Y >= h0 * D) & (Y <= h1 * D) & (X >= w0 * D) & (X <= w1 * D)
        return out

    res, v0, adv = None, None, 0
    for t in range(steps):
        if t not in timed:
            continue
        v1 = vel[t][:, :, :, None]                                           # [R, B, 2, 1]
        if res is None:
            res = count(np.ones((R, B, P), bool))
        else:
            alive = ex < 0
            dead = np.zeros_like(alive)
            for j in range(n):
                nk1, nk2 = n * v0 + j * (v1 - v0), n * v0 + (j + 1) * (v1 - v0)
                act = alive & ~dead
                xa, ya = X + 2 * nk1[:, :, 0], Y + 2 * nk1[:, :, 1]
                dead |= act & ~inside(xa, ya)
                act2 = act & inside(xa, ya)
                xn, yn = X + (nk1 + nk2)[:, :, 0], Y + (nk1 + nk2)[:, :, 1]
                dead |= act2 & ~inside(xn, yn)
                ok = act2 & inside(xn, yn)
                X, Y = np.where(ok, xn, X), np.where(ok, yn, Y)
            ex = np.where(dead, adv, ex)
            adv += 1
            res = res + count(alive & ~dead)
        v0 = v1
    pos = np.stack([X, Y], axis=2).astype(np.float64) / D
    return dict(pos=pos, exit=ex.astype(np.int32), res=res.astype(np.int32))


def touches(px, py, hw, pixel):
    """Whether the bilinear cell of the inside positions px, py holds the pixel (h, w)."""
    j0 = np.minimum(np.floor(px).astype(np.int64), hw[1] - 2)
    i0 = np.minimum(np.floor(py).astype(np.int64), hw[0] - 2)
    return ((i0 == pixel[0]) | (i0 + 1 == pixel[0])) & ((j0 == pixel[1]) | (j0 + 1 == pixel[1]))


# ---- 2: the bound of the mirror against the fp64 scheme --------------------------------------------------------------------------------
def bound_case(i):
    """Inputs for the comparison of the mirror with the fp64 scheme on the shapes of case i: the lattice without the frame
    (inner_lattice) and velocities under 0.24 pixels per kept step, so that over Tn - 1 <= 3 advections no particle comes closer
    to the frame than 1 - 0.72 pixel -> (xs, a, o, lattice, boxes, n, timed)."""
    S, B, fi, padded, n, Tn = CASES[i]
    hw, stride = FIELDS[fi]
    xs, sd, mu, u = real_inputs(S, B, hw, Tn + 1, 500 + i, amp=0.04)
    a, o = tables(sd, mu, u, B)
    return xs, a, o, inner_lattice(hw, stride), boxes_of(hw), n, range(1, Tn + 1)


def slope_and_size(xs, a, o, timed):
    """(G, Vm) of the module docstring over the timed steps of xs, from the fp64 planes."""
    G = Vm = 0.0
    a64, o64 = np.abs(a.astype(np.float64))[None, :, :, None, None], np.abs(o.astype(np.float64))[None, :, :, None, None]
    for t in timed:
        f = convert(xs[t], a, o, np.float64)
        gx = np.abs(np.diff(f, axis=-1)).max() if f.shape[-1] > 1 else 0.0
        gy = np.abs(np.diff(f, axis=-2)).max() if f.shape[-2] > 1 else 0.0
        G = max(G, float(gx + gy))
        Vm = max(Vm, float((a64 * np.abs(xs[t][:, :, :2].astype(np.float64)) + o64).max()))
    return G, Vm


def position_bound(G, Vm, X, n, advections, extra=0.0):
    """The recursion of the module docstring after `advections` advections of n substeps; extra: what the caller's velocities are
    uncertain by beyond C_K, in units of u Vm."""
    h = 1.0 / n
    hG = h * G
    amp = 1.0 + hG + hG * hG / 2.0
    add = U24 * (X * (1.0 + hG / 2.0) + h * Vm * ((C_K + extra) * (1.0 + hG / 2.0) + 3.0 + hG))
    delta = 0.0
    for _ in range(advections * n):
        delta = delta * amp + add
    return delta


# ---- 3: the finalize formulas in fp64, on a given state ---------------------------------------------------------------------------------
class _Welford:
    """Welford over the members in member order, elementwise, counting only the valid entries (the kernel's lagr_push)."""

    def __init__(self, shape):
        self.n, self.mean, self.m2 = np.zeros(shape, np.int64), np.zeros(shape), np.zeros(shape)

    def push(self, v, valid):
        n1 = self.n + valid
        with np.errstate(invalid="ignore", divide="ignore"):
            d = v - self.mean
            mean = self.mean + d / n1.astype(np.float64)
            m2 = self.m2 + d * (v - mean)
        self.mean, self.m2, self.n = np.where(valid, mean, self.mean), np.where(valid, m2, self.m2), n1

    def out(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(self.n > 0, self.mean, np.nan)
            var = np.where(self.n > 0, np.maximum(self.m2, 0.0) / self.n.astype(np.float64), np.nan)
        return mean, var


def restate(pos, exit_, res, lattice, fl):
    """The kernel's finalize formulas in fp64.  pos [R, B, 2, P] (fp32 values), exit [R, B, P], res [R, B, nb, P], fl = (dx, dy,
    step_dt, T_int) -> (out, err): out the published arrays in fp64 (ftle_count int64) plus the per-member ones, err the counted
    absolute bounds of the same names (module docstring; 0 for the exact ones)."""
    dx, dy, step_dt, T_int = [float(v) for v in fl]
    Gh, Gw, oy, ox, sy, sx = lattice
    R, B, _, P = pos.shape
    S, nb = R - 1, res.shape[2]
    p64 = np.asarray(pos, dtype=np.float64).reshape(R, B, 2, Gh, Gw)
    alive = (np.asarray(exit_) < 0).reshape(R, B, Gh, Gw)
    X, Y = p64[:, :, 0] * dx, p64[:, :, 1] * dy
    ddx, ddy, t2 = (2.0 * sx) * dx, (2.0 * sy) * dy, 2.0 * T_int
    ftle = np.full((R, B, Gh, Gw), np.nan)
    ferr = np.zeros((R, B, Gh, Gw))
    valid = np.zeros((R, B, Gh, Gw), bool)
    if Gh > 2 and Gw > 2:
        c = (slice(None), slice(None), slice(1, -1), slice(1, -1))
        E, W_, N, S_ = [(slice(None), slice(None), slice(1 + di, Gh - 1 + di), slice(1 + dj, Gw - 1 + dj))
                        for di, dj in ((0, 1), (0, -1), (-1, 0), (1, 0))]
        valid[c] = alive[c] & alive[E] & alive[W_] & alive[N] & alive[S_]
        F11, F21 = (X[E] - X[W_]) / ddx, (Y[E] - Y[W_]) / ddx
        F12, F22 = (X[S_] - X[N]) / ddy, (Y[S_] - Y[N]) / ddy
        C11, C12, C22 = F11 * F11 + F21 * F21, F11 * F12 + F21 * F22, F12 * F12 + F22 * F22
        hd = 0.5 * (C11 - C22)
        lam = 0.5 * (C11 + C22) + np.sqrt(hd * hd + C12 * C12)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = np.log(lam) / t2
            m11, m21 = (np.abs(X[E]) + np.abs(X[W_])) / ddx, (np.abs(Y[E]) + np.abs(Y[W_])) / ddx
            m12, m22 = (np.abs(X[S_]) + np.abs(X[N])) / ddy, (np.abs(Y[S_]) + np.abs(Y[N])) / ddy
            M11, M12, M22 = m11 * m11 + m21 * m21, m11 * m12 + m21 * m22, m12 * m12 + m22 * m22
            hm = 0.5 * (M11 + M22)
            lmag = hm + np.sqrt(hm * hm + M12 * M12)
            fe = E53 * (C_LAM * lmag / lam + 4.0 * np.abs(np.log(lam))) / t2
        ftle[c] = np.where(valid[c], val, np.nan)
        ferr[c] = np.where(valid[c], fe, 0.0)
    ii, jj = np.divmod(np.arange(P), Gw)
    x0, y0 = (ox + jj * sx).astype(np.float64).reshape(Gh, Gw), (oy + ii * sy).astype(np.float64).reshape(Gh, Gw)
    dX, dY = (p64[:, :, 0] - x0) * dx, (p64[:, :, 1] - y0) * dy
    rt = np.asarray(res, dtype=np.float64).reshape(R, B, nb, Gh, Gw) * step_dt
    both = alive[:S] & alive[S][None]
    ex_, ey_ = X[:S] - X[S][None], Y[:S] - Y[S][None]
    dist = np.sqrt(ex_ * ex_ + ey_ * ey_)
    derr = E53 * (4.0 * (np.abs(X[:S]) + np.abs(X[S])[None] + np.abs(Y[:S]) + np.abs(Y[S])[None]) + 4.0 * dist)
    wf, wdx, wdy, wex, wey, werr = [_Welford((B, Gh, Gw)) for _ in range(6)]
    wres = _Welford((B, nb, Gh, Gw))
    for r in range(S):
        wf.push(ftle[r], valid[r])
        wdx.push(dX[r], alive[r]), wdy.push(dY[r], alive[r])
        wex.push(X[r], alive[r]), wey.push(Y[r], alive[r])
        werr.push(dist[r], both[r])
        wres.push(rt[r], np.ones((B, nb, Gh, Gw), bool))
    out, err = {}, {}

    def put(name, w, row_err, mags, valid_rows):
        """mean / std of one Welford with their bounds: the rows move by at most row_err, their magnitude is at most mags."""
        mean, var = w.out()
        std = np.sqrt(var)
        big = lambda v: np.where(valid_rows, v, 0.0).max(0)                   # noqa: E731
        c = big(row_err) + 4 * S * E53 * big(mags)
        dq = 4.0 * c * big(mags) + c * c
        with np.errstate(divide="ignore", invalid="ignore"):
            bstd = np.minimum(np.sqrt(dq), np.where(std > 0, dq / np.maximum(std, 1e-300), np.inf))
        return mean, std, c, c + bstd

    with np.errstate(invalid="ignore"):
        m, s, em, es = put("ftle", wf, ferr[:S], np.abs(np.nan_to_num(ftle[:S])), valid[:S])
    out["ftle_mean"], out["ftle_std"], err["ftle_mean"], err["ftle_std"] = m, s, em, es
    out["target_ftle"], err["target_ftle"] = ftle[S], ferr[S]
    out["ftle_count"], err["ftle_count"] = wf.n, np.zeros((B, Gh, Gw))
    dm, ds, dem, des = [], [], [], []
    for w, v in ((wdx, dX), (wdy, dY)):
        m, s, em, es = put("disp", w, 2 * E53 * np.abs(v[:S]), np.abs(v[:S]), alive[:S])
        dm.append(m), ds.append(s), dem.append(em), des.append(es)
    out["disp_mean"], out["disp_std"], err["disp_mean"], err["disp_std"] = [np.stack(v, axis=1) for v in (dm, ds, dem, des)]
    out["target_disp"] = np.where(alive[S][:, None], np.stack([dX[S], dY[S]], axis=1), np.nan)
    err["target_disp"] = 2 * E53 * np.abs(np.nan_to_num(out["target_disp"]))
    out["alive_frac"], err["alive_frac"] = wex.n.astype(np.float64) / float(S), 2 * E53 * np.ones((B, Gh, Gw))
    out["target_alive"], err["target_alive"] = alive[S].astype(np.float64), np.zeros((B, Gh, Gw))
    if nb:
        m, s, em, es = put("res", wres, E53 * rt[:S], rt[:S], np.ones(rt[:S].shape, bool))
        out["res_time_mean"], out["res_time_std"], err["res_time_mean"], err["res_time_std"] = m, s, em, es
        out["target_res_time"], err["target_res_time"] = rt[S], E53 * rt[S]
    m, _, em, _ = put("err", werr, derr, dist, both)
    out["end_err_mean"], err["end_err_mean"] = m, em
    sx_ = put("ex", wex, E53 * np.abs(X[:S]), np.abs(X[:S]), alive[:S])
    sy_ = put("ey", wey, E53 * np.abs(Y[:S]), np.abs(Y[:S]), alive[:S])
    _, vx = wex.out()
    _, vy = wey.out()
    out["end_spread"] = np.sqrt(vx + vy)
    err["end_spread"] = 2.0 * (sx_[3] + sy_[3]) + 4 * E53 * np.nan_to_num(out["end_spread"])   # |sqrt(a+b) - sqrt(a'+b')| <= |da| + |db| in std units
    out["member_ftle"], err["member_ftle"] = np.moveaxis(ftle[:S], 0, 1), np.moveaxis(ferr[:S], 0, 1)
    out["member_end"] = np.moveaxis(np.asarray(pos[:S]).reshape(S, B, 2, Gh, Gw), 0, 1)
    out["member_exit"] = np.moveaxis(np.asarray(exit_[:S]).reshape(S, B, Gh, Gw), 0, 1)
    return out, err


FIELD_KEYS = ("ftle_mean", "ftle_std", "target_ftle", "ftle_count", "disp_mean", "disp_std", "target_disp", "alive_frac", "target_alive",
              "end_err_mean", "end_spread")
RES_KEYS = ("res_time_mean", "res_time_std", "target_res_time")
MEMBER_KEYS = ("member_ftle", "member_end", "member_exit")
META_KEYS = ("transport_seeds", "transport_boxes", "transport_time")


def check_outputs(got, ref, err, what, keys=None):
    """The published arrays `got` (numpy) against restate()'s (ref, err): |got - ref| <= u |ref| + err, NaN exactly where the
    reference has it; the integer arrays and member_end exactly -> the worst share of the bound reached."""
    worst = 0.0
    for name in keys if keys is not None else [k for k in FIELD_KEYS + RES_KEYS + MEMBER_KEYS if k in got]:
        g, r = np.asarray(got[name]), ref[name]
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        if name in ("ftle_count", "member_exit"):
            assert g.dtype == np.int32 and np.array_equal(g, r), "%s %s" % (what, name)
            continue
        assert g.dtype == F32, (what, name, g.dtype)
        if name == "member_end":
            assert np.array_equal(g, r), "%s member_end is not pos" % what
            continue
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s %s: NaN pattern" % (what, name)
        fin = np.isfinite(r)
        assert np.array_equal(g[~fin & ~np.isnan(r)], r[~fin & ~np.isnan(r)].astype(F32)), "%s %s: infinities" % (what, name)
        e = np.abs(g.astype(np.float64) - r)[fin]
        b = (U24 * np.abs(r) + err[name])[fin]
        share = float(np.where(e > 0, e / np.maximum(b, 1e-300), 0.0).max()) if fin.any() else 0.0
        assert share <= 1.0, "%s %s: off by %.3g of its bound" % (what, name, share)
        worst = max(worst, share)
    return worst


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
KAT_GRID, KAT_DT = (0.5, 0.25), 0.5                                           # a = step_dt / d = (1, 2) with out_std = 1, out_mu = 0


def kat_shear(g=0.25, hw=(9, 24), Tn=4, S=2):
    """Simple shear: pixel velocity (g_r py, 0) with a dyadic g_r per row -> (xs [Tn + 1, S + 1, 1, 3, H, W] fp32 for out_std = 1,
    out_mu = 0 and KAT_GRID / KAT_DT, gs [S + 1]).  x_T = x_0 + g py (Tn - 1) exactly; lam = (2 + q^2 + q sqrt(q^2 + 4)) / 2 with
    q = g (Tn - 1) dx / dy."""
    Hh, Ww = hw
    gs = g * (1.0 + np.arange(S + 1))
    a = np.array([KAT_DT / KAT_GRID[0], KAT_DT / KAT_GRID[1]])
    xs = np.zeros((Tn + 1, S + 1, 1, 3, Hh, Ww))
    xs[:, :, 0, 0] = (gs[None, :, None, None] * np.arange(Hh, dtype=np.float64)[None, None, :, None]) / a[0]
    xs[0] = 5.0                                                              # the untimed step: never read
    return xs.astype(F32), gs


def kat_saddle(al=0.25, hw=(17, 17), Tn=3):
    """Steady saddle about the field's centre: pixel velocity (al (px - cx), -al (py - cy)), one member that equals the target ->
    xs [Tn + 1, 2, 1, 3, H, W].  Per advection (substeps = 1) px - cx grows by 1 + al + al^2 / 2 and py - cy by 1 - al + al^2 / 2."""
    Hh, Ww = hw
    cy, cx = (Hh - 1) / 2.0, (Ww - 1) / 2.0
    a = np.array([KAT_DT / KAT_GRID[0], KAT_DT / KAT_GRID[1]])
    xs = np.zeros((Tn + 1, 2, 1, 3, Hh, Ww))
    xs[:, :, 0, 0] = (al * (np.arange(Ww) - cx))[None, None, None, :] / a[0]
    xs[:, :, 0, 1] = (-al * (np.arange(Hh) - cy))[None, None, :, None] / a[1]
    xs[0] = -3.0
    return xs.astype(F32), (cy, cx)
