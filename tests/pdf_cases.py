"""Case tables, reference and named defects of the pooled ensemble PDFs (tests/test_pdf_cpu.py, tests/test_pdf_gpu.py).

Definitions (include/tmglow_hip_pdf.h, tmg_ops.EnsemblePdfs), word for word.

Fields.  There are up to 8, each one of: a channel 0..C-1 (aliases "ux", "uy", "p" for 0, 1, 2), "speed", "vort", "div".  The three
derived fields need grid = (dx, dy).
Values for a channel field.  The value binned is d = x, the raw normalised value: u out_std > 0 keeps the order, and comparisons have
no rounding.  With an optional centre it is one rounded fp32 subtraction, d = fl(x - c_raw[b, c, p]).
Values for a derived field.  The physical value is formed in fp32 with every operation rounded on its own (contraction off, no fused
multiply-add, so that a numpy float32 mirror reproduces it exactly):
  t = fl(fl(sd x) + mu), then v = fl(u t).
  The 3x3 first-derivative stencil of pc/ is applied with zero padding: a neighbour outside the field is 0 in physical units, with
  exactly the neighbours, weights and summation order of ens_turb_accum_kernel: right column first, then left, each in the order
  centre * 2, up, down (d/dx); lower row first, then upper, each in the order centre * 2, left, right (d/dy).
  rdx = fl(0.125f / fl(dx)), rdy = fl(0.125f / fl(dy)).
  vort = fl(fl(vx rdx) - fl(uy rdy)), vx = d/dx of channel 1, uy = d/dy of channel 0.
  div = fl(fl(ux_x rdx) + fl(vy_y rdy)), with the same stencil transposed: ux_x = d/dx of channel 0, vy_y = d/dy of channel 1.
  speed = sqrt_rn(fl(fl(U U) + fl(V V))), with a correctly rounded square root.
Edges.  Each field has nb uniform inner bins, 1 <= nb <= 128, the same nb for all fields.  The physical edges are
E_j = lo + j (hi - lo) / nb, j = 0..nb, formed in fp64.  The device table e[b][f][j] is fp32, formed in fp64 and rounded once:
  channel field without centre: (E_j / u[b,c] - mu[c]) / sd[c]
  channel field with centre:    E_j / (u[b,c] sd[c]), with c_raw = float32((center / u - mu) / sd)
  derived field:                E_j itself
Edges that are not strictly increasing after rounding are a ValueError.
Bin index.  Defined by comparisons alone: idx(d) = #{ j in 0..nb : d >= e_j }.  So 0 is the underflow bin (d < e_0), nb + 1 is the
overflow bin (d >= e_nb), and a value ON an edge belongs to the bin above it.  Non-finite members are not supported.
Regions.  There are up to 4 pixel boxes (x0, x1, y0, y1), half open, x along W.  They may overlap.  Each must be non-empty and inside
the field.  A pixel is counted in every region that holds it.  A derived field at a region's border still uses its neighbours outside
the region.  Only the field border pads with zeros.
Joint histograms.  There are up to 2 pairs (fi, fj) of distinct listed fields.  Each axis has nbj uniform bins, 1 <= nbj <= 32, over
the same [lo, hi] as its field, with its own rounded edge table and the same index rule.  The table is (nbj + 2)^2 counts and fi
indexes its rows.

The reference uses none of the kernel's devices: np.searchsorted(edges, v, side="right") on the values gives the indices, np.bincount
and np.histogram2d on explicit region slices give the tables, the time aggregates are plain sums over the timed steps.  The derived
fields come from shifted slices of a zero-padded array, once in float32 (the mirror: numpy rounds every float32 operation on its
own, and adding the zeros of the padding is exact) and once in fp64.
The floats come from other formulas than tmg_ops': w1 as the integral of |F^-1 - G^-1| over the merged breakpoints of the two
cumulative distributions (cross-multiplied to integers, so the breakpoints are exact), js as H(M) - (H(P) + H(Q)) / 2, the densities as
share / width.

Float tolerance (the issue's): |got - ref| <= 2^-24 |ref| + 2^-40: the one final rounding to float32 plus the fp64 formulas' own
rounding (at most 34^2 = 1156 terms of magnitude <= 1: under 2^-42).

Near-edge samples of a derived field (real data).  The fp64 value of a sample lies within 14 * 2^-24 * A of an edge, A the sum of the
absolute stencil terms times rdx / rdy.  An absolute term is taken as u (sd |x| + |mu|) >= |u (sd x + mu)|, which also covers the
cancellation inside the un-normalisation: a term carries 3 roundings (3 u of it), the six additions of one derivative at most u of
the running sum of absolute terms each, the product with rdx one, the final sum one, rdx itself (one division of a rounded dx) two:
3 + 6 + 1 + 1 + 2 = 13 <= 14.  For speed A = the two absolute terms |U|a + |V|a: |dU| + |dV| <= 3 u A from the inputs, and the two
squares, the sum and the root add at most 2 u speed <= 2 u A."""
import functools

import numpy as np
import torch

import event_cases as EC
import structure_cases as SC

F32 = np.float32
T = 3
U24 = 2.0 ** -24
TOL_ABS = 2.0 ** -40
NEAR = 14 * U24
SD, MU, GRID = SC.SD, EC.MU, SC.GRID
KINDS = {"ux": 0, "uy": 1, "p": 2, "speed": 4, "vort": 5, "div": 6}
INT_KEYS = ("pdf_count", "target_count", "joint_count", "target_joint_count", "time_member_count", "time_count", "time_target_count",
            "time_joint_count", "time_target_joint_count")
FLOAT_KEYS = ("pdf", "target_pdf", "time_pdf", "time_pdf_mean", "time_pdf_std", "time_target_pdf", "w1", "js", "time_w1", "time_js",
              "time_member_w1", "time_joint_js")
META_KEYS = ("pdf_edges", "joint_edges", "pdf_ranges", "pdf_fields", "pdf_joint", "pdf_regions")
ALL_KEYS = INT_KEYS + FLOAT_KEYS + META_KEYS
DEFECTS = ("edge_side", "drop_overflow", "region_closed", "region_pads", "wrap", "center_skip", "joint_transposed", "member_pooled",
           "target_counted", "untimed_counted")

F1, F2 = ("div",), ("ux", "uy")
F5 = ("ux", "uy", "speed", "vort", "div")
F8 = (0, 1, 2, 3, "speed", "vort", "div", "ux")                              # C = 4; "ux" twice, the second with its own range
CH3 = ("p", "ux", "uy")
# (S, B, C, (H, W), t_start, chunk kind, padded, nb, nbj, fields, pairs, region kind, centre)
INT_TABLE = [
    (1, 1, 2, (1, 2), 0, 0, False, 1, 1, F2, (("ux", "uy"),), 0, False),
    (2, 3, 3, (2, 1), 1, 2, True, 2, 8, F5, (("ux", "uy"), ("vort", "div")), 0, True),
    (1024, 1, 2, (1, 5), 0, 2, False, 16, 32, F2, (), 1, False),
    (5, 3, 3, (7, 9), 1, 1, True, 64, 8, F5, (("speed", "vort"),), 3, False),
    (17, 3, 4, (5, 13), 1, 1, True, 128, 32, F8, (("ux", "uy"), (2, "div")), 5, True),
    (64, 1, 3, (16, 17), 0, 2, False, 16, 8, F1, (), 4, False),
    (130, 1, 2, (16, 33), 0, 1, True, 2, 1, F5, (("uy", "ux"),), 3, True),
    (5, 1, 3, (50, 58), 1, 2, False, 64, 32, F5, (("ux", "uy"), ("vort", "speed")), 2, False),
    (17, 3, 2, (3, 70), 0, 1, True, 16, 8, F2, (("ux", "uy"),), 4, True),
    (2, 1, 4, (66, 3), 1, 0, False, 128, 1, F8, (), 1, False),
    (5, 1, 2, (66, 130), 0, 2, True, 64, 8, F2, (("uy", "ux"),), 2, True),
    (1024, 1, 3, (7, 9), 0, 1, False, 1, 32, CH3, (("p", "ux"),), 3, False),
    (64, 3, 2, (16, 33), 1, 0, True, 16, 8, F1, (), 0, False),
]
LONG_CASE = (2, 1, 2, (181, 183), 0, 2, False, 64, 8, F5, (("ux", "uy"),), 2, False)   # 33 slices per row, two steps
# (S, B, C, (H, W), kind, with_u, nb, nbj, fields, pairs, region kind, centre, ranges per case)
REAL_TABLE = [
    (5, 3, 3, (7, 9), "gauss", True, 16, 8, F5, (("ux", "uy"),), 0, False, False),
    (16, 1, 4, (16, 17), "smooth", False, 64, 32, F8, (("ux", "uy"), ("vort", "div")), 3, True, False),
    (17, 3, 2, (5, 13), "biased", True, 128, 8, F5, (("speed", "vort"),), 4, False, True),
    (64, 1, 3, (16, 33), "gauss", False, 64, 32, CH3, (("ux", "uy"),), 3, True, False),
    (17, 3, 3, (50, 58), "smooth", True, 128, 8, F5, (("ux", "uy"), ("vort", "speed")), 2, True, True),
    (2, 3, 3, (50, 58), "biased", False, 16, 1, F5, (), 5, False, False),
    (5, 1, 2, (3, 70), "smooth", True, 64, 8, F1, (), 0, False, False),
    (7, 3, 3, (66, 3), "gauss", True, 16, 32, F5, (("div", "vort"),), 1, True, True),
    (5, 1, 3, (50, 58), "gauss", True, 128, 32, CH3, (("p", "ux"), ("ux", "uy")), 2, True, False),
]
FIELDS = EC.FIELDS
# what tmg_ens_pdf_plan can report: the instance (0: channel fields only, 1: with derived fields) and whether a row has one slice or
# several (the slice length, the pixels per thread and the number of histogram copies are constants)
PLAN_BRANCHES = {(0, False), (0, True), (1, False), (1, True)}
INT_RANGE = {0: (-2.0, 2.0), 1: (-2.0, 2.0), 2: (-2.0, 2.0), 3: (-2.0, 2.0), 4: (0.0, 4.0), 5: (-4.0, 4.0), 6: (-4.0, 4.0)}


def kind_of(f):
    return KINDS[f] if isinstance(f, str) else int(f)


def kinds_of(fields):
    return [kind_of(f) for f in fields]


def pairs_of(fields, joint):
    ks = kinds_of(fields)
    return [(ks.index(kind_of(a)), ks.index(kind_of(b))) for a, b in joint]


def plan_branch(plan):
    return plan["instance"], plan["NSL"] > 1


def regions_of(kind, hw):
    """0: the whole field (None); 1: one pixel; 2: a box that straddles the first slice boundary (pixel 1024; the field's middle rows
    when it has one slice); 3: two overlapping boxes; 4: a box on the field border; 5: four boxes."""
    Hh, Ww = hw
    one = (Ww // 2, Ww // 2 + 1, Hh // 2, Hh // 2 + 1)
    h0 = 1024 // Ww if Hh * Ww > 1024 else Hh // 2
    straddle = (Ww // 4, Ww, max(0, h0 - 1), min(Hh, h0 + 2))
    over = ((0, (2 * Ww + 2) // 3, 0, (2 * Hh + 2) // 3), (Ww // 3, Ww, Hh // 3, Hh))
    border = (0, max(1, Ww // 2), 0, Hh)
    return {0: None, 1: (one,), 2: (straddle,), 3: over, 4: (border,), 5: (border, one) + over}[kind]


def boxes_of(regions, hw):
    return [(0, hw[1], 0, hw[0])] if regions is None else [tuple(r) for r in regions]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def int_case(idx):
    """-> dict of an integer case: members and target in -3..3 with mu = 0, sd = 1, no u; dx, dy = GRID give rdx = 1/2, rdy = 1/4, so
    every stencil value is a multiple of 1/4 and exact in fp32 and fp64 alike; the ranges put edges ON data values; the centre holds
    integers in -1..1."""
    case = LONG_CASE if idx == len(INT_TABLE) else INT_TABLE[idx]
    S, B, Cc, hw, t_start, chunk, padded, nb, nbj, fields, joint, rk, centred = case
    steps = 2 if case is LONG_CASE else T
    xs, tgt = SC.int_inputs("small", S, B, Cc, hw, 9700 + idx, steps)
    ks = kinds_of(fields)
    ranges = [INT_RANGE[k] for k in ks]
    if len(ks) == 8:
        ranges[7] = (-1.0, 3.0)                                              # the repeated field: its own range
    cen = None
    if centred:
        cen = torch.randint(-1, 2, (B, Cc) + tuple(hw), generator=torch.Generator().manual_seed(9800 + idx)).float().numpy()
    return dict(S=S, B=B, C=Cc, hw=hw, t_start=min(t_start, steps - 1), chunk=chunk, padded=padded, nb=nb, nbj=nbj, fields=fields,
                joint=joint, regions=regions_of(rk, hw), center=cen, xs=xs, tgt=tgt, mu=np.zeros(Cc, F32), sd=np.ones(Cc, F32), u=None,
                ranges=np.broadcast_to(np.array(ranges, np.float64), (B, len(ks), 2)).copy(), grid=GRID, steps=steps)


def real_case(idx):
    """-> dict of a real case: SC.real_inputs at SD, MU, GRID; the ranges are the 1 % and 99 % quantiles of each field's fp64 values
    over members and target (per case where the table says so); the centre is the target's time mean in physical units."""
    S, B, Cc, hw, kind, with_u, nb, nbj, fields, joint, rk, centred, per_case = REAL_TABLE[idx]
    xs, tgt = SC.real_inputs(S, B, Cc, hw, kind, 9900 + idx)
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))).numpy().astype(F32) if with_u else None
    mu, sd = np.asarray(MU[:Cc], F32), np.asarray(SD[:Cc], F32)
    ks = kinds_of(fields)
    allx = np.concatenate([xs, tgt[:, None]], 1)
    cen = None
    if centred:
        cen = physical(tgt, mu, sd, u, np.float64).mean(0).astype(F32)
    vals = field_values(allx, ks, mu, sd, u, GRID, None if cen is None else c_raw(cen, mu, sd, u), np.float64, physical_units=True)
    ranges = np.zeros((B, len(ks), 2))
    for f in range(len(ks)):
        for b in range(B):
            v = vals[f][:, :, b] if per_case else vals[f]
            ranges[b, f] = np.percentile(v, [1.0, 99.0])
    return dict(S=S, B=B, C=Cc, hw=hw, t_start=idx % 2, chunk=idx % 3, padded=idx % 2 == 0, nb=nb, nbj=nbj, fields=fields, joint=joint,
                regions=regions_of(rk, hw), center=cen, xs=xs, tgt=tgt, mu=mu, sd=sd, u=u, ranges=ranges, grid=GRID, steps=T)


# ---- values ---------------------------------------------------------------------------------------------------------------------------
def _scale(u, B, Cc, dtype):
    return np.ones((B, Cc), dtype) if u is None else np.asarray(u, F32).reshape(B, Cc).astype(dtype)


def physical(x, mu, sd, u, dtype):
    """x [.., B, C, H, W] -> u (sd x + mu) in dtype, every operation rounded on its own."""
    B, Cc = x.shape[-4], x.shape[-3]
    m, s = np.asarray(mu, F32).astype(dtype).reshape(Cc, 1, 1), np.asarray(sd, F32).astype(dtype).reshape(Cc, 1, 1)
    t = s * x.astype(dtype)
    t = t + m
    return _scale(u, B, Cc, dtype).reshape(B, Cc, 1, 1) * t


def c_raw(center, mu, sd, u):
    """center [B, C, H, W] float32 (physical) -> float32((center / u - mu) / sd), formed in fp64."""
    B, Cc = center.shape[:2]
    sc = _scale(u, B, Cc, np.float64).reshape(B, Cc, 1, 1)
    m, s = np.asarray(mu, F32).astype(np.float64).reshape(1, Cc, 1, 1), np.asarray(sd, F32).astype(np.float64).reshape(1, Cc, 1, 1)
    return ((center.astype(np.float64) / sc - m) / s).astype(F32)


def _pad(a, wrap):
    if wrap:
        return np.pad(a, [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)], mode="wrap")
    out = np.zeros(a.shape[:-2] + (a.shape[-2] + 2, a.shape[-1] + 2), a.dtype)
    out[..., 1:-1, 1:-1] = a
    return out


def _ddx(p):
    """Right column first, then left, each in the order centre * 2, up, down (p: padded by one)."""
    two = p.dtype.type(2)
    a = two * p[..., 1:-1, 2:]
    a = a + p[..., :-2, 2:]
    a = a + p[..., 2:, 2:]
    a = a - two * p[..., 1:-1, :-2]
    a = a - p[..., :-2, :-2]
    return a - p[..., 2:, :-2]


def _ddy(p):
    """Lower row first, then upper, each in the order centre * 2, left, right."""
    two = p.dtype.type(2)
    a = two * p[..., 2:, 1:-1]
    a = a + p[..., 2:, :-2]
    a = a + p[..., 2:, 2:]
    a = a - two * p[..., :-2, 1:-1]
    a = a - p[..., :-2, :-2]
    return a - p[..., :-2, 2:]


def rd_of(grid, dtype):
    if dtype == F32:
        return F32(0.125) / F32(grid[0]), F32(0.125) / F32(grid[1])
    return 0.125 / float(grid[0]), 0.125 / float(grid[1])


def derived(x, mu, sd, u, grid, dtype, wrap=False, box=None):
    """x [.., B, C, H, W] -> (speed, vort, div) [.., B, H, W] in dtype.  box (the region_pads defect): the velocity is zeroed outside
    the box before the stencil."""
    ph = physical(x[..., :2, :, :], mu[:2], sd[:2], None if u is None else np.asarray(u)[:, :2], dtype)
    if box is not None:
        keep = np.zeros(ph.shape[-2:], dtype)
        keep[box[2]:box[3], box[0]:box[1]] = 1
        ph = ph * keep
    U, V = ph[..., 0, :, :], ph[..., 1, :, :]
    rdx, rdy = rd_of(grid, dtype)
    pu, pv = _pad(U, wrap), _pad(V, wrap)
    vort = _ddx(pv) * rdx - _ddy(pu) * rdy
    div = _ddx(pu) * rdx + _ddy(pv) * rdy
    return np.sqrt(U * U + V * V), vort, div


def field_values(x, kinds, mu, sd, u, grid, craw, dtype, defect=None, box=None, physical_units=False):
    """x [.., B, C, H, W] -> per field the binned values [.., B, H, W]: a channel raw (minus craw in float32), a derived field physical
    in dtype.  physical_units: the channels physical as well (for choosing ranges; a centred channel u sd (x - craw))."""
    der = None
    out = []
    for k in kinds:
        if k < 4:
            v = x[..., k, :, :]
            if craw is not None and defect != "center_skip":
                v = v - craw[:, k]
            if physical_units:
                B, Cc = x.shape[-4], x.shape[-3]
                if craw is None:
                    v = physical(x, mu, sd, u, np.float64)[..., k, :, :]
                else:
                    v = (_scale(u, B, Cc, np.float64)[:, k] * float(np.asarray(sd, F32)[k])).reshape(B, 1, 1) * v.astype(np.float64)
            out.append(v)
        else:
            if der is None:
                der = derived(x, mu, sd, u, grid, dtype, wrap=defect == "wrap", box=box if defect == "region_pads" else None)
            out.append(der[k - 4])
    return out


def near_bound(x, kinds, mu, sd, u, grid):
    """Per derived field the bound 14 * 2^-24 * A [.., B, H, W] in fp64 (None for a channel field)."""
    B, Cc = x.shape[-4], x.shape[-3]
    m, s = np.abs(np.asarray(mu, F32).astype(np.float64)).reshape(Cc, 1, 1), np.asarray(sd, F32).astype(np.float64).reshape(Cc, 1, 1)
    a = _scale(u, B, Cc, np.float64).reshape(B, Cc, 1, 1) * (s * np.abs(x.astype(np.float64)) + m)
    au, av = _pad(a[..., 0, :, :], False), _pad(a[..., 1, :, :], False)
    sx = lambda p: 2 * p[..., 1:-1, 2:] + p[..., :-2, 2:] + p[..., 2:, 2:] + 2 * p[..., 1:-1, :-2] + p[..., :-2, :-2] + p[..., 2:, :-2]   # noqa: E731
    sy = lambda p: 2 * p[..., 2:, 1:-1] + p[..., 2:, :-2] + p[..., 2:, 2:] + 2 * p[..., :-2, 1:-1] + p[..., :-2, :-2] + p[..., :-2, 2:]   # noqa: E731
    rdx, rdy = rd_of(grid, np.float64)
    A = {4: a[..., 0, :, :] + a[..., 1, :, :], 5: sx(av) * rdx + sy(au) * rdy, 6: sx(au) * rdx + sy(av) * rdy}
    return [NEAR * A[k] if k >= 4 else None for k in kinds]


# ---- edges ----------------------------------------------------------------------------------------------------------------------------
def edge_tables(kinds, ranges, n, mu, sd, u, centred):
    """-> (E [B, F, n + 1] fp64 physical, e [B, F, n + 1] float32 device table)."""
    B, F = ranges.shape[:2]
    Cc = len(mu)
    sc = _scale(u, B, Cc, np.float64)
    m, s = np.asarray(mu, F32).astype(np.float64), np.asarray(sd, F32).astype(np.float64)
    j = np.arange(n + 1, dtype=np.float64)
    E = ranges[..., 0:1] + j * (ranges[..., 1:2] - ranges[..., 0:1]) / n
    e = E.copy()
    for f, k in enumerate(kinds):
        if k < 4:
            e[:, f] = E[:, f] / (sc[:, k:k + 1] * s[k]) if centred else (E[:, f] / sc[:, k:k + 1] - m[k]) / s[k]
    return E, e.astype(F32)


# ---- integer reference ------------------------------------------------------------------------------------------------------------------
def _indices(v, e, defect):
    """v [.., B, H, W], e [B, n + 1] -> idx = #{j : v >= e_j} by searchsorted, case by case (in the dtype of v)."""
    out = np.zeros(v.shape, np.int64)
    for b in range(e.shape[0]):
        out[..., b, :, :] = np.searchsorted(e[b].astype(v.dtype), v[..., b, :, :], side="left" if defect == "edge_side" else "right")
    return out


def tables(x, c, dtype, defect=None):
    """x [N, B, C, H, W] (rows: the members, or the target alone) of case dict c -> (marg [N, B, R, F, nb + 2], joint
    [N, B, R, P, nbj + 2, nbj + 2]) int64, the tables of every row."""
    ks, hw = kinds_of(c["fields"]), c["hw"]
    pairs = pairs_of(c["fields"], c["joint"])
    boxes = boxes_of(c["regions"], hw)
    craw = None if c["center"] is None else c_raw(c["center"], c["mu"], c["sd"], c["u"])
    _, e = edge_tables(ks, c["ranges"], c["nb"], c["mu"], c["sd"], c["u"], craw is not None)
    jk = [ks[i] for pr in pairs for i in pr]
    _, je = edge_tables(jk, c["ranges"][:, [i for pr in pairs for i in pr]], c["nbj"], c["mu"], c["sd"], c["u"], craw is not None)
    N, B = x.shape[:2]
    nb, nbj = c["nb"], c["nbj"]
    marg = np.zeros((N, B, len(boxes), len(ks), nb + 2), np.int64)
    joint = np.zeros((N, B, len(boxes), len(pairs), nbj + 2, nbj + 2), np.int64)
    vals = None
    for r, (x0, x1, y0, y1) in enumerate(boxes):
        if vals is None or defect == "region_pads":
            vals = field_values(x, ks, c["mu"], c["sd"], c["u"], c["grid"], craw, dtype, defect, (x0, x1, y0, y1))
            idx = [_indices(v, e[:, f], defect) for f, v in enumerate(vals)]
            jidx = [(_indices(vals[a], je[:, 2 * p], defect), _indices(vals[bq], je[:, 2 * p + 1], defect)) for p, (a, bq) in enumerate(pairs)]
        if defect == "region_closed":
            x1, y1 = min(x1 + 1, hw[1]), min(y1 + 1, hw[0])
        rows = np.arange(N * B, dtype=np.int64).reshape(-1, 1)
        flat = lambda a: a[:, :, y0:y1, x0:x1].reshape(N * B, -1)             # noqa: E731
        for f in range(len(ks)):
            marg[:, :, r, f] = np.bincount((flat(idx[f]) + rows * (nb + 2)).ravel(), minlength=N * B * (nb + 2)).reshape(N, B, nb + 2)
        for p in range(len(pairs)):
            ia, ib = flat(jidx[p][0]), flat(jidx[p][1])
            if defect == "joint_transposed":
                ia, ib = ib, ia
            # one 2-d histogram for all rows: the row number is folded into the first coordinate
            first = np.arange(N * B * (nbj + 2) + 1) - 0.5
            h2 = np.histogram2d((ia + rows * (nbj + 2)).ravel(), ib.ravel(), bins=[first, np.arange(nbj + 3) - 0.5])[0]
            joint[:, :, r, p] = h2.astype(np.int64).reshape(N, B, nbj + 2, nbj + 2)
    if defect == "drop_overflow":
        marg[..., -1] = 0
        joint[..., -1, :] = 0
        joint[..., :, -1] = 0
    return marg, joint


def integers(c, dtype=F32, defect=None):
    """-> the integer outputs of EnsemblePdfs for case dict c, int64, plus member_steps: every member's table of every step."""
    xs, tgt, t_start = c["xs"], c["tgt"], c["t_start"]
    Tn, S, B = xs.shape[:3]
    em, ej, tm, tjn = [], [], [], []
    for t in range(Tn):
        a, bq = tables(xs[t], c, dtype, defect)
        em.append(a)
        ej.append(bq)
        a, bq = tables(tgt[t][None], c, dtype, defect)
        tm.append(a[0])
        tjn.append(bq[0])
    em, ej, tm, tjn = np.stack(em), np.stack(ej), np.stack(tm), np.stack(tjn)  # [T, S, B, ..], [T, B, ..]
    pool, poolj = em.sum(1), ej.sum(1)
    if defect == "target_counted":
        pool, poolj = pool + tm, poolj + tjn
    t0 = 0 if defect == "untimed_counted" else t_start
    mem = em[t0:].sum(0)                                                     # [S, B, R, F, nb + 2]
    if defect == "member_pooled":
        mem = np.broadcast_to(mem.sum(0, keepdims=True), mem.shape).copy()
    out = {"pdf_count": pool.swapaxes(0, 1), "target_count": tm.swapaxes(0, 1), "joint_count": poolj.swapaxes(0, 1),
           "target_joint_count": tjn.swapaxes(0, 1), "time_member_count": mem.swapaxes(0, 1), "time_count": mem.sum(0),
           "time_target_count": tm[t0:].sum(0), "time_joint_count": poolj[t0:].sum(0), "time_target_joint_count": tjn[t0:].sum(0)}
    if defect == "target_counted":
        out["time_count"] = pool[t0:].sum(0)
    out["member_steps"] = em                                                 # [T, S, B, R, F, nb + 2]: every member's table of every step
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


# ---- float reference --------------------------------------------------------------------------------------------------------------------
def _density(cnt, h):
    tot = cnt.sum(-1, keepdims=True).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (cnt[..., 1:-1] / tot) / h


def _w1_one(p, q):
    """The integral of |F^-1 - G^-1| over (0, 1] in bin widths, on the merged breakpoints; the cumulative counts are cross-multiplied
    to the common denominator Np Nq, so the breakpoints are exact integers."""
    Np, Nq = int(p.sum()), int(q.sum())
    if Np == 0 or Nq == 0:
        return float("nan")
    cp, cq = np.cumsum(p).astype(object) * Nq, np.cumsum(q).astype(object) * Np
    ts = sorted(set(cp.tolist()) | set(cq.tolist()) | {0})
    tot, den = 0, Np * Nq
    for lo, hi in zip(ts[:-1], ts[1:]):
        mid2 = lo + hi                                                        # twice the midpoint
        ip = next(i for i, v in enumerate(cp) if 2 * v >= mid2)
        iq = next(i for i, v in enumerate(cq) if 2 * v >= mid2)
        tot += (hi - lo) * abs(ip - iq)
    return float(tot) / float(den)


def _entropy(P):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(P > 0, P * np.log2(np.where(P > 0, P, 1.0)), 0.0).sum(-1)


def _js(p, q):
    with np.errstate(invalid="ignore", divide="ignore"):
        P, Q = p / p.sum(-1, keepdims=True).astype(np.float64), q / q.sum(-1, keepdims=True).astype(np.float64)
    out = _entropy(0.5 * (P + Q)) - 0.5 * (_entropy(P) + _entropy(Q))
    return np.where((p.sum(-1) == 0) | (q.sum(-1) == 0), np.nan, out)                # a distribution with no samples gives NaN


def _w1(p, q, h):
    p, q = np.broadcast_arrays(p, q)
    out = np.zeros(p.shape[:-1])
    for i in np.ndindex(*p.shape[:-1]):
        out[i] = _w1_one(p[i], q[i])
    return out * h


def floats(ints, ranges, nb):
    """The float outputs in fp64 from the integer outputs (int64 arrays) by the formulas of this file."""
    B, F = ranges.shape[:2]
    h = (ranges[..., 1] - ranges[..., 0]) / nb
    h5, h4 = h.reshape(B, 1, 1, F, 1), h.reshape(B, 1, F, 1)
    o = {"pdf": _density(ints["pdf_count"], h5), "target_pdf": _density(ints["target_count"], h5),
         "time_pdf": _density(ints["time_count"], h4), "time_target_pdf": _density(ints["time_target_count"], h4)}
    dm = _density(ints["time_member_count"], h5)
    o["time_pdf_mean"], o["time_pdf_std"] = dm.mean(1), dm.std(1)
    o["w1"], o["js"] = _w1(ints["pdf_count"], ints["target_count"], h5[..., 0]), _js(ints["pdf_count"], ints["target_count"])
    o["time_w1"], o["time_js"] = _w1(ints["time_count"], ints["time_target_count"], h4[..., 0]), _js(ints["time_count"], ints["time_target_count"])
    o["time_member_w1"] = _w1(ints["time_member_count"], ints["time_target_count"][:, None], h5[..., 0])
    fl = lambda a: a.reshape(a.shape[:-2] + (a.shape[-2] * a.shape[-1],))                            # noqa: E731
    o["time_joint_js"] = _js(fl(ints["time_joint_count"]), fl(ints["time_target_joint_count"]))
    return o


@functools.lru_cache(maxsize=None)
def int_reference(idx):
    c = int_case(idx)
    ints = integers(c)
    return c, ints, floats(ints, c["ranges"], c["nb"])


@functools.lru_cache(maxsize=None)
def real_reference(idx):
    c = real_case(idx)
    ints = integers(c)
    return c, ints, floats(ints, c["ranges"], c["nb"])


@functools.lru_cache(maxsize=None)
def near_counts(idx):
    """Real case idx -> (ints64: the integer outputs with the derived fields in fp64, near [T, B, R, F, nb + 1]: per step, case,
    region, field and edge the number of samples (members and target) whose fp64 value lies within the bound of the edge, samples:
    the samples per (step, case, region))."""
    c = real_case(idx)
    ks, hw = kinds_of(c["fields"]), c["hw"]
    boxes = boxes_of(c["regions"], hw)
    _, e = edge_tables(ks, c["ranges"], c["nb"], c["mu"], c["sd"], c["u"], c["center"] is not None)
    allx = np.concatenate([c["xs"], c["tgt"][:, None]], 1)                   # [T, S + 1, B, C, H, W]
    vals = field_values(allx, ks, c["mu"], c["sd"], c["u"], c["grid"], None, np.float64)
    bound = near_bound(allx, ks, c["mu"], c["sd"], c["u"], c["grid"])
    Tn, B = allx.shape[0], c["B"]
    near = np.zeros((Tn, B, len(boxes), len(ks), c["nb"] + 1), np.int64)
    for f, k in enumerate(ks):
        if k < 4:
            continue
        for b in range(B):
            for j in range(c["nb"] + 1):
                hit = np.abs(vals[f][:, :, b] - float(e[b, f, j])) <= bound[f][:, :, b]          # [T, S + 1, H, W]
                for r, (x0, x1, y0, y1) in enumerate(boxes):
                    near[:, b, r, f, j] = hit[:, :, y0:y1, x0:x1].sum((1, 2, 3))
    samples = np.array([(x1 - x0) * (y1 - y0) * allx.shape[1] for x0, x1, y0, y1 in boxes], np.int64)
    return integers(c, np.float64), near, samples


def defect_applies(defect, c):
    ks = kinds_of(c["fields"])
    return {"edge_side": True, "drop_overflow": True, "region_closed": any(x1 < c["hw"][1] or y1 < c["hw"][0] for _, x1, _, y1 in boxes_of(c["regions"], c["hw"])),
            "region_pads": c["regions"] is not None and any(k >= 5 for k in ks) and c["hw"][0] * c["hw"][1] > 2,
            "wrap": any(k >= 5 for k in ks) and any(x0 == 0 or y0 == 0 or x1 == c["hw"][1] or y1 == c["hw"][0]
                                                     for x0, x1, y0, y1 in boxes_of(c["regions"], c["hw"])), "center_skip": c["center"] is not None and any(k < 4 for k in ks),
            "joint_transposed": len(c["joint"]) > 0, "member_pooled": c["S"] > 1, "target_counted": True,
            "untimed_counted": c["t_start"] > 0}[defect]


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def check_floats(got, ref, what):
    """Every float32 output within 2^-24 |ref| + 2^-40 of the reference, NaNs where the reference has them -> the worst share."""
    worst = 0.0
    for key in FLOAT_KEYS:
        g, r = np.asarray(got[key]), np.asarray(ref[key], np.float64)
        assert g.dtype == F32 and g.shape == r.shape, "%s %s: %s %s against %s" % (what, key, g.dtype, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s %s: NaNs differ" % (what, key)
        ok = ~np.isnan(r)
        share = np.abs(g.astype(np.float64)[ok] - r[ok]) / (U24 * np.abs(r[ok]) + TOL_ABS)
        if share.size:
            assert float(share.max()) <= 1.0, "%s %s: worst error is %.3f of its bound" % (what, key, float(share.max()))
            worst = max(worst, float(share.max()))
    return worst


def check_integers(got, ref, what, keys=INT_KEYS):
    for key in keys:
        g = np.asarray(got[key])
        assert g.dtype == np.int64 and g.shape == ref[key].shape, "%s %s: %s %s against %s" % (what, key, g.dtype, g.shape, ref[key].shape)
        assert np.array_equal(g, ref[key]), "%s %s: %d integers differ" % (what, key, int((g != ref[key]).sum()))


def check_identities(ints, c, what):
    """Counts of a field sum to S |region| (the target's to |region|), time_count is the sum of pdf_count over the timed steps, and a
    joint table's marginals are the marginal histograms when nbj == nb."""
    S, t0 = c["S"], c["t_start"]
    area = np.array([(x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in boxes_of(c["regions"], c["hw"])], np.int64)
    assert np.array_equal(ints["pdf_count"].sum(-1), np.broadcast_to((S * area)[:, None], ints["pdf_count"].shape[:-1])), what
    assert np.array_equal(ints["target_count"].sum(-1), np.broadcast_to(area[:, None], ints["target_count"].shape[:-1])), what
    assert np.array_equal(ints["time_count"], ints["pdf_count"][:, t0:].sum(1)), what
    assert np.array_equal(ints["time_count"], ints["time_member_count"].sum(1)), what
    assert np.array_equal(ints["time_target_count"], ints["target_count"][:, t0:].sum(1)), what
    assert np.array_equal(ints["time_joint_count"], ints["joint_count"][:, t0:].sum(1)), what
    if c["nbj"] == c["nb"]:
        for p, (fi, fj) in enumerate(pairs_of(c["fields"], c["joint"])):
            assert np.array_equal(ints["joint_count"][:, :, :, p].sum(-1), ints["pdf_count"][:, :, :, fi]), what
            assert np.array_equal(ints["joint_count"][:, :, :, p].sum(-2), ints["pdf_count"][:, :, :, fj]), what
