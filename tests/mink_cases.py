"""The cases and the references of the excursion-set morphology tests (test_mink_cpu.py, test_mink_gpu.py).

The int64 reference is written from the definitions of include/tmglow_hip_mink.h: J direct compares give the rank, the set of level j
is {rank > j}, and the five counts are sums over slices of the mask joined by `&`.  A second statement counts connected pieces and
holes with a small flood-fill labeller over the padded mask and its complement (chi4 = pieces4 - holes8, chi8 = pieces8 - holes4),
cross-checked against scipy.ndimage.label where scipy imports.  The fp64 formulas of every host output are restated here on numpy
arrays.  Named mutations of the reference are the ways a kernel of this shape can go wrong; the comparison the GPU test uses must
catch each of them."""
import functools

import numpy as np

U24 = 2.0 ** -24
TOL_ABS = 2.0 ** -40
TIMED = (False, True, True)                                                   # the steps of every case: the first one is not timed
TILE = (64, 63)                                                               # the kernel's tile (rows, columns): the plan reports it
GRID = (0.5, 0.25)                                                            # (dx along W, dy along H)
HIGH, LOW = 1000.0, -1000.0                                                   # above / below every ladder of the table
CURVES = ("count", "edges", "euler4", "euler8")
INT_KEYS = ("mink_edges", "mink_euler4", "mink_euler8", "mink_below", "mink_equal")
FLOAT_KEYS = ("mink_area", "mink_perimeter", "mink_euler4_density", "mink_euler8_density", "mink_mean", "mink_std", "mink_l1")
STEP_KEYS = ("mink_raw",) + INT_KEYS + FLOAT_KEYS
ALL_KEYS = STEP_KEYS + tuple("time_" + k for k in STEP_KEYS) + ("mink_levels",)
MUTATIONS = ("nonstrict", "row_wrap", "tile_edge_dropped", "tile_edge_twice", "nd_three", "nan_in")       # of the raw counts
CURVE_MUTATIONS = ("chi8_plus",)                                                                        # of the curves

# (S, B, C, (H, W), F, J, kind, padded): padded feeds channel slices of 4-channel storage.  The fields sit on every edge of the
# 64 x 63 tile; these small grids run one member per block (S = 1, 2, 3, 5), GROUP_CASES groups of 2 and 4.
TABLE = [
    (1, 2, 2, (1, 1), 1, 1, "int", False),
    (2, 2, 3, (1, 7), 3, 2, "int", True),
    (3, 2, 4, (2, 2), 4, 31, "smooth", False),
    (5, 2, 3, (3, 130), 1, 32, "int", True),
    (5, 2, 3, (64, 63), 3, 32, "smooth", False),
    (2, 2, 2, (65, 62), 2, 2, "int", True),
    (3, 2, 3, (70, 69), 3, 31, "int", False),
    (2, 1, 4, (70, 69), 1, 1, "smooth", False),
    (2, 2, 3, (17, 23), 3, 4, "allin", False),
    (2, 2, 3, (17, 23), 3, 4, "nonein", True),
    (3, 2, 3, (33, 70), 2, 8, "ties", False),
    (3, 2, 3, (33, 70), 2, 8, "decr", True),
    (2, 2, 3, (70, 69), 3, 32, "nonfinite", False),
]
# one tile x 512 cases: 512 x ceil(5 / 4) >= 1024 blocks, so the five members run as groups of 4 + 1; x 350 cases: 350 x 2 < 1024 <=
# 350 x 3, groups of 2 + 2 + 1 (and of 2 + 1, 1 in the chunkings: every side of the group)
GROUP_CASES = [(5, 512, 2, (1, 7), 2, 3, "int", False), (5, 350, 2, (1, 7), 1, 2, "int", False)]


def group(planes, k):
    """The members one block takes of a chunk of k (include/tmglow_hip_mink.h), planes = tiles x cases."""
    G = 4 if planes * -(-k // 4) >= 1024 else 2 if planes * -(-k // 2) >= 1024 else 1
    return min(G, k)


def planes(case):
    S, B, Cc, hw, F, J, kind, _ = case
    return -(-hw[0] // TILE[0]) * -(-hw[1] // TILE[1]) * B


def chunk_sizes(S, kind):
    """0: one chunk; 1: one member per chunk; 2: an uneven split."""
    if kind == 0 or S == 1:
        return [S]
    if kind == 1:
        return [1] * S
    return [S // 2, S - S // 2]


def fields_for(Cc, F):
    """F distinct channels of Cc, not in storage order when there is a choice."""
    return tuple(reversed(range(Cc)))[:F] if F < Cc else tuple((c + 1) % Cc for c in range(Cc))


def ladder(kind, F, J):
    """The physical ladder [F][J] of a case, as Python floats, strictly ascending (the test's out_mu = 0, out_std = 1, u = 1: the raw
    ladder is its float32 rounding)."""
    if kind in ("int", "decr"):                                               # ON data values: multiples of 0.5
        base = [0.5 * (j - J // 2) for j in range(J)]
    elif kind == "ties":                                                      # neighbours that differ in fp64 and are equal in float32
        base = [0.5 * (j // 2 - J // 4) + (1e-12 if j % 2 else 0.0) for j in range(J)]
    elif kind == "allin":
        base = [-10.0 + j for j in range(J)]
    elif kind == "nonein":
        base = [5.0 + j for j in range(J)]
    else:
        base = [0.0] if J == 1 else [-1.5 + 3.0 * j / (J - 1) for j in range(J)]
    return tuple(tuple(v + 0.25 * (f if kind in ("smooth", "nonfinite") else 0) for v in base) for f in range(F))


def raw_ladder(case):
    """The raw ladder [B, F, J] float32 the device compares with; `decr` runs it in decreasing order."""
    S, B, Cc, hw, F, J, kind, _ = case
    thr = np.array(ladder(kind, F, J), np.float64).astype(np.float32)
    if kind == "decr":
        thr = thr[:, ::-1]
    return np.ascontiguousarray(np.broadcast_to(thr, (B, F, J)))


def tile_corners(hw):
    """The last pixel (row, column) of every tile that has a tile below or to its right: rows 63, 127, .., columns 62, 125, ..; a
    field that is one tile high (wide) still has its column (row) edges, marked at its middle row (column)."""
    Hh, Ww = hw
    rows = [r for r in range(TILE[0] - 1, Hh - 1, TILE[0])]
    cols = [c for c in range(TILE[1] - 1, Ww - 1, TILE[1])]
    if not rows and not cols:
        return []
    return [(r, c) for r in (rows or [max(0, Hh // 2 - 1)]) for c in (cols or [max(0, Ww // 2 - 1)])]


def plant(x, variant):
    """At every tile corner of the field x [H, W]: clear a window to LOW, then set to HIGH (0) the full quad that straddles the
    corner, (1) its diagonal pair, (2) a horizontal pair across the vertical tile edge and a vertical pair across the horizontal one,
    (3) the other diagonal.  Pixels outside the field are skipped."""
    Hh, Ww = x.shape
    for r, c in tile_corners((Hh, Ww)):
        x[max(0, r - 3):r + 5, max(0, c - 3):c + 5] = LOW
        px = {0: [(r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1)], 1: [(r, c), (r + 1, c + 1)],
              2: [(r - 2, c), (r - 2, c + 1), (r, c - 2), (r + 1, c - 2)], 3: [(r, c + 1), (r + 1, c)]}[variant % 4]
        for i, j in px:
            if 0 <= i < Hh and 0 <= j < Ww:
                x[i, j] = HIGH


def make_inputs(case, seed):
    """-> (xs [Tk, S, B, C, H, W], tgt [Tk, B, C, H, W]) float32, Tk = len(TIMED)."""
    S, B, Cc, hw, F, J, kind, _ = case
    rng = np.random.default_rng(seed)
    Tk, (Hh, Ww) = len(TIMED), hw
    shape = (Tk, S + 1, B, Cc, Hh, Ww)
    if kind in ("int", "ties", "decr"):
        v = 0.5 * rng.integers(-J // 2 - 2, J // 2 + 3, shape)                # multiples of 0.5 around the ladder: ties with it
    else:
        yy, xx = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
        ph = rng.uniform(0, 2 * np.pi, shape[:4] + (2, 1, 1))
        k1, k2 = rng.uniform(0.05, 0.4, shape[:4] + (2, 1, 1))[..., 0, :, :], rng.uniform(0.05, 0.4, shape[:4] + (2, 1, 1))[..., 1, :, :]
        v = np.sin(k1 * xx + ph[..., 0, :, :]) * np.cos(k2 * yy + ph[..., 1, :, :]) + 0.2 * rng.standard_normal(shape)
        if kind in ("allin", "nonein"):
            v = np.clip(v, -2.0, 2.0)
    v = v.astype(np.float32)
    for t in range(Tk):
        for m in range(S + 1):
            for b in range(B):
                for c in range(Cc):
                    if kind not in ("allin", "nonein"):
                        plant(v[t, m, b, c], t + m + b + c)
    if kind == "nonfinite":
        n = v.size
        flat = v.reshape(-1)
        idx = rng.choice(n, 3 * max(6, n // 50), replace=False)
        third = len(idx) // 3
        flat[idx[:third]] = np.nan
        flat[idx[third:2 * third]] = np.inf
        flat[idx[2 * third:]] = -np.inf
    return np.ascontiguousarray(v[:, :S]), np.ascontiguousarray(v[:, S])


@functools.lru_cache(maxsize=None)
def inputs(idx):
    xs, tgt = make_inputs(TABLE[idx], 100 + idx)
    xs.setflags(write=False)
    tgt.setflags(write=False)
    return xs, tgt


# ---- the int64 reference, from the definitions ------------------------------------------------------------------------------------------
def counts(x, thr, mutation=None):
    """x [H, W] float32, thr [J] float32 -> [J, 5] int64 (N, Nh, Nv, Nq, Nd) of the sets {rank > j}, rank = #{j : x > thr_j}."""
    J = len(thr)
    rank = np.zeros(x.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(J):
            rank += (x >= thr[j]) if mutation == "nonstrict" else (x > thr[j])
    if mutation == "nan_in":
        rank[np.isnan(x)] = J
    out = np.zeros((J, 5), np.int64)
    th, tw = TILE
    for j in range(J):
        m = rank > j
        a, b, c, d = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
        hp, vp, q = m[:, :-1] & m[:, 1:], m[:-1] & m[1:], a & b & c & d
        dg = (a & d & ~b & ~c) | (b & c & ~a & ~d)
        if mutation == "nd_three":
            dg = dg | ((a.astype(np.int64) + b + c + d) == 3)
        N, Nh, Nv, Nq, Nd = m.sum(), hp.sum(), vp.sum(), q.sum(), dg.sum()
        if mutation == "row_wrap":                                            # flat neighbours p, p + 1, across the row ends too
            f = m.reshape(-1)
            Nh = (f[:-1] & f[1:]).sum()
        if mutation in ("tile_edge_dropped", "tile_edge_twice"):              # what straddles a tile edge: lost, or counted by both tiles
            s = -1 if mutation == "tile_edge_dropped" else 1
            ce = (np.arange(m.shape[1] - 1) % tw) == tw - 1
            re_ = (np.arange(m.shape[0] - 1) % th) == th - 1
            Nh = Nh + s * hp[:, ce].sum()
            Nv = Nv + s * vp[re_].sum()
            edge = re_[:, None] | ce[None, :]
            Nq = Nq + s * (q & edge).sum()
            Nd = Nd + s * (dg & edge).sum()
        out[j] = (N, Nh, Nv, Nq, Nd)
    return out


def reference(xs, tgt, thr, fields, mutation=None):
    """xs [Tk, S, B, C, H, W], tgt [Tk, B, C, H, W], thr [B, F, J] float32 -> mink_raw [B, Tk, F, S + 1, J, 5] int64."""
    Tk, S, B = xs.shape[:3]
    F, J = thr.shape[1:]
    out = np.zeros((B, Tk, F, S + 1, J, 5), np.int64)
    for b in range(B):
        for t in range(Tk):
            for f, ch in enumerate(fields):
                for m in range(S + 1):
                    x = tgt[t, b, ch] if m == S else xs[t, m, b, ch]
                    out[b, t, f, m] = counts(np.asarray(x, np.float32), thr[b, f], mutation)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(idx):
    case = TABLE[idx]
    xs, tgt = inputs(idx)
    ref = reference(xs, tgt, raw_ladder(case), fields_for(case[2], case[4]))
    ref.setflags(write=False)
    return ref


def curves(raw, mutation=None):
    """raw [..., J, 5] -> the integer curves [..., 4, J]: N, edges, chi4, chi8."""
    N, Nh, Nv, Nq, Nd = (raw[..., i] for i in range(5))
    chi4 = N - Nh - Nv + Nq
    chi8 = chi4 + Nd if mutation == "chi8_plus" else chi4 - Nd
    return np.stack([N, 4 * N - 2 * Nh - 2 * Nv, chi4, chi8], -2)


# ---- the second statement: pieces and holes by flood fill --------------------------------------------------------------------------------
def label_count(mask, conn):
    """The number of conn-connected (4 or 8) components of a boolean mask: a flood fill with an explicit stack."""
    Hh, Ww = mask.shape
    todo = mask.copy()
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    n = 0
    for i0, j0 in zip(*np.nonzero(mask)):
        if not todo[i0, j0]:
            continue
        n += 1
        todo[i0, j0] = False
        stack = [(i0, j0)]
        while stack:
            i, j = stack.pop()
            for di, dj in steps:
                a, b = i + di, j + dj
                if 0 <= a < Hh and 0 <= b < Ww and todo[a, b]:
                    todo[a, b] = False
                    stack.append((a, b))
    return n


def scipy_count(mask, conn):
    from scipy import ndimage
    return int(ndimage.label(mask, structure=np.ones((3, 3), int) if conn == 8 else None)[1])


def euler_by_labels(mask, count=label_count):
    """(chi4, chi8) of a mask: 4-connected pieces minus the 8-connected holes, 8-connected pieces minus the 4-connected holes; the
    holes are the components of the complement of the padded mask other than the outer one."""
    pad = np.pad(mask, 1)
    return count(pad, 4) - (count(~pad, 8) - 1), count(pad, 8) - (count(~pad, 4) - 1)


def edges_by_differences(mask):
    """The exposed unit edges of a mask: the differences of the padded mask along both axes."""
    p = np.pad(mask, 1).astype(np.int64)
    return int(np.abs(np.diff(p, axis=0)).sum() + np.abs(np.diff(p, axis=1)).sum())


def mask_of(x, thr, j):
    with np.errstate(invalid="ignore"):
        return sum((x > t).astype(np.int64) for t in thr) > j


# ---- the host outputs in fp64 ---------------------------------------------------------------------------------------------------------------
def outputs_reference(raw, S, Hh, Ww, grid, steps, levels, mutation=None):
    """raw [..., S + 1, J, 5] int64, levels broadcastable to [..., J] float64 -> the keys of tmg_ops.mink_outputs, floats in fp64."""
    dx, dy = grid
    P = Hh * Ww * steps
    A = P * dx * dy
    N, Nh, Nv = (raw[..., i].astype(np.float64) for i in range(3))
    cur = curves(raw, mutation)
    per = (dy * (2 * N - 2 * Nh) + dx * (2 * N - 2 * Nv)) / A
    o = {"mink_area": N / P, "mink_perimeter": per, "mink_edges": cur[..., 1, :], "mink_euler4": cur[..., 2, :], "mink_euler8": cur[..., 3, :],
         "mink_euler4_density": cur[..., 2, :] / A, "mink_euler8_density": cur[..., 3, :] / A}
    mem, tg = cur[..., :S, :, :], cur[..., S:, :, :]
    o["mink_mean"] = mem.astype(np.float64).mean(-3)
    o["mink_std"] = mem.astype(np.float64).std(-3)
    o["mink_below"] = (mem < tg).sum(-3)
    o["mink_equal"] = (mem == tg).sum(-3)
    lv = np.asarray(levels, np.float64)
    four = np.stack([N / P, per, cur[..., 2, :] / A, cur[..., 3, :] / A], -2)   # [..., S + 1, 4, J]
    d = np.abs(four[..., :S, :, :] - four[..., S:, :, :])
    w = np.diff(lv, axis=-1)[..., None, None, :]
    o["mink_l1"] = (0.5 * (d[..., 1:] + d[..., :-1]) * w).sum(-1)
    return o


def full_reference(raw, S, Hh, Ww, grid, levels, timed=TIMED, mutation=None):
    """raw [B, Tk, F, S + 1, J, 5], levels [B, F, J] -> every key of EnsembleMorphology.finalize."""
    out = {"mink_raw": raw, "mink_levels": np.asarray(levels, np.float64)}
    out.update(outputs_reference(raw, S, Hh, Ww, grid, 1, np.asarray(levels)[:, None], mutation))
    traw = raw[:, [t for t, on in enumerate(timed) if on]].sum(1)
    out["time_mink_raw"] = traw
    for k, v in outputs_reference(traw, S, Hh, Ww, grid, sum(timed), levels, mutation).items():
        out["time_" + k] = v
    return out


def mismatches(got, want, keys):
    """The keys whose arrays are not equal bit for bit."""
    return [k for k in keys if not (np.asarray(got[k]).shape == np.asarray(want[k]).shape and np.array_equal(got[k], want[k]))]


def check_floats(got, want, keys, what):
    """Every float32 output within 2^-24 |ref| + 2^-40 of the fp64 formula -> the worst share of that tolerance."""
    worst = 0.0
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k], np.float64)
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        err, tol = np.abs(g.astype(np.float64) - w), U24 * np.abs(w) + TOL_ABS
        assert bool((err <= tol).all()), "%s: %s off by %.3e of its tolerance" % (what, k, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()) if err.size else 0.0)
    return worst


def levels_of(case):
    S, B, Cc, hw, F, J, kind, _ = case
    return np.broadcast_to(np.array(ladder(kind, F, J), np.float64), (B, F, J))
