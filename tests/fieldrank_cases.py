"""Cases and references of the ensemble field-rank tests (tests/test_fieldranks_cpu.py, tests/test_fieldranks_gpu.py): the sweep, the
seeded inputs, the int64 numpy reference written from the definitions, a brute-force band depth, and the comparison both files use.

Definitions (case b, kept step t, channel c, pixel p).  Rows x_0 .. x_{S-1} are the members, x_S is the target, raw normalised fp32.
For row i over the S other rows j != i:
  lt = #{j : x_j < x_i}, eq = #{j : x_j == x_i}, gt = S - lt - eq
  A_i(p) = 2 lt + eq
  D_i(p) = C(S,2) - C(lt,2) - C(gt,2): the pairs {j, k} of other rows with min(x_j, x_k) <= x_i <= max(x_j, x_k)
  O(p)   = [lt_S == S or gt_S == S], target only
  pre_raw[b, t, c, i] = (sum_p A_i, sum_p D_i); outside_count[b, t, c] = sum_p O; time_outside_count[b, c, p] = sum over the timed t
Every quantity is an integer: the device result must EQUAL this reference; no tolerance appears anywhere."""
import functools
import itertools

import numpy as np
import torch

F32 = np.float32
T = 4
R = 8                 # FRANK_R of csrc/tmg_frank.hip: S + 1 rows fall on R - 1, R, R + 1, 2 R - 1, 2 R, 2 R + 1 and a ragged last block
FIELDS = ((5, 7), (16, 17), (3, 300))     # one partial wave; a second block of 16 lanes; a long row (four blocks, the last ragged)
SWEEP = [(S, B, Cc, hw) for S in (1, 2, 6, 7, 8, 15, 16, 17, 33) for B in (1, 3) for Cc in (2, 3, 4) for hw in FIELDS] \
    + [(1024, 1, 2, (5, 7))]
GROUPS = {2: ((0, 1),), 3: ((0, 1), (2,)), 4: ((0, 3), (1,))}      # per channel count; with 4 channels one is in no group


def features(idx):
    """(t_start, channel-padded y and target, chunking) of sweep entry idx; chunking 0: one member per chunk, 1: three members per
    chunk, 2: the whole ensemble.  Half the entries are padded, t_start is 0 or 2."""
    ih, ic, ib, iS = idx % 3, (idx // 3) % 3, (idx // 9) % 2, idx // 18
    return 2 * ((ih + ib + iS) % 2), (ih + ic) % 2 == 1, (ih + ic + ib + iS) % 3


def chunk_sizes(S, kind):
    per = (1, 3, S)[kind]
    return [min(per, S - m0) for m0 in range(0, S, per)]


@functools.lru_cache(maxsize=None)
def inputs(idx, ties=False):
    """Sweep entry idx -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W]) numpy float32, seeded.  Continuous: members N(0.3, 1) plus an
    offset per case, target N(0.3, 1).  ties: integers in {-2..2}, ties everywhere."""
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    return make_inputs(S, B, Cc, Hh, Ww, 8100 + idx, ties)


def make_inputs(S, B, Cc, Hh, Ww, seed, ties=False):
    g = torch.Generator().manual_seed(seed + (500000 if ties else 0))
    if ties:
        xs = torch.randint(-2, 3, (T, S, B, Cc, Hh, Ww), generator=g).float()
        tgt = torch.randint(-2, 3, (T, B, Cc, Hh, Ww), generator=g).float()
    else:
        xs = torch.randn(T, S, B, Cc, Hh, Ww, generator=g) + 0.3 + (0.2 * torch.arange(B, dtype=torch.float32) - 0.2).view(1, 1, B, 1, 1, 1)
        tgt = torch.randn(T, B, Cc, Hh, Ww, generator=g) + 0.3
    return xs.numpy(), tgt.numpy()


# ---- the reference: int64 numpy, from the definitions ------------------------------------------------------------------------------
MUTATIONS = ("le", "self", "open", "no_target", "no_clt")


def choose2(n):
    return n * (n - 1) // 2


def pixel_terms(xs, tgt, mutate=None):
    """xs [T, S, B, C, H, W], tgt [T, B, C, H, W] -> (A, D) int64 [T, S + 1, B, C, H, W] and O int64 [T, B, C, H, W].  Row j is
    compared with all rows at once; a row is not compared with itself.  mutate (tests/test_fieldranks_cpu.py): 'le' (<= for <),
    'self' (a row counts itself as equal), 'open' (the open band: lt gt), 'no_target' (the target is not among the other rows of a
    member), 'no_clt' (C(lt,2) is not subtracted)."""
    S = xs.shape[1]
    x = np.concatenate([xs, tgt[:, None]], axis=1)                           # [T, S + 1, ..]
    lt = np.zeros(x.shape, dtype=np.int64)
    eq = np.zeros(x.shape, dtype=np.int64)
    rows = np.arange(S + 1).reshape((1, S + 1) + (1,) * (x.ndim - 2))
    for j in range(S + 1):
        other = rows != j
        if mutate == "self":
            other = np.ones_like(other)
        if mutate == "no_target" and j == S:
            other = rows == -1
        xj = x[:, j:j + 1]
        lt += ((xj <= x) if mutate == "le" else (xj < x)) & other
        eq += (xj == x) & other
    gt = S - lt - eq
    A = 2 * lt + eq
    if mutate == "open":
        D = lt * gt
    else:
        D = choose2(S) - (0 if mutate == "no_clt" else choose2(lt)) - choose2(gt)
    O = ((lt[:, S] == S) | (gt[:, S] == S)).astype(np.int64)
    return A, D, O


def band_depth_brute(xs, tgt):
    """D by enumerating the pairs {j, k} of other rows and testing the closed band: int64 [T, S + 1, B, C, H, W].  Small S only."""
    S = xs.shape[1]
    x = np.concatenate([xs, tgt[:, None]], axis=1)
    D = np.zeros(x.shape, dtype=np.int64)
    for i in range(S + 1):
        others = [j for j in range(S + 1) if j != i]
        for j, k in itertools.combinations(others, 2):
            lo, hi = np.minimum(x[:, j], x[:, k]), np.maximum(x[:, j], x[:, k])
            D[:, i] += (lo <= x[:, i]) & (x[:, i] <= hi)
    return D


def rank_of_target(pre):
    """pre [.., S + 1] -> (below, equal) of the last row among the others."""
    return (pre[..., :-1] < pre[..., -1:]).sum(-1).astype(np.int64), (pre[..., :-1] == pre[..., -1:]).sum(-1).astype(np.int64)


def hist_loop(below, equal, S):
    """below, equal [B, Tn, G] -> [B, G, S + 1] float64: step by step, bin by bin."""
    B, Tn, G = below.shape
    h = np.zeros((B, G, S + 1), dtype=np.float64)
    for n in range(Tn):
        for b in range(B):
            for g in range(G):
                lo, k = int(below[b, n, g]), int(equal[b, n, g])
                for r in range(lo, lo + k + 1):
                    h[b, g, r] += 1.0 / (k + 1)
    return h


def reference(xs, tgt, t_start, groups, mutate=None):
    """-> dict of numpy arrays in the layout of EnsembleFieldRanks.finalize(); the steps t >= t_start are the timed ones."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    A, D, O = pixel_terms(xs, tgt, mutate)
    pre_raw = np.stack([A.sum((-2, -1)), D.sum((-2, -1))], axis=-1).transpose(2, 0, 3, 1, 4)      # [B, T, C, S + 1, 2]
    out = {"pre_raw": np.ascontiguousarray(pre_raw), "outside_count": np.ascontiguousarray(O.sum((-2, -1)).transpose(1, 0, 2)),
           "time_outside_count": O[t_start:].sum(0)}
    out["outside_frac"] = out["outside_count"].astype(np.float64) / float(Hh * Ww)
    out["time_outside_frac"] = out["time_outside_count"].astype(np.float64) / float(Tn - t_start)
    for j, kind in enumerate(("avg", "depth")):
        pre = np.stack([sum(pre_raw[:, :, ch, :, j] for ch in g) for g in groups], axis=2)        # [B, T, G, S + 1]
        out[kind + "_prerank"] = pre
        below, equal = rank_of_target(pre)
        out[kind + "_rank_below"], out[kind + "_rank_equal"] = below, equal
        out[kind + "_rank_hist"] = hist_loop(below[:, t_start:], equal[:, t_start:], S)
        traj = pre[:, t_start:].sum(1)
        out["traj_" + kind + "_prerank"] = traj
        out["traj_" + kind + "_rank_below"], out["traj_" + kind + "_rank_equal"] = rank_of_target(traj)
    out["depth_median"] = np.argmax(out["depth_prerank"][..., :S], axis=-1).astype(np.int64)      # the first of the largest
    out["traj_depth_median"] = np.argmax(out["traj_depth_prerank"][..., :S], axis=-1).astype(np.int64)
    return out


FLOAT_KEYS = ("outside_frac", "time_outside_frac", "avg_rank_hist", "depth_rank_hist")
DEVICE_KEYS = ("pre_raw", "outside_count", "time_outside_count")


def mismatches(got, ref):
    """The keys whose values are not EQUAL in dtype, shape and every element (the comparison of the GPU test; no tolerance)."""
    bad = [k for k in ref if k not in got]
    for k, v in ref.items():
        if k in got:
            g = np.asarray(got[k])
            want = np.float64 if k in FLOAT_KEYS else np.int64
            if g.dtype != want or v.dtype != want or g.shape != v.shape or not np.array_equal(g, v):
                bad.append(k)
    return bad + [k for k in got if k not in ref]


def assert_equal(got, ref, what):
    bad = mismatches(got, ref)
    assert not bad, "%s: %s differ from the int64 reference" % (what, bad)
