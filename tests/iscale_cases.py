"""Cases and references of the intensity-scale verification (tmg_iscale.hip / tmg_ops.EnsembleIntensityScale /
utils.modelPredIntensityScale).

The reference is written from the definitions in int64 numpy: the indicators of every member and of the target, zero-padded to a
multiple of the block size, `reshape(.., b, .., b).sum`, squared or multiplied, summed.  A second, independent statement
(`haar_energies`) builds the Haar components explicitly by `np.kron` of block means and takes their squared norms;
tests/test_iscale_cpu.py holds the two against each other, so the reference itself is tested.  `host_reference` restates
tmg_ops.iscale_outputs in fp64 from the definitions of the scores.

MUTATIONS names the defects the comparison must see: each changes at least one compared table on the case set (test_iscale_cpu.py).

Data: integer-valued fields with the thresholds ON data values (ties: strictness shows), smooth real fields (events with spatial
structure at several scales); with four events the third holds every pixel and the fourth none."""
import functools

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
TOL_ABS = 2.0 ** -40
RAW_KEYS = ("iscale_member_raw", "iscale_target_raw", "iscale_ens_raw")
FLOAT_KEYS = ("iscale_mse", "iscale_skill", "iscale_energy", "iscale_energy_bias", "iscale_brier", "iscale_brier_skill", "iscale_spread",
              "iscale_spread_skill")
ALL_KEYS = RAW_KEYS + FLOAT_KEYS + tuple("time_" + k for k in RAW_KEYS + FLOAT_KEYS) + ("iscale_blocks",)
MUTATIONS = ("origin_shifted", "non_strict", "remainder_dropped", "previous_target", "nan_in_event")
TIMED = (False, True, True)                                                    # Tk = 3 kept steps, the first one untimed
BIG = 1.0e30


def events_for(Cc, K):
    """K = 1: reverse flow; K = 4: both directions with thresholds on integer data values, then an event every finite pixel is in and
    one no pixel is in; every channel of 2..4 is reached."""
    return ((0, 0.0, "<"),) if K == 1 else ((0, 0.0, "<"), (1, 1.0, ">"), (Cc - 1, -BIG, ">"), (0, BIG, ">"))


# (S, B, C, (H, W), K, L, kind, padded): (H, W) on every edge of the 64 x 64 tile and of the 4 x 4 patch, each with L = 1, 3, 6; K 1
# and 4; S 1, 2, 5; C 2, 3, 4; padded: the chunk and the target are channel slices at offset 1 of 4-channel NaN-filled storage
TABLE = [
    (1, 2, 2, (1, 1), 1, 1, "int", False),
    (2, 2, 3, (1, 1), 4, 3, "int", True),
    (5, 2, 3, (1, 1), 4, 6, "smooth", False),
    (5, 2, 3, (3, 130), 4, 1, "smooth", True),
    (1, 2, 4, (3, 130), 1, 3, "int", False),
    (2, 2, 2, (3, 130), 4, 6, "int", False),
    (2, 2, 3, (64, 64), 1, 1, "smooth", False),
    (5, 2, 3, (64, 64), 4, 3, "int", True),
    (1, 2, 2, (64, 64), 4, 6, "smooth", True),
    (1, 2, 3, (65, 63), 4, 1, "int", False),
    (2, 2, 4, (65, 63), 1, 3, "smooth", False),
    (5, 2, 3, (65, 63), 4, 6, "int", True),
    (2, 2, 2, (70, 70), 4, 1, "smooth", True),
    (5, 2, 3, (70, 70), 1, 3, "int", False),
    (5, 2, 3, (70, 70), 4, 6, "smooth", False),
]
NONFINITE_CASE = (5, 2, 3, (65, 63), 4, 6, "smooth", True)
# the member groups of the chunk kernel (group below): the table's cases run 1 or 2 members per block; these run 4 and 8, with a last
# group of one member, on many small planes
GROUP_CASES = [(5, 32, 2, (3, 130), 4, 6, "int", False), (9, 64, 2, (3, 130), 4, 3, "smooth", False)]
SMALL = [(3, 2, 3, (5, 7), 4, 2, "int", False), (2, 1, 2, (8, 8), 4, 3, "smooth", False), (1, 2, 4, (1, 1), 1, 1, "int", False),
         (4, 1, 3, (9, 4), 4, 6, "smooth", False), (2, 1, 3, (3, 17), 1, 4, "int", False)]


def group(planes, k):
    """The members one block of tmg_ens_iscale_chunk takes of a chunk of k members when one member group is `planes` = tiles K B blocks:
    min(k, G) with G the largest of 8, 4, 2 that gives 512 blocks, else 2 (include/tmglow_hip_iscale.h)."""
    G = 8
    while G > 2 and planes * -(-k // G) < 512:
        G //= 2
    return min(G, k)


def planes(case):
    S, B, Cc, (Hh, Ww), K, L, kind, _ = case
    return -(-Hh // 64) * -(-Ww // 64) * K * B


def chunk_sizes(S, kind):
    """kind 0: one chunk (S,); 1: one member per chunk; 2: an uneven split, (2, 3) at S = 5."""
    if kind == 0 or S == 1:
        return [S]
    if kind == 1:
        return [1] * S
    a = max(1, (2 * S) // 5)
    return [a, S - a]


def make_inputs(case, seed):
    """-> xs [Tk, S, B, C, H, W], tgt [Tk, B, C, H, W] float32 (raw normalised values; the tests use out_mu = 0, out_std = 1)."""
    S, B, Cc, (Hh, Ww), K, L, kind, _ = case
    Tk = len(TIMED)
    rs = np.random.RandomState(seed)
    shape = (Tk, S + 1, B, Cc, Hh, Ww)
    if kind == "int":
        x = rs.randint(-2, 3, size=shape).astype(F32)
    else:
        # a few random plane waves per row plus a little noise: the rows share the large scales and differ in the small ones
        yy, xx = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
        x = 0.15 * rs.standard_normal(shape)
        for wl in (48.0, 16.0, 5.0):
            ph = rs.uniform(0, 2 * np.pi, size=(Tk, 1, B, Cc, 1, 1)) + (6.0 / wl) * rs.standard_normal((Tk, S + 1, B, Cc, 1, 1))
            ang = rs.uniform(0, np.pi, size=(Tk, 1, B, Cc, 1, 1))
            x += np.sin(2 * np.pi * (np.cos(ang) * xx + np.sin(ang) * yy) / wl + ph)
        x = (x + 0.2).astype(F32)
    return np.ascontiguousarray(x[:, :S]), np.ascontiguousarray(x[:, S])


def plant_nonfinite(xs, tgt, seed):
    """NaN, +Inf and -Inf at one entry in sixteen of the members and of the target, in place."""
    rs = np.random.RandomState(seed)
    for v in (xs, tgt):
        r = rs.randint(0, 48, size=v.shape)
        v[r == 0] = np.nan
        v[r == 1] = np.inf
        v[r == 2] = -np.inf


@functools.lru_cache(maxsize=None)
def inputs(idx):
    xs, tgt = make_inputs(TABLE[idx], 300 + idx)
    xs.setflags(write=False)
    tgt.setflags(write=False)
    return xs, tgt


def thresholds(events, B):
    """thr [B, K] float32 for out_mu = 0, out_std = 1 and no u: the values themselves."""
    return np.array([[v for _, v, _ in events]] * B, dtype=F32)


def indicators(x, thr, events, mutate=None):
    """x [..., B, C, H, W] float32 -> [..., B, K, H, W] int64 in {0, 1}: strict float32 comparisons, false for NaN."""
    out = []
    B = x.shape[-4]
    for k, (ch, _, d) in enumerate(events):
        v = x[..., ch, :, :]
        th = np.asarray(thr, dtype=F32)[:, k].reshape(B, 1, 1)
        with np.errstate(invalid="ignore"):
            if mutate == "non_strict":
                e = v >= th if d == ">" else v <= th
            else:
                e = v > th if d == ">" else v < th
        if mutate == "nan_in_event":
            e = e | np.isnan(v)
        out.append(e)
    return np.stack(out, -3).astype(np.int64)


def block_sums(z, l, shift=0):
    """z [..., H, W] int64 -> the sums over the 2^l x 2^l blocks aligned at pixel (-shift, -shift), zeros outside the field."""
    b = 1 << l
    Hh, Ww = z.shape[-2:]
    Hp, Wp = -(-(Hh + shift) // b) * b, -(-(Ww + shift) // b) * b
    pad = [(0, 0)] * (z.ndim - 2) + [(shift, Hp - Hh - shift), (shift, Wp - Ww - shift)]
    zp = np.pad(z, pad)
    return zp.reshape(z.shape[:-2] + (Hp // b, b, Wp // b, b)).sum((-3, -1))


def reference(xs, tgt, thr, events, L, mutate=None):
    """The raw tables of xs [Tk, S, B, C, H, W] against tgt [Tk, B, C, H, W] -> dict of int64 arrays iscale_member_raw [B, Tk, K, S,
    L + 1, 2] = (A, X), iscale_target_raw [B, Tk, K, L + 1] = Cc, iscale_ens_raw [B, Tk, K, L + 1, 2] = (AN, XN)."""
    Im = indicators(xs, thr, events, mutate)                                   # [Tk, S, B, K, H, W]
    o = indicators(tgt, thr, events, mutate)                                   # [Tk, B, K, H, W]
    ox = np.concatenate([o[:1], o[:-1]]) if mutate == "previous_target" else o
    n = Im.sum(1)
    shift = 1 if mutate == "origin_shifted" else 0
    mem, tt, en = [], [], []
    for l in range(L + 1):
        sI, so, sox, sn = (block_sums(v, l, shift if l else 0) for v in (Im, o, ox, n))
        dead = mutate == "remainder_dropped" and l == L
        f = 0 if dead else 1
        mem.append(np.stack([(sI * sI).sum((-2, -1)), (sI * sox[:, None]).sum((-2, -1))], -1) * f)      # [Tk, S, B, K, 2]
        tt.append((so * so).sum((-2, -1)) * f)                                                          # [Tk, B, K]
        en.append(np.stack([(sn * sn).sum((-2, -1)), (sn * sox).sum((-2, -1))], -1) * f)                # [Tk, B, K, 2]
    mem = np.stack(mem, -2).transpose(2, 0, 3, 1, 4, 5)                        # [Tk, S, B, K, L+1, 2] -> [B, Tk, K, S, L+1, 2]
    tt = np.stack(tt, -1).transpose(1, 0, 2, 3)                                # [Tk, B, K, L+1] -> [B, Tk, K, L+1]
    en = np.stack(en, -2).transpose(1, 0, 2, 3, 4)
    return {"iscale_member_raw": np.ascontiguousarray(mem), "iscale_target_raw": np.ascontiguousarray(tt),
            "iscale_ens_raw": np.ascontiguousarray(en)}


@functools.lru_cache(maxsize=None)
def case_reference(idx):
    S, B, Cc, hw, K, L, kind, _ = TABLE[idx]
    xs, tgt = inputs(idx)
    ev = events_for(Cc, K)
    ref = reference(xs, tgt, thresholds(ev, B), ev, L)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def numerators(Q):
    """Q [..., L + 1] int64 level sums -> the integer numerators [..., L + 1]: 4 Q[c-1] - Q[c] for c = 1..L, then Q[L]."""
    Q = np.asarray(Q)
    return np.concatenate([4 * Q[..., :-1] - Q[..., 1:], Q[..., -1:]], -1)


def divisors(L):
    return np.array([4 ** c for c in range(1, L + 1)] + [4 ** L], dtype=np.int64)


def haar_components(z, L):
    """z [H, W] (any real field) -> the L + 1 fields on the domain zero-padded to multiples of 2^L: the Haar components of block size
    2, 4, .., 2^L (the block mean at half the size minus the block mean at the size) and the remainder (the block mean at 2^L).  They
    sum to the padded field and are orthogonal."""
    b = 1 << L
    Hh, Ww = z.shape
    Hp, Wp = -(-Hh // b) * b, -(-Ww // b) * b
    zp = np.zeros((Hp, Wp), np.float64)
    zp[:Hh, :Ww] = z

    def mean(l):
        s = 1 << l
        m = zp.reshape(Hp // s, s, Wp // s, s).mean((1, 3))
        return np.kron(m, np.ones((s, s)))

    means = [mean(l) for l in range(L + 1)]
    return [means[c - 1] - means[c] for c in range(1, L + 1)] + [means[L]]


def haar_energies(z, L):
    """The squared norms of haar_components times their divisors 4^c (4^L for the remainder), rounded -> [L + 1] int64."""
    return np.array([int(round(float((c * c).sum()) * d)) for c, d in zip(haar_components(z, L), divisors(L))], dtype=np.int64)


def level_sums(z, L):
    """z [H, W] int64 -> [L + 1] the sums over the blocks of level l of the squared block sums."""
    return np.array([int((block_sums(z, l) ** 2).sum()) for l in range(L + 1)], dtype=np.int64)


def host_reference(ref, S, HW, steps=1):
    """tmg_ops.iscale_outputs restated in fp64 from the scores' definitions, on the raw tables of `ref` (pooled over `steps` steps)."""
    mem, tt, en = (np.asarray(ref[k]) for k in RAW_KEYS)
    L = tt.shape[-1] - 1
    N = float(HW * steps)
    A, X = mem[..., 0], mem[..., 1]
    Cc = tt[..., None, :]
    AN, XN = en[..., 0], en[..., 1]
    div = divisors(L).astype(np.float64)
    energy = lambda Q: numerators(Q).astype(np.float64) / div                # noqa: E731
    o = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        mse = energy(A - 2 * X + Cc) / N
        f, ob = A[..., :1] / N, Cc[..., :1] / N
        o["iscale_mse"] = mse
        o["iscale_skill"] = 1.0 - (L + 1) * mse / (f * (1.0 - ob) + ob * (1.0 - f))
        Ef, Eo = energy(A) / N, energy(Cc) / N
        o["iscale_energy"] = np.concatenate([Ef, Eo], -2)
        o["iscale_energy_bias"] = (Ef - Eo) / (Ef + Eo)
        brier = energy(AN - 2 * S * XN + S * S * tt) / (S * S * N)
        p2 = AN[..., :1] / (S * S * N)                                         # mean p^2
        p1 = A[..., 0].sum(-1)[..., None] / (S * N)                            # mean p: I^2 = I
        ot = tt[..., :1] / N
        o["iscale_brier"] = brier
        o["iscale_brier_skill"] = 1.0 - (L + 1) * brier / ((p2 - p1 * ot) + ot * (1.0 - p1))
        spread = energy(S * A.sum(-2) - AN) / (S * S * N)
        o["iscale_spread"] = spread
        o["iscale_spread_skill"] = spread / brier
    return o


def full_reference(ref, S, HW, timed=TIMED):
    """Every key of EnsembleIntensityScale.finalize() from the per-step raw tables: the per-step scores, the raw sums summed over the
    timed steps and the scores of those."""
    L = ref["iscale_target_raw"].shape[-1] - 1
    o = dict(ref)
    o.update(host_reference(ref, S, HW))
    keep = [i for i, t in enumerate(timed) if t]
    pooled = {k: ref[k][:, keep].sum(1) for k in RAW_KEYS}
    for k in RAW_KEYS:
        o["time_" + k] = pooled[k]
    for k, v in host_reference(pooled, S, HW, len(keep)).items():
        o["time_" + k] = v
    o["iscale_blocks"] = np.array([2 ** c for c in range(1, L + 1)] + [0], dtype=np.int64)
    return o


def check_identities(ref, S, HW, mismatched=None):
    """The identities of the raw tables: AN[0] and XN[0] against the members' level 0, the components sum to level 0, every numerator
    is a non-negative integer, the spread is non-negative, and D[0] counts the mismatched pixels [B, Tk, K, S] when given."""
    mem, tt, en = (np.asarray(ref[k]) for k in RAW_KEYS)
    A, X, Cc = mem[..., 0], mem[..., 1], tt[..., None, :]
    D = A - 2 * X + Cc
    DN = en[..., 0] - 2 * S * en[..., 1] + S * S * tt
    SP = S * A.sum(-2) - en[..., 0]
    L = tt.shape[-1] - 1
    div = divisors(L)
    scale = div.max() // div                                                   # components over a common divisor 4^L
    for Q in (A, Cc, D, DN, SP):
        num = numerators(Q)
        assert bool((num >= 0).all())
        assert np.array_equal((num * scale).sum(-1), Q[..., 0] * div.max())
    assert np.array_equal(en[..., 0, 1], X[..., 0].sum(-1))                    # XN[0] = sum_m X[m][0]
    assert bool((X[..., 0] <= np.minimum(A[..., 0], Cc[..., 0])).all())
    assert bool((A[..., 0] <= HW).all()) and bool((tt[..., 0] <= HW).all())
    assert bool((np.diff(A, axis=-1) >= 0).all()) and bool((A[..., 1:] <= 4 * A[..., :-1]).all())
    if mismatched is not None:
        assert np.array_equal(D[..., 0], mismatched)


def mismatches(got, ref, keys):
    """The keys whose arrays are not the reference's bit for bit (dtype, shape, values)."""
    bad = []
    for key in keys:
        g, r = got.get(key), ref[key]
        if g is None or g.dtype != r.dtype or g.shape != r.shape or not np.array_equal(g, r):
            bad.append(key)
    return bad


def check_floats(got, ref, keys, what):
    """float32 outputs within 2^-24 |ref| + 2^-40 of the fp64 reference, NaN and infinities where it has them -> worst share."""
    worst = 0.0
    for key in keys:
        g, r = np.asarray(got[key]), np.asarray(ref[key], dtype=np.float64)
        assert g.dtype == F32 and g.shape == r.shape, "%s: %s is %s %s, expected float32 %s" % (what, key, g.dtype, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), "%s: %s NaN pattern" % (what, key)
        inf = np.isinf(r)
        assert np.array_equal(g[inf].astype(np.float64), r[inf]), "%s: %s infinities" % (what, key)
        ok = np.isfinite(r)
        if ok.any():
            err = np.abs(g[ok].astype(np.float64) - r[ok])
            tol = U24 * np.abs(r[ok]) + TOL_ABS
            assert bool((err <= tol).all()), "%s: %s error %.3e of tolerance" % (what, key, float((err / tol).max()))
            worst = max(worst, float((err / tol).max()))
    return worst
