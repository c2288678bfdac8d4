"""Ensemble prediction intervals on the device (`-m gpu`): tmg_ens_score_store / tmg_ens_quant_step through tmg_ops.EnsembleQuantiles
against a numpy float32 mirror of the kernel (bitwise) and against np.quantile in fp64, and utils.modelPredQuantiles against np.quantile
over modelPred's samples.

Definitions (case b, kept step t, channel c, pixel p; members x_0..x_{S-1} and target y raw normalised fp32):
  rank_m = #{n : x_n < x_m} + #{n < m : x_n == x_m}: a permutation of 0..S-1; x_(r) is the member of rank r
  level q: h = q (S - 1) in fp64, lo = min(floor(h), S - 1), hi = min(lo + 1, S - 1), w = float32(h - lo)     (tmg_ops.quantile_levels)
  qraw = x_(lo) + w (x_(hi) - x_(lo))       three rounded fp32 operations
  quant = sc * fmaf(out_std, qraw, out_mu), sc = u[b, c] or 1
  exceed_prob = float32(#{m : x_m > thr}) * float32(1 / S) (or <, both strict), thr = float32((value / sc - out_mu) / out_std)
  time_quant: fp32 running mean of quant over the timed steps; time_below_count = #{timed t : y < qraw}; time_exceed_count = sum of
  the member counts over the timed steps.
The mirror is numpy float32, operation by operation: order statistics are values of the set, so every exact selection gives the same
bits, and with out_mu = 0, out_std = 1, u = None the un-normalisation is exact (fmaf(1, q, 0) = q, 1 * q = q): `quant`, `exceed_prob` and
both counts must be EQUAL to the mirror.

Bounds where a tolerance is needed (u = 2^-24, s = max_m |x_m| of the element):
  qraw against np.quantile(float64): the rounding of w, the subtraction and the product each act on |x_(hi) - x_(lo)| <= 2 s (2 u s
  each), the addition on a result <= s (u s): 7 u s.  (numpy's own fp64 lerp differs from the statement by ~1e-16 s.)
  quant with a real normalisation: + the fma (one rounding of out_std qraw + out_mu) + the product with sc:
      |quant - ref64| <= 9 u sc (out_std s + |out_mu|) + 1e-6 |ref|
  time_quant: the steps' own errors average to <= 9 u max_t scale; the running mean m += (v - m) tn adds <= 3 T u scale (the count of
  tests/test_scores_gpu.py's docstring): 9 + 3 T.  Against the mirror's own quant values (identity un-normalisation) only the 3 T.
  end to end against modelPred's samples: modelPred un-normalises every member in fp32 (product, sum, product: 3 roundings), so 12 in
  place of 9.
That these bounds leave the checks sensitive is tests/test_quant_cpu.py, which runs without a GPU on the inputs of this file."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

U24 = 2.0 ** -24
T = 4
R = 8                 # QUANT_R of csrc/tmg_quant.hip
MU = [0.3, -0.2, 0.5, 1.0]
SD = [1.7, 0.6, 2.5, 0.9]
LEVELS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 1.0 / 3.0)
ONE_LEVEL = (0.9,)
F32 = np.float32

# member counts 1, 2, R - 1, R, R + 1, 4 R + 1, 8 R; fields: one partial wave, a second pixel block of 16 lanes, a long row; and the
# largest member count once
SWEEP = [(S, B, Cc, hw) for S in (1, 2, 7, 8, 9, 33, 64) for B in (1, 3) for Cc in (2, 3, 4) for hw in ((5, 7), (16, 17), (3, 300))] \
    + [(1024, 1, 2, (5, 7))]


def thresholds(Cc):
    """Two thresholds in opposite directions, on the first and the last channel."""
    return ((0, 0.25, ">"), (Cc - 1, -0.1, "<"))


def features(idx):
    """(t_start, channel-padded y and target, chunking) of sweep entry idx; chunking 0: one member per chunk, 1: three members per
    chunk, 2: the whole ensemble."""
    ih, ic, ib, iS = idx % 3, (idx // 3) % 3, (idx // 9) % 2, idx // 18
    return 2 * ((ih + ib + iS) % 2), (ih + ic) % 2 == 1, (ih + ic + ib + iS) % 3


def chunk_sizes(S, kind):
    per = (1, 3, S)[kind]
    return [min(per, S - m0) for m0 in range(0, S, per)]


@functools.lru_cache(maxsize=None)
def inputs(idx):
    """Sweep entry idx -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W]) numpy float32, seeded: members N(0.3, 1) plus an offset per
    case, target N(0.3, 1), all continuous."""
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    g = torch.Generator().manual_seed(7000 + idx)
    xs = torch.randn(T, S, B, Cc, Hh, Ww, generator=g) + 0.3 + (0.2 * torch.arange(B, dtype=torch.float32) - 0.2).view(1, 1, B, 1, 1, 1)
    tgt = torch.randn(T, B, Cc, Hh, Ww, generator=g) + 0.3
    return xs.numpy(), tgt.numpy()


def tie_inputs(S=9, B=3, Cc=3, Hh=16, Ww=17, seed=91):
    """Integer data in {-2..2}, members and target: ties everywhere, also with the thresholds at 0."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randint(-2, 3, (T, S, B, Cc, Hh, Ww), generator=g).float()
    tgt = torch.randint(-2, 3, (T, B, Cc, Hh, Ww), generator=g).float()
    return xs.numpy(), tgt.numpy()


TIE_THRESHOLDS = ((0, 0.0, ">"), (2, 0.0, "<"))


# ---- the mirror: the kernel in numpy float32 ---------------------------------------------------------------------------------------
def ranks(x, tiebreak=True):
    """x [S, ..] -> rank [S, ..] by counting: #{n : x_n < x_m} + #{n < m : x_n == x_m} (the second term only with tiebreak)."""
    S = x.shape[0]
    r = np.zeros(x.shape, dtype=np.int64)
    for n in range(S):
        r += x[n] < x
        if tiebreak and n + 1 < S:
            r[n + 1:] += x[n] == x[n + 1:]
    return r


def order_stats(x, rank):
    """The kernel's slots: NaN where no member takes the rank, else the member of that rank."""
    srt = np.full(x.shape, np.nan, dtype=F32)
    np.put_along_axis(srt, np.minimum(rank, x.shape[0] - 1), x, axis=0)
    return srt


def level_table(S, levels):
    """The fp64 statement of the host level table, written out here independently of tmg_ops.quantile_levels."""
    h = np.asarray(levels, dtype=np.float64) * (S - 1)
    lo = np.minimum(np.floor(h), S - 1).astype(np.int64)
    hi = np.minimum(lo + 1, S - 1)
    return lo, hi, (h - lo).astype(F32)


def mirror(xs, tgt, levels, exceed, t_start, thr=None, defect=None, srt=None):
    """The kernel under the identity un-normalisation, numpy float32.  xs [T, S, B, C, H, W], tgt [T, B, C, H, W] (or None).
    thr: raw thresholds [B, K] float32 (default: float32(value)); srt: the order statistics, when the caller has them.  -> dict in the layout of EnsembleQuantiles.finalize(), plus 'qraw'.
    defect (tests/test_quant_cpu.py): 'rank_off' (every wanted rank one too high), 'swap' (lo and hi swapped), 'no_tiebreak',
    'below_le' (<= for < in the below count), 'exceed_ge' (>= for > and <= for < in the exceedance count)."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    x = np.ascontiguousarray(np.moveaxis(xs, 1, 0))                          # [S, T, B, C, H, W]
    if srt is None:
        srt = order_stats(x, ranks(x, tiebreak=defect != "no_tiebreak"))
    lo, hi, w = level_table(S, levels)
    if defect == "rank_off":
        lo, hi = np.minimum(lo + 1, S - 1), np.minimum(hi + 1, S - 1)
    if defect == "swap":
        lo, hi = hi, lo
    a, b = srt[lo], srt[hi]                                                  # [Q, T, B, C, H, W]
    d = (b - a).astype(F32)
    qraw = (a + (w.reshape(-1, 1, 1, 1, 1, 1) * d).astype(F32)).astype(F32)
    out = {"qraw": qraw, "quant": np.ascontiguousarray(qraw.transpose(2, 1, 0, 3, 4, 5))}
    if tgt is not None:
        below = (tgt[None] <= qraw) if defect == "below_le" else (tgt[None] < qraw)
        out["time_below_count"] = below[:, t_start:].sum(1).transpose(1, 0, 2, 3, 4).astype(np.int64)
    if exceed:
        cnts = []
        for k, (ch, value, direction) in enumerate(exceed):
            tv = (np.full(B, F32(value), dtype=F32) if thr is None else thr[:, k]).reshape(1, 1, B, 1, 1)
            xc = x[:, :, :, ch]                                              # [S, T, B, H, W]
            if defect == "exceed_ge":
                hit = xc >= tv if direction == ">" else xc <= tv
            else:
                hit = xc > tv if direction == ">" else xc < tv
            cnts.append(hit.sum(0))                                          # [T, B, H, W]
        cnt = np.stack(cnts, 2).transpose(1, 0, 2, 3, 4)                     # [B, T, K, H, W]
        out["exceed_prob"] = (cnt.astype(F32) * F32(1.0 / S)).astype(F32)
        out["time_exceed_count"] = cnt[:, t_start:].sum(1).astype(np.int64)
    return out


# ---- the device side ----------------------------------------------------------------------------------------------------------------
def run_quant(xs, tgt, levels, exceed, t_start, sizes, padded, mu=None, sd=None, u=None):
    """Feed EnsembleQuantiles as utils.modelPredQuantiles does, in chunks of `sizes` members per step; padded: y and target are channel
    slices of wider NaN-filled NHWC buffers.  The outputs are pre-filled with NaN.  -> dict of numpy arrays."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape
    xd = torch.from_numpy(xs).to(DEV)
    td = None if tgt is None else torch.from_numpy(tgt).to(DEV)

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), float("nan"), device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    q = ops.EnsembleQuantiles(S, B, Cc, Hh, Ww, Tn, DEV, torch.zeros(Cc) if mu is None else mu, torch.ones(Cc) if sd is None else sd,
                              u=u, levels=levels, exceed=exceed)
    for v in q.out.values():
        v.fill_(float("nan"))
    for t in range(Tn):
        target = None if td is None else nhwc(td[t])
        m0 = 0
        for k in sizes:
            q.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
    got = {k: v.cpu().numpy() for k, v in q.finalize().items()}
    for k, v in got.items():
        assert not np.isnan(v).any(), "%s holds NaN" % k
    return got


def check_bitwise(got, ref, S, Tw, what):
    """quant, exceed_prob and the counts equal the mirror; time_quant within 3 T u s of the fp64 mean of the mirror's quant."""
    assert got["quant"].dtype == F32 and np.array_equal(got["quant"], ref["quant"]), "%s quant" % what
    for name in ("time_below_count", "time_exceed_count"):
        if name in ref:
            assert got[name].dtype == np.int64 and np.array_equal(got[name], ref[name]), "%s %s" % (what, name)
    if "exceed_prob" in ref:
        assert got["exceed_prob"].dtype == F32 and np.array_equal(got["exceed_prob"], ref["exceed_prob"]), "%s exceed_prob" % what
        assert np.array_equal(got["time_exceed_prob"], (ref["time_exceed_count"].astype(np.float64) / (S * Tw)).astype(F32)), what
    if "time_below_count" in ref:
        assert np.array_equal(got["below_frac"], (ref["time_below_count"].astype(np.float64) / Tw).astype(F32)), what
    tq = ref["quant"][:, -Tw:].astype(np.float64)
    bnd = 3 * Tw * U24 * np.abs(tq).max(1) if Tw > 1 else 0.0
    share = np.abs(got["time_quant"].astype(np.float64) - tq.mean(1)) / np.maximum(bnd, 1e-300)
    assert bool((np.abs(got["time_quant"].astype(np.float64) - tq.mean(1)) <= bnd).all()), \
        "%s time_quant: worst error is %.3f of its bound" % (what, float(share.max()))
    return float(share.max()) if Tw > 1 else 0.0


@pytest.mark.parametrize("idx", range(len(SWEEP)))
def test_quantiles_equal_the_mirror(idx):
    """Every member count, case count, channel count and field of the sweep; the features rotate: t_start 0 or 2, chunks of one member /
    three members / the whole ensemble, y and target contiguous or NaN-surrounded channel slices.  Eight levels, then one level."""
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    xs, tgt = inputs(idx)
    t_start, padded, kind = features(idx)
    ex = thresholds(Cc)
    what = "sweep %s" % (SWEEP[idx],)
    got = run_quant(xs, tgt, LEVELS, ex, t_start, chunk_sizes(S, kind), padded)
    x = np.ascontiguousarray(np.moveaxis(xs, 1, 0))
    srt = order_stats(x, ranks(x))
    ref = mirror(xs, tgt, LEVELS, ex, t_start, srt=srt)
    assert got["quant"].shape == (B, T, len(LEVELS), Cc, Hh, Ww) and got["time_quant"].shape == (B, len(LEVELS), Cc, Hh, Ww)
    assert got["exceed_prob"].shape == (B, T, 2, Hh, Ww) and got["time_exceed_count"].shape == (B, 2, Hh, Ww)
    assert got["time_below_count"].shape == (B, len(LEVELS), Cc, Hh, Ww)
    assert got["levels"].dtype == np.float64 and np.array_equal(got["levels"], np.asarray(LEVELS, dtype=np.float64))
    worst = check_bitwise(got, ref, S, T - t_start, what)
    print("%s: time_quant's worst share of its bound %.3f" % (what, worst))
    xm = np.moveaxis(xs, 1, 0)                                               # level 0 is the smallest member, level 1 the largest
    assert np.array_equal(got["quant"][:, :, 0], xm.min(0).transpose(1, 0, 2, 3, 4))
    assert np.array_equal(got["quant"][:, :, 6], xm.max(0).transpose(1, 0, 2, 3, 4))
    one = run_quant(xs, None, ONE_LEVEL, (), t_start, chunk_sizes(S, (kind + 1) % 3), not padded)
    assert set(one) == {"quant", "time_quant", "levels"}
    check_bitwise(one, mirror(xs, None, ONE_LEVEL, (), t_start, srt=srt), S, T - t_start, what + " one level")


def test_ties_are_broken_by_member_index():
    xs, tgt = tie_inputs()
    S = xs.shape[1]
    got = run_quant(xs, tgt, LEVELS, TIE_THRESHOLDS, 1, chunk_sizes(S, 1), False)
    check_bitwise(got, mirror(xs, tgt, LEVELS, TIE_THRESHOLDS, 1), S, T - 1, "ties")


def test_equal_members_return_their_value_and_an_equal_target_is_not_below():
    S, B, Cc, Hh, Ww = 9, 3, 3, 16, 17
    _, tgt = inputs(SWEEP.index((S, B, Cc, (Hh, Ww))))
    xs = np.ascontiguousarray(np.broadcast_to(tgt[:, None], (T, S, B, Cc, Hh, Ww)))
    got = run_quant(xs, tgt, LEVELS, (), 0, chunk_sizes(S, 1), True)
    assert np.array_equal(got["quant"], np.broadcast_to(tgt.transpose(1, 0, 2, 3, 4)[:, :, None], got["quant"].shape))
    assert not got["time_below_count"].any()                                 # strict: the target equals every quantile
    above = run_quant(xs, np.nextafter(tgt, F32(-np.inf)), LEVELS, (), 0, chunk_sizes(S, 2), False)
    assert bool((above["time_below_count"] == T).all())


@pytest.mark.parametrize("S", [9, 33])
def test_member_order_does_not_matter(S):
    idx = SWEEP.index((S, 3, 3, (16, 17)))
    xs, tgt = inputs(idx)
    srt = np.sort(xs, axis=1)
    ex = thresholds(3)
    outs = [run_quant(v, tgt, LEVELS, ex, 0, chunk_sizes(S, 1), False) for v in (srt, np.ascontiguousarray(srt[:, ::-1]), xs)]
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name]), name


@pytest.mark.parametrize("S,B,Cc,hw", [(7, 3, 3, (16, 17)), (33, 3, 4, (5, 7)), (33, 1, 2, (3, 300))])
def test_outputs_are_bitwise_the_same_for_every_feed(S, B, Cc, hw):
    xs, tgt = inputs(SWEEP.index((S, B, Cc, hw)))
    ex = thresholds(Cc)
    mu, sd = torch.tensor(MU[:Cc]), torch.tensor(SD[:Cc])
    u = 0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(3))
    outs = [run_quant(xs, tgt, LEVELS, ex, 1, chunk_sizes(S, kind), padded, mu=mu, sd=sd, u=u)
            for kind, padded in ((0, False), (1, True), (2, False), (2, True))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name]), name


def raw_thresholds(exceed, u, mu, sd, B):
    """thr[b][k] = float32((value / sc[b][c_k] - out_mu[c_k]) / out_std[c_k]), in fp64 from the fp32 values the kernel holds."""
    sc = np.ones((B, len(mu))) if u is None else u.double().numpy()
    m, s = mu.double().numpy(), sd.double().numpy()
    return np.stack([((value / sc[:, ch] - m[ch]) / s[ch]).astype(F32) for ch, value, _ in exceed], 1)


@pytest.mark.parametrize("S,B,Cc,hw,with_u", [(7, 3, 3, (16, 17), True), (9, 3, 4, (16, 17), True), (33, 3, 4, (5, 7), False),
                                              (64, 1, 2, (3, 300), True), (2, 3, 3, (5, 7), True)])
def test_real_normalisation_stays_in_the_rounding_bound(S, B, Cc, hw, with_u):
    """|quant - ref64| <= 9 u sc (out_std s + |out_mu|) + 1e-6 |ref| and time_quant with 9 + 3 T (the counts of the module docstring);
    the counts are exact: selection and comparison happen on the raw values."""
    xs, tgt = inputs(SWEEP.index((S, B, Cc, hw)))
    mu, sd = torch.tensor(MU[:Cc]), torch.tensor(SD[:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=torch.Generator().manual_seed(11))) if with_u else None
    ex = ((0, 0.4, ">"), (Cc - 1, 0.1, "<"))
    t_start = 1
    Tw = T - t_start
    got = run_quant(xs, tgt, LEVELS, ex, t_start, chunk_sizes(S, 1), False, mu=mu, sd=sd, u=u)
    ref = mirror(xs, tgt, LEVELS, ex, t_start, thr=raw_thresholds(ex, u, mu, sd, B))
    for name in ("time_below_count", "time_exceed_count", "exceed_prob"):
        assert np.array_equal(got[name], ref[name]), name
    sc = (np.ones((B, Cc)) if u is None else u.double().numpy()).reshape(B, 1, 1, Cc, 1, 1)
    m64, s64 = mu.double().numpy().reshape(1, 1, 1, Cc, 1, 1), sd.double().numpy().reshape(1, 1, 1, Cc, 1, 1)
    q64 = np.quantile(xs.astype(np.float64), LEVELS, axis=1, method="linear").transpose(2, 1, 0, 3, 4, 5)    # [B, T, Q, C, H, W]
    ref64 = sc * (s64 * q64 + m64)
    s = np.abs(xs.astype(np.float64)).max(1).transpose(1, 0, 2, 3, 4)[:, :, None]                             # [B, T, 1, C, H, W]
    scale = sc * (s64 * s + np.abs(m64))
    share = float((np.abs(got["quant"].astype(np.float64) - ref64) / (9 * U24 * scale + 1e-6 * np.abs(ref64))).max())
    tref = ref64[:, t_start:].mean(1)
    tbnd = (9 + 3 * Tw) * U24 * scale[:, t_start:].max(1) + 1e-6 * np.abs(tref)
    tshare = float((np.abs(got["time_quant"].astype(np.float64) - tref) / tbnd).max())
    print("S=%d: worst share of the bound: quant %.3f, time_quant %.3f" % (S, share, tshare))
    assert share <= 1.0, "quant: worst error is %.3f of its bound" % share
    assert tshare <= 1.0, "time_quant: worst error is %.3f of its bound" % tshare


# ---- end to end: modelPredQuantiles == np.quantile over modelPred's samples --------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_quantiles_matches_numpy_over_model_pred(monkeypatch, tmp_path, case):
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    mu = model.out_mu.detach().double().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().double().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    tall = torch.cat([b[1].cpu() for b in te]).double().numpy()                    # the normalised target series [N, T, C, H, W]
    pmed = float(np.median(u0.reshape(-1, 1, 1, 1) ** 2 * (sd[2] * tall[:, :, 2] + mu[2])))   # the target's median pressure
    ex = ((0, 0.0, "<"), (2, pmed, ">"))
    for _ in range(2):                                                        # two folded runs: modelPredQuantiles, modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    for bi, B in enumerate(batches):
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    torch.manual_seed(77)
    got = utils.modelPredQuantiles(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows,
                                   levels=LEVELS, exceed=ex)
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    new = {"quant", "time_quant", "time_below_count", "below_frac", "exceed_prob", "time_exceed_count", "time_exceed_prob", "levels"}
    assert set(got) == set(stats) | new
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W], un-normalised
    Tk = p.shape[2]
    y = tgt.double().numpy()[:, ::stride][:, :Tk]                            # [N, Tk, C, H, W]
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    Tw = Tk - t_start
    Q = len(LEVELS)
    assert tuple(got["quant"].shape) == (N, Tk, Q, Cc, Hh, Ww) and tuple(got["exceed_prob"].shape) == (N, Tk, 2, Hh, Ww)
    ref = np.quantile(p, LEVELS, axis=0, method="linear").transpose(1, 2, 0, 3, 4, 5)                         # [N, Tk, Q, C, H, W]
    # the normalised magnitudes recovered in fp64: x = (xh / uc - out_mu) / out_std
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]                              # [N, C]
    xn = (p / uc.reshape(1, N, 1, Cc, 1, 1) - mu[:Cc].reshape(1, 1, 1, Cc, 1, 1)) / sd[:Cc].reshape(1, 1, 1, Cc, 1, 1)
    scale = uc.reshape(N, 1, Cc, 1, 1) * (sd[:Cc].reshape(1, 1, Cc, 1, 1) * np.abs(xn).max(0) + np.abs(mu[:Cc]).reshape(1, 1, Cc, 1, 1))
    bnd = 12 * U24 * scale[:, :, None] + 1e-6 * np.abs(ref)                  # [N, Tk, Q, C, H, W]
    share = float((np.abs(got["quant"].double().numpy() - ref) / bnd).max())
    tref = ref[:, t_start:].mean(1)
    tbnd = (12 + 3 * Tw) * U24 * scale[:, t_start:].max(1)[:, None] + 1e-6 * np.abs(tref)
    tshare = float((np.abs(got["time_quant"].double().numpy() - tref) / tbnd).max())
    print("%s: worst share of the bound: quant %.3f, time_quant %.3f" % (case, share, tshare))
    assert share <= 1.0, "%s quant: worst error is %.3f of its bound" % (case, share)
    assert tshare <= 1.0, "%s time_quant: worst error is %.3f of its bound" % (case, tshare)
    # counts, element by element: |got - ref| <= near, near = the comparisons that the roundings above can turn
    yq = y[:, :, None]                                                       # [N, Tk, 1, C, H, W]
    below = (yq < ref)[:, t_start:].sum(1)
    near_b = (np.abs(ref - yq) <= 2 * bnd)[:, t_start:].sum(1)
    assert got["time_below_count"].dtype == torch.int64 and got["time_exceed_count"].dtype == torch.int64
    assert bool((np.abs(got["time_below_count"].numpy() - below) <= near_b).all()), "%s time_below_count" % case
    assert np.array_equal(got["below_frac"].numpy(), (got["time_below_count"].double().numpy() / Tw).astype(F32))
    near_total, compared = int(near_b.sum()), below.size
    for k, (ch, value, direction) in enumerate(ex):
        pc = p[:, :, :, ch]                                                  # [S, N, Tk, H, W]
        cnt = ((pc > value) if direction == ">" else (pc < value)).sum(0)    # [N, Tk, H, W]
        near = (np.abs(pc - value) <= 4 * U24 * scale[None, :, :, ch]).sum(0)
        assert bool((np.abs(got["exceed_prob"][:, :, k].double().numpy() * S - cnt) <= near + 1e-3).all()), "%s exceed_prob %d" % (case, k)
        assert bool((np.abs(got["time_exceed_count"][:, k].numpy() - cnt[:, t_start:].sum(1)) <= near[:, t_start:].sum(1)).all()), \
            "%s time_exceed_count %d" % (case, k)
        near_total += int(near[:, t_start:].sum())
        compared += cnt[:, t_start:].sum(1).size
    assert np.array_equal(got["time_exceed_prob"].numpy(), (got["time_exceed_count"].double().numpy() / (S * Tw)).astype(F32))
    print("%s: comparisons within the rounding of their threshold: %d of %d compared elements (%.2e)"
          % (case, near_total, compared, near_total / compared))
    assert near_total <= 0.01 * compared, "%s: the allowance covers %d of %d elements" % (case, near_total, compared)
