"""Ensemble calibration scores on the device (`-m gpu`): tmg_ens_score_store / tmg_ens_score_step through tmg_ops.EnsembleScores against
fp64 torch statements of the definitions, and utils.modelPredScores against fp64 numpy scores of modelPred's samples.

Definitions (case b, kept step t, channel c, pixel p; members x_1..x_S and target y raw normalised fp32; a = u[b, c] out_std[c];
xh = u (out_std x + out_mu), yh likewise):
  crps      = (1/S) sum_m |xh_m - yh| - (1 / (2 S^2))       sum_m sum_n |xh_m - xh_n|
  crps_fair = (1/S) sum_m |xh_m - yh| - (1 / (2 S (S - 1))) sum_m sum_n |xh_m - xh_n|      (S = 1: crps)
  rank      = #{m : x_m < y}  (strict, on the raw fp32 values: exact)
The reference forms the scores from xh / yh WITH out_mu, which the kernels never see: the test also checks that dropping it is right.

The bound.  u = 2^-24, s = max_m |x_m| + |y| of the element, scale_e = a s.  |got - ref| <= n u scale_e + 1e-6 |ref| with n the
roundings along the kernel's longest path (the sum order is stated in csrc/tmg_scores.hip; R = 8 members are held in registers,
nb = ceil(S / R) register blocks):
  first term, <= s after the 1/S:   1 (the subtraction in |x_m - y|) + min(R, S) (the block's chain a1) + nb (t1 += a1)
                                    + 2 (1/S rounded on the host, the product)                                   = n1
  pair term, <= s after its factor: 1 (the subtraction in |x_i - x_n|) + (S - 1) (one accumulator per held member: the block's later
                                    members, then the streamed ones) + R (ap = the sum of the R accumulators) + nb (tp += ap)
                                    + 2 (the factor rounded on the host, the product)                            = np
  result:                           1 (first - pair) + 1 (times a) + 1 (a = u out_std is itself an fp32 product) = 3
  n_step(S) = n1 + np + 3:  S = 1: 20, 2: 22, 7: 32, 8: 34, 9: 37, 33: 67   (a single accumulator over all pairs would carry S^2 / 2)
  time means: the steps' own errors average to <= n_step u max_t scale_e; the running mean m += (v - m) tn adds per step the
  subtraction, tn = 1 / (t + 1) and the product (together <= 3 tn u scale_e) and the addition (u scale_e), damped by the later steps:
  <= (3 + (T + 1) / 2) u scale_e <= 3 T u scale_e for T >= 2, and nothing for T = 1.  n_time(S, T) = n_step(S) + 3 T.
That these n leave the checks sensitive (a dropped member or a <= for the < moves the measure by more than 10 bounds) is
tests/test_scores_cpu.py::test_reference_is_sensitive_at_ten_bounds, which runs without a GPU on the inputs of this sweep."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import test_ensemble_gpu as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

R = 8                 # SCORE_R of csrc/tmg_scores.hip
U24 = 2.0 ** -24
T = 4
KEYS = ("crps", "crps_fair", "time_crps", "time_crps_fair")
MU = [0.3, -0.2, 0.5, 1.0]
SD = [1.7, 0.6, 2.5, 0.9]
SEEDS = (77, 78, 79)   # end to end: host RNG seeds tried in order

# member counts 1, 2, R - 1, R, R + 1, 4 R + 1; fields: one partial wave, a second pixel block of 16 lanes, a long row
SWEEP = [(S, B, Cc, hw) for S in (1, 2, R - 1, R, R + 1, 4 * R + 1) for B in (1, 3) for Cc in (3, 4)
         for hw in ((5, 7), (16, 17), (3, 300))] + [(R + 1, 3, 2, (5, 7))]


def n_step(S):
    nb = -(-S // R)
    return (1 + min(R, S) + nb + 2) + (1 + (S - 1) + R + nb + 2) + 3


def n_time(S, Tw):
    return n_step(S) + 3 * Tw


def features(idx):
    """(u given, t_start, channel-padded y and target, chunk count) of sweep entry idx, mixed so that every member count >= 3 and
    every field meets each value of each feature."""
    ih, ic, ib, iS = idx % 3, (idx // 3) % 2, (idx // 6) % 2, idx // 12
    return (ih + ib) % 2 == 0, 2 * ((ic + ib + iS) % 2), (ih + ic) % 2 == 1, 1 + (ih + ic + ib + iS) % 3


@functools.lru_cache(maxsize=None)
def inputs(idx):
    """Sweep entry idx -> (xs [T, S, B, C, H, W], tgt [T, B, C, H, W], u [B, C] or None, mu [C], sd [C]) on the host, fp32, seeded:
    members N(0, 1) plus an offset per case, target N(0.3, 1), all continuous."""
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    g = torch.Generator().manual_seed(5000 + idx)
    xs = torch.randn(T, S, B, Cc, Hh, Ww, generator=g) + (0.2 * torch.arange(B, dtype=torch.float32) - 0.2).view(1, 1, B, 1, 1, 1)
    tgt = torch.randn(T, B, Cc, Hh, Ww, generator=g) + 0.3
    u = (0.5 + torch.rand(B, Cc, generator=g)) if features(idx)[0] else None
    return xs, tgt, u, torch.tensor(MU[:Cc]), torch.tensor(SD[:Cc])


def ref_scores(xs, tgt, u, mu, sd, t_start, strict=True):
    """fp64 statement of the definitions.  -> (ref dict in the layout of EnsembleScores.finalize(), parts): parts holds the two terms
    'first', 'pair', 'pair_fair' [B, T, C, H, W], the per-pixel 'rank' [B, T, C, H, W], a [B, C] and s = max_m |x_m| + |y|."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    a = sd.double().view(1, Cc).expand(B, Cc) if u is None else u.double() * sd.double().view(1, Cc)
    av, mv = a.view(1, 1, B, Cc, 1, 1), (a * mu.double().view(1, Cc) / sd.double().view(1, Cc)).view(1, 1, B, Cc, 1, 1)
    xh = av * xs.double() + mv                                               # = u (out_std x + out_mu)
    yh = (av * tgt.double().unsqueeze(1) + mv)
    first = (xh - yh).abs().mean(1)
    pair = torch.zeros_like(first)
    for m in range(S):
        pair += (xh[:, m:m + 1] - xh).abs().sum(1)
    pair_fair = pair / (2.0 * S * (S - 1)) if S > 1 else torch.zeros_like(pair)
    pair = pair / (2.0 * S * S)
    below = (xs < tgt.unsqueeze(1)) if strict else (xs <= tgt.unsqueeze(1))  # raw fp32 values: exact
    rank = below.sum(1)                                                      # [T, B, C, H, W]
    hist = torch.nn.functional.one_hot(rank.reshape(Tn, B, Cc, Hh * Ww), S + 1).sum(3)   # [T, B, C, S + 1]
    bt = lambda v: v.transpose(0, 1).contiguous()                            # noqa: E731  [T, B, ..] -> [B, T, ..]
    ref = {"crps": bt(first - pair), "crps_fair": bt(first - pair_fair), "rank_hist": bt(hist)}
    ref["time_crps"] = ref["crps"][:, t_start:].mean(1)
    ref["time_crps_fair"] = ref["crps_fair"][:, t_start:].mean(1)
    ref["time_rank_hist"] = ref["rank_hist"][:, t_start:].sum(1)
    s = bt(xs.double().abs().amax(1) + tgt.double().abs())
    return ref, {"first": bt(first), "pair": bt(pair), "pair_fair": bt(pair_fair), "rank": bt(rank), "a": a, "s": s}


def bounds(ref, parts, S, t_start):
    """The element-wise bound of every score output."""
    B, Cc = parts["a"].shape
    scale = parts["a"].view(B, 1, Cc, 1, 1) * parts["s"]
    tscale = scale[:, t_start:].amax(1)
    Tw = scale.shape[1] - t_start
    return {"crps": n_step(S) * U24 * scale + 1e-6 * ref["crps"].abs(),
            "crps_fair": n_step(S) * U24 * scale + 1e-6 * ref["crps_fair"].abs(),
            "time_crps": n_time(S, Tw) * U24 * tscale + 1e-6 * ref["time_crps"].abs(),
            "time_crps_fair": n_time(S, Tw) * U24 * tscale + 1e-6 * ref["time_crps_fair"].abs()}


def check_scores(got, ref, bnd, what):
    """-> the worst share of the bound over the four score outputs (asserted <= 1)."""
    worst = 0.0
    for name in KEYS:
        gv = got[name].double()
        assert gv.shape == ref[name].shape, (name, gv.shape, ref[name].shape)
        assert bool(torch.isfinite(gv).all()), "%s %s: non-finite" % (what, name)
        share = ((gv - ref[name]).abs() / bnd[name]).max()
        worst = max(worst, float(share))
        assert float(share) <= 1.0, "%s %s: worst error is %.3f of its bound" % (what, name, float(share))
    return worst


def check_hists(got, ref, HW, what):
    for name in ("rank_hist", "time_rank_hist"):
        assert got[name].dtype == torch.int64, name
        assert torch.equal(got[name].cpu(), ref[name].cpu()), "%s %s" % (what, name)
    assert bool((got["rank_hist"].sum(-1) == HW).all()), "%s: a histogram does not hold every pixel once" % what


def run_scores(xs, tgt, u, sd, t_start, nchunks, padded):
    """Feed EnsembleScores as utils.modelPredScores does, in nchunks unequal chunks per step; padded: y and target are channel
    slices of wider NaN-filled NHWC buffers."""
    import tmg_ops as ops
    Tn, S, B, Cc, Hh, Ww = xs.shape

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), float("nan"), device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    sc = ops.EnsembleScores(S, B, Cc, Hh, Ww, Tn, DEV, sd, u=u)
    sizes = E._chunks(S, nchunks)
    for t in range(Tn):
        target = nhwc(tgt[t])
        m0 = 0
        for k in sizes:
            sc.add(nhwc(xs[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
    return sc.finalize()


def _dev(idx):
    xs, tgt, u, mu, sd = inputs(idx)
    return xs.to(DEV), tgt.to(DEV), None if u is None else u.to(DEV), mu.to(DEV), sd.to(DEV)


@pytest.mark.parametrize("idx", range(len(SWEEP)))
def test_scores_match_fp64(idx):
    """Every member count, case count, channel count and field of the sweep; the features rotate: 1 / 2 / 3 unequal chunks, u given or
    absent, y and target contiguous or NaN-surrounded channel slices, t_start = 0 or 2."""
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    xs, tgt, u, mu, sd = _dev(idx)
    _, t_start, padded, nchunks = features(idx)
    got = run_scores(xs, tgt, u, sd, t_start, nchunks, padded)
    ref, parts = ref_scores(xs, tgt, u, mu, sd, t_start)
    assert tuple(got["crps"].shape) == (B, T, Cc, Hh, Ww) and tuple(got["time_crps"].shape) == (B, Cc, Hh, Ww)
    assert tuple(got["rank_hist"].shape) == (B, T, Cc, S + 1) and tuple(got["time_rank_hist"].shape) == (B, Cc, S + 1)
    check_hists(got, ref, Hh * Ww, "sweep %s" % (SWEEP[idx],))
    worst = check_scores(got, ref, bounds(ref, parts, S, t_start), "sweep %s" % (SWEEP[idx],))
    print("sweep %s: worst share of the bound %.3f" % (SWEEP[idx], worst))
    if S == 1:                                                               # closed form: crps == crps_fair == a |x - y|
        assert torch.equal(got["crps"], got["crps_fair"])
        a = parts["a"].view(B, 1, Cc, 1, 1)
        closed = a * (xs[:, 0].double() - tgt.double()).abs().transpose(0, 1)
        assert bool(((got["crps"].double() - closed).abs() <= n_step(1) * U24 * a * parts["s"] + 1e-6 * closed).all())


def tie_inputs(S=9, B=3, Cc=3, Hh=16, Ww=17, seed=77):
    """Continuous inputs with two tie sets: at the pixels of set A the target is a copy of member 4, at those of set B every member is a
    copy of the target.  -> (xs, tgt, mask A, mask B), host."""
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(T, S, B, Cc, Hh, Ww, generator=g)
    tgt = torch.randn(T, B, Cc, Hh, Ww, generator=g) + 0.3
    pix = torch.arange(Hh * Ww).view(Hh, Ww)
    A, Bm = (pix % 7 == 0), (pix % 7 == 3)
    tgt[..., A] = xs[:, 4][..., A]
    xs[..., Bm] = tgt.unsqueeze(1).expand_as(xs)[..., Bm]
    return xs, tgt, A, Bm


def test_ties_are_decided_by_the_strict_count():
    xs, tgt, A, Bm = tie_inputs()
    Tn, S, B, Cc, Hh, Ww = xs.shape
    sd = torch.tensor(SD[:Cc])
    ref, parts = ref_scores(xs, tgt, None, torch.tensor(MU[:Cc]), sd, 0)
    assert bool((parts["rank"][..., Bm] == 0).all())                          # the definition: nobody is below an equal target
    assert bool((parts["rank"][..., A] == (xs < xs[:, 4:5]).sum(1).transpose(0, 1)[..., A]).all())
    loose, _ = ref_scores(xs, tgt, None, torch.tensor(MU[:Cc]), sd, 0, strict=False)
    assert not torch.equal(loose["rank_hist"], ref["rank_hist"])
    got = run_scores(xs.to(DEV), tgt.to(DEV), None, sd.to(DEV), 0, 2, padded=False)
    check_hists(got, ref, Hh * Ww, "ties")
    check_scores(got, {k: v.to(DEV) for k, v in ref.items()}, {k: v.to(DEV) for k, v in bounds(ref, parts, S, 0).items()}, "ties")
    # every pixel of set B alone: all of them in bin 0
    every = tgt.unsqueeze(1).expand_as(xs).contiguous()
    got = run_scores(every.to(DEV), tgt.to(DEV), None, sd.to(DEV), 0, 3, padded=True)
    assert bool((got["rank_hist"][..., 0] == Hh * Ww).all()) and bool((got["rank_hist"][..., 1:] == 0).all())
    assert bool((got["crps"] == 0).all()) and bool((got["crps_fair"] == 0).all())


@pytest.mark.parametrize("S,B,Cc,hw", [(R - 1, 3, 3, (16, 17)), (4 * R + 1, 3, 4, (5, 7)), (4 * R + 1, 1, 3, (3, 300))])
def test_outputs_are_bitwise_the_same_for_every_feed(S, B, Cc, hw):
    idx = SWEEP.index((S, B, Cc, hw))
    xs, tgt, u, mu, sd = _dev(idx)
    outs = [run_scores(xs, tgt, u, sd, 1, n, padded) for n, padded in ((1, False), (2, True), (3, False), (3, False))]
    for o in outs[1:]:
        for name, v in outs[0].items():
            assert torch.equal(v, o[name]), name


def test_target_above_every_member_has_rank_s():
    S, B, Cc, Hh, Ww = 9, 3, 3, 16, 17
    xs, _, _, mu, sd = _dev(SWEEP.index((S, B, Cc, (Hh, Ww))))
    tgt = xs.amax(1) + 0.5
    got = run_scores(xs, tgt, None, sd, 0, 2, padded=False)
    assert bool((got["rank_hist"][..., S] == Hh * Ww).all()) and bool((got["rank_hist"][..., :S] == 0).all())
    assert bool((got["time_rank_hist"][..., S] == T * Hh * Ww).all())


def test_identical_members_score_the_absolute_error():
    S, B, Cc, Hh, Ww = 9, 3, 3, 16, 17
    xs, tgt, _, mu, sd = _dev(SWEEP.index((S, B, Cc, (Hh, Ww))))
    xs = xs[:, :1].expand(T, S, B, Cc, Hh, Ww).contiguous()
    u = torch.full((B, Cc), 1.3, device=DEV)
    got = run_scores(xs, tgt, u, sd, 0, 3, padded=True)
    assert torch.equal(got["crps"], got["crps_fair"])                          # a zero pair term
    ref, parts = ref_scores(xs, tgt, u, mu, sd, 0)
    a = parts["a"].view(B, 1, Cc, 1, 1)
    closed = a * (xs[:, 0].double() - tgt.double()).abs().transpose(0, 1)
    assert bool(((ref["crps"] - closed).abs() <= 1e-12 * (1 + closed)).all())
    assert bool(((got["crps"].double() - closed).abs() <= n_step(S) * U24 * a * parts["s"] + 1e-6 * closed).all())


# ---- end to end: modelPredScores == fp64 numpy scores of modelPred's samples ------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_scores_matches_numpy_over_model_pred(monkeypatch, tmp_path, case):
    import tmg_ops as ops
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)

    def roll(seed):
        for _ in range(2):                                                    # two folded runs: modelPredScores, modelPredStats
            for bi, B in enumerate(batches):
                per = max(1, max_rows // B)
                for t in range(tmax):
                    for m0 in range(0, S, per):
                        kp.queue_fold(bi, t, m0, min(per, S - m0))
        for bi, B in enumerate(batches):
            for m in range(S):
                for t in range(tmax):
                    kp.queue_serial(bi, t, m)
        torch.manual_seed(seed)
        got = utils.modelPredScores(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
        torch.manual_seed(seed)
        stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
        assert not kp.fold
        torch.manual_seed(seed)
        pred, tgt, _ = utils.modelPred(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax)
        assert not kp.serial
        return got, stats, pred.double().numpy(), tgt.double().numpy()

    # modelPred un-normalises in fp32, which can merge a member with a target it differs from by less than 4 u ymax: the histograms are
    # compared exactly only under a seed with no such (member, pixel) pair; the first of the fixed list that has none is used
    for seed in SEEDS:
        got, stats, p, y = roll(seed)                                        # p [S, N, Tk, C, H, W], un-normalised
        Tk = p.shape[2]
        y = y[:, ::stride][:, :Tk]                                           # [N, Tk, C, H, W]
        ymax = max(float(np.abs(p).max()), float(np.abs(y).max()))
        close = int((np.abs(p - y[None]) < 4 * U24 * ymax).sum())
        print("%s seed %d: (member, pixel) pairs closer to the target than 4 u ymax: %d" % (case, seed, close))
        if close == 0:
            break
    assert close == 0, "no seed of %s without a near-tie" % (SEEDS,)
    assert set(got) == set(stats) | set(KEYS) | {"rank_hist", "time_rank_hist"}
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    N, Cc, Hh, Ww = y.shape[0], y.shape[2], y.shape[3], y.shape[4]
    first = np.abs(p - y[None]).mean(0)
    pair = sum(np.abs(p[m][None] - p).sum(0) for m in range(S))
    ref = {"crps": first - pair / (2.0 * S * S), "crps_fair": first - pair / (2.0 * S * (S - 1))}
    ref["time_crps"] = ref["crps"][:, t_start:].mean(1)
    ref["time_crps_fair"] = ref["crps_fair"][:, t_start:].mean(1)
    rank = (p < y[None]).sum(0)                                               # [N, Tk, C, H, W]
    hist = np.stack([(rank == r).sum((-2, -1)) for r in range(S + 1)], -1)    # [N, Tk, C, S + 1]
    assert np.array_equal(got["rank_hist"].numpy(), hist)
    assert np.array_equal(got["time_rank_hist"].numpy(), hist[:, t_start:].sum(1))
    assert float(got["rank_hist"].sum(-1).min()) == Hh * Ww == float(got["rank_hist"].sum(-1).max())
    # bound 3 with the normalised magnitudes recovered in fp64: x = (xh / uc - out_mu) / out_std
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).double().numpy()
    uc = np.stack([u0, u0, u0 ** 2], 1)[:, :Cc]                              # [N, C]
    mu, sd = model.out_mu.detach().double().cpu().numpy().reshape(-1)[:Cc], model.out_std.detach().double().cpu().numpy().reshape(-1)[:Cc]
    a = (uc * sd[None]).reshape(N, 1, Cc, 1, 1)
    xn = (p / uc.reshape(1, N, 1, Cc, 1, 1) - mu.reshape(1, 1, 1, Cc, 1, 1)) / sd.reshape(1, 1, 1, Cc, 1, 1)
    yn = (y / uc.reshape(N, 1, Cc, 1, 1) - mu.reshape(1, 1, Cc, 1, 1)) / sd.reshape(1, 1, Cc, 1, 1)
    scale = a * (np.abs(xn).max(0) + np.abs(yn))
    tscale = scale[:, t_start:].max(1)
    for name in KEYS:
        timed = name.startswith("time_")
        bnd = (n_time(S, Tk - t_start) * tscale if timed else n_step(S) * scale) * U24 + 1e-6 * np.abs(ref[name])
        share = float((np.abs(got[name].double().numpy() - ref[name]) / bnd).max())
        print("%s %s: worst share of the bound %.3f" % (case, name, share))
        assert share <= 1.0, "%s %s: worst error is %.3f of its bound" % (case, name, share)
    assert float(got["crps"].max()) > 0
