"""CPU-side checks of the ensemble calibration scores: the two kernel entries are declared, listed and exported, the ops /
post-processing entry points exist with their signatures (the pinned ones unchanged), the argument errors come in the documented order
without a GPU, an fp32 torch emulation of the step kernel's data flow stays inside the GPU test's bound against fp64 at the GPU test's
shapes (the evidence for the bound where there is no GPU), and the fp64 reference is sensitive at ten bounds."""
import ctypes
import functools
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import common as C
import test_scores_gpu as G

NEW_SYMBOLS = ["tmg_ens_score_store", "tmg_ens_score_step"]


def test_new_symbols_declared_listed_and_exported():
    import tmg_hip
    hdr = open(os.path.join(C.ROOT, "include", "tmglow_hip.h")).read()
    ret = dict((n, t) for t, n in re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", hdr))
    lib = ctypes.CDLL(tmg_hip.build())
    for name in NEW_SYMBOLS:
        assert ret.get(name) == "int", name
        assert name in tmg_hip.EXPORTS, name
        assert name not in tmg_hip.RET_I64, name
        assert hasattr(lib, name), name
    assert len(tmg_hip.EXPORTS) == len(set(tmg_hip.EXPORTS)) == 89
    assert "tmg_scores.hip" in tmg_hip.SOURCES and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_scores.hip"))
    assert all(callable(getattr(tmg_hip, n)) for n in ("ens_score_store", "ens_score_step"))


def test_entry_points_and_pinned_signatures():
    from utils import utils
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredScores).parameters
    assert list(sig) == old
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleScores.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_std", "u"]
    assert init["u"].default is None
    add = inspect.signature(tmg_ops.EnsembleScores.add).parameters
    assert list(add) == ["self", "y", "m0", "target", "time"] and add["time"].default is True
    # the pinned ones keep their parameter lists
    assert list(inspect.signature(utils.modelPredStats).parameters) == old
    assert list(inspect.signature(utils.modelPredTurbulence).parameters) == old
    assert list(inspect.signature(utils.modelPredSpectra).parameters) == old + ["window"]
    assert list(inspect.signature(tmg_ops.EnsembleStats.__init__).parameters) == [
        "self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid"]


def _scores(members=3, B=2, Cc=3, out_std=None, u=None, device="cpu"):
    import tmg_ops
    return tmg_ops.EnsembleScores(members, B, Cc, 4, 5, 2, device, torch.ones(Cc) if out_std is None else out_std, u=u)


BAD_STD = torch.tensor([1.0, float("nan"), 1.0])


# every case is wrong in the named argument AND in every later one of the documented order (channels, members, entries of out_std,
# values of out_std / u, device): the earliest decides the message
@pytest.mark.parametrize("Cc", [1, 5])
def test_bad_channel_count_raises_first(Cc):
    with pytest.raises(ValueError, match="channels"):
        _scores(members=0, Cc=Cc, out_std=BAD_STD)


@pytest.mark.parametrize("members", [0, 1025, -1])
def test_bad_member_count_raises_second(members):
    with pytest.raises(ValueError, match="members"):
        _scores(members=members, out_std=BAD_STD[:2])


def test_short_out_std_raises_third():
    with pytest.raises(ValueError, match="entries"):
        _scores(out_std=BAD_STD[:2])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_bad_out_std_or_u_raises_before_the_device(bad):
    sd = torch.tensor([1.0, bad, 2.0])
    with pytest.raises(ValueError, match=r"^out_std must"):
        _scores(out_std=sd, u=torch.full((2, 3), bad))
    u = torch.ones(2, 3)
    u[1, 2] = bad
    with pytest.raises(ValueError, match=r"^u must"):
        _scores(u=u)


@pytest.mark.parametrize("members", [1, 1024])
def test_cpu_device_raises_last(members):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _scores(members=members, u=torch.full((2, 3), 0.5))


def test_model_pred_scores_on_cpu_raises():
    from nn.tmGlow import TMGlow
    from utils import utils
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**C.build_kwargs(C.CFG_TINY)).eval()
    log = SimpleNamespace(log=lambda *a, **k: None)
    x = torch.zeros(2, 3, C.CFG_TINY["in_features"], *C.CFG_TINY["_in_hw"])
    loader = [(x, torch.zeros(2, 3, 3, 16, 16), torch.ones(2))]
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.modelPredScores(SimpleNamespace(device=None), m, loader, log, samples=2, tmax=2)


# ---- the step kernel's data flow in fp32 torch ------------------------------------------------------------------------------------
def _emulate_step(x, y, a):
    """csrc/tmg_scores.hip's ens_score_step_kernel in fp32 torch, operation by operation (torch's elementwise fp32 add / sub / mul
    are the kernel's rounded ones; nothing is fused): x [S, B, C, H, W], y [B, C, H, W], a [B, C] fp32 -> (crps, crps_fair, rank)."""
    S = x.shape[0]
    f32 = torch.float32
    c1 = torch.tensor(1.0 / S, dtype=f32)
    cp = torch.tensor(1.0 / (float(S) * S), dtype=f32)
    cpf = torch.tensor(1.0 / (float(S) * (S - 1)) if S > 1 else 0.0, dtype=f32)
    t1, tp = torch.zeros_like(y), torch.zeros_like(y)
    below = torch.zeros(y.shape, dtype=torch.int64)
    for m0 in range(0, S, G.R):
        nr = min(G.R, S - m0)
        r = x[m0:m0 + nr]
        acc = torch.zeros_like(r)
        a1 = torch.zeros_like(y)
        for i in range(nr):
            a1 = a1 + (r[i] - y).abs()
            below += r[i] < y
        for j in range(1, nr):                                               # acc[i] takes the block's later members in order
            acc[:j] = acc[:j] + (r[:j] - r[j]).abs()
        for n in range(m0 + G.R, S):                                         # then the streamed ones
            acc = acc + (r - x[n]).abs()
        ap = acc[0]
        for i in range(1, nr):
            ap = ap + acc[i]                                                 # (the kernel's unused accumulators add exact zeros)
        t1 = t1 + a1
        tp = tp + ap
    av = a.view(a.shape[0], a.shape[1], 1, 1)
    first = t1 * c1
    return av * (first - tp * cp), av * (first - tp * cpf), below


def _emulate(xs, tgt, u, sd, t_start):
    """EnsembleScores over the steps: the step kernel's scores, the rank histogram, and the in-place fp32 running time means."""
    Tn, S, B, Cc, Hh, Ww = xs.shape
    a = sd.view(1, Cc).expand(B, Cc).contiguous() if u is None else u * sd.view(1, Cc)        # fp32 product, as the constructor
    out = {"crps": torch.empty(B, Tn, Cc, Hh, Ww), "crps_fair": torch.empty(B, Tn, Cc, Hh, Ww)}
    hist = torch.zeros(B, Tn, Cc, S + 1, dtype=torch.int64)
    tm = [torch.zeros(B, Cc, Hh, Ww), torch.zeros(B, Cc, Hh, Ww)]
    for t in range(Tn):
        v0, v1, below = _emulate_step(xs[t], tgt[t], a)
        out["crps"][:, t], out["crps_fair"][:, t] = v0, v1
        hist[:, t] = torch.nn.functional.one_hot(below.reshape(B, Cc, Hh * Ww), S + 1).sum(2)
        if t >= t_start:
            tn = torch.tensor(1.0, dtype=torch.float32) / float(t - t_start + 1)
            tm = [m + (v - m) * tn for m, v in zip(tm, (v0, v1))]
    out.update(time_crps=tm[0], time_crps_fair=tm[1], rank_hist=hist, time_rank_hist=hist[:, t_start:].sum(1))
    return out


@functools.lru_cache(maxsize=None)
def _reference(idx):
    xs, tgt, u, mu, sd = G.inputs(idx)
    return G.ref_scores(xs, tgt, u, mu, sd, G.features(idx)[1])


def test_rounding_counts_are_the_documented_ones():
    assert [G.n_step(S) for S in (1, 2, 7, 8, 9, 33)] == [20, 22, 32, 34, 37, 67]
    assert G.n_time(33, 4) == 79
    assert sorted(set(s[0] for s in G.SWEEP)) == [1, 2, G.R - 1, G.R, G.R + 1, 4 * G.R + 1]


@pytest.mark.parametrize("idx", range(len(G.SWEEP)))
def test_fp32_emulation_of_the_step_kernel_stays_in_the_gpu_bound(idx):
    S, B, Cc, (Hh, Ww) = G.SWEEP[idx]
    xs, tgt, u, mu, sd = G.inputs(idx)
    t_start = G.features(idx)[1]
    ref, parts = _reference(idx)
    got = _emulate(xs, tgt, u, sd, t_start)
    G.check_hists(got, ref, Hh * Ww, "sweep %s" % (G.SWEEP[idx],))
    worst = G.check_scores(got, ref, G.bounds(ref, parts, S, t_start), "sweep %s" % (G.SWEEP[idx],))
    print("sweep %s: the emulation's worst share of the bound %.3f" % (G.SWEEP[idx], worst))


@pytest.mark.parametrize("idx", [i for i, s in enumerate(G.SWEEP) if s[0] >= 2])
def test_reference_is_sensitive_at_ten_bounds(idx):
    """On the fp64 reference alone: leaving member 0 out of the first term, or member 0's pairs out of the pair term, moves the score
    by at least ten bounds at >= 99 % of the elements."""
    S, B, Cc, (Hh, Ww) = G.SWEEP[idx]
    xs, tgt, u, mu, sd = G.inputs(idx)
    ref, parts = _reference(idx)
    bnd = G.bounds(ref, parts, S, G.features(idx)[1])
    a = parts["a"].view(1, B, Cc, 1, 1)
    bt = lambda v: v.transpose(0, 1)                                         # noqa: E731
    d_first = bt(a * (xs[:, 0].double() - tgt.double()).abs() / S)            # the first term without member 0
    d_pairs = bt(a * (xs[:, :1].double() - xs.double()).abs().sum(1))         # sum_n |x_0 - x_n|: twice in sum_m sum_n
    for name, moved in (("crps", d_first), ("crps_fair", d_first), ("crps", d_pairs / (S * S)), ("crps_fair", d_pairs / (S * (S - 1)))):
        share = float((moved >= 10 * bnd[name]).double().mean())
        assert share >= 0.99, "%s %s: only %.4f of the elements move by ten bounds" % (G.SWEEP[idx], name, share)
    # the time means: the same omission in every step of the window moves the mean by the mean of the moves
    t0 = G.features(idx)[1]
    for name, moved in (("time_crps", d_first), ("time_crps_fair", d_pairs / (S * (S - 1)))):
        share = float((moved[:, t0:].mean(1) >= 10 * bnd[name]).double().mean())
        assert share >= 0.99, "%s %s: only %.4f of the elements move by ten bounds" % (G.SWEEP[idx], name, share)


def test_a_loose_comparison_moves_every_tie_pixel():
    """<= for < at the tie pixels of the GPU tie case: every pixel of set A moves up by exactly one bin (member 4 alone equals the
    target), every pixel of set B from bin 0 to bin S; nothing else moves."""
    xs, tgt, A, Bm = G.tie_inputs()
    S, Cc = xs.shape[1], xs.shape[3]
    mu, sd = torch.tensor(G.MU[:Cc]), torch.tensor(G.SD[:Cc])
    strict, ps = G.ref_scores(xs, tgt, None, mu, sd, 0)
    loose, pl = G.ref_scores(xs, tgt, None, mu, sd, 0, strict=False)
    d = pl["rank"] - ps["rank"]
    assert bool((d[..., A] == 1).all()) and bool((ps["rank"][..., Bm] == 0).all()) and bool((pl["rank"][..., Bm] == S).all())
    assert bool((d[..., ~(A | Bm)] == 0).all())
    assert not torch.equal(strict["rank_hist"], loose["rank_hist"])
    assert int((strict["rank_hist"] - loose["rank_hist"]).abs().sum()) >= 2 * int(Bm.sum())
