"""Batched ensemble prediction on the device (`-m gpu`): the keyed latent draw (tmg_gauss_sample_keyed) against single-key calls,
the ensemble-statistics kernels (tmg_ens_accum / tmg_ens_time_finalize) against an fp64 torch statement, TMGlow.sampleEnsemble
against the serial sample roll-out member by member, and utils.modelPredStats against numpy statistics of modelPred's samples."""
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

LOG = SimpleNamespace(log=lambda *a, **k: None, warning=lambda *a, **k: None, error=lambda *a, **k: None)


# ---- keyed latent draw ---------------------------------------------------------------------------------------------------------
def _keys(K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 62, 2 ** 62, (K, 2), generator=g, dtype=torch.int64).to(DEV)


def _draw(H, hz, z1, keys, rows_per_key, site, limits, clip):
    B, Hh, Ww, C2 = hz.shape
    Ch = C2 // 2
    out = torch.empty(B, Hh, Ww, 2 * Ch if z1 is not None else Ch, device=DEV)
    eps = torch.empty(B, Hh, Ww, Ch, device=DEV)
    logp = torch.zeros(B, device=DEV)
    if rows_per_key is None:
        H.gauss_sample(hz, None, z1, out, logp, clip, limits, eps_out=eps, nonce=keys, site=site)
    else:
        H.gauss_sample_keyed(hz, None, z1, out, logp, clip, limits, keys, rows_per_key, site=site, eps_out=eps)
    return out, eps, logp


# (B, K, h, w, Ch): vector (Ch % 4 == 0) and scalar forms; (7, 3, 128, 128, .) makes the folded grid cap (98 blocks per image for
# 21 images) bind while the 7-image calls run 128 / 112 blocks per image: the counters must not depend on the launch plan
@pytest.mark.parametrize("B,K,Hh,Ww,Ch", [(2, 3, 8, 8, 4), (1, 4, 5, 7, 3), (7, 3, 128, 128, 8), (7, 3, 128, 128, 7)])
@pytest.mark.parametrize("with_z1", [False, True])
def test_keyed_draw_is_bitwise_k_single_key_draws(B, K, Hh, Ww, Ch, with_z1):
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator().manual_seed(5 + B * Ch)
    hz = (1.5 * torch.randn(B, Hh, Ww, 2 * Ch, generator=g)).to(DEV)
    z1 = torch.randn(B, Hh, Ww, Ch, generator=g).to(DEV) if with_z1 else None
    limits, clip, site = (ops.SPLIT_LIMITS, 1, 1) if with_z1 else (ops.TOP_LIMITS, 0, 3)
    keys = _keys(K, 100 + K)
    out, eps, logp = _draw(H, hz.repeat(K, 1, 1, 1), None if z1 is None else z1.repeat(K, 1, 1, 1), keys, B, site, limits, clip)
    for m in range(K):
        o1, e1, l1 = _draw(H, hz, z1, keys[m].clone(), None, site, limits, clip)
        rows = slice(m * B, (m + 1) * B)
        assert torch.equal(out[rows], o1), "member %d: sample" % m
        assert torch.equal(eps[rows], e1), "member %d: latents" % m
        torch.testing.assert_close(logp[rows], l1, rtol=1e-5, atol=1e-3)     # one float atomic per block: the sum order may differ
    # distinct keys: the members differ; equal keys: they repeat each other
    assert not torch.equal(eps[:B], eps[B:2 * B])
    same = keys[:1].repeat(K, 1).contiguous()
    _, eps_s, _ = _draw(H, hz.repeat(K, 1, 1, 1), None if z1 is None else z1.repeat(K, 1, 1, 1), same, B, site, limits, clip)
    for m in range(1, K):
        assert torch.equal(eps_s[m * B:(m + 1) * B], eps_s[:B])
    assert torch.equal(eps_s[:B], eps[:B])


# ---- ensemble statistics kernels ---------------------------------------------------------------------------------------------
def _chunks(S, n):
    """n chunks of unequal size (as far as S allows) covering 0..S-1."""
    n = min(n, S)
    if n == 1:
        return [S]
    if n == 2:
        a = max(1, (2 * S) // 3)
        return [a, S - a] if a < S else [S - 1, 1]
    a = max(1, S // 5)
    b = max(1, (S - a) // 2 + 1)
    if a + b >= S:
        a, b = 1, 1
    return [a, b, S - a - b]


def _ref_stats(ys, u, mu, sd, t_start):
    """fp64 statement: ys [T, S, B, C, H, W] raw model outputs -> the outputs of EnsembleStats, and max |yh|."""
    yh = ys.double() * sd.double().view(1, 1, 1, -1, 1, 1) + mu.double().view(1, 1, 1, -1, 1, 1)
    if u is not None:
        yh = yh * u.double().view(1, 1, *u.shape, 1, 1)
    mag = torch.sqrt(yh[:, :, :, 0] ** 2 + yh[:, :, :, 1] ** 2)
    ref = {"mean": yh.mean(1).permute(1, 0, 2, 3, 4), "std": yh.std(1, unbiased=False).permute(1, 0, 2, 3, 4),
           "mag_mean": mag.mean(1).permute(1, 0, 2, 3), "mag_std": mag.std(1, unbiased=False).permute(1, 0, 2, 3)}
    tw = yh[t_start:]
    tmean = tw.mean(0)                                                        # [S, B, C, H, W]
    trms = torch.sqrt(((tw - tmean.unsqueeze(0)) ** 2).mean(0))
    ref.update(time_mean_mean=tmean.mean(0), time_mean_std=tmean.std(0, unbiased=False), time_rms_mean=trms.mean(0),
               time_rms_std=trms.std(0, unbiased=False))
    return ref, float(yh.abs().max())


def _run_stats(ys, u, mu, sd, t_start, nchunks, padded):
    import tmg_ops as ops
    T, S, B, Cc, Hh, Ww = ys.shape
    st = ops.EnsembleStats(S, B, Cc, Hh, Ww, T, DEV, mu, sd, u=u)
    sizes = _chunks(S, nchunks)
    for t in range(T):
        m0 = 0
        for k in sizes:
            y = ys[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww).permute(0, 2, 3, 1)         # NHWC [k*B, H, W, C]
            if padded:                                                                  # a channel slice of a wider NHWC buffer
                wide = torch.full((k * B, Hh, Ww, Cc + 3), float("nan"), device=DEV)
                wide[..., 1:1 + Cc] = y
                y = wide[..., 1:1 + Cc]
            else:
                y = y.contiguous()
            st.add(y.permute(0, 3, 1, 2), m0, time=t >= t_start)
            m0 += k
    return st.finalize()


def _check(got, ref, ymax, what):
    for name, r in ref.items():
        gv = got[name].double()
        assert gv.shape == r.shape, (name, gv.shape, r.shape)
        assert bool(torch.isfinite(gv).all()), "%s %s: non-finite" % (what, name)
        err = (gv - r).abs()
        bound = 4e-6 * ymax + 1e-5 * r.abs()
        assert bool((err <= bound).all()), "%s %s: max err %.3e, bound at that element %.3e" % (
            what, name, float(err.max()), float(bound.flatten()[int(err.argmax())]))


SWEEP = [(S, B, Cc, hw) for S in (1, 2, 7, 33) for B in (1, 3) for Cc in (3, 4) for hw in ((5, 7), (256, 256))]


def _features(idx):
    """(u given, t_start, channel-padded input, chunk count) of sweep entry idx, mixed so that every field size and member count
    >= 3 meets each value of each feature."""
    hw, c, b = idx % 2, (idx // 2) % 2, (idx // 4) % 2
    return (hw ^ c) == 0, c ^ b, (hw ^ b) == 1, 1 + (idx + idx // 8) % 3


@pytest.mark.parametrize("idx", range(len(SWEEP)))
def test_stats_kernels_match_fp64(idx):
    """Every member count, case count, channel count and field size of the sweep; the features rotate over the sweep: members fed in
    1 / 2 / 3 chunks of unequal size, u given or absent, a channel-padded NHWC input, t_start = 0 or 1."""
    S, B, Cc, (Hh, Ww) = SWEEP[idx]
    T = 3
    g = torch.Generator(device=DEV).manual_seed(1000 + idx)
    ys = torch.randn(T, S, B, Cc, Hh, Ww, device=DEV, generator=g) * 0.8 + 0.1
    mu = torch.tensor([0.3, -0.2, 0.5, 1.0][:Cc], device=DEV)
    sd = torch.tensor([1.7, 0.6, 2.5, 0.9][:Cc], device=DEV)
    u_given, t_start, padded, nchunks = _features(idx)
    u = (0.5 + torch.rand(B, Cc, device=DEV, generator=g)) if u_given else None
    got = _run_stats(ys, u, mu, sd, t_start, nchunks, padded)
    ref, ymax = _ref_stats(ys, u, mu, sd, t_start)
    _check(got, ref, ymax, "sweep %s" % (SWEEP[idx],))


def test_stats_constant_members_have_zero_spread():
    S, B, Cc, Hh, Ww, T = 7, 3, 3, 16, 20, 3
    g = torch.Generator(device=DEV).manual_seed(3)
    one = torch.randn(T, 1, B, Cc, Hh, Ww, device=DEV, generator=g) * 3.0
    ys = one.expand(T, S, B, Cc, Hh, Ww).contiguous()
    got = _run_stats(ys, torch.full((B, Cc), 1.3, device=DEV), torch.zeros(Cc, device=DEV) + 0.1, torch.ones(Cc, device=DEV) * 1.1, 0, 3,
                     padded=False)
    for name in ("std", "mag_std", "time_mean_std", "time_rms_std"):
        assert not bool(torch.isnan(got[name]).any()), name
        assert bool((got[name] == 0).all()), name


def test_stats_large_offset_field_stays_in_bound():
    """1e3 + 1e-2 N(0, 1): a naive fp32 E[y^2] - E[y]^2 loses the spread entirely here."""
    S, B, Cc, Hh, Ww, T = 33, 3, 4, 64, 64, 4
    g = torch.Generator(device=DEV).manual_seed(4)
    ys = 1e3 + 1e-2 * torch.randn(T, S, B, Cc, Hh, Ww, device=DEV, generator=g)
    one, zero = torch.ones(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    got = _run_stats(ys, None, zero, one, 1, 3, padded=True)
    ref, ymax = _ref_stats(ys, None, zero, one, 1)
    _check(got, ref, ymax, "offset field")
    assert abs(float(got["std"].mean()) - 1e-2) < 1e-3


# ---- folded roll-out == serial roll-out ------------------------------------------------------------------------------------------
def _model(cfg, seed=12345, kw=None):
    from nn.tmGlow import TMGlow
    import contextlib
    import io
    C.seed_all(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TMGlow(**(kw or C.build_kwargs(cfg)))
    C.perturb_(m, 7, *C.perturb_scales(cfg))
    return m.to(DEV).eval()


class _KeyPatch:
    """Deterministic latent keys: key(tag, t, m) for member m at step t; the folded run's latent_nonces(k) calls and the serial
    run's latent_nonce calls are handed the keys in the order each run asks for them."""

    def __init__(self, monkeypatch, ops):
        self.fold, self.serial = [], []
        monkeypatch.setattr(ops, "latent_nonces", lambda device, k: self.fold.pop(0))
        monkeypatch.setattr(ops, "latent_nonce", lambda device: self.serial.pop(0))

    @staticmethod
    def key(tag, t, m):
        return torch.tensor([1000003 * t + 7919 * m + 104729 * tag + 17, -(65537 * m + 257 * t + 3 * tag + 5)], dtype=torch.int64)

    def queue_fold(self, tag, t, m0, k):
        self.fold.append(torch.stack([self.key(tag, t, m) for m in range(m0, m0 + k)]).to(DEV))

    def queue_serial(self, tag, t, m):
        self.serial.append(self.key(tag, t, m).to(DEV))


def _cat_states(states):
    return [tuple(torch.cat([s[lv][i] for s in states]) for i in (0, 1)) for lv in range(len(states[0]))]


@pytest.mark.parametrize("cfg_name", ["CFG_TINY", "CFG_TINY3"])
def test_folded_rollout_equals_serial(monkeypatch, cfg_name):
    import tmg_ops as ops
    cfg = getattr(C, cfg_name)
    model = _model(cfg)
    S, B, T, chunks = 5, 2, 7, [(0, 3), (3, 2)]
    up = cfg["_up"]
    hw = (cfg["_in_hw"][0] * up, cfg["_in_hw"][1] * up)
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, cfg["in_features"], *cfg["_in_hw"], generator=g).to(DEV) for _ in range(T)]
    seeds = [torch.LongTensor(B).random_(0, int(1e8), generator=g) for _ in range(S)]
    anchors = [model.initLSTMStates(s, hw, cache=False) for s in seeds]
    kp = _KeyPatch(monkeypatch, ops)

    def reanchor(h0, key):
        return [(0.5 * h + 0.5 * hk, 0.5 * c + 0.5 * ck) for (h, c), (hk, ck) in zip(h0, key)]

    fold_y, fold_h = [[None] * S for _ in range(T)], [[None] * S for _ in range(T)]
    with torch.no_grad():
        cur = [[(h.clone(), c.clone()) for h, c in _cat_states(anchors[m0:m0 + k])] for m0, k in chunks]
        for t in range(T):
            for ci, (m0, k) in enumerate(chunks):
                kp.queue_fold(0, t, m0, k)
                y, _, cur[ci] = model.sampleEnsemble(xs[t], cur[ci], k)
                for j in range(k):
                    rows = slice(j * B, (j + 1) * B)
                    fold_y[t][m0 + j] = y[rows].clone()
                    fold_h[t][m0 + j] = [(h[rows].clone(), c[rows].clone()) for h, c in cur[ci]]
                if t % 3 == 0:
                    cur[ci] = reanchor(cur[ci], _cat_states(anchors[m0:m0 + k]))
        assert not kp.fold
        bitwise = True
        for m in range(S):
            h0 = [(h.clone(), c.clone()) for h, c in anchors[m]]
            for t in range(T):
                kp.queue_serial(0, t, m)
                y, _, h0 = model.sample(xs[t], h0)
                C.assert_field(fold_y[t][m], y, "%s member %d step %d: prediction" % (cfg_name, m, t))
                bitwise = bitwise and torch.equal(fold_y[t][m], y)
                for lv, ((hf, cf), (hs, cs)) in enumerate(zip(fold_h[t][m], h0)):
                    C.assert_field(hf, hs, "member %d step %d level %d: h" % (m, t, lv), atol=C.STATE_ATOL, rtol=0)
                    C.assert_field(cf, cs, "member %d step %d level %d: c" % (m, t, lv), atol=C.STATE_ATOL, rtol=0)
                    bitwise = bitwise and torch.equal(hf, hs) and torch.equal(cf, cs)
                if t % 3 == 0:
                    h0 = reanchor(h0, anchors[m])
        assert not kp.serial
    print("%s folded == serial bitwise: %s" % (cfg_name, bitwise))
    # members differ from each other (distinct keys)
    assert not torch.equal(fold_y[T - 1][0], fold_y[T - 1][1])


# ---- end to end: modelPredStats == numpy statistics of modelPred's samples ----------------------------------------------------
def _cylinder_case(tmp_path):
    from utils.dataLoader import DataLoaderAuto
    C.write_synthetic_cylinder_data(str(tmp_path), cases=(0, 47, 95, 96, 97), seed=98, hw=(8, 8), up=4)
    kw = dict(in_features=3, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=4, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(C.CFG_TINY3, seed=21, kw=kw)
    args = SimpleNamespace(exp_type='cylinder-array', ntrain=3, ntest=2, training_data_dir=str(tmp_path), testing_data_dir=str(tmp_path),
                           epoch_start=0, batch_size=2, test_batch_size=2, noise_std=0.0, seed=1)
    _, _, te = DataLoaderAuto.init_data_loaders(args, SimpleNamespace(module=model), LOG)
    return model, te


def _step_case(tmp_path):
    from utils.dataLoader import BackwardStepLoader
    C.write_synthetic_step_data(str(tmp_path), hw=(8, 8))
    kw = dict(in_features=4, out_features=3, enc_blocks=[1, 1], glow_blocks=[2, 2], cond_features=4, cglow_upscale=2, growth_rate=4,
              init_features=8, rec_features=4)
    model = _model(C.CFG_TINY3, seed=22, kw=kw)
    ld = BackwardStepLoader(str(tmp_path), str(tmp_path), shuffle=False, device=torch.device(DEV))
    te = ld.createTestingLoader([0, 1], C.LOADER_U0, inUpscale=1, batch_size=2)
    with torch.no_grad():
        model.in_mu.copy_(torch.tensor([0.1, -0.3, 0.2])); model.in_std.copy_(torch.tensor([1.2, 0.8, 1.5]))
        model.out_mu.copy_(torch.tensor([0.4, -0.1, 0.25])); model.out_std.copy_(torch.tensor([1.6, 0.7, 2.2]))
    return model, te


@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_stats_matches_numpy_over_model_pred(monkeypatch, tmp_path, case):
    import tmg_ops as ops
    from utils import utils
    model, te = (_cylinder_case if case == "cylinder" else _step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    batches = [int(b[0].shape[0]) for b in te]
    kp = _KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    for bi, B in enumerate(batches):
        per = max(1, max_rows // B)
        for t in range(tmax):
            for m0 in range(0, S, per):
                kp.queue_fold(bi, t, m0, min(per, S - m0))
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    assert per * B <= max_rows < S * B
    torch.manual_seed(77)
    got = utils.modelPredStats(args, model, te, LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    torch.manual_seed(77)
    pred, tgt, inp = utils.modelPred(args, model, te, LOG, samples=S, stride=stride, tmax=tmax)
    assert not kp.serial
    torch.testing.assert_close(got["target"], tgt, rtol=0, atol=0)
    torch.testing.assert_close(got["input"], inp, rtol=0, atol=0)
    p = pred.double().numpy()                                                # [S, N, Tk, C, H, W]
    mag = np.sqrt(p[:, :, :, 0] ** 2 + p[:, :, :, 1] ** 2)
    tw = p[:, :, t_start:]
    tmean = np.mean(tw, axis=2)
    trms = np.sqrt(np.mean((tw - tmean[:, :, None]) ** 2, axis=2))
    ref = {"mean": np.mean(p, axis=0), "std": np.std(p, axis=0), "mag_mean": np.mean(mag, axis=0), "mag_std": np.std(mag, axis=0),
           "time_mean_mean": np.mean(tmean, axis=0), "time_mean_std": np.std(tmean, axis=0),
           "time_rms_mean": np.mean(trms, axis=0), "time_rms_std": np.std(trms, axis=0)}
    assert set(got) == set(ref) | {"target", "input"}
    ymax = float(np.abs(p).max())
    _check({k: got[k] for k in ref}, {k: torch.from_numpy(v) for k, v in ref.items()}, ymax, case)
    assert float(got["std"].abs().max()) > 0                                  # the members are distinct samples
