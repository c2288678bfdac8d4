"""The growth-gradient stash of a level's backward pass as per-layer planes (large levels: TMG_LAYER_PLANES_MIN pixels and more).

  tmg_layer_unplanes: [K][npix][2] -> [npix][CP], the exact inverse of tmg_layer_planes on its first K planes, channels from 2K on
  zero - on pixel counts that are not a multiple of the kernel's 64-pixel block: (npix, CP) = (1, 4), (65, 32), (130, 8), with K = CP / 2
  and with padding planes (K < CP / 2).  From CP = 256 on the 64 staging rows of CP + 2 words exceed 64 KB (66 048 bytes) and the
  launcher takes the LDS opt-in: (65, 256, 128), (130, 256, 100), (65, 512, 256) (131 584 bytes) and (1, 512, 3); the forward
  tmg_layer_planes runs at these CP in thin_cases.PLANES_CASES.  Pure data movement: bit for bit.
  The level node (LevelCouplingFn through LSTMFLowBlock, C = 16, 2 x 20 x 24, both directions in one backward) with
  TMG_LAYER_PLANES_MIN=1 (planes: dense2_bwd writes plane k, the thin grouped weight gradient reads one plane per group, one
  re-interleaving launch in front of the conditioning side) against the default (960 pixels: the interleaved stash).  The stash
  layout changes no summation order on the way to dx, so dx must be bit for bit the default's - asserted whenever the default
  reproduces its own dx bit for bit in a second run (float atomics upstream of the node can make it differ from itself); every
  gradient within the bounds of test_level_fused_node_matches_per_layer_path in any case."""
import os

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("shape,CP,K", [((1, 1, 1), 4, 2), ((1, 5, 13), 32, 16), ((2, 5, 13), 8, 4), ((1, 5, 13), 32, 15), ((2, 5, 13), 8, 1),
                                        ((1, 5, 13), 256, 128), ((2, 5, 13), 256, 100), ((1, 5, 13), 512, 256), ((1, 1, 1), 512, 3)])
def test_layer_unplanes_inverts_layer_planes(shape, CP, K):
    import tmg_hip as H
    assert (64 * (CP + 2) * 4 > 64 * 1024) == (CP >= 256)      # the launcher's staging rows: 66 048 bytes at CP = 256, 131 584 at 512
    g = torch.Generator().manual_seed(CP + K)
    src = torch.randn(*shape, CP, generator=g).to(DEV)
    planes = H.layer_planes(src)
    assert planes.shape == (CP // 2,) + shape + (2,)
    back = H.layer_unplanes(planes[:K].contiguous(), CP)
    torch.cuda.synchronize()
    want = src.clone()
    want[..., 2 * K:] = 0.0
    assert back.shape == src.shape and torch.equal(back, want)
    assert bool((back[..., 2 * K:] == 0).all()), "padding channels must be zero"


def test_layer_unplanes_declines_bad_arguments():
    import tmg_hip as H
    p = torch.zeros(3, 1, 2, 2, 2, device=DEV)
    with pytest.raises((RuntimeError, AssertionError)):
        H.layer_unplanes(p, 4)          # 2 K > CP
    d = torch.full((4, 6), float("nan"), device=DEV)
    assert H.lib().tmg_layer_unplanes(H._ptr(p), H._ptr(d), H.c_i64(4), H.c_i64(6), H.c_i64(3), H._stream()) == -1      # CP % 4
    torch.cuda.synchronize()
    assert bool(torch.isnan(d).all())


def test_level_node_backward_with_planes_matches_interleaved_stash(monkeypatch):
    from nn.modules.flowLSTMBlock import LSTMFLowBlock
    import tmg_hip as H
    calls = []
    real = H.layer_unplanes

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(H, "layer_unplanes", spy)
    C.seed_all(78)
    blk = LSTMFLowBlock(4, 32, 16, 5, LUdecompose=True, train_sampling=True, do_split=True, squeeze_type=0)
    C.perturb_(blk, 5, 0.05, 0.1, 0.05)
    blk.to(DEV)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 4, 40, 48, generator=g).to(DEV)
    cond = torch.randn(2, 32, 20, 24, generator=g).to(DEV)
    res, n_calls = {}, {}
    for tag, env in (("default", None), ("default2", None), ("planes", "1")):
        if env:
            monkeypatch.setenv("TMG_LAYER_PLANES_MIN", env)
        else:
            monkeypatch.delenv("TMG_LAYER_PLANES_MIN", raising=False)
        del calls[:]
        blk.zero_grad()
        xi = x.clone().requires_grad_(True)
        ci = cond.clone().requires_grad_(True)
        z, ld, st, eps = blk.forward(xi, ci, None, return_eps=True)
        xr, ldr, _ = blk.reverse(z, ci, None, eps=eps.detach())
        ((z ** 2).sum() + ld.sum() * 0.01 + (xr ** 2).sum() * 0.5 + ldr.sum() * 0.02).backward()
        res[tag] = (z.detach(), ld.detach(), xr.detach(), {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None},
                    xi.grad.clone(), ci.grad.clone())
        n_calls[tag] = len(calls)
    assert n_calls == {"default": 0, "default2": 0, "planes": 2}, n_calls      # one re-interleave per level node and direction
    a, b = res["planes"], res["default"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), "the forward values must not depend on the stash layout"
    reproducible = torch.equal(res["default2"][4], b[4])
    print("dx: default reproduces itself bit for bit: %s; planes equal default: %s; max |diff| %.3e of max |dx| %.3e"
          % (reproducible, torch.equal(a[4], b[4]), float((a[4] - b[4]).abs().max()), float(b[4].abs().max())))
    if reproducible:
        assert torch.equal(a[4], b[4]), "dx: the stash layout changes no summation order"
    ga, gb = dict(a[3]), dict(b[3])
    ga.update({"@dx": a[4], "@dcond": a[5]})
    gb.update({"@dx": b[4], "@dcond": b[5]})
    C.assert_grads(ga, gb, "planes vs interleaved stash", global_tol=1e-4, tensor_tol=2e-3)
