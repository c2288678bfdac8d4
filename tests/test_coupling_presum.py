"""The summed form of the narrow levels' per-layer backward pair (tmg_coupling_bwd with G0 == NULL, tmg_dense2_bwd with g0_masked).

Separate form (tests/test_coupling_kernels.py): cpl_bwd writes dtin half 1 = dto1 (the pass-through gradient) and G0 (the zero
conv's input gradient w.r.t. relu(x1), BEFORE the ReLU mask); dense2_bwd reads both and x1: dt1 = dto1 + [x1 > 0] (G0 + growth share).
Summed form: cpl_bwd reads x1 and leaves ONE tensor and the mask,
  dtin half 1 = dto1 + [x1 > 0] G0        GD = (d d1, d d2, bits, 0), bit c of `bits` = [x1_c > 0] (an integer pattern in a float slot)
and dense2_bwd completes it in place without reading x1: dt1 = dtin half 1 + [bit] (growth share).
(The mask has to be applied where the sum is formed: dto1 passes the ReLU by, G0 does not - a sum dto1 + G0 cannot be masked later.)

What is checked:
  1. cpl_bwd summed against the fp64 reference of tests/test_coupling_kernels.py (cpl_bwd_ref): its dtin half 1 + [x1 > 0] G0, with
     that test's measure and bound (TOL_BWD on max|a - ref| / max(1, max|ref|)) applied to the sum.  Every envelope point C = 8, 16,
     24, 32 (all four instantiations, PERM and not), both directions, and the addressing forms: one tensor (a channel-slice view of a
     NaN parent, through the binding; generative also the interleaved C entry, which derives x1 from x itself) and two halves.
     Shapes: 2 x 5 x 5 (one tile, all four borders and corners), 1 x 16 x 17 (a second tile column of width 1), 3 x 18 x 35 (interior,
     edge and partial tiles, a tile loop with image changes).
     Against the separate-output launch on the same operands, bit for bit: DH, dtin half 2, GD channels 0, 1; GD channel 2 = the
     mask word computed from x1, channel 3 = 0; and the summed half 1 = fl(dtin1 + [x1 > 0] G0) of the separate launch - the
     accumulator chain is the same in both forms and the sum is one fp32 addition, so this holds for any data, not only integers.
     NaN parents and the NaN channels next to every view stay intact.
  2. dense2_bwd lean, masked form, g0 aliased to out, on one case per instantiation that D2_LEAN_CASES reaches at those shapes
     (<2,5>, <4,5>, <4,4>): against fp64 (d2_ref, TOL_D2) and bit for bit against the un-aliased call on the same summed input.
  3. The level node (LevelCouplingFn through LSTMFLowBlock, C = 16, B = 2, 20 x 24, density and generative direction in one
     backward) against the per-layer path, with the tolerances of test_level_fused_node_matches_per_layer_path; the fused path must
     have taken the summed form in every layer."""
import functools
import os

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import test_coupling_kernels as K

pytestmark = pytest.mark.gpu
DEV = K.DEV
NAN = K.NAN

SHAPES = [(2, 5, 5), (1, 16, 17), (3, 18, 35)]
FORMS = ["slice", "halves", "inter"]


@functools.lru_cache(maxsize=None)
def _case(C_, dens, shape):
    """Inputs and fp64 reference of one (C, direction, shape), shared by the addressing forms; never modified."""
    B, Hh, Ww = shape
    inp = K.cpl_inputs(C_, B, Hh, Ww, seed=1000 + 37 * C_ + 7 * Hh + Ww + (1 if dens else 0))
    ref, fw = K.cpl_bwd_ref(inp, dens, True, K._ref_dev(B * Hh * Ww))
    return inp, ref, fw


def _mask_word(x1):
    ch = x1.shape[3]
    w = (x1 > 0).to(torch.int32) << torch.arange(ch, device=x1.device, dtype=torch.int32)
    return w.sum(3).to(torch.int32)


def _launch(dv, db, xb, r, g, layout, dens, summed):
    """One cpl_bwd launch on fresh NaN outputs -> dict(dtin Buf, DH, DH parent, G0 or None, GD)."""
    H = K._H()
    B, Hh, Ww, C_ = dv["x"].shape
    ch = C_ // 2
    DHb, DH = K._stash(B, Hh, Ww, C_)
    tb = K.Buf((B, Hh, Ww, C_), layout)
    G0 = None if summed else torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    GD = torch.full((B, Hh, Ww, 4), NAN, device=DEV)
    if layout == "inter":     # tmg_coupling_bwd itself (generative form): x whole, x1 = its first half
        dout, x, dtin = db.arg, xb.arg, tb.arg
        dims = H._i64(B, Hh, Ww, C_, H.seg(dout)[1], H.seg(x)[1], H.seg(DH)[1], H.seg(dtin)[1], dv["wz"].shape[1], ch + K.CC)
        rc = H.lib().tmg_coupling_bwd(H._ptr(dout), H._ptr(x), H._ptr(r), H._ptr(g), H._ptr(dv["Wm"]), H._ptr(dv["wz"]),
                                      H._ptr(dv["kappa"]), H._ptr(DH), H._ptr(dtin), H._ptr(G0), H._ptr(GD), dims, H._stream())
        assert rc == 0, rc
    else:
        assert H.coupling_bwd(db.arg, xb.half(1), r, g, dv["Wm"], dv["wz"], dv["kappa"], DH, tb.arg, G0, GD, ch + K.CC, fwd=dens,
                              x1=xb.half(0) if summed else None)
    torch.cuda.synchronize()
    return dict(tb=tb, DH=DH, DHb=DHb, G0=G0, GD=GD)


CPL_CASES = [(C_, dens, shape, form) for C_ in (8, 16, 24, 32) for dens in (False, True) for shape in SHAPES for form in FORMS
             if not (dens and form == "inter")]


@pytest.mark.parametrize("C_,dens,shape,form", CPL_CASES,
                         ids=["C%d-%s-%dx%dx%d-%s" % ((c, "dens" if d else "gen") + s + (f,)) for c, d, s, f in CPL_CASES])
def test_cpl_bwd_summed(C_, dens, shape, form):
    B, Hh, Ww = shape
    ch = C_ // 2
    inp, ref, fw = _case(C_, dens, shape)
    dv = K._to_dev(inp)
    db = K.Buf((B, Hh, Ww, C_), form, dv["dout"])
    src = dv["x"].clone()
    if dens:
        src[..., ch:] = fw["y2"].float().to(DEV)
    xb = K.Buf((B, Hh, Ww, C_), form, src)
    r = fw["r"].float().to(DEV).contiguous()
    sep = _launch(dv, db, xb, r, dv["g"], form, dens, summed=False)
    got = _launch(dv, db, xb, r, dv["g"], form, dens, summed=True)
    x1 = dv["x"][..., :ch]
    m = x1 > 0
    rdev = ref["dtin"].device
    # fp64: the separate form's two references, summed under the mask
    ref_sum = ref["dtin"][..., :ch] + m.to(rdev).double() * ref["G0"]
    gt, st = got["tb"].value(), sep["tb"].value()
    errs = dict(sum1=K._err(gt[..., :ch], ref_sum) / K.TOL_BWD, dtin2=K._err(gt[..., ch:], ref["dtin"][..., ch:]) / K.TOL_BWD,
                DH=K._err(got["DH"], ref["DH"]) / K.TOL_BWD, GD=K._err(got["GD"][..., :2], ref["GD"][..., :2]) / K.TOL_BWD)
    print("cpl_bwd summed C=%d dens=%d %s %s: err / tol %s" % (C_, dens, shape, form, {k: "%.2e" % v for k, v in errs.items()}))
    for b in (db, xb, got["tb"], sep["tb"]):
        assert b.outside_intact(), "wrote outside a channel-slice view"
    assert K._stash_intact(got["DHb"], C_) and K._stash_intact(sep["DHb"], C_), "wrote outside the DH slice"
    assert torch.equal(xb.value(), src) and torch.equal(db.value(), dv["dout"]), "an input was modified"
    for k, v in errs.items():
        assert v <= 1.0, "cpl_bwd summed %s: err %.3e x tol" % (k, v)
    # against the separate-output launch, bit for bit
    assert torch.equal(got["DH"], sep["DH"]), "DH differs from the separate form"
    assert torch.equal(gt[..., ch:], st[..., ch:]), "dtin half 2 differs from the separate form"
    assert torch.equal(got["GD"][..., :2], sep["GD"][..., :2]), "GD (d1, d2) differs from the separate form"
    gdi = got["GD"].view(torch.int32)
    assert torch.equal(gdi[..., 2], _mask_word(x1)), "GD channel 2 is not the mask word of x1"
    assert bool((gdi[..., 3] == 0).all()), "GD channel 3 must be zero"
    want = st[..., :ch] + torch.where(m, sep["G0"], torch.zeros_like(sep["G0"]))
    assert torch.equal(gt[..., :ch], want), "summed half 1 is not fl(dtin1 + [x1 > 0] G0) of the separate form"


# (ch, B, H, W) of D2_LEAN_CASES that reach <2,5>, <4,5>, <4,4>
D2_MASKED_CASES = [(8, 2, 6, 33, (2, 5)), (12, 2, 17, 40, (4, 5)), (16, 3, 13, 13, (4, 4))]


@pytest.mark.parametrize("ch,B,Hh,Ww,inst", D2_MASKED_CASES)
def test_dense2_bwd_lean_masked_in_place(ch, B, Hh, Ww, inst):
    assert (ch, B, Hh, Ww) in [c[:4] for c in K.D2_LEAN_CASES]
    p = K.d2_plan(B, Hh, Ww, ch + 4, ch, True, False)
    assert (p["NQ"], p["twl"]) == inst, p
    H = K._H()
    cc = K.CC
    inp = K.d2_inputs(ch, cc, B, Hh, Ww, seed=ch + B + Hh + Ww)
    x1 = inp["x1"].to(DEV)
    m = x1 > 0
    G0 = inp["G0"][..., :ch].contiguous().to(DEV)
    add0 = inp["add0"].to(DEV)
    s = add0 + torch.where(m, G0, torch.zeros_like(G0))          # what cpl_bwd's summed form leaves (fp32, one rounding)
    D = inp["D"].to(DEV)
    GD = inp["GD"].to(DEV).clone()
    GD.view(torch.int32)[..., 2] = _mask_word(x1)
    # the mask must come from GD alone: the x1 operand handed to the kernel is NaN
    tin = torch.full((B, Hh, Ww, 2 * ch), NAN, device=DEV)
    res = {}
    for tag in ("aliased", "separate"):
        dtin = torch.full((B, Hh, Ww, 2 * ch), NAN, device=DEV)
        dt1 = dtin[..., :ch]
        if tag == "aliased":
            dt1.copy_(s)
            g0 = dt1
        else:
            g0 = s.clone()
        DD = torch.full((B, Hh, Ww, 8), NAN, device=DEV)
        H.dense2_bwd([tin[..., :ch], D], inp["w1"].to(DEV), inp["w2"].to(DEV), None, None, GD, D, [g0], [dt1], ch, add0=None, rows1=ch,
                     rows2=ch + 1, split2=ch, gap2=cc, dd1=DD[..., 2:3], dd2=DD[..., 3:4], g0_masked=True)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dtin[..., ch:]).all()), "wrote past the output view"
        assert bool(torch.isnan(DD[..., :2]).all()) and bool(torch.isnan(DD[..., 4:]).all()), "wrote outside the dd pair"
        if tag == "separate":
            assert torch.equal(g0, s), "the un-aliased input was modified"
        res[tag] = (dt1.clone(), DD[..., 2:4].clone())
    rd = K._ref_dev(B * Hh * Ww)
    W2 = torch.cat([inp["w2"][:, :ch], inp["w2"][:, ch + cc:ch + cc + 1]], 1)
    gt, g1, g2, _, _ = K.d2_ref(inp["x1"], inp["D"], inp["G0"][..., :ch], inp["GD"], inp["w1"][:, :ch], W2, rd)
    out, dd = res["aliased"]
    errs = dict(out=K._err(out, gt + inp["add0"].to(rd, torch.float64)) / K.TOL_D2, dd1=K._err(dd[..., 0:1], g1) / K.TOL_D2,
                dd2=K._err(dd[..., 1:2], g2) / K.TOL_D2)
    print("dense2 lean masked ch=%d %dx%dx%d plan %s: err / tol %s" % (ch, B, Hh, Ww, p, {k: "%.2e" % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v <= 1.0, "dense2 lean masked %s: err %.3e x tol" % (k, v)
    assert torch.equal(res["aliased"][0], res["separate"][0]) and torch.equal(res["aliased"][1], res["separate"][1]), \
        "the aliased call differs from the un-aliased one"


def test_dense2_bwd_masked_form_outside_the_lean_shape_is_an_error():
    """The general kernel takes its mask from the inputs: the masked form with weight gradients requested must be declined."""
    H = K._H()
    ch, B, Hh, Ww = 8, 1, 4, 4
    inp = K.d2_inputs(ch, K.CC, B, Hh, Ww, seed=5)
    dv = {k: v.to(DEV) for k, v in inp.items()}
    out = torch.full((B, Hh, Ww, ch), NAN, device=DEV)
    DD = torch.full((B, Hh, Ww, 2), NAN, device=DEV)
    dW1, dW2 = torch.zeros(1, ch, 3, 3, device=DEV), torch.zeros(1, ch + 1, 3, 3, device=DEV)
    with pytest.raises(RuntimeError):
        H.dense2_bwd([dv["x1"], dv["D"]], dv["w1"][:, :ch].contiguous(), torch.cat([dv["w2"][:, :ch], dv["w2"][:, -1:]], 1).contiguous(), dW1,
                     dW2, dv["GD"], dv["D"], [dv["G0"][..., :ch].contiguous()], [out], ch, add0=None, rows1=ch, rows2=ch + 1,
                     dd1=DD[..., 0:1], dd2=DD[..., 1:2], g0_masked=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(DD).all()) and not bool(dW1.any()) and not bool(dW2.any())


def test_level_node_summed_backward_matches_per_layer_path(monkeypatch):
    from nn.modules.flowLSTMBlock import LSTMFLowBlock
    import tmg_hip as H
    forms = []
    real = H.coupling_bwd

    def spy(*a, **k):
        forms.append(a[9] is None)      # G0
        return real(*a, **k)

    monkeypatch.setattr(H, "coupling_bwd", spy)
    C.seed_all(78)
    blk = LSTMFLowBlock(4, 32, 16, 5, LUdecompose=True, train_sampling=True, do_split=True, squeeze_type=0)
    C.perturb_(blk, 5, 0.05, 0.1, 0.05)
    blk.to(DEV)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 4, 40, 48, generator=g).to(DEV)          # squeezed: C = 16 at 20 x 24
    cond = torch.randn(2, 32, 20, 24, generator=g).to(DEV)
    res = {}
    try:
        for tag, env in (("fused", None), ("plain", "1")):
            if env:
                os.environ["TMG_NO_LEVEL_FUSION"] = env
            else:
                os.environ.pop("TMG_NO_LEVEL_FUSION", None)
            blk.zero_grad()
            xi = x.clone().requires_grad_(True)
            ci = cond.clone().requires_grad_(True)
            z, ld, st, eps = blk.forward(xi, ci, None, return_eps=True)
            xr, ldr, _ = blk.reverse(z, ci, None, eps=eps.detach())
            ((z ** 2).sum() + ld.sum() * 0.01 + (xr ** 2).sum() * 0.5 + ldr.sum() * 0.02).backward()
            res[tag] = (z.detach(), ld.detach(), xr.detach(), {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None},
                        xi.grad.clone(), ci.grad.clone())
            if tag == "fused":
                n_fused = len(forms)
    finally:
        os.environ.pop("TMG_NO_LEVEL_FUSION", None)
    assert n_fused >= 2 and all(forms[:n_fused]), "the fused node must take the summed form in both directions: %s" % forms
    a, b = res["fused"], res["plain"]
    C.assert_field(a[0], b[0], "z")
    C.assert_logdet(a[1], b[1])
    C.assert_field(a[2], b[2], "x_rec")
    ga, gb = dict(a[3]), dict(b[3])
    ga.update({"@dx": a[4], "@dcond": a[5]})
    gb.update({"@dx": b[4], "@dcond": b[5]})
    C.assert_grads(ga, gb, "summed fused vs per-layer grads", global_tol=1e-4, tensor_tol=2e-3)
