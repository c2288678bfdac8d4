"""Non-finite values must reach the outputs ("Non-finite values"): every case of nonfinite_cases.py through its tmg_hip
wrapper, one poisoned element per launch, judged against the fp64 reference of the kernel's home test file on the same poisoned data.

  rule 1  nothing is swallowed: R non-finite -> A non-finite (no tolerance);
  rule 2  nothing leaks: R finite -> A finite and within the home file's bound on the clean data (the Winograd forwards alone may be
          non-finite on nonfinite_cases.wino_footprint);
  rule 3  operands and outputs are views inside NaN parents (test_conv_kernels.Buf, test_wino_kernels.Flat): everything outside the
          output views is NaN afterwards.
Each run prints "NONFINITE <family> <case> <label> <output> swallowed= leaked= off= share=" before it asserts.

Families: direct convolutions (forward on the lean, fallback, k = 1 and stride-2 instances, weight gradient, direct input gradient,
replicate-border fold), Winograd (f32 and bf16x3 forwards, narrow, weight gradient, grouped), growth-layer kernels (c1_fwd, c1x2_fwd,
c1_bwd, the thin grouped weight gradient), the fused coupling (coupling_fwd, coupling_bwd, dense2_bwd, masked_add, affine_apply,
affine_bwd), diagonal Gaussian (forward / backward in both modes, clip on and off; the draw with eps given on both instances), Adam,
the BatchNorm chain, the basic ensemble statistics, phys_fwd / phys_rms / phys_fields / phys_bwd, the nodes CouplingTailFn, ConvLSTMCellFn,
DenseBlockFn (train and eval), MixFn and ConvFn forward and backward, and the whole tiny model against the fp64 oracle.

On an MI355X: 400 tests in 4.7 s; the slowest, test_conv_dgrad_direct[dg_s2_k3_odd-dy.a.nan], 0.8 s (the first launch of the process),
test_whole_model 0.5 s.  Against the parent commit's library and wrappers 154 of the 400 fail (LAB_NOTES.md, "Non-finite values")."""
import math

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import conv_cases as CC
import nonfinite_cases as N
import wino_cases as WC
from test_conv_kernels import Buf, _dev, _kappa, _split
from test_wino_kernels import Flat

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _H():
    import tmg_hip as H
    return H


def outside_nan(b):
    """Rule 3 for a Buf / Flat: every float of the parent that is not part of the view is still NaN."""
    view = b.view if isinstance(b, Buf) else b.t
    mark = torch.zeros_like(b.flat, dtype=torch.bool)
    mark.as_strided(view.shape, view.stride(), view.storage_offset() - b.flat.storage_offset()).fill_(True)
    return bool(torch.isnan(b.flat[~mark]).all())


def _settle(case, label, run, got, bufs):
    torch.cuda.synchronize()
    N.assert_not_vacuous(dict(run, glob=run["glob"] or label in case["glob"]))
    v = N.judge(run, got)
    for name, r in v.items():
        print("NONFINITE %s %s %s %s swallowed=%d leaked=%d off=%d share=%.4f" % (
            case["family"], case["name"], label, name, r["swallowed"], r["leaked"], r["off"], r["share"]))
    bad = N.failures(v)
    assert not bad, "%s %s %s: %s" % (case["family"], case["name"], label, "; ".join(bad))
    assert all(outside_nan(b) for b in bufs), "%s %s %s: written outside a view" % (case["family"], case["name"], label)


def _params(family):
    return [pytest.param(c, lab, id="%s-%s" % (c["name"], lab)) for c in N.CASES if c["family"] == family for lab in c["labels"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# direct convolutions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("conv_fwd"))
def test_conv_fwd(case, label):
    H = _H()
    cc = CC.FWD_BY_NAME[case["name"]]
    run = case["build"](label, H)
    d, B = run["d"], run["B"]
    Hh, Ww = cc["hw"]
    Ho, Wo = CC.out_hw(Hh, Ww, cc["s"])
    sw, k, s = cc["sw"], cc["k"], cc["s"]
    cout = sum(o[0] for o in cc["outs"])
    ins = _split(d["x"], cc["ins"], (B, Hh, Ww))
    outs = _split(d["prev"], cc["outs"], (B, Ho, Wo))
    add = Buf((B, Ho, Wo), cc["add"], d["add"]) if cc["add"] is not None else None
    kw = dict(bias=_dev(d["bias"]), kappa=_kappa(d["kappa"]), in_scale=_dev(d["scale"]), in_shift=_dev(d["shift"]),
              relu_in="relu_in" in sw, pad_rep="rep" in sw, relu_out="relu_out" in sw, accumulate="acc" in sw,
              add=add.view if add is not None else None)
    p = H.conv_fwd_plan([b.view for b in ins], cout, k, s, [b.view for b in outs], **kw)
    assert p["rc"] == 0 and CC.fwd_instance(p) == cc["want"] and all(p[f] == v for f, v in cc["plan"].items()), (case["name"], p)
    H.conv_fwd([b.view for b in ins], H.conv_pack(_dev(d["w"]), 0), cout, k, s, [b.view for b in outs], **kw)
    _settle(case, label, run, {"out": torch.cat([b.view for b in outs], 3)}, outs)


@pytest.mark.parametrize("case,label", _params("conv_wgrad"))
def test_conv_wgrad(case, label, monkeypatch):
    H = _H()
    cc = CC.WG_BY_NAME[case["name"]]
    monkeypatch.setattr(H, "conv_wino_wgrad", lambda *a, **k: pytest.fail("routed to the Winograd weight-gradient kernel"))
    CC.wg_plan(H, cc)
    run = case["build"](label, H)
    d = run["d"]
    B, Hh, Ww = cc["shape"]
    Ho, Wo = CC.out_hw(Hh, Ww, cc["s"])
    sw, k, s, cin, cout = cc["sw"], cc["k"], cc["s"], cc["cin"], cc["cout"]
    cd, cv, cs, o0, o1 = cc["layout"]
    ins = _split(d["x"], cc["ins"], (B, Hh, Ww))
    dy = Buf((B, Ho, Wo), cc["dy"], d["dy"])
    dW = Flat(d["prevW"] if d["prevW"] is not None else torch.zeros(cout, cd or cin, k * k))
    db = Flat(d["prevb"] if d["prevb"] is not None else torch.zeros(cout)) if "dbias" in sw else None
    kw = dict(kappa=_kappa(d["kappa"]), in_scale=_dev(d["scale"]), in_shift=_dev(d["shift"]), relu_in="relu_in" in sw,
              pad_rep="rep" in sw, use_ws=cc["ws"], cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    H.conv_wgrad([b.view for b in ins], dy.view, dW.t, db.t if db else None, k, s, **kw)
    got = {"dW": dW.t}
    if db is not None:
        got["dbias"] = db.t
    _settle(case, label, run, got, [dW] + ([db] if db else []))


@pytest.mark.parametrize("case,label", _params("conv_dgrad"))
def test_conv_dgrad_direct(case, label):
    H = _H()
    run = case["build"](label, H)
    d = run["d"]
    B, Hin, Win, cin = d["shape"]
    k, s = d["k"], d["s"]
    Ho, Wo = CC.out_hw(Hin, Win, s)
    cout = d["w"].shape[0]
    dy = Buf((B, Ho, Wo), d["dys"] or CC.seg(cout), d["dy"])
    dx = Buf((B, Hin, Win), d["dxs"] or CC.seg(cin), None)
    H.conv_dgrad_direct(dy.view, _dev(d["w"]), dx.view, k, s, accumulate=False)
    _settle(case, label, run, {"dx": dx.view}, [dx])


@pytest.mark.parametrize("case,label", _params("conv_border"))
def test_conv_rep_border_fix(case, label):
    H = _H()
    cc = dict(CC.BD_BY_NAME[case["name"]], kappa=True)
    CC.bd_plan(H, cc)
    run = case["build"](label, H)
    d = run["d"]
    B, Hh, Ww = cc["shape"]
    dy = Buf((B, Hh, Ww), cc["dy"], d["dy"])
    outs = _split(d["prev"], cc["outs"], (B, Hh, Ww))
    H.conv_rep_border_fix(dy.view, H.conv_pack(_dev(d["w"]), 1), [b.view for b in outs], kappa=_kappa(d["kappa"]))
    _settle(case, label, run, {"out": torch.cat([b.view for b in outs], 3)}, outs)


# ---------------------------------------------------------------------------------------------------------------------------------
# Winograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _wino_fwd(case, label, arith):
    H = _H()
    narrow = case["family"] == "wino_narrow"
    wc = (WC.NARROW_BY_NAME if narrow else WC.FWD_BY_NAME)[case["name"].rsplit("-", 1)[0] if not narrow else case["name"]]
    run = case["build"](label, H)
    d, B = run["d"], run["B"]
    Hh, Ww = wc["hw"]
    ins = _split(d["x"], wc["ins"], (B, Hh, Ww))
    outs = _split(None, wc["outs"], (B, Hh, Ww))
    _, cout, _, kw = WC.fwd_args(wc, B)
    kw["bias"] = _dev(d["bias"])
    p = WC.fwd_plan_fn(H, wc, arith)([b.view for b in ins], cout, [b.view for b in outs], **kw)
    assert WC.fwd_plan_ok(wc, arith, p), (case["name"], arith, p)
    wd = _dev(d["w"])
    iv, ov = [b.view for b in ins], [b.view for b in outs]
    if narrow:
        ok = H.conv_wino_narrow(iv, H.conv_wino_pack(wd, 0, 0), cout, ov, **kw)
    elif arith == "bf16x3":
        ok = H.conv_wino_fwd3(iv, H.conv_wino_pack3(wd, 0, 0), cout, ov, **kw)
    else:
        ok = H.conv_wino_fwd(iv, H.conv_wino_pack(wd, 0, 0), cout, ov, **kw)
    assert ok, "the launcher declined the case"
    _settle(case, label, run, {"out": torch.cat(ov, 3)}, outs)


@pytest.mark.parametrize("case,label", _params("wino_fwd"))
def test_wino_fwd(case, label):
    _wino_fwd(case, label, case["name"].rsplit("-", 1)[1])


@pytest.mark.parametrize("case,label", _params("wino_narrow"))
def test_wino_narrow(case, label):
    _wino_fwd(case, label, "f32")


@pytest.mark.parametrize("case,label", _params("wino_wgrad"))
def test_wino_wgrad(case, label):
    H = _H()
    wc = WC.WG_BY_NAME[case["name"]]
    run = case["build"](label, H)
    d, B = run["d"], run["B"]
    _, Hh, Ww = wc["shape"]
    sw = wc["sw"]
    cd, cv, cs, o0, o1 = wc["layout"]
    ins = _split(d["x"], wc["ins"], (B, Hh, Ww))
    dy = Buf((B, Hh, Ww), wc["dy"], d["dy"])
    dW = Flat(d["prevW"])
    db = Flat(d["prevb"]) if "dbias" in sw else None
    kw = dict(relu_in="relu_in" in sw, pad_rep="rep" in sw, cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    p = H.conv_wino_wgrad_plan([b.view for b in ins], dy.view, dbias=db.t if db else None, **kw)
    assert WC.wg_plan_ok(wc, p), (case["name"], p)
    ok = H.conv_wino_wgrad([b.view for b in ins], dy.view, dW.t, db.t if db else None, **kw)
    assert ok, "the launcher declined the case"
    got = {"dW": dW.t}
    if db is not None:
        got["dbias"] = db.t
    _settle(case, label, run, got, [dW] + ([db] if db else []))


@pytest.mark.parametrize("case,label", _params("wino_wgrad_grouped"))
def test_wino_wgrad_grouped(case, label, monkeypatch):
    H = _H()
    wc = WC.GROUPED_BY_NAME[case["name"]]
    run = case["build"](label, H)
    ds = run["d"]
    G, cin, cg = wc["G"], wc["cin"], wc["cout"]
    B, Hh, Ww = wc["shape"]
    sw = wc["sw"]
    cd, cv, cs, o0, o1 = wc["layout"]
    ins = [Buf((B, Hh, Ww), CC.seg(cin, cin + 8, 4) if g % 2 == 0 else CC.seg(cin), d["x"]) for g, d in enumerate(ds)]
    dy = Buf((B, Hh, Ww), CC.seg(G * cg, G * cg + 8, 4) if wc["dy_slice"] else CC.seg(G * cg), torch.cat([d["dy"] for d in ds], 3))
    dW = Flat(torch.stack([d["prevW"] for d in ds]).reshape(G, cg, cd or cin, 3, 3))
    db = Flat(torch.stack([d["prevb"] for d in ds])) if "dbias" in sw else None
    kw = dict(relu_in="relu_in" in sw, pad_rep="rep" in sw, cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    monkeypatch.setattr(H.lib(), "tmg_conv_wgrad_grouped", lambda *a, **k: pytest.fail("fell through to the direct grouped kernel"))
    ok = H.conv_wgrad_grouped([[b.view] for b in ins], dy.view, cg, dW.t, db.t if db else None, 3, 1, **kw)
    assert ok
    got = {}
    for g in range(G):
        got["dW%d" % g] = dW.t[g].reshape(cg, cd or cin, 9)
        if db is not None:
            got["dbias%d" % g] = db.t[g]
    _settle(case, label, run, got, [dW] + ([db] if db else []))


# ---------------------------------------------------------------------------------------------------------------------------------
# diagonal Gaussian, Adam, ensemble statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def _pw_intact(bufs):
    import test_pointwise_kernels as PW
    return all(PW.intact(base, off, cn) for base, off, cn in bufs)


@pytest.mark.parametrize("case,label", _params("gauss"))
def test_gauss(case, label):
    import test_pointwise_kernels as PW
    H = _H()
    name, B, Hh, Ww, Ch, mode, clip, has_zout, has_dzin, has_dzout, has_g = N.GAUSS[case["name"]][:11]
    run = case["build"](label, H)
    d = run["d"]
    _, hz = PW.view(B, Hh, Ww, 2 * Ch, 3, 5, d["hz"])
    _, zin = PW.view(B, Hh, Ww, Ch, 1, 2, d["v"])
    zb, zout = PW.view(B, Hh, Ww, Ch, 2, 1) if has_zout else (None, None)
    lp = d["lp0"].to(DEV)
    H.gauss_fwd(hz, zin, zout, lp, mode, clip, d["lim"])
    _, dzin = PW.view(B, Hh, Ww, Ch, 2, 2, d["dz"]) if has_dzin else (None, None)
    dzb, dzout = PW.view(B, Hh, Ww, Ch, 1, 1) if has_dzout else (None, None)
    dhb, dhz = PW.view(B, Hh, Ww, 2 * Ch, 3, 2)
    H.gauss_bwd(hz, zin, dzin, d["g"].to(DEV) if has_g else None, dzout, dhz, mode, clip, d["lim"])
    got = {"logp": lp, "dhz": dhz, "zout": zout, "dzout": dzout}
    _settle(case, label, run, got, [])
    assert _pw_intact([(dhb, 3, 2 * Ch)] + ([(zb, 2, Ch)] if has_zout else []) + ([(dzb, 1, Ch)] if has_dzout else []))
    if mode == 1 and has_dzout:
        assert bool(torch.isnan(dzout).all()), "mode 1 writes no dzout"


@pytest.mark.parametrize("case,label", _params("gauss_sample"))
def test_gauss_sample(case, label):
    import test_param_kernels as PK
    import test_pointwise_kernels as PW
    H = _H()
    _, B, Hh, Ww, Ch, hoff, oextra, site, key, has_z1, vec, plan = N.DRAW[case["name"]]
    run = case["build"](label, H)
    d = run["d"]
    _, hz = PW.view(B, Hh, Ww, 2 * Ch, hoff, (4 - hoff) % 4, d["hz"])
    ob = torch.full((B, Hh, Ww, 2 * Ch + oextra), float("nan"), device=DEV)
    out = ob[..., :2 * Ch]
    z1 = d["z1"].to(DEV) if has_z1 else None
    eps = d["eps"].to(DEV)
    lp = d["lp0"].to(DEV)
    assert PK.draw_plan(B, Hh * Ww, Ch, hz, out, None, z1)[0] == vec
    H.gauss_sample(hz, eps, z1, out, lp, d["clip"], d["lim"])
    _settle(case, label, run, {"out": out[..., Ch:], "logp": lp}, [])
    if has_z1:
        assert torch.equal(out[..., :Ch].cpu(), d["z1"])
    else:
        assert bool(torch.isnan(out[..., :Ch]).all())


@pytest.mark.parametrize("case,label", _params("adam"))
def test_adam(case, label):
    import test_param_kernels as PK
    H = _H()
    run = case["build"](label, H)
    d = run["d"]
    sizes, gap = N.ADAM_SIZES, 3
    offs, tot = [], gap
    for n in sizes:
        offs.append(tot)
        tot += n + gap
    live = torch.zeros(tot, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        live[o:o + n] = True
    dev = {}
    for k in PK.KINDS:
        h = torch.full((tot,), float("nan"))
        h[live] = d["vals"][k]
        dev[k] = h.to(DEV)
    tab = torch.tensor([[dev[k].data_ptr() + 4 * o for k in PK.KINDS] for o in offs], dtype=torch.int64).to(DEV)
    chunks = PK.adam_chunks(sizes)
    H.adam_step(tab, torch.tensor(chunks, dtype=torch.int32).to(DEV), len(chunks), PK.LR, PK.B1, PK.B2, PK.AEPS, d["wd"], d["bc1"], d["bc2s"],
                d["ams"])
    torch.cuda.synchronize()
    got = {k: dev[k].cpu() for k in PK.KINDS}
    for k in PK.KINDS:
        assert bool(torch.isnan(got[k][~live]).all()), (k, "a gap was written")
    _settle(case, label, run, {k: got[k][live] for k in PK.KINDS}, [])


@pytest.mark.parametrize("case,label", _params("ensemble"))
def test_ensemble_basic_statistics(case, label):
    """The outputs are allocated by tmg_ops.EnsembleStats itself: rule 3 has nothing to look at here."""
    import test_turbulence_gpu as TG
    run = case["build"](label, _H())
    d = run["d"]
    mv = lambda t: t.to(DEV) if t is not None else None      # noqa: E731
    got = TG._run_stats(mv(d["ys"]), mv(d["u"]), mv(d["mu"]), mv(d["sd"]), d["t_start"], d["nchunks"], True, (TG.DX, TG.DY))
    _settle(case, label, run, got, [])


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole model
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("model"))
def test_whole_model(case, label):
    """One NaN input pixel / one NaN parameter: the reverse loss is NaN, and every parameter gradient that is non-finite in the fp64
    oracle is non-finite here (rule 1; the run goes through LevelCouplingFn and LevelMixFoldFn)."""
    from nn.tmGlow import TMGlow
    run = case["build"](label, _H())
    d = run["d"]
    model = TMGlow(**C.build_kwargs(d["cfg"]))
    model.load_state_dict(d["sd"])
    model.to(DEV).train()
    h_in = [(h.to(DEV), c.to(DEV)) for h, c in d["h_in"]]
    yr, ld, _ = model.reconstruct(d["x"].to(DEV), h_in, [e.to(DEV) if e is not None else None for e in d["eps"]])
    loss = C.loss_reverse(yr, ld)
    loss.backward()
    got = {"loss": loss.detach().reshape(1)}
    for k, p in model.named_parameters():
        if "grad " + k in run["R"]:
            assert p.grad is not None, k
            got["grad " + k] = p.grad
    assert set(got) == set(run["R"])
    assert bool(torch.isnan(run["R"]["loss"]).all())
    _settle(case, label, run, got, [])


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm chain
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("batchnorm"))
def test_batchnorm_chain(case, label):
    import test_pointwise_kernels as PW
    H = _H()
    Cn, B, Hh, Ww = N.BN[case["name"]]
    n = B * Hh * Ww
    run = case["build"](label, H)
    d = run["d"]
    xb, x = PW.view(B, Hh, Ww, Cn, 3, 5, d["x"])
    gb_, gy = PW.view(B, Hh, Ww, Cn, 4, 4, d["gy"])
    gd, bd = d["gamma"].to(DEV), d["beta"].to(DEV)
    got = {}
    # the fp32 two-pass statistics -> bn_finalize
    sums, sq = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, None, None, None, None, None, sums, sq, 0)
    c0, c1 = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, None, sums, None, None, None, c0, c1, 0, divisor=n)
    out32 = torch.full((7, Cn), float("nan"), device=DEV)
    rm, rv = d["rm0"].to(DEV), d["rv0"].to(DEV)
    H.bn_finalize(sums, c1, gd, bd, rm, rv, out32[1:6], n, PW.EPS, PW.MOM)
    got.update({k + "32": out32[1 + i] for i, k in enumerate(N.BN_ROWS)})
    got.update(running_mean32=rm, running_var32=rv)
    # the fp64 one-pass moments -> bn_finalize64
    acc = torch.zeros(2 * Cn, dtype=torch.float64, device=DEV)
    H.chan_moments(x, acc)
    out = torch.full((7, Cn), float("nan"), device=DEV)
    rm, rv = d["rm0"].to(DEV), d["rv0"].to(DEV)
    H.bn_finalize64(acc, gd, bd, rm, rv, out[1:6], n, PW.EPS, PW.MOM, counter=torch.tensor(41, dtype=torch.int64, device=DEV))
    got.update({k: out[1 + i] for i, k in enumerate(N.BN_ROWS)})
    got.update(running_mean=rm, running_var=rv)
    # chan_reduce mode 1 and bn_bwd_apply
    o = out[1:6]
    m0, m1 = torch.zeros(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    H.chan_reduce(x, gy, o[3], o[4], o[0], o[2], m0, m1, 1)
    db, dx = PW.view(B, Hh, Ww, Cn, 2, 3, None)
    H.bn_bwd_apply(x, gy, o[3], o[4], o[0], o[2], gd, m0, m1, dx, 0, divisor=n)
    got.update(dbeta=m0, dgamma=m1, dx=dx)
    _settle(case, label, run, got, [])
    assert PW.intact(db, 2, Cn) and PW.intact(gb_, 4, Cn)
    assert bool(torch.isnan(out32[0]).all() and torch.isnan(out32[6]).all() and torch.isnan(out[0]).all() and torch.isnan(out[6]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# physics loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("phys_fwd"))
def test_phys_fwd(case, label):
    import test_phys_kernels as PH
    run = case["build"](label, _H())
    sums, ps, us = PH.run_fwd(run["d"]["y"], run["d"]["t"])         # asserts the guards of its three outputs itself
    _settle(case, label, run, {"us": us, "ps": ps}, [])
    # the sums are global: each is non-finite when the reference's is
    for got, ref in zip(sums.tolist(), run["sums"]):
        assert math.isfinite(ref) or not math.isfinite(got), (label, sums, run["sums"])


@pytest.mark.parametrize("case,label", _params("phys_rms"))
def test_phys_rms(case, label):
    import test_phys_kernels as PH
    run = case["build"](label, _H())
    m, c, s = PH.run_rms(run["d"]["y"], run["d"]["trms"], True)
    _settle(case, label, run, {"mean": m, "coef": c}, [])
    assert not math.isfinite(s), "the sum of squared rms errors is global"


# ---------------------------------------------------------------------------------------------------------------------------------
# growth-layer forwards
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("thin"))
def test_growth_layer_forward(case, label):
    import thin_cases as T
    import test_thin_kernels as TK
    H = _H()
    two = "c1x2_fwd" in case["entry"]
    tc = (T.C1X2_BY_NAME if two else T.C1_BY_NAME)[case["name"]]
    run = case["build"](label, H)
    d = run["d"]
    B, (Hh, Ww) = tc["B"], tc["hw"]
    ins = TK._segments(d["x"], tc["ins"])
    if two:
        w1, w2 = d["w1"].float().to(DEV).contiguous(), d["w2"].float().to(DEV).contiguous()
        a1 = TK._in(d["add1"], T.seg(1, 2, 0)) if d["add1"] is not None else None
        a2 = TK._in(d["add2"], T.seg(1, 2, 1)) if d["add2"] is not None else None
        out = TK.Buf((B, Hh, Ww, 4), width=8).arm()
        w_rows, split, gap, d1row, _ = T._w_params(tc)
        kw = dict(w_rows=w_rows, w2_d1_row=d1row, add1=a1, add2=a2, w_split=split, w_gap=gap, relu_in="relu_in" in tc["sw"])
        TK._same_plan(H.c1x2_fwd_plan(ins, out.view, **kw), T.c1x2_plan(H, tc))
        H.c1x2_fwd(ins, w1, w2, out.view, **kw)
    else:
        assert not ({"inplace", "fill4"} & tc["sw"])
        ad = TK._in(d["add"], T.seg(1, 2, 1)) if d["add"] is not None else None
        out = TK.Buf((B, Hh, Ww, 1), width=4).arm()
        _, split, gap, _, _ = T._c1_params(tc)
        kw = dict(w_rows=tc["w_rows"], fill4=False, add=ad, w_split=split, w_gap=gap, relu_in="relu_in" in tc["sw"])
        TK._same_plan(H.c1_fwd_plan(ins, out.view, **kw), T.c1_plan(H, tc))
        H.c1_fwd(ins, d["w1"].float().to(DEV).contiguous(), out.view, **kw)
    _settle(case, label, run, {"out": out.view}, [])
    assert out.intact(), "%s: wrote outside its output view" % case["name"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the autograd nodes, forward and backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("node"))
def test_node(case, label):
    import test_nodes_fp64 as TN
    run = case["build"](label, _H())
    d, kind = run["d"], run["kind"]
    if kind == "coupling":
        got, _ = TN._run_coupling(d)
    elif kind == "cell":
        got, _ = TN._run_cell(d)
    elif kind == "dense":
        got, _ = TN._run_dense(d)
    elif kind == "mix":
        got = TN._run_mix(d)
    else:
        got = TN._run_conv(d)
    assert set(run["R"]) <= set(got), sorted(set(run["R"]) - set(got))
    _settle(case, label, run, got, [])


# ---------------------------------------------------------------------------------------------------------------------------------
# fused coupling kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("coupling_fwd"))
def test_coupling_fwd(case, label):
    import test_coupling_kernels as CK
    C_, reverse, B, Hh, Ww, layout, mix = N.CPL_FWD[case["name"]]
    run = case["build"](label, _H())
    dv = CK._to_dev(run["d"])
    ch = C_ // 2
    xb = CK.Buf((B, Hh, Ww, C_), layout, dv["x"])
    ob = CK.Buf((B, Hh, Ww, C_), layout)
    rsave = torch.full((B, Hh, Ww, ch), float("nan"), device=DEV)
    y2save = torch.full((B, Hh, Ww, ch), float("nan"), device=DEV)
    logdet = dv["ld0"].clone()
    assert CK.launch_cpl_fwd(dv, xb.arg, ob.arg, rsave, y2save, logdet, reverse, mix, "bind")
    _settle(case, label, run, {"out": ob.value(), "r": rsave, "y2": y2save, "logdet": logdet}, [])
    assert xb.outside_intact() and ob.outside_intact() and CK._stash_intact(dv["Hc"], C_), "wrote outside a channel-slice view"


@pytest.mark.parametrize("case,label", _params("coupling_bwd"))
def test_coupling_bwd(case, label):
    import test_coupling_kernels as CK
    if case["name"] in N.CPL_BWD_SUM:
        return _coupling_bwd_summed(case, label)
    C_, dens, B, Hh, Ww, layout, with_g = N.CPL_BWD[case["name"]]
    run = case["build"](label, _H())
    dv, fw = CK._to_dev(run["d"]), run["fw"]
    ch = C_ // 2
    db = CK.Buf((B, Hh, Ww, C_), layout, dv["dout"])
    src = dv["x"].clone()
    if dens:
        src[..., ch:] = fw["y2"].float().to(DEV)
    xb = CK.Buf((B, Hh, Ww, C_), layout, src)
    r = fw["r"].float().to(DEV).contiguous()
    DHb, DH = CK._stash(B, Hh, Ww, C_)
    tb = CK.Buf((B, Hh, Ww, C_), layout)
    G0 = torch.full((B, Hh, Ww, ch), float("nan"), device=DEV)
    GD = torch.full((B, Hh, Ww, 4), float("nan"), device=DEV)
    assert CK.launch_cpl_bwd(dv, db.arg, xb.half(1), r, dv["g"] if with_g else None, DH, tb.arg, G0, GD, dens, "bind")
    _settle(case, label, run, dict(dtin=tb.value(), DH=DH, G0=G0, GD=GD), [])
    assert db.outside_intact() and xb.outside_intact() and tb.outside_intact() and CK._stash_intact(DHb, C_), "wrote outside a view"


@pytest.mark.parametrize("case,label", _params("dense2_bwd"))
def test_dense2_bwd(case, label):
    import test_coupling_kernels as CK
    H = _H()
    if case["name"] in N.D2_GENERAL:
        return _dense2_general(case, label)
    ch, B, Hh, Ww, dd_quad = N.D2_LEAN[case["name"]]
    run = case["build"](label, H)
    inp, cc = run["d"], CK.CC
    CK.d2_plan(B, Hh, Ww, ch + 4, ch, True, False)
    tin = torch.full((B, Hh, Ww, 2 * ch), float("nan"), device=DEV)
    tin[..., :ch] = inp["x1"].to(DEV)
    x1 = tin[..., :ch]
    D, GD = inp["D"].to(DEV), inp["GD"].to(DEV)
    G0 = inp["G0"][..., :ch].contiguous().to(DEV)
    dtin = torch.full((B, Hh, Ww, 2 * ch), float("nan"), device=DEV)
    dt1 = dtin[..., :ch]
    NLp = 4
    DD = torch.full((B, Hh, Ww, 2 * NLp), float("nan"), device=DEV)
    k = NLp - 2 if dd_quad else 1
    H.dense2_bwd([x1, D], inp["w1"].to(DEV), inp["w2"].to(DEV), None, None, GD, D, [G0], [dt1], ch, add0=inp["add0"].to(DEV), rows1=ch,
                 rows2=ch + 1, split2=ch, gap2=cc, dd1=DD[..., 2 * k:2 * k + 1], dd2=DD[..., 2 * k + 1:2 * k + 2], dd_quad=dd_quad)
    _settle(case, label, run, {"out": dt1, "dd1": DD[..., 2 * k:2 * k + 1], "dd2": DD[..., 2 * k + 1:2 * k + 2]}, [])
    assert bool(torch.isnan(dtin[..., ch:]).all()), "wrote past the output view"
    assert bool(torch.isnan(DD[..., :2 * k]).all()) and (dd_quad or bool(torch.isnan(DD[..., 2 * k + 2:]).all())), "wrote outside the dd pair"


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise coupling pieces
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("affine_apply"))
def test_affine_apply(case, label):
    import test_pointwise_kernels as PW
    H = _H()
    name, B, Hh, Ww, Ch, rev, pas, rs, xlay, (hoff, hextra), expect, capped = N.AFF_F[case["name"]]
    run = case["build"](label, H)
    d = run["d"]
    hb, hh = PW.view(B, Hh, Ww, 2 * Ch, hoff, hextra, d["hh"])
    x1, x2, y1, y2, guards = PW._xy_layout(B, Hh, Ww, Ch, xlay, d["x"], pas)
    rsave = torch.full((B, Hh, Ww, Ch), float("nan"), device=DEV) if rs else None
    ld = d["ld0"].to(DEV)
    assert PW.aff_fwd_plan(hh, x2, y2, rsave, x1 if pas else None, y1 if pas else None, Ch, Hh * Ww)[0] == expect
    H.affine_apply(hh, x2, y2, rsave, ld, rev, x1=x1 if pas else None, y1=y1 if pas else None)
    _settle(case, label, run, {"y2": y2, "ld": ld}, [])
    assert all(PW.intact(base, off, n) for base, off, n in guards) and (pas or bool(torch.isnan(y1).all()))


@pytest.mark.parametrize("case,label", _params("affine_bwd"))
def test_affine_bwd(case, label):
    import test_pointwise_kernels as PW
    H = _H()
    name, B, Hh, Ww, Ch, rev, has_g, kappa, (doff, dextra), pair, capped = N.AFF_B[case["name"]]
    run = case["build"](label, H)
    d = run["d"]
    dy, yb = d["dy"].to(DEV), d["y"].to(DEV)
    dx = torch.full((B, Hh, Ww, 2 * Ch), float("nan"), device=DEV)
    db, dhh = PW.view(B, Hh, Ww, 2 * Ch, doff, dextra)
    kd = torch.tensor([d["kappa"]], device=DEV) if d["kappa"] is not None else None
    H.affine_bwd(dy[..., Ch:], yb[..., Ch:], d["r"].to(DEV), d["g"].to(DEV) if has_g else None, dx[..., Ch:], dhh, rev, kappa=kd)
    _settle(case, label, run, {"gin": dx[..., Ch:], "dhh": dhh}, [])
    assert bool(torch.isnan(dx[..., :Ch]).all()) and PW.intact(db, doff, 2 * Ch)


@pytest.mark.parametrize("case,label", _params("masked_add"))
def test_masked_add(case, label):
    import test_pointwise_kernels as PW
    H = _H()
    name, B, Hh, Ww, n, (off, extra), vec, capped = N.MADD[case["name"]]
    run = case["build"](label, H)
    d = run["d"]
    _, src = PW.view(B, Hh, Ww, n, off, extra, d["src"])
    _, ref = PW.view(B, Hh, Ww, n, off, extra, d["ref"])
    _, add = PW.view(B, Hh, Ww, n, off, extra, d["add"])
    db, dst = PW.view(B, Hh, Ww, n, off, extra, d["dst"])
    H.masked_add(dst, src=src, ref=ref, add=add, accumulate=True)
    _settle(case, label, run, {"dst": dst}, [])
    assert PW.intact(db, off, n)


@pytest.mark.parametrize("case,label", _params("phys_fields"))
def test_phys_fields(case, label):
    import test_phys_kernels as PH
    run = case["build"](label, _H())
    d = run["d"]
    us, ps = PH.run_fields(d["u"], d["p"], d["k1"], d["k2"], d["scale"])       # asserts the guards of both outputs itself
    _settle(case, label, run, {"us": us, "ps": ps}, [])


# ---------------------------------------------------------------------------------------------------------------------------------
# thin grouped weight gradient, c1_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label", _params("thin_wgrad"))
def test_thin_wgrad(case, label):
    import thin_cases as T
    import test_thin_kernels as TK
    H = _H()
    tc = T.THIN_BY_NAME[case["name"]]
    G, dyc, cin = tc["G"], tc["dyc"], tc["cin"]
    run = case["build"](label, H)
    d = run["d"]
    groups = []
    for g in range(G):
        specs = [T.seg(n, 2 * n if (g == 0 and i == 0) else (n + 3) // 4 * 4, 0) for i, n in enumerate(tc["segs"])]
        groups.append(TK._segments(d["x"][g], specs))
    dy = TK._in(d["dy"], (dyc * G, tc["dy_width"], tc["dy_off"], tc["dy_mis"]))
    dW = TK.Buf((1, G * 4 * cin * 9), data=d["prev"] if d["prev"] is not None else torch.zeros(G * 4 * cin * 9)).arm()
    TK._same_plan(H.conv_wgrad_thin_grouped_plan(tc["shape"], tc["segs"], G, dy.data_ptr(), dy.stride(2), dyc, relu_in="relu_in" in tc["sw"]),
                  T.thin_plan(H, tc))
    assert H.conv_wgrad_thin_grouped(groups, dy, dyc, dW.view.view(G, 4, cin, 3, 3), relu_in="relu_in" in tc["sw"]) == 0
    _settle(case, label, run, {"dW": dW.view.view(G, 4, cin, 3, 3)}, [])
    assert dW.intact()


@pytest.mark.parametrize("case,label", _params("c1_bwd"))
def test_c1_bwd(case, label):
    H = _H()
    B, Hh, Ww, segs = N.C1_BWD[case["name"]]
    run = case["build"](label, H)
    d = run["d"]
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)      # noqa: E731
    cin = sum(segs)
    xd = [nhwc(t) for t in d["xs"]]
    wd = d["w"].to(DEV).reshape(cin, 9).contiguous()
    dW = torch.zeros(cin, 9, device=DEV)
    gs = [torch.zeros_like(t) for t in xd]
    H.c1_bwd(xd, wd, dW, nhwc(d["dd"]), nhwc(d["dref"]), gs, relu_in=True)
    got = {"dW": dW.reshape(1, cin, 3, 3), "gin": torch.cat([t.detach().cpu().permute(0, 3, 1, 2) for t in gs], 1)}
    _settle(case, label, run, got, [])


@pytest.mark.parametrize("case,label", _params("phys_bwd"))
def test_phys_bwd(case, label):
    import test_phys_kernels as PH
    run = case["build"](label, _H())
    d = run["d"]
    got = PH.run_bwd(d["y"], d["t"], d["mean"], d["coef"], d["T"], d["co"], None)       # asserts the guards of its output itself
    _settle(case, label, run, {"dy": got}, [])


def _dense2_general(case, label):
    import test_coupling_kernels as CK
    H = _H()
    ch, B, Hh, Ww, with_wg = N.D2_GENERAL[case["name"]]
    run = case["build"](label, H)
    cc = CK.CC
    cin = ch + cc
    p = CK.d2_plan(B, Hh, Ww, cin + 4, ch, False, with_wg)
    dv = {k: v.to(DEV) for k, v in run["d"].items()}
    o1 = torch.full((B, Hh, Ww, ch), float("nan"), device=DEV)
    o2 = torch.full((B, Hh, Ww, cc), float("nan"), device=DEV)
    g0 = [dv["G0"][..., :ch].contiguous(), dv["G0"][..., ch:].contiguous()]
    DD = torch.full((B, Hh, Ww, 4), float("nan"), device=DEV)
    dW1, dW2 = dv["dW1"].clone(), dv["dW2"].clone()
    H.dense2_bwd([dv["x1"], dv["cond"], dv["D"]], dv["w1"], dv["w2"], dW1, dW2, dv["GD"], dv["D"], g0, [o1, o2], cin, add0=dv["add0"],
                 rows1=cin, rows2=cin + 1, dd1=DD[..., 1:2], dd2=DD[..., 2:3])
    _settle(case, label, run, {"out0": o1, "out1": o2, "dd1": DD[..., 1:2], "dd2": DD[..., 2:3], "dW1": dW1, "dW2": dW2}, [])
    assert bool(torch.isnan(DD[..., 0]).all()) and bool(torch.isnan(DD[..., 3]).all()), "wrote outside the dd pair"


def _coupling_bwd_summed(case, label):
    import test_coupling_kernels as CK
    import test_coupling_presum as CP
    C_, dens, B, Hh, Ww, layout, with_g = N.CPL_BWD_SUM[case["name"]]
    run = case["build"](label, _H())
    dv, fw = CK._to_dev(run["d"]), run["fw"]
    ch = C_ // 2
    db = CK.Buf((B, Hh, Ww, C_), layout, dv["dout"])
    src = dv["x"].clone()
    if dens:
        src[..., ch:] = fw["y2"].float().to(DEV)
    xb = CK.Buf((B, Hh, Ww, C_), layout, src)
    got = CP._launch(dv, db, xb, fw["r"].float().to(DEV).contiguous(), dv["g"] if with_g else None, layout, dens, summed=True)
    gt = got["tb"].value()
    _settle(case, label, run, {"sum1": gt[..., :ch], "dtin2": gt[..., ch:], "DH": got["DH"], "GD01": got["GD"][..., :2]}, [])
    assert db.outside_intact() and xb.outside_intact() and got["tb"].outside_intact() and CK._stash_intact(got["DHb"], C_)
    # the packed mask: bit c is set unless x1_c <= 0, so a NaN x1 sets it and dense2_bwd(g0_masked) passes the gradient there
    x1 = dv["x"][..., :ch]
    word = ((~(x1 <= 0)).to(torch.int32) << torch.arange(ch, device=DEV, dtype=torch.int32)).sum(3).to(torch.int32)
    gdi = got["GD"].view(torch.int32)
    assert torch.equal(gdi[..., 2], word), "GD channel 2 is not the mask word of x1"
    assert bool((gdi[..., 3] == 0).all()), "GD channel 3 must be zero"
