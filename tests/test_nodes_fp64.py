"""The hand-written autograd nodes of tmg_ops.py (LevelCouplingFn / LevelMixFoldFn excepted) and the module code that feeds them, each
against plain fp64 torch autograd of the same operation (node_cases.py: the oracle's coupling / lstm_coupling, nn.BatchNorm2d + conv2d,
einsum), on every branch the node or the module takes.  Every output, the gradient of every input and of every parameter is compared
in full: inputs are chosen (node_cases.py, the seed rule) so that no ReLU the node computes sits within 1e-4 of its kink, and nothing is
masked or left out.

Coverage map (node -> branch -> case; shapes are (B, H, W, ...)):
  CouplingTailFn mode 0, AffineCouplingLayer.run      test_coupling_layer: c8 (2,9,7,C 8,Cc 4), c64 (2,8,12,64,32), c16_1x1 (2,1,1,16,8:
      ring and corners of the replicate adjoint fold onto the pixel), c12_odd (1,5,6,12,5: no segment a multiple of 4), each forward and
      reverse.  test_coupling_layer_variants on c8 / c64: clamp (scale > ln 4: d scale exactly 0), no_ld (dld absent), slice (x a channel
      slice of a NaN-filled wider buffer), nchw (x the NHWC view of an NCHW tensor: the node's own .contiguous()), gy_noncontig.
      test_coupling_tail_apply_directly: CouplingTailFn.apply itself.
  LSTMAffineCouplingLayer.run (CouplingTailFn mode 1, LeadingChannelsFn join, ConvLSTMCellFn, out conv with _grad_premasked)
      test_lstm_coupling_layer: l8 (2,9,7,C 8,Cc 4,R 4), l16_r64 (2,8,8,16,32,64: 40 input channels, the cell's split weight gradient),
      l12_pad2 (2,6,10,12,4,4 with pad 2 through PadHalvesFn: padded weights built per call, padding channels of y exactly 0, gradients
      on the un-padded parameters), each forward / reverse x state None / given; test_lstm_coupling_layer_y_only (dh, dc None).
      test_lstm_window: two steps inside bptt_window, win.backward: gradients summed over both steps through the sink and, padded,
      through the DerivedCache proxies built ONCE.
  ConvLSTMCellFn   test_cell_node: r4 (2,9,7,[4,4],R 4), r64 (1,8,8,[8,32],64) x c_none, h_only (dc None), c_only (dh None),
      first_seg_only (only the first segment needs a gradient); test_cell_second_backward_raises;
      test_gradient_slots_the_nodes_promise_none (the backward passes called on the nodes' contexts: cell, MixFn, ConvFn).
  DenseBlockFn through DenseBlock.run    test_dense_block: d6 (2,9,7,c0 6,g 3,L 3), d16 (3,10,10,16,4,4), d8_row (2,1,5,8,4,2) x train /
      eval (running statistics non-default, untouched), d6 with track_running_stats=False; running_mean / running_var (unbiased) /
      num_batches_tracked.  test_dense_block_variants on d6: slice, gy_noncontig (caller's gradient unchanged), layers
      (TMG_NO_DENSE_BLOCK_NODE: the per-layer path against the SAME fp64 reference); test_dense_block_no_grad_path (the no-grad path
      against fp64 and against the node's output); test_dense_second_backward_raises.
  BNReLUConvFn through _DenseLayer.grow  test_dense_layer_grow: layer12 (2,9,7,12,4,1) train and eval.
  MixFn   test_mix_node: widths 16, 6, 64 (tmg_hip.mix_f32 takes 16 and 64, declines 6: asked of the function itself) x 2x9x7, 1x1x1 x
      bias given / None; test_mix_node_strided_input; test_mix_node_f16 (C 16, fp16 operand bound, weight gradient at the fp32 bound).
  ConvFn  test_conv_stride2_odd: (2,9,7,[8],16) and (1,5,5,[5],9), k 3 stride 2 (conv_dgrad_direct); test_conv_sliced_upstream_gradient:
      a pixel-linear channel slice (addressed in place) and a slice that is not (copied); test_conv_with_four_segments_is_refused_loudly:
      a shape the node accepts and the launcher declines (four input segments) is tmg_hip._chk's RuntimeError, not numbers.

Error measure: err(a, ref) = max|a - ref| / max(1, max|ref|), NaN infinite (test_hip_ops._close); log-dets image by image against
max(1, sum_image |sg|) (test_coupling_kernels.py).  u = 2^-24.

Bounds.  None is chosen here: each is the sum, along the node's path, of what the kernel-level tests allow the kernels on it.
  A convolution stage (conv_fwd, conv3x3_auto / Winograd, c1_fwd, conv_wgrad, the input-gradient convs, conv_dgrad_direct): the kernel
    tests (test_conv_kernels.py, test_wino_kernels.py, test_thin_kernels.py) allow |a_i - ref_i| <= (K + 8) u S_i (K + 4, K + 3 in the
    thin / mix files), S_i the fp64 sum of |terms| of element i, K the length of its sum (9 Cin forward, 9 Cout input gradient,
    B Hout Wout weight gradient).  In the measure above: stage(K, rho) = (K + 8) u rho, rho = max_i S_i / max(1, max|result|), computed
    in fp64 by node_cases.Rec for every stage's result, input gradient and weight gradient of the very case.
  Pointwise kernels (test_pointwise_kernels.py): TOL_AFF = 10.2 u, TOL_AFFB = 20.4 u, TOL_LSTM_H = 32.6 u, TOL_LSTM_B = 51.9 u,
    BatchNorm's folded affine 12 u, bn_bwd_apply (12 + sqrt n) u, chan_reduce (8 + sqrt n) u, running statistics 9 u + 2 u, dkappa
    (1 + sqrt K) u; dense2_bwd: TOL_D2 = 1e-5 (test_coupling_kernels.py).
  forward (y, h', c', block output) = sum of the stages' forward terms [x 2 for a node that ends in the affine: |dy2 / dr| <= 2 |y2|,
    as TOL_OUT's derivation] + the pointwise terms on the path (TOL_AFF; TOL_LSTM_H; 12 u per BatchNorm).
  log-det = (2 + sqrt N) u [pointwise TOL_LD(N)] + 2 x forward x max|hh| x sqrt(N) / sum_image |sg|, N = values of sg per image: every sg
    carries twice the zero conv's error (|dsg / dr| <= 2), N independent errors add like sqrt(N) (the kernel files' sum model).
  backward (every input and parameter gradient) = forward (the activations the gradients are evaluated at) + the stages' input- and
    weight-gradient terms + TOL_AFFB + TOL_D2 + dkappa (coupling tail), + TOL_LSTM_B (cell), + per BatchNorm layer bn_bwd_apply +
    chan_reduce.  Running statistics of layer i: 11 u + 2 x the forward terms of the layers before it.
  MixFn under f16: (2 x 2^-11 + (C + 3) u) rho for output and input gradient (two fp16 operand roundings per product, fp32 sums: the
    model of test_hip_ops.test_mix_f16_kernel); weight gradient at the fp32 bound (the code keeps it fp32).
Typical values: 7e-5 (c8 forward) .. 2e-3 (l16_r64 backward: K = 936); mutations of the reference (test_node_cases_cpu.py) move an
output to >= 80x its bound.

Measured on an MI355X, 86 tests in 4 s, the longest 1.0 s (the first launch); largest err / bound per output kind (case, output, err):
  coupling layer   forward 0.004 (c8 clamp, y, 2.6e-7), log-det 0.0008 (c8 rev0, 1.9e-8), gradient 0.007 (c8 rev1, d scale, 1.0e-6)
  LSTM coupling    forward 0.003 (l8, c', 4.5e-7), log-det 0.0009 (l8, 7.0e-8), gradient 0.033 (l8 y_only, d scale, 1.0e-5); two-step window
                   forward 0.001, log-det 0.0001, gradient 0.002 (l8, d zero-conv weight, 1.4e-6)
  ConvLSTM cell    forward 0.029 (r4 c_none, c', 6.0e-7), gradient 0.028 (r4 c_none, db, 1.4e-6)
  dense block      forward 0.008 (d6 eval, 3.0e-7), gradient 0.005 (d8_row train, d gamma, 1.8e-7), running statistics 0.13 (d8_row,
                   running_var of layer 1, 8.5e-8 of a 6.6e-7 bound); _DenseLayer.grow forward 0.021, gradient 0.005, statistics 0.064
  MixFn            forward 0.11 (C 6, 6.5e-8), gradient 0.097 (C 6 at 1x1x1, dW, 5.2e-8); f16: forward 0.27 (4.3e-4), input gradient 0.25
  ConvFn           forward 0.024 (s1_slice, 2.7e-7), gradient 0.007 (dx, 3.8e-7)
No output needs more than its bound: the conv stages' worst-case K u terms leave one to two orders above the measured errors, as in the
kernel files.  c12_odd (no segment a multiple of 4) is computed, not declined, and meets the same bounds."""
import os

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import node_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _back(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


class Judge:
    """Collects err / bound of every checked output of one test, prints each figure, and fails at the end with all of them."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def add(self, kind, name, e, tol):
        share = e / tol
        print("NODESHARE %-12s %-40s %-44s err %.3e bound %.3e share %.4f" % (kind, self.what, name, e, tol, share))
        if not share <= 1.0:
            self.bad.append("%s: err %.3e > bound %.3e" % (name, e, tol))

    def check(self, d, name, got, ref=None, tol=None, kind=None):
        assert got is not None, "%s: %s is None" % (self.what, name)
        e = N.out_err(d, name, got, ref)
        kind = kind or ("logdet" if name == "ld" else "forward" if name in ("y", "y1", "h", "c", "out") else
                        "statistics" if name.startswith("stat:") else "gradient")
        self.add(kind, name, e, N.tol_of(d, name) if tol is None else tol)

    def done(self):
        assert not self.bad, "%s: %s" % (self.what, "; ".join(self.bad))


def _param_grads(mod):
    return {"d:" + k: p.grad for k, p in mod.named_parameters()}


def _check_all(j, d, got):
    """Every output of the reference has a counterpart, and nothing else was produced."""
    assert set(got) == set(d.ref), sorted(set(got) ^ set(d.ref))
    for k, r in d.ref.items():
        if r is None:
            assert got[k] is None, k
        elif not r.is_floating_point():
            assert int(got[k]) == int(r), (k, int(got[k]), int(r))
        else:
            j.check(d, k, got[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. CouplingTailFn mode 0
# ---------------------------------------------------------------------------------------------------------------------------------
def _coupling_layer(d):
    from nn.modules.flowAffine import AffineCouplingLayer
    lay = AffineCouplingLayer(d.shape[3], d.shape[4])
    lay.load_state_dict(d.sd)
    return lay.to(DEV)


def _run_coupling(d, variant=None, direct=False):
    import tmg_ops as ops
    B, Hh, Ww, C_, Cc = d.shape
    lay = _coupling_layer(d)
    condn = _nhwc(d.t["cond"]).requires_grad_(True)
    wide = None
    if variant == "slice":
        wide = torch.full((B, Hh, Ww, C_ + 8), NAN, device=DEV)
        wide[..., 4:4 + C_] = _nhwc(d.t["x"])
        wide.requires_grad_(True)
        xn = wide[..., 4:4 + C_]
    elif variant == "nchw":
        xl = d.t["x"].to(DEV).contiguous().requires_grad_(True)
        xn = xl.permute(0, 2, 3, 1)
        assert xn.stride(3) != 1
    else:
        xl = _nhwc(d.t["x"]).requires_grad_(True)
        xn = xl
    if direct:
        db, zc = lay.coupling_nn.dense_block, lay.coupling_nn.zero_conv
        y, ld = ops.CouplingTailFn.apply(xn, condn, db.denselayer1.conv1.weight, db.denselayer2.conv1.weight, zc.conv.weight, zc.conv.bias,
                                         zc.scale, d.reverse, 0)
    else:
        y, ld = lay.run(xn, condn, d.reverse)
    if variant == "gy_noncontig":
        gy = d.t["gy"].to(DEV).contiguous().permute(0, 2, 3, 1)
        assert not gy.is_contiguous()
    else:
        gy = _nhwc(d.t["gy"])
    if d.use_ld:
        torch.autograd.backward([y, ld], [gy, d.t["gl"].to(DEV)])
    else:
        torch.autograd.backward([y], [gy])
    if wide is not None:
        g = wide.grad
        assert bool((g[..., :4] == 0).all()) and bool((g[..., 4 + C_:] == 0).all()), "gradient outside the slice"
        dx = _back(g[..., 4:4 + C_])
    else:
        dx = xl.grad.detach().cpu() if variant == "nchw" else _back(xl.grad)
    got = {"y": _back(y), "ld": ld, "dx": dx, "dcond": _back(condn.grad)}
    got.update(_param_grads(lay))
    return got, lay


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(N.COUPLING_SHAPES))
def test_coupling_layer(name, reverse):
    d = N.coupling_data(name, reverse)
    j = Judge("coupling %s rev%d" % (name, reverse))
    got, _ = _run_coupling(d)
    _check_all(j, d, got)
    j.done()


@pytest.mark.parametrize("variant", N.COUPLING_VARIANTS)
@pytest.mark.parametrize("name", ["c8", "c64"])
def test_coupling_layer_variants(name, variant):
    d = N.coupling_data(name, True, variant == "clamp", variant != "no_ld")
    j = Judge("coupling %s %s" % (name, variant))
    got, lay = _run_coupling(d, variant)
    _check_all(j, d, got)
    if variant == "clamp":
        g = lay.coupling_nn.zero_conv.scale.grad
        assert bool((g == 0).all()), "the clamp binds: d scale must be exactly 0, got %r" % g.flatten().tolist()
    j.done()


def test_coupling_tail_apply_directly():
    d = N.coupling_data("c8", False)
    j = Judge("coupling c8 apply")
    got, _ = _run_coupling(d, direct=True)
    _check_all(j, d, got)
    j.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. LSTMAffineCouplingLayer.run
# ---------------------------------------------------------------------------------------------------------------------------------
def _lstm_layer(d):
    from nn.modules.flowAffine import LSTMAffineCouplingLayer
    lay = LSTMAffineCouplingLayer(d.shape[3], d.shape[4], d.shape[5])
    lay.load_state_dict(d.sd)
    return lay.to(DEV)


def _lstm_step(lay, d, xl, condn, st, j=None):
    """One call of the layer in the layout its level uses: padded through PadHalvesFn when the case says so."""
    import tmg_ops as ops
    C_, pad = d.shape[3], d.shape[6]
    ch = C_ // 2
    xn = ops.PadHalvesFn.apply(xl, ch, pad, True) if pad else xl
    y, ld, (h, c) = lay.run(xn, condn, st, d.reverse, pad=pad)
    if pad:
        assert y.shape[3] == 2 * (ch + pad)
        assert bool((y[..., ch:ch + pad] == 0).all()) and bool((y[..., 2 * ch + pad:] == 0).all()), "padding channels of y are not exactly 0"
        y = ops.PadHalvesFn.apply(y, ch, pad, False)
    return y, ld, h, c


class _CountBuilds:
    """Counts the evaluations of DerivedCache builders (the padded weights) through a wrapper of DerivedCache.get."""

    def __enter__(self):
        import tmg_ops as ops
        self.ops, self.orig, self.n = ops, ops.DerivedCache.get, 0
        me = self

        def get(cache, name, params, extra, build, proxies=False):
            def counted():
                me.n += 1
                return build()
            return me.orig(cache, name, params, extra, counted, proxies=proxies)
        ops.DerivedCache.get = get
        return self

    def __exit__(self, *a):
        self.ops.DerivedCache.get = self.orig
        return False


def _run_lstm(d):
    lay = _lstm_layer(d)
    xl, condn = _nhwc(d.t["x"]).requires_grad_(True), _nhwc(d.t["cond"]).requires_grad_(True)
    st = (_nhwc(d.t["h0"]).requires_grad_(True), _nhwc(d.t["c0"]).requires_grad_(True)) if d.with_state else None
    with _CountBuilds() as cnt:
        y, ld, h, c = _lstm_step(lay, d, xl, condn, st)
    assert cnt.n == (1 if d.shape[6] else 0), "outside a window the padded weights are built per call (%d builds)" % cnt.n
    outs, grads = [y], [_nhwc(d.t["gy"])]
    if d.full_loss:
        outs += [ld, h, c]
        grads += [d.t["gl"].to(DEV), _nhwc(d.t["gh"]), _nhwc(d.t["gc"])]
    torch.autograd.backward(outs, grads)
    got = {"y": _back(y), "ld": ld, "h": _back(h), "c": _back(c), "dx": _back(xl.grad), "dcond": _back(condn.grad)}
    if st is not None:
        got.update(dh0=_back(st[0].grad), dc0=_back(st[1].grad))
    got.update(_param_grads(lay))
    return got


@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", list(N.LSTM_SHAPES))
def test_lstm_coupling_layer(name, reverse, with_state):
    d = N.lstm_data(name, reverse, with_state)
    j = Judge("lstm %s rev%d state%d" % (name, reverse, with_state))
    _check_all(j, d, _run_lstm(d))
    j.done()


@pytest.mark.parametrize("name", list(N.LSTM_SHAPES))
def test_lstm_coupling_layer_y_only(name):
    """The loss uses y alone: dld, dh and dc reach the nodes as None / zeros; every gradient still equals the reference."""
    d = N.lstm_data(name, True, True, False)
    j = Judge("lstm %s y_only" % name)
    _check_all(j, d, _run_lstm(d))
    j.done()


@pytest.mark.parametrize("name", ["l8", "l12_pad2"])
def test_lstm_window(name):
    import tmg_ops as ops
    d = N.window_data(name, True)
    j = Judge("window %s" % name)
    lay = _lstm_layer(d)
    t = d.t
    xs = [_nhwc(t["x"]).requires_grad_(True), _nhwc(t["x2"]).requires_grad_(True)]
    conds = [_nhwc(t["cond"]).requires_grad_(True), _nhwc(t["cond2"]).requires_grad_(True)]
    gl = t["gl"].to(DEV)
    with _CountBuilds() as cnt:
        with ops.bptt_window() as win:
            y1, ld1, h1, c1 = _lstm_step(lay, d, xs[0], conds[0], None)
            y2, ld2, h, c = _lstm_step(lay, d, xs[1], conds[1], (h1, c1))
            loss = (y1 * _nhwc(t["gy"])).sum() + (ld1 * gl).sum() + (y2 * _nhwc(t["gy2"])).sum() + (ld2 * gl).sum() + \
                (h * _nhwc(t["gh"])).sum() + (c * _nhwc(t["gc"])).sum()
            win.backward(loss)
    assert cnt.n == (1 if d.shape[6] else 0), "inside a window the padded weights are built once (%d builds)" % cnt.n
    assert ops.DerivedCache.window_depth == 0 and ops._GradSink.active is None
    got = {"y": _back(y2), "y1": _back(y1), "ld": ld2, "h": _back(h), "c": _back(c), "dx": _back(xs[1].grad), "dx1": _back(xs[0].grad),
           "dcond": _back(conds[1].grad), "dcond1": _back(conds[0].grad)}
    got.update(_param_grads(lay))
    _check_all(j, d, got)
    j.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ConvLSTMCellFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_cell(d, retain=False):
    import tmg_ops as ops
    t, v = d.t, d.variant
    first_only = v == "first_seg_only"
    xd = [x.to(DEV).requires_grad_(i == 0 or not first_only) for i, x in enumerate(t["xs"])]
    hd = t["h0"].to(DEV).requires_grad_(not first_only)
    cd = None if v == "c_none" else t["c0"].to(DEV).requires_grad_(True)
    wd, bd = t["w"].to(DEV).requires_grad_(True), t["b"].to(DEV).requires_grad_(True)
    h2, c2 = ops.ConvLSTMCellFn.apply(wd, bd, hd, cd, *xd)
    outs, grads = [], []
    if v != "c_only":
        outs.append(h2), grads.append(t["gh"].to(DEV))
    if v != "h_only":
        outs.append(c2), grads.append(t["gc"].to(DEV))
    torch.autograd.backward(outs, grads, retain_graph=retain)
    got = {"h": h2.detach(), "c": c2.detach(), "dW": wd.grad, "db": bd.grad, "dx0": xd[0].grad}
    if first_only:
        assert all(x.grad is None for x in xd[1:]) and hd.grad is None
    else:
        got.update({"dx%d" % i: x.grad for i, x in enumerate(xd)})
        got["dh0"] = hd.grad
    if cd is not None:
        got["dc0"] = cd.grad
    return got, (outs, grads)


@pytest.mark.parametrize("variant", N.CELL_VARIANTS)
@pytest.mark.parametrize("name", list(N.CELL_SHAPES))
def test_cell_node(name, variant):
    d = N.cell_data(name, variant)
    j = Judge("cell %s %s" % (name, variant))
    got, _ = _run_cell(d)
    _check_all(j, d, got)
    j.done()


def test_gradient_slots_the_nodes_promise_none():
    """The backward passes called on the nodes' own contexts: the slots of absent or gradient-free inputs are None (autograd itself
    hides them: a tensor that needs no gradient has .grad None whatever the node returns)."""
    import tmg_ops as ops
    with torch.enable_grad():
        d = N.cell_data("r4", "c_none")
        t = d.t
        xd = [x.to(DEV).requires_grad_(True) for x in t["xs"]]
        wd, bd, hd = t["w"].to(DEV).requires_grad_(True), t["b"].to(DEV).requires_grad_(True), t["h0"].to(DEV).requires_grad_(True)
        h2, c2 = ops.ConvLSTMCellFn.apply(wd, bd, hd, None, *xd)
    with torch.no_grad():
        slots = ops.ConvLSTMCellFn.backward(h2.grad_fn, t["gh"].to(DEV), None)         # (dW, db, dh, dc, dx0, dx1)
    assert len(slots) == 6 and slots[3] is None and all(slots[i] is not None for i in (0, 1, 2, 4, 5))
    with torch.enable_grad():
        xd = [x.to(DEV).requires_grad_(i == 0) for i, x in enumerate(t["xs"])]
        h2, c2 = ops.ConvLSTMCellFn.apply(wd, bd, t["h0"].to(DEV), t["c0"].to(DEV).requires_grad_(True), *xd)
    with torch.no_grad():
        slots = ops.ConvLSTMCellFn.backward(h2.grad_fn, None, t["gc"].to(DEV))
    assert slots[2] is None and slots[5] is None and slots[4] is not None and slots[3] is not None
    j = Judge("cell r4 slots")
    j.check(N.cell_data("r4", "c_only"), "dx0", slots[4])
    j.done()
    dm = N.mix_data(16, "9x7", False)
    with torch.enable_grad():
        y = ops.MixFn.apply(dm.t["x"].to(DEV).requires_grad_(True), dm.t["W"].to(DEV).requires_grad_(True), None)
    with torch.no_grad():
        slots = ops.MixFn.backward(y.grad_fn, dm.t["gy"].to(DEV))
    assert len(slots) == 3 and slots[2] is None and slots[0] is not None and slots[1] is not None
    dc = N.conv_data("s2_5x5")
    with torch.enable_grad():
        y = ops.conv([_nhwc(dc.t["xs"][0]).requires_grad_(True)], dc.t["w"].to(DEV).requires_grad_(True), ksize=3, stride=2, relu_in=True)
    with torch.no_grad():
        slots = ops.ConvFn.backward(y.grad_fn, _nhwc(dc.t["gy"]))                       # (dW, db, dkappa, opts, dx)
    assert len(slots) == 5 and slots[1] is None and slots[2] is None and slots[3] is None and slots[0] is not None and slots[4] is not None


def test_cell_second_backward_raises():
    d = N.cell_data("r4", "h_only")
    _, (outs, grads) = _run_cell(d, retain=True)
    with pytest.raises(RuntimeError, match="consumed by a previous backward pass"):
        torch.autograd.backward(outs, grads)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. DenseBlockFn, BNReLUConvFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _dense_block(d):
    from nn.modules.denseBlock import DenseBlock
    B, Hh, Ww, c0, growth, L = d.shape
    blk = DenseBlock(num_layers=L, in_features=c0, growth_rate=growth, drop_rate=0.)
    blk.load_state_dict(d.sd)
    blk.to(DEV).train(d.mode == "train")
    if d.mode == "notrack":
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.track_running_stats = False
    return blk


def _dense_stats(d, blk):
    """Running statistics as the reference reports them (none without tracking); untouched buffers wherever they must not move."""
    out = {}
    sdn = blk.state_dict()
    for k, v in sdn.items():
        if "running" in k or "num_batches" in k:
            if d.mode == "train":
                out[("count:" if "num_batches" in k else "stat:") + k] = v.detach().cpu()
            else:
                assert torch.equal(v.cpu(), d.sd[k]), "%s moved in %s mode" % (k, d.mode)
                if d.mode == "eval":
                    out[("count:" if "num_batches" in k else "stat:") + k] = v.detach().cpu()
    return out


def _run_dense(d, variant=None):
    B, Hh, Ww, c0, growth, L = d.shape
    blk = _dense_block(d)
    if variant == "slice":
        wide = torch.full((B, Hh, Ww, c0 + 6), NAN, device=DEV)
        wide[..., 2:2 + c0] = _nhwc(d.t["x"])
        wide.requires_grad_(True)
        xn = wide[..., 2:2 + c0]
    else:
        wide = None
        xn = _nhwc(d.t["x"]).requires_grad_(True)
    if variant == "layers":
        os.environ["TMG_NO_DENSE_BLOCK_NODE"] = "1"
    try:
        y = blk.run(xn)
        if variant == "gy_noncontig":
            gy = d.t["gy"].to(DEV).contiguous().permute(0, 2, 3, 1)
            assert not gy.is_contiguous()
            keep = gy.clone()
        else:
            gy = _nhwc(d.t["gy"])
        y.backward(gy)
    finally:
        os.environ.pop("TMG_NO_DENSE_BLOCK_NODE", None)
    if variant == "gy_noncontig":
        assert torch.equal(gy, keep), "the node wrote into the caller's gradient tensor"
    if wide is not None:
        g = wide.grad
        assert bool((g[..., :2] == 0).all()) and bool((g[..., 2 + c0:] == 0).all())
        dx = _back(g[..., 2:2 + c0])
    else:
        dx = _back(xn.grad)
    got = {"out": _back(y), "dx": dx}
    got.update(_param_grads(blk))
    got.update(_dense_stats(d, blk))
    return got, y


@pytest.mark.parametrize("name,mode", [(n, m) for n in ("d6", "d16", "d8_row") for m in N.DENSE_MODES if m != "notrack" or n == "d6"])
def test_dense_block(name, mode):
    d = N.dense_data(name, mode)
    j = Judge("dense %s %s" % (name, mode))
    got, _ = _run_dense(d)
    _check_all(j, d, got)
    j.done()


@pytest.mark.parametrize("variant", ["slice", "gy_noncontig", "layers"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_dense_block_variants(mode, variant):
    d = N.dense_data("d6", mode)
    j = Judge("dense d6 %s %s" % (mode, variant))
    got, _ = _run_dense(d, variant)
    _check_all(j, d, got)
    j.done()


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_dense_block_no_grad_path(mode):
    """DenseBlock.run without grad mode (per-layer grow into one buffer) against the fp64 reference and against the node's output."""
    d = N.dense_data("d6", mode)
    j = Judge("dense d6 %s nograd" % mode)
    _, y_node = _run_dense(d)
    blk = _dense_block(d)
    with torch.no_grad():
        y = blk.run(_nhwc(d.t["x"]))
    assert not y.requires_grad
    j.check(d, "out", _back(y))
    j.check(d, "out", _back(y), ref=_back(y_node), kind="forward")
    for k, v in _dense_stats(d, blk).items():
        if k.startswith("stat:"):
            j.check(d, k, v)
        else:
            assert int(v) == int(d.ref[k]), k
    j.done()


def test_dense_second_backward_raises():
    d = N.dense_data("d6", "train")
    blk = _dense_block(d)
    y = blk.run(_nhwc(d.t["x"]).requires_grad_(True))
    gy = _nhwc(d.t["gy"])
    y.backward(gy, retain_graph=True)
    with pytest.raises(RuntimeError, match="a second backward through the same graph is not supported"):
        y.backward(gy)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_dense_layer_grow(mode):
    """BNReLUConvFn through _DenseLayer.grow: the new channels; the reference's dx also carries the pass-through share of gy."""
    d = N.dense_data("layer12", mode)
    j = Judge("layer12 %s" % mode)
    c0 = d.shape[3]
    blk = _dense_block(d)
    xn = _nhwc(d.t["x"]).requires_grad_(True)
    new = blk.denselayer1.grow(xn)
    gy = _nhwc(d.t["gy"])
    new.backward(gy[..., c0:].contiguous())
    got = {"out": torch.cat([d.t["x"], _back(new)], 1), "dx": _back(xn.grad) + d.t["gy"][:, :c0]}
    got.update(_param_grads(blk))
    got.update(_dense_stats(d, blk))
    _check_all(j, d, got)
    j.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. MixFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _mix_takes(width):
    """Whether tmg_hip.mix_f32 takes the width: its own answer on a probe call."""
    import tmg_hip as H
    x = torch.zeros(1, 1, 2, width, device=DEV)
    return bool(H.mix_f32(x, torch.eye(width, device=DEV), None, torch.empty_like(x)))


def _run_mix(d, strided=False):
    import tmg_ops as ops
    t = d.t
    if strided:
        xl = t["x"].permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True)     # NCHW leaf; the node sees its NHWC view
        x = xl.permute(0, 2, 3, 1)
        assert x.stride(3) != 1 or x.shape[1] * x.shape[2] == 1
    else:
        xl = t["x"].to(DEV).requires_grad_(True)
        x = xl
    W = t["W"].to(DEV).requires_grad_(True)
    b = t["b"].to(DEV).requires_grad_(True) if d.with_b else None
    y = ops.MixFn.apply(x, W, b)
    y.backward(t["gy"].to(DEV))
    got = {"y": y.detach(), "dx": xl.grad.permute(0, 2, 3, 1) if strided else xl.grad, "dW": W.grad}
    if d.with_b:
        got["db"] = b.grad
    return got


def _judge_mix(j, d, got, f16=False):
    assert set(got) == set(d.ref)
    for k in d.ref:
        j.check(d, k, got[k], tol=N.mix_tol(d, k, f16), kind=("forward" if k == "y" else "gradient") + (" f16" if f16 and k in ("y", "dx") else ""))


def test_mix_widths_cover_both_paths():
    takes = {w: _mix_takes(w) for w in N.MIX_WIDTHS}
    print("NODEMIX mix_f32 takes", takes)
    assert any(takes.values()) and not all(takes.values()), takes


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("shape", list(N.MIX_SHAPES))
@pytest.mark.parametrize("width", N.MIX_WIDTHS)
def test_mix_node(width, shape, with_b):
    d = N.mix_data(width, shape, with_b)
    j = Judge("mix C%d %s b%d (mix_f32 %s)" % (width, shape, with_b, "takes" if _mix_takes(width) else "declines"))
    _judge_mix(j, d, _run_mix(d))
    j.done()


@pytest.mark.parametrize("width", N.MIX_WIDTHS)
def test_mix_node_strided_input(width):
    d = N.mix_data(width, "9x7", True)
    j = Judge("mix C%d strided" % width)
    _judge_mix(j, d, _run_mix(d, strided=True))
    j.done()


def test_mix_node_f16():
    import tmg_ops as ops
    d = N.mix_data(16, "9x7", True)
    j = Judge("mix C16 f16")
    before = ops.mix_precision()
    ops.set_mix_precision("f16")
    try:
        got = _run_mix(d)
    finally:
        ops.set_mix_precision(before)
    _judge_mix(j, d, got, f16=True)
    j.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. ConvFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_conv(d, gy_view=None):
    import tmg_ops as ops
    B, Hh, Ww, segs, Cout, k, stride, relu_in = d.shape
    xd = [_nhwc(x).requires_grad_(True) for x in d.t["xs"]]
    wd = d.t["w"].to(DEV).requires_grad_(True)
    y = ops.conv(xd, wd, ksize=k, stride=stride, relu_in=relu_in)
    y.backward(_nhwc(d.t["gy"]) if gy_view is None else gy_view)
    got = {"y": _back(y), "dW": wd.grad}
    got.update({"dx%d" % i: _back(x.grad) for i, x in enumerate(xd)})
    return got


@pytest.mark.parametrize("name", ["s2_9x7", "s2_5x5"])
def test_conv_stride2_odd(name):
    d = N.conv_data(name)
    j = Judge("conv %s" % name)
    _check_all(j, d, _run_conv(d))
    j.done()


@pytest.mark.parametrize("linear", [True, False])
def test_conv_sliced_upstream_gradient(linear):
    import tmg_hip as H
    d = N.conv_data("s1_slice")
    j = Judge("conv s1_slice linear%d" % linear)
    gy = _nhwc(d.t["gy"])
    B, Hh, Ww, Cout = gy.shape
    if linear:      # a channel slice of a wider tensor: pixels equally spaced, addressed in place
        wide = torch.full((B, Hh, Ww, Cout + 8), NAN, device=DEV)
        view = wide[..., 4:4 + Cout]
    else:           # a slice in W as well: rows are not equally spaced, the node copies
        wide = torch.full((B, Hh, Ww + 2, Cout + 8), NAN, device=DEV)
        view = wide[:, :, 1:1 + Ww, 4:4 + Cout]
    view.copy_(gy)
    assert H._pixel_linear(view) == linear and not view.is_contiguous()
    _check_all(j, d, _run_conv(d, view))
    assert int(torch.isnan(wide).sum()) == wide.numel() - view.numel(), "the upstream gradient's parent was written"
    j.done()


def test_conv_with_four_segments_is_refused_loudly():
    """tmg_ops.conv takes any list of segments, the kernels three (TMG_MAX_IN_SEG; NoNormDenseBlock.run re-concatenates beyond that):
    the launcher declines with an error code, which must surface as tmg_hip._chk's RuntimeError and never as numbers."""
    import tmg_ops as ops
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(1, 5, 6, 4, generator=g).to(DEV).requires_grad_(True) for _ in range(4)]
    w = (0.2 * torch.randn(8, 16, 3, 3, generator=g)).to(DEV).requires_grad_(True)
    kap = torch.zeros(1, 1, 1, 1, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match=r"tmg_conv_fwd failed with code -3"):
        ops.conv(xs, w, kappa=kap, pad_rep=True)
