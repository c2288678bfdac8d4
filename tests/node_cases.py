"""Case tables, fp64 references, the seed rule and the reference mutations of the autograd-node tests (test_nodes_fp64.py on the
device, test_node_cases_cpu.py without one).  Importable without a GPU: everything here is plain torch on the CPU.

References.  Plain fp64 torch autograd.  The coupling layers are stated by oracle/tmglow_oracle.py (coupling, lstm_coupling and, through
them, resid_lstm, conv_lstm_cell, dense2_nonorm, zero_conv); the functions below (ref_coupling, ref_lstm_coupling) restate the same
arithmetic, operation for operation, with the two additions the oracle has no room for: a recorder (Rec) that notes every convolution
stage and every rectified pre-activation, and switches for the reference MUTATIONS.  test_node_cases_cpu.py asserts that
the un-mutated restatement equals the oracle BIT FOR BIT in fp64; the expected values that the GPU tests compare with are the
oracle's.  The dense block is nn.BatchNorm2d(..).double() + F.conv2d in a loop, the mix an einsum, the ConvLSTM cell the formula of
test_hip_ops.test_conv_lstm_cell_node_matches_fp64, the strided convolution that of test_hip_ops.test_conv_forward_and_grads.

Seed rule.  Inputs are N(0, 1), weights 0.2 N(0, 1) (BatchNorm: gamma 1 + 0.3 N, beta 0.2 N), drawn from torch.Generator().manual_seed(s).
A case takes the first s in 0 .. 15 at which, in the fp64 reference alone, every rectified pre-activation THE NODE COMPUTES (d1, d2, the
LSTM block's out-conv output, bn(x) of every dense layer) has |value| >= MARGIN = 1e-4: the fp32 error of these values is 4e-7 .. 4e-6,
so no fp32 evaluation flips a ReLU and no element of any output has to be left out of a comparison.  Values rectified on the way in
(x1, cond, h) are exact in both precisions and need no margin.

Error measure.  err(a, ref) = max|a - ref| / max(1, max|ref|), NaN = infinite (test_hip_ops._close); log-dets image by image against
max(1, sum_image |sg|) (test_coupling_kernels.py).

Bounds (derivation: docstring of test_nodes_fp64.py).  One convolution stage with K-term sums is allowed what the kernel tests allow it,
(K + 8) 2^-24 S elementwise (conv_cases.gauss bound; the thin / Winograd files use K + 4 / K + 3 of the same S), S the fp64 sum of the
|terms|; in the measure above that is (K + 8) 2^-24 rho, rho = max S / max(1, max|result|), which the recorder evaluates in fp64 for
the forward result, the input gradient and the weight gradient of every stage.  A node's forward bound is the sum over its stages plus
the pointwise kernels' bounds (test_pointwise_kernels.py), its backward bound the forward bound plus the stages' gradient terms plus
TOL_D2 / TOL_AFFB / TOL_LSTM_B."""
import functools
import math
import types

import torch
import torch.nn as tnn
import torch.nn.functional as F

import common as C  # noqa: F401  (sets sys.path)
from oracle import tmglow_oracle as O
U = 2.0 ** -24
# Restated from the kernel tests (test_node_cases_cpu.test_constants_are_the_kernel_tests_own compares them with the originals)
TOL_D2 = 1e-5                                       # test_coupling_kernels.py: dense2_bwd outputs, dW1 / dW2
EXP, TANH, SIG = 4.2 * U, 4.3 * U, 10 * U           # test_pointwise_kernels.py
TOL_AFF, TOL_AFFB = 6 * U + EXP, 12 * U + 2 * EXP
TOL_LSTM_H, TOL_LSTM_B = 2 * (SIG + TANH) + 4 * U, 3 * (SIG + TANH) + 9 * U


def tol_sum(K, base=1.0):
    """test_pointwise_kernels.tol_sum: a K-term fp32 sum is allowed (base + sqrt K) u of the sum of the |terms|."""
    return (base + math.sqrt(K)) * U


MARGIN = 1e-4
MAX_SEEDS = 16
LOG4 = math.log(4.0)
F64 = torch.float64
BN_FWD = 12 * U                   # test_pointwise_kernels.py: bn_finalize64 a 9 u, bsh 12 u
BN_STAT = 11 * U                  # running statistics 9 u + the statistic's own 2 u


# ---------------------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------------------
def err(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == ref.shape, (tuple(a.shape), tuple(ref.shape))
    if a.numel() == 0:
        return 0.0
    if bool(torch.isnan(a).any()):
        return math.inf
    return float((a - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def ld_err(ld, ref, sg_abs):
    """Image by image: |ld_b - ref_b| / max(1, sum_image |sg|)."""
    ld, ref = ld.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    assert ld.shape == ref.shape == sg_abs.shape, (ld.shape, ref.shape, sg_abs.shape)
    if bool(torch.isnan(ld).any()):
        return math.inf
    return float(((ld - ref).abs() / sg_abs.clamp(min=1.0)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorder: convolution stages (K and rho of result, input gradient, weight gradient) and rectified pre-activations
# ---------------------------------------------------------------------------------------------------------------------------------
class Rec:
    def __init__(self):
        self.stages = []
        self.pre = []           # (name, detached pre-activation)
        self.sg_abs = None      # [B] sum_image |sg| of a coupling
        self.hh_scale = 1.0     # max(1, max|zero-conv output|)
        self.n_sg = 0

    def conv(self, name, x, w, b, y, stride, padding):
        with torch.no_grad():
            S = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), stride=stride, padding=padding)
            st = dict(name=name, K=w[0].numel(), Kd=w.shape[0] * w.shape[2] * w.shape[3], Kw=y.numel() // y.shape[1],
                      rho_f=float(S.max()) / max(1.0, float(y.abs().max())), rho_d=0.0, rho_w=0.0)
        self.stages.append(st)
        if y.requires_grad:
            xd, wd = x.detach(), w.detach()

            def hook(g):
                with torch.no_grad():
                    kw = dict(stride=stride, padding=padding)
                    Sd = torch.nn.grad.conv2d_input(xd.shape, wd.abs(), g.abs(), **kw)
                    d = torch.nn.grad.conv2d_input(xd.shape, wd, g, **kw)
                    st["rho_d"] = float(Sd.max()) / max(1.0, float(d.abs().max()))
                    Sw = torch.nn.grad.conv2d_weight(xd.abs(), wd.shape, g.abs(), **kw)
                    dw = torch.nn.grad.conv2d_weight(xd, wd.shape, g, **kw)
                    st["rho_w"] = float(Sw.max()) / max(1.0, float(dw.abs().max()))
            y.register_hook(hook)

    def rect(self, name, z):
        self.pre.append((name, z.detach()))

    def margin(self):
        return min((float(z.abs().min()) for _, z in self.pre), default=math.inf)

    def fwd(self, upto=None):
        """Sum of the forward bounds of the stages (the first `upto` of them)."""
        return sum((s["K"] + 8) * U * s["rho_f"] for s in self.stages[:upto])

    def grads(self):
        return sum((s["Kd"] + 8) * U * s["rho_d"] + (s["Kw"] + 8) * U * s["rho_w"] for s in self.stages)


def _conv(rec, name, x, w, b=None, padding=0, stride=1):
    y = F.conv2d(x, w, b, stride=stride, padding=padding)
    if rec is not None:
        rec.conv(name, x, w, b, y, stride, padding)
    return y


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randomise(mod, g):
    """0.2 N(0, 1) on every parameter; BatchNorm: gamma 1 + 0.3 N, beta 0.2 N."""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, tnn.BatchNorm2d):
                m.weight.copy_(1 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
            else:
                for p in m.parameters(recurse=False):
                    p.copy_(0.2 * torch.randn(p.shape, generator=g))


def _leaf(t, dtype, grad=True):
    return t.detach().to(dtype).clone().requires_grad_(grad)


def _params(sd, dtype):
    return O.params_from_state_dict(sd, dtype=dtype)


def _search(build):
    """The seed rule: the first seed in 0 .. 15 whose fp64 reference keeps every rectified pre-activation MARGIN away from 0."""
    best = None
    for seed in range(MAX_SEEDS):
        d = build(seed)
        if d.margin >= MARGIN:
            return d
        best = d if best is None or d.margin > best.margin else best
    best.seed_ok = False
    return best


# ---------------------------------------------------------------------------------------------------------------------------------
# the coupling tail (dense2 + zero conv + affine) with its mutations
# ---------------------------------------------------------------------------------------------------------------------------------
class _RepConvZeroAdjoint(torch.autograd.Function):
    """conv3x3_valid(pad_replicate(t)) whose INPUT gradient is the adjoint of the zero-padded conv: the border fix missing."""

    @staticmethod
    def forward(ctx, t, w):
        ctx.save_for_backward(t, w)
        return F.conv2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), w)

    @staticmethod
    def backward(ctx, g):
        t, w = ctx.saved_tensors
        dt = torch.nn.grad.conv2d_input(t.shape, w, g, padding=1)
        dw = torch.nn.grad.conv2d_weight(F.pad(t, (1, 1, 1, 1), mode="replicate"), w.shape, g)
        return dt, dw


def _relu(t, n_through):
    """relu(t); the first n_through channels with a straight-through backward (mutation: the out-conv's ReLU mask missing)."""
    r = F.relu(t)
    if n_through:
        r = torch.cat([t[:, :n_through] + (r[:, :n_through] - t[:, :n_through]).detach(), r[:, n_through:]], 1)
    return r


def _tail(P, pre_dense, pre_zero, t, x1, x2, reverse, mut, rec, n_through=0):
    """oracle dense2_nonorm + zero_conv + affine_apply on the network input t."""
    for j in (1, 2):
        w = P[pre_dense + "denselayer%d.conv1.weight" % j]
        if j == 2 and mut == "w2_pad_row_after_d1":
            # padded layout [t0 | 0 x pad | d1]: with the zero rows AFTER the d1 row, d1's weights meet a zero channel and d1 meets zeros
            w = torch.cat([w[:, :-1], w[:, -1:] * 0], 1)
        d = _conv(rec, "d%d" % j, _relu(t, n_through), w, None, 1)
        if rec is not None:
            rec.rect("d%d" % j, d)
        t = torch.cat([t, d], 1)
    t = _relu(t, n_through)
    wz, bz, kap = P[pre_zero + "conv.weight"], P[pre_zero + "conv.bias"], P[pre_zero + "scale"]
    s = torch.exp(torch.clamp(kap, -4.0, LOG4))
    if mut == "zc_zero_adjoint":
        h = (_RepConvZeroAdjoint.apply(t, wz) + bz.view(1, -1, 1, 1)) * s
    elif mut == "dkappa_no_bias":
        h = F.conv2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), wz) * s + bz.view(1, -1, 1, 1) * s.detach()
    else:
        h = _conv(rec, "zero", F.pad(t, (1, 1, 1, 1), mode="replicate"), wz, bz) * s
    x2n, ld = O.affine_apply(h, x2, reverse)
    if rec is not None:
        with torch.no_grad():
            sg = 2.0 * F.softsign(h[:, 1::2])
            rec.sg_abs = sg.abs().reshape(h.shape[0], -1).sum(1)
            rec.n_sg = sg[0].numel()
            rec.hh_scale = max(1.0, float(h.abs().max()))
    if mut == "dld_dropped":
        ld = ld.detach()
    return torch.cat([x1, x2n], 1), ld


def ref_coupling(P, x, cond, reverse, mut=None, rec=None):
    """oracle.coupling (AffineCouplingLayer), keys without prefix."""
    x1, x2 = x.chunk(2, 1)
    return _tail(P, "coupling_nn.dense_block.", "coupling_nn.zero_conv.", torch.cat([x1, cond], 1), x1, x2, reverse, mut, rec)


def ref_lstm_coupling(P, x, cond, state, reverse, mut=None, rec=None):
    """oracle.lstm_coupling (LSTMAffineCouplingLayer): ConvLSTM cell, out conv + ReLU, then the tail."""
    x1, x2 = x.chunk(2, 1)
    t = torch.cat([x1.detach() if mut == "x1_join_missing" else x1, cond], 1)
    w = P["resid_lstm.convLSTM.conv.weight"]
    hid = w.shape[0] // 4
    if state is None:
        shape = (t.shape[0], hid, t.shape[2], t.shape[3])
        h_cur, c_cur = t.new_zeros(shape), t.new_zeros(shape)
    else:
        h_cur, c_cur = state
    gates = _conv(rec, "gates", torch.cat([t, h_cur], 1), w, P["resid_lstm.convLSTM.conv.bias"], 1)
    gi, gf, go, gg = torch.split(gates, hid, 1)
    c_next = torch.sigmoid(gf) * c_cur + torch.sigmoid(gi) * torch.tanh(gg)
    h_next = torch.sigmoid(go) * torch.tanh(c_next)
    o = _conv(rec, "out", torch.cat([t, h_next], 1), P["resid_lstm.out_seq.LSTM_out_conv.weight"],
              P["resid_lstm.out_seq.LSTM_out_conv.bias"], 1)
    if rec is not None:
        rec.rect("out", o)
    through = o.shape[1] if mut == "out_mask_missing" else 0
    y, ld = _tail(P, "dense_nn.dense_block.", "out_conv.zero_conv.", _relu(o, through), x1, x2, reverse, mut, rec, through)
    return y, ld, (h_next, c_next)


def _tail_tols(rec, n_pw_f=0.0, n_pw_b=0.0):
    """(forward, log-det, backward) bounds of a node that ends in the coupling tail (docstring of test_nodes_fp64.py)."""
    f = 2 * rec.fwd() + TOL_AFF + n_pw_f
    # |d sg / d r| <= 2: each of the N = n_sg terms carries twice the zero conv's error; N independent errors add up like sqrt(N)
    ld = tol_sum(rec.n_sg, 2.0) + 2 * rec.fwd() * rec.hh_scale * math.sqrt(rec.n_sg) / max(1.0, float(rec.sg_abs.min()))
    b = f + rec.grads() + TOL_AFFB + TOL_D2 + tol_sum(rec.stages[-1]["K"] * rec.stages[-1]["Kd"] // 9) + n_pw_b
    return f, ld, b


# ---------------------------------------------------------------------------------------------------------------------------------
# node 1: CouplingTailFn mode 0 (AffineCouplingLayer)
# ---------------------------------------------------------------------------------------------------------------------------------
COUPLING_SHAPES = {"c8": (2, 9, 7, 8, 4), "c64": (2, 8, 12, 64, 32), "c16_1x1": (2, 1, 1, 16, 8), "c12_odd": (1, 5, 6, 12, 5)}
COUPLING_VARIANTS = ("clamp", "no_ld", "slice", "nchw", "gy_noncontig")        # on c8 and c64
COUPLING_MUTATIONS = ("zc_zero_adjoint", "dkappa_no_bias", "dld_dropped")


def _coupling_outputs(P, x, cond, y, ld):
    out = {"y": y.detach(), "ld": ld.detach(), "dx": x.grad, "dcond": cond.grad}
    for k, v in P.items():
        if v.requires_grad:
            out["d:" + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return out


def _coupling_run(sd, t, reverse, use_ld, dtype, fn, mut=None, rec=None):
    P = _params(sd, dtype)
    x, cond = _leaf(t["x"], dtype), _leaf(t["cond"], dtype)
    y, ld = fn(P, x, cond, reverse, mut, rec)
    loss = (y * t["gy"].to(dtype)).sum()
    if use_ld:
        loss = loss + (ld * t["gl"].to(dtype)).sum()
    loss.backward()
    return _coupling_outputs(P, x, cond, y, ld)


@functools.lru_cache(maxsize=None)
def coupling_data(name, reverse, clamp=False, use_ld=True):
    from nn.modules.flowAffine import AffineCouplingLayer
    B, Hh, Ww, C_, Cc = COUPLING_SHAPES[name]

    def build(seed):
        g = _gen(seed)
        lay = AffineCouplingLayer(C_, Cc)
        _randomise(lay, g)
        if clamp:
            with torch.no_grad():
                lay.coupling_nn.zero_conv.scale.fill_(LOG4 + 0.25)
        sd = {k: v.detach().clone() for k, v in lay.state_dict().items()}
        t = dict(x=torch.randn(B, C_, Hh, Ww, generator=g), cond=torch.randn(B, Cc, Hh, Ww, generator=g),
                 gy=torch.randn(B, C_, Hh, Ww, generator=g), gl=torch.randn(B, generator=g))
        rec = Rec()
        mine = _coupling_run(sd, t, reverse, use_ld, F64, ref_coupling, None, rec)
        f, ld, b = _tail_tols(rec)
        return types.SimpleNamespace(seed=seed, seed_ok=True, margin=rec.margin(), rec=rec, sd=sd, t=t, mine=mine, shape=(B, Hh, Ww, C_, Cc),
                                     reverse=reverse, use_ld=use_ld, tol_f=f, tol_ld=ld, tol_b=b)

    d = _search(build)
    d.ref = _coupling_run(d.sd, d.t, reverse, use_ld, F64, lambda P, x, c, r, m, rc: O.coupling(P, "", x, c, r))
    d.run = lambda mut=None, dtype=F64, rec=None: _coupling_run(d.sd, d.t, reverse, use_ld, dtype, ref_coupling, mut, rec)
    return d


def tol_of(d, name):
    """The bound of one checked output of a case."""
    if name in ("y", "y1", "h", "c", "out"):
        return d.tol_f
    if name == "ld":
        return d.tol_ld
    if name.startswith("stat:"):
        return d.tol_stat[name]
    return d.tol_b


def out_err(d, name, got, ref=None):
    ref = d.ref[name] if ref is None else ref
    if name == "ld":
        return ld_err(got, ref, d.rec.sg_abs)
    return err(got, ref)


def moved(d, mutated):
    """Largest err / bound over the checked outputs between a mutated reference and the reference."""
    worst = 0.0
    for k, r in d.ref.items():
        if r is None or not r.is_floating_point():
            continue
        worst = max(worst, out_err(d, k, mutated[k]) / tol_of(d, k))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# node 2: LSTMAffineCouplingLayer.run
# ---------------------------------------------------------------------------------------------------------------------------------
#                      B  H  W   C  Cc   R  pad
LSTM_SHAPES = {"l8": (2, 9, 7, 8, 4, 4, 0), "l16_r64": (2, 8, 8, 16, 32, 64, 0), "l12_pad2": (2, 6, 10, 12, 4, 4, 2)}
LSTM_MUTATIONS = ("x1_join_missing", "out_mask_missing")
LSTM_PAD_MUTATIONS = ("w2_pad_row_after_d1",)


def _lstm_run(sd, t, reverse, with_state, full_loss, dtype, fn, mut=None, rec=None):
    P = _params(sd, dtype)
    x, cond = _leaf(t["x"], dtype), _leaf(t["cond"], dtype)
    st = (_leaf(t["h0"], dtype), _leaf(t["c0"], dtype)) if with_state else None
    y, ld, (h, c) = fn(P, x, cond, st, reverse, mut, rec)
    loss = (y * t["gy"].to(dtype)).sum()
    if full_loss:
        loss = loss + (ld * t["gl"].to(dtype)).sum() + (h * t["gh"].to(dtype)).sum() + (c * t["gc"].to(dtype)).sum()
    loss.backward()
    out = _coupling_outputs(P, x, cond, y, ld)
    out.update(h=h.detach(), c=c.detach())
    if with_state:
        out.update(dh0=st[0].grad, dc0=st[1].grad)
    return out


def _lstm_inputs(g, B, Hh, Ww, C_, Cc, R):
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=r(B, C_, Hh, Ww), cond=r(B, Cc, Hh, Ww), h0=r(B, R, Hh, Ww), c0=r(B, R, Hh, Ww), gy=r(B, C_, Hh, Ww), gl=r(B),
                gh=r(B, R, Hh, Ww), gc=r(B, R, Hh, Ww))


def _lstm_tols(rec):
    # the cell's pointwise kernels sit between the gate conv and the out conv
    return _tail_tols(rec, TOL_LSTM_H, TOL_LSTM_B)


@functools.lru_cache(maxsize=None)
def lstm_data(name, reverse, with_state, full_loss=True):
    from nn.modules.flowAffine import LSTMAffineCouplingLayer
    B, Hh, Ww, C_, Cc, R, pad = LSTM_SHAPES[name]

    def build(seed):
        g = _gen(seed)
        lay = LSTMAffineCouplingLayer(C_, Cc, R)
        _randomise(lay, g)
        sd = {k: v.detach().clone() for k, v in lay.state_dict().items()}
        t = _lstm_inputs(g, B, Hh, Ww, C_, Cc, R)
        rec = Rec()
        mine = _lstm_run(sd, t, reverse, with_state, full_loss, F64, ref_lstm_coupling, None, rec)
        f, ld, b = _lstm_tols(rec)
        return types.SimpleNamespace(seed=seed, seed_ok=True, margin=rec.margin(), rec=rec, sd=sd, t=t, mine=mine, reverse=reverse,
                                     shape=(B, Hh, Ww, C_, Cc, R, pad), with_state=with_state, full_loss=full_loss, tol_f=f, tol_ld=ld, tol_b=b)

    d = _search(build)
    d.ref = _lstm_run(d.sd, d.t, reverse, with_state, full_loss, F64, lambda P, x, c, s, r, m, rc: O.lstm_coupling(P, "", x, c, s, r))
    d.run = lambda mut=None, dtype=F64, rec=None: _lstm_run(d.sd, d.t, reverse, with_state, full_loss, dtype, ref_lstm_coupling, mut, rec)
    return d


WINDOW_MUTATIONS = ("last_step_only",)


def _window_run(sd, t, reverse, dtype, fn, mut=None, rec=None):
    """Two steps on the same parameters: step 2 takes step 1's (h, c); the loss uses both steps' y and log-det and the last state."""
    P = _params(sd, dtype)
    P1 = {k: v.detach() for k, v in P.items()} if mut == "last_step_only" else P
    xs, conds = [_leaf(t["x"], dtype), _leaf(t["x2"], dtype)], [_leaf(t["cond"], dtype), _leaf(t["cond2"], dtype)]
    y1, ld1, st = fn(P1, xs[0], conds[0], None, reverse, None, rec)
    y2, ld2, (h, c) = fn(P, xs[1], conds[1], st, reverse, None, rec)
    gy, gl = t["gy"].to(dtype), t["gl"].to(dtype)
    loss = (y1 * gy).sum() + (ld1 * gl).sum() + (y2 * t["gy2"].to(dtype)).sum() + (ld2 * gl).sum() + (h * t["gh"].to(dtype)).sum() + \
        (c * t["gc"].to(dtype)).sum()
    loss.backward()
    out = {"y": y2.detach(), "y1": y1.detach(), "ld": ld2.detach(), "h": h.detach(), "c": c.detach(), "dx": xs[1].grad, "dx1": xs[0].grad,
           "dcond": conds[1].grad, "dcond1": conds[0].grad}
    for k, v in P.items():
        if v.requires_grad:
            out["d:" + k] = v.grad
    return out


@functools.lru_cache(maxsize=None)
def window_data(name, reverse):
    from nn.modules.flowAffine import LSTMAffineCouplingLayer
    B, Hh, Ww, C_, Cc, R, pad = LSTM_SHAPES[name]

    def build(seed):
        g = _gen(seed)
        lay = LSTMAffineCouplingLayer(C_, Cc, R)
        _randomise(lay, g)
        sd = {k: v.detach().clone() for k, v in lay.state_dict().items()}
        t = _lstm_inputs(g, B, Hh, Ww, C_, Cc, R)
        t.update(x2=torch.randn(B, C_, Hh, Ww, generator=g), cond2=torch.randn(B, Cc, Hh, Ww, generator=g),
                 gy2=torch.randn(B, C_, Hh, Ww, generator=g))
        rec = Rec()
        mine = _window_run(sd, t, reverse, F64, ref_lstm_coupling, None, rec)
        # the second step's stages are recorded last: its tail sets sg_abs; both steps' stages add up along the chain
        f, ld, b = _lstm_tols(rec)
        return types.SimpleNamespace(seed=seed, seed_ok=True, margin=rec.margin(), rec=rec, sd=sd, t=t, mine=mine, reverse=reverse,
                                     shape=(B, Hh, Ww, C_, Cc, R, pad), tol_f=f, tol_ld=ld, tol_b=b)

    d = _search(build)
    d.ref = _window_run(d.sd, d.t, reverse, F64, lambda P, x, c, s, r, m, rc: O.lstm_coupling(P, "", x, c, s, r))
    d.run = lambda mut=None, dtype=F64, rec=None: _window_run(d.sd, d.t, reverse, dtype, ref_lstm_coupling, mut, rec)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# node 3: ConvLSTMCellFn
# ---------------------------------------------------------------------------------------------------------------------------------
#                   B  H  W  segments  R
CELL_SHAPES = {"r4": (2, 9, 7, (4, 4), 4), "r64": (1, 8, 8, (8, 32), 64)}
CELL_VARIANTS = ("c_none", "h_only", "c_only", "first_seg_only")
CELL_MUTATIONS = {"c_none_as_ones": ("c_none",), "gate_order_ifgo": CELL_VARIANTS}


def _cell_run(t, variant, dtype, mut=None, rec=None):
    """NHWC tensors, as test_hip_ops.test_conv_lstm_cell_node_matches_fp64."""
    first_only = variant == "first_seg_only"
    xs = [_leaf(v, dtype, grad=(i == 0 or not first_only)) for i, v in enumerate(t["xs"])]
    h0 = _leaf(t["h0"], dtype, grad=not first_only)
    c0 = None if variant == "c_none" else _leaf(t["c0"], dtype)
    w, b = _leaf(t["w"], dtype), _leaf(t["b"], dtype)
    R = h0.shape[3]
    inp = torch.cat(xs + [h0], 3).permute(0, 3, 1, 2)
    gates = _conv(rec, "gates", inp, w, b, 1).permute(0, 2, 3, 1)
    if mut == "gate_order_ifgo":
        i_, f_, g_, o_ = torch.split(gates, R, 3)
    else:
        i_, f_, o_, g_ = torch.split(gates, R, 3)
    cp = c0 if c0 is not None else (torch.ones_like(h0) if mut == "c_none_as_ones" else torch.zeros_like(h0))
    cn = torch.sigmoid(f_) * cp + torch.sigmoid(i_) * torch.tanh(g_)
    hn = torch.sigmoid(o_) * torch.tanh(cn)
    loss = 0.0
    if variant != "c_only":
        loss = loss + (hn * t["gh"].to(dtype)).sum()
    if variant != "h_only":
        loss = loss + (cn * t["gc"].to(dtype)).sum()
    loss.backward()
    out = {"h": hn.detach(), "c": cn.detach(), "dW": w.grad, "db": b.grad, "dx0": xs[0].grad}
    if not first_only:
        out.update({"dx%d" % i: x.grad for i, x in enumerate(xs)})
        out["dh0"] = h0.grad
    if c0 is not None:
        out["dc0"] = c0.grad
    return out


@functools.lru_cache(maxsize=None)
def cell_data(name, variant):
    B, Hh, Ww, segs, R = CELL_SHAPES[name]
    g = _gen(0)         # nothing is rectified: seed 0
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(xs=[r(B, Hh, Ww, c) for c in segs], h0=r(B, Hh, Ww, R), c0=r(B, Hh, Ww, R), w=0.2 * r(4 * R, sum(segs) + R, 3, 3),
             b=0.2 * r(4 * R), gh=r(B, Hh, Ww, R), gc=r(B, Hh, Ww, R))
    rec = Rec()
    ref = _cell_run(t, variant, F64, None, rec)
    f = rec.fwd() + TOL_LSTM_H
    d = types.SimpleNamespace(seed=0, seed_ok=True, margin=math.inf, rec=rec, t=t, ref=ref, mine=ref, shape=(B, Hh, Ww, segs, R),
                              variant=variant, tol_f=f, tol_b=f + rec.grads() + TOL_LSTM_B)
    d.run = lambda mut=None, dtype=F64, rec=None: _cell_run(t, variant, dtype, mut, rec)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# node 4: DenseBlockFn / BNReLUConvFn
# ---------------------------------------------------------------------------------------------------------------------------------
#                    B  H   W  c0  g  L
# d16: 3 x 10 x 14 (36 960 pre-activations) has no training-mode seed with the margin among 0 .. 15; 3 x 10 x 10 has
DENSE_SHAPES = {"d6": (2, 9, 7, 6, 3, 3), "d16": (3, 10, 10, 16, 4, 4), "d8_row": (2, 1, 5, 8, 4, 2), "layer12": (2, 9, 7, 12, 4, 1)}
DENSE_MODES = ("train", "eval", "notrack")          # notrack: track_running_stats=False (batch statistics in eval mode too)
DENSE_MUTATIONS = {"layer_contrib_dropped": ("train", "eval", "notrack"), "eval_as_train": ("eval",), "train_as_eval": ("train", "notrack"),
                   "running_var_biased": ("train",)}


def _bn_manual(bn, x, mut):
    bm, bv = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    if mut == "eval_as_train":      # the value of eval mode, the derivative of training mode (batch means subtracted)
        m, v = bn.running_mean + (bm - bm.detach()), bn.running_var + (bv - bv.detach())
    else:                           # train_as_eval: batch statistics taken as constants
        with torch.no_grad():
            bn(x)                   # the running statistics move as in training
        m, v = bm.detach(), bv.detach()
    sh = (1, -1, 1, 1)
    return (x - m.view(sh)) * torch.rsqrt(v + bn.eps).view(sh) * bn.weight.view(sh) + bn.bias.view(sh)


def ref_dense(bns, ws, x, mut=None, rec=None):
    """x <- cat(x, conv3x3(relu(bn(x)))) per layer (reference denseBlock.py:49-67); bns: nn.BatchNorm2d modules of the data's dtype."""
    L = len(bns)
    for i, (bn, w) in enumerate(zip(bns, ws)):
        xin = x.detach() if (mut == "layer_contrib_dropped" and i == L - 1) else x
        batch = bn.training or not bn.track_running_stats
        if (mut == "eval_as_train" and not batch) or (mut == "train_as_eval" and batch):
            z = _bn_manual(bn, xin, mut)
        elif mut == "running_var_biased" and bn.training and bn.track_running_stats:
            rv0 = bn.running_var.clone()
            z = bn(xin)
            bn.biased_var = ((1 - bn.momentum) * rv0 + bn.momentum * xin.var((0, 2, 3), unbiased=False)).detach()   # read by _dense_run
        else:
            z = bn(xin)
        if rec is not None:
            rec.rect("bn%d" % i, z)
        x = torch.cat([x, _conv(rec, "grow%d" % i, F.relu(z), w, None, 1)], 1)
    return x


def dense_modules(d, dtype=F64):
    """Fresh BatchNorm2d modules (data's statistics before the call) and leaf conv weights of a case."""
    track = d.mode != "notrack"
    bns, ws = [], []
    for i in range(d.L):
        pre = "denselayer%d." % (i + 1)
        bn = tnn.BatchNorm2d(d.sd[pre + "norm1.weight"].shape[0], track_running_stats=track).to(dtype)
        bn.load_state_dict({k[len(pre + "norm1."):]: v for k, v in d.sd.items() if k.startswith(pre + "norm1.") and (track or "running" not in k
                                                                                                                    and "num_batches" not in k)})
        bn.train(d.mode == "train")
        bns.append(bn)
        ws.append(_leaf(d.sd[pre + "conv1.weight"], dtype))
    return bns, ws


def _dense_run(d, dtype, mut=None, rec=None):
    bns, ws = dense_modules(d, dtype)
    x = _leaf(d.t["x"], dtype)
    y = ref_dense(bns, ws, x, mut, rec)
    (y * d.t["gy"].to(dtype)).sum().backward()
    out = {"out": y.detach(), "dx": x.grad}
    for i, (bn, w) in enumerate(zip(bns, ws)):
        pre = "denselayer%d." % (i + 1)
        out["d:" + pre + "norm1.weight"], out["d:" + pre + "norm1.bias"], out["d:" + pre + "conv1.weight"] = bn.weight.grad, bn.bias.grad, w.grad
        if bn.track_running_stats:
            out["stat:" + pre + "norm1.running_mean"] = bn.running_mean.detach().clone()
            out["stat:" + pre + "norm1.running_var"] = getattr(bn, "biased_var", bn.running_var).detach().clone()
            out["count:" + pre + "norm1.num_batches_tracked"] = bn.num_batches_tracked.detach().clone()
    return out


@functools.lru_cache(maxsize=None)
def dense_data(name, mode):
    from nn.modules.denseBlock import DenseBlock
    B, Hh, Ww, c0, growth, L = DENSE_SHAPES[name]

    def build(seed):
        g = _gen(seed)
        blk = DenseBlock(num_layers=L, in_features=c0, growth_rate=growth, drop_rate=0.)
        _randomise(blk, g)
        with torch.no_grad():       # running statistics away from their defaults: mean != 0, var != 1
            for m in blk.modules():
                if isinstance(m, tnn.BatchNorm2d):
                    m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                    m.num_batches_tracked.fill_(3)
        sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
        t = dict(x=torch.randn(B, c0, Hh, Ww, generator=g), gy=torch.randn(B, c0 + L * growth, Hh, Ww, generator=g))
        d = types.SimpleNamespace(seed=seed, seed_ok=True, sd=sd, t=t, mode=mode, L=L, shape=(B, Hh, Ww, c0, growth, L))
        d.rec = Rec()
        d.ref = d.mine = _dense_run(d, F64, None, d.rec)
        d.margin = d.rec.margin()
        n = B * Hh * Ww
        d.tol_f = d.rec.fwd() + L * BN_FWD
        # bn_bwd_apply: (12 + sqrt n) u per layer; chan_reduce (dgamma, dbeta): (8 + sqrt n) u
        d.tol_b = d.tol_f + d.rec.grads() + L * (tol_sum(n, 12.0) + tol_sum(n, 8.0))
        # layer i's statistics see the input (exact) and the growth channels of the layers before it
        d.tol_stat = {}
        for i in range(L):
            for s in ("running_mean", "running_var"):
                d.tol_stat["stat:denselayer%d.norm1.%s" % (i + 1, s)] = BN_STAT + 2 * d.rec.fwd(i) + i * BN_FWD
        return d

    d = _search(build)
    d.run = lambda mut=None, dtype=F64, rec=None: _dense_run(d, dtype, mut, rec)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# node 5: MixFn
# ---------------------------------------------------------------------------------------------------------------------------------
MIX_WIDTHS = (16, 6, 64)
MIX_SHAPES = {"9x7": (2, 9, 7), "1x1": (1, 1, 1)}
MIX_MUTATIONS = ("dx_with_W",)
U16 = 2.0 ** -11            # fp16 unit roundoff


class _MixWrongDx(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return torch.einsum("oc,bhwc->bhwo", W, x)

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        return torch.einsum("co,bhwo->bhwc", W, g), torch.einsum("bhwo,bhwc->oc", g, x)      # W where W^T belongs


def _mix_run(t, with_b, dtype, mut=None):
    x, W = _leaf(t["x"], dtype), _leaf(t["W"], dtype)
    b = _leaf(t["b"], dtype) if with_b else None
    y = _MixWrongDx.apply(x, W) if mut == "dx_with_W" else torch.einsum("oc,bhwc->bhwo", W, x)
    if with_b:
        y = y + b
    (y * t["gy"].to(dtype)).sum().backward()
    out = {"y": y.detach(), "dx": x.grad, "dW": W.grad}
    if with_b:
        out["db"] = b.grad
    return out


@functools.lru_cache(maxsize=None)
def mix_data(width, shape, with_b):
    B, Hh, Ww = MIX_SHAPES[shape]
    g = _gen(0)
    t = dict(x=torch.randn(B, Hh, Ww, width, generator=g), W=torch.randn(width, width, generator=g) / math.sqrt(width),
             b=0.2 * torch.randn(width, generator=g), gy=torch.randn(B, Hh, Ww, width, generator=g))
    ref = _mix_run(t, with_b, F64)
    x, W, gy = t["x"].double(), t["W"].double(), t["gy"].double()
    n = B * Hh * Ww
    rho = lambda S, r: float(S.max()) / max(1.0, float(r.abs().max()))  # noqa: E731
    Sy = torch.einsum("oc,bhwc->bhwo", W.abs(), x.abs()) + (t["b"].double().abs() if with_b else 0)
    Sd = torch.einsum("oc,bhwo->bhwc", W.abs(), gy.abs())
    Sw = torch.einsum("bhwo,bhwc->oc", gy.abs(), x.abs())
    d = types.SimpleNamespace(seed=0, seed_ok=True, margin=math.inf, t=t, ref=ref, mine=ref, shape=(B, Hh, Ww, width), with_b=with_b,
                              # thin_cases mix bound (K + 3) u S; the weight gradient is conv_wgrad's (K + 8) u S with K = pixels
                              tol_f=(width + 3) * U * rho(Sy, ref["y"]), tol_dx=(width + 3) * U * rho(Sd, ref["dx"]),
                              tol_dw=(n + 8) * U * max(rho(Sw, ref["dW"]), rho(gy.abs().sum((0, 1, 2)), gy.sum((0, 1, 2)))),
                              # fp16 operands: each product carries two roundings of 2^-11, the sum is fp32 (test_mix_f16_kernel's model)
                              tol_f16=(2 * U16 + (width + 3) * U) * rho(Sy, ref["y"]), tol_dx16=(2 * U16 + (width + 3) * U) * rho(Sd, ref["dx"]))
    d.tol_b = max(d.tol_dx, d.tol_dw)
    d.run = lambda mut=None, dtype=F64, rec=None: _mix_run(t, with_b, dtype, mut)
    return d


def mix_tol(d, name, f16=False):
    if name == "y":
        return d.tol_f16 if f16 else d.tol_f
    if name == "dx":
        return d.tol_dx16 if f16 else d.tol_dx
    return d.tol_dw


# ---------------------------------------------------------------------------------------------------------------------------------
# node 6: ConvFn, stride-2 input gradient at odd sizes, and upstream gradients that are channel slices
# ---------------------------------------------------------------------------------------------------------------------------------
#               B  H  W  segs  Cout k  s  relu_in
CONV_SHAPES = {"s2_9x7": (2, 9, 7, (8,), 16, 3, 2, True), "s2_5x5": (1, 5, 5, (5,), 9, 3, 2, True),
               "s1_slice": (2, 9, 7, (8,), 12, 3, 1, False)}


@functools.lru_cache(maxsize=None)
def conv_data(name):
    """The reference of test_hip_ops.test_conv_forward_and_grads (zero padding, no bias / kappa) at these shapes."""
    B, Hh, Ww, segs, Cout, k, stride, relu_in = CONV_SHAPES[name]
    g = _gen(0)
    t = dict(xs=[torch.randn(B, c, Hh, Ww, generator=g) for c in segs], w=0.2 * torch.randn(Cout, sum(segs), k, k, generator=g))
    xr, wr = [_leaf(v, F64) for v in t["xs"]], _leaf(t["w"], F64)
    inp = torch.cat(xr, 1)
    rec = Rec()
    yr = _conv(rec, "conv", F.relu(inp) if relu_in else inp, wr, None, 1, stride)
    t["gy"] = torch.randn(yr.shape, generator=g)
    (yr * t["gy"].double()).sum().backward()
    ref = {"y": yr.detach(), "dW": wr.grad}
    ref.update({"dx%d" % i: x.grad for i, x in enumerate(xr)})
    f = rec.fwd()
    return types.SimpleNamespace(seed=0, seed_ok=True, margin=math.inf, rec=rec, t=t, ref=ref, shape=CONV_SHAPES[name], tol_f=f,
                                 tol_b=f + rec.grads())


# ---------------------------------------------------------------------------------------------------------------------------------
# the table of every case that carries a seed (test_node_cases_cpu.py walks it)
# ---------------------------------------------------------------------------------------------------------------------------------
def seeded_cases():
    """(label, thunk -> data, mutations that apply)."""
    out = []
    for name in COUPLING_SHAPES:
        for rev in (False, True):
            out.append(("coupling %s rev%d" % (name, rev), functools.partial(coupling_data, name, rev), COUPLING_MUTATIONS))
    for name in ("c8", "c64"):
        out.append(("coupling %s clamp" % name, functools.partial(coupling_data, name, True, True, True), ()))
        out.append(("coupling %s no_ld" % name, functools.partial(coupling_data, name, False, False, False), ()))
    for name, shp in LSTM_SHAPES.items():
        muts = LSTM_MUTATIONS + (LSTM_PAD_MUTATIONS if shp[6] else ())
        for rev in (False, True):
            for with_state in (False, True):
                out.append(("lstm %s rev%d state%d" % (name, rev, with_state), functools.partial(lstm_data, name, rev, with_state), muts))
        out.append(("lstm %s y_only" % name, functools.partial(lstm_data, name, True, True, False), ()))
    for name in ("l8", "l12_pad2"):
        out.append(("window %s" % name, functools.partial(window_data, name, True), WINDOW_MUTATIONS))
    for name in DENSE_SHAPES:
        for mode in DENSE_MODES:
            if mode == "notrack" and name != "d6":
                continue
            muts = tuple(m for m, modes in DENSE_MUTATIONS.items() if mode in modes)
            out.append(("dense %s %s" % (name, mode), functools.partial(dense_data, name, mode), muts))
    return out


def unseeded_cases():
    out = []
    for name in CELL_SHAPES:
        for v in CELL_VARIANTS:
            out.append(("cell %s %s" % (name, v), functools.partial(cell_data, name, v), tuple(m for m, vs in CELL_MUTATIONS.items() if v in vs)))
    for wdt in MIX_WIDTHS:
        for shp in MIX_SHAPES:
            for with_b in (True, False):
                out.append(("mix C%d %s b%d" % (wdt, shp, with_b), functools.partial(mix_data, wdt, shp, with_b), MIX_MUTATIONS))
    return out
