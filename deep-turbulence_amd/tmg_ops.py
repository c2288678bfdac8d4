"""torch.autograd glue over the HIP kernels: one Function per primitive of the TM-Glow hot path.

Forward and backward of every Function are kernel launches from tmg_hip (libtmglow_hip.so); torch
only provides tensors, the stream and the autograd tape.  Gradients w.r.t. tiny parameter tensors
that are pure bookkeeping (e.g. d(kappa) from <W,dW>+<b,db>) are a handful of scalar torch ops.

All activations are NHWC ([B,H,W,C] contiguous, or channel-slice views of such tensors).
"""
import collections
import math
import numbers

import os
import threading
import weakref

import torch

import tmg_hip as H

LOG5 = math.log(5.0)
LOG4 = math.log(4.0)
SPLIT_LIMITS = (-2.0, LOG5, -2.0, LOG5)      # hardtanh(-2, ln5) on both halves (flowUtils.py:262,274)
TOP_LIMITS = (0.0, 0.0, -10.0, LOG5)         # only the log-std is clamped (flowUtils.py:163)


class _ZeroPool:
    """Zero-initialised scratch for the many parameter-sized gradient / statistics buffers of a step (~170 `torch.zeros` launches
    of a few microseconds each): buffers of up to LIMIT floats are carved, 256-byte aligned, from ONE zero-filled chunk per
    (device, stream), so a step pays one or two fill launches instead.  A carved buffer is an ordinary tensor on the chunk's storage:
    it keeps the chunk alive and is never handed out twice; chunks are freed by the caching allocator once every buffer is gone (for
    parameter gradients: at the next zero_grad).  Bypassed during hipGraph capture - a replay would not re-zero a chunk filled before the
    capture."""
    CHUNK = 8 << 20
    LIMIT = 2 << 20

    def __init__(self):
        self.lock = threading.Lock()
        self.cur = {}

    def zeros(self, shape, device):
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = math.prod(shape)
        device = torch.device(device)
        if n == 0 or n > self.LIMIT or device.type != "cuda" or torch.cuda.is_current_stream_capturing():
            return torch.zeros(shape, device=device, dtype=torch.float32)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        need = (n + 63) & ~63
        with self.lock:
            buf, off = self.cur.get(key, (None, 0))
            if buf is None or off + need > buf.numel():
                buf, off = torch.zeros(self.CHUNK, device=device, dtype=torch.float32), 0
            self.cur[key] = (buf, off + need)
        # not a view: a tensor of its own on the chunk's storage - views of one base share a version counter, and an in-place torch
        # op on one carved buffer would invalidate every other one that some autograd node has saved
        return empty(0, device).set_(buf.untyped_storage(), off, shape)


_pool = _ZeroPool()


def zeros(shape, device):
    """fp32 zeros on `device` (pooled when small, see _ZeroPool)."""
    return _pool.zeros(shape, device)


def zeros_like(t):
    return _pool.zeros(t.shape, t.device)


def empty(shape, device):
    """Uninitialised fp32 buffer on `device`: an activation or gradient that the launch after it writes whole."""
    return torch.empty(shape, device=device, dtype=torch.float32)


def carve(device, *shapes):
    """One view per shape, back to back in the order given, of ONE zero-filled flat buffer: the parameter gradients of a node for
    one zeros() call."""
    sizes = [math.prod(s) for s in shapes]
    flat = zeros(sum(sizes), device)
    views, o = [], 0
    for s, n in zip(shapes, sizes):
        views.append(flat[o:o + n].view(s))
        o += n
    return views


# Bumped by every writer of parameter memory that torch's version counters do not see (tmg_optim.HipAdam updates the parameters
# from a kernel launched through ctypes): part of the key of every value derived from parameters (DerivedCache).
PARAM_GENERATION = H.PARAM_GENERATION      # (one list object: tmg_hip's pack plan keys on it too)


class DerivedCache:
    """Tensors derived from parameters by pure functions - zero-padded weights of the 3-channel layout, the folded ActNorm + PLU
    mixes of a level - that a BPTT window evaluates T = 10 times on unchanged parameters (reference trainFlowParallel.py:256-287:
    the optimizer steps once per window).  An entry is valid while its source parameters are unchanged (data pointer, torch version
    counter, PARAM_GENERATION), for the same grad mode, and - when it carries an autograd graph - until a backward pass has gone
    through it (a hook on every differentiable tensor marks it stale: the graph is freed then).  So a window builds it once, T
    forward passes share it, autograd sums the T gradients and runs its backward once; a single-step loop rebuilds it every step,
    exactly as before.  proxies=True: the tensors are also gradient-sink targets (see _GradSink) - the T gradients per tensor are
    summed by multi-tensor launches and handed to autograd once, on leaving fused_grad_accumulation."""

    window_depth = 0         # > 0 inside `with bptt_window():` - the only place where values that carry an autograd graph are shared

    def __init__(self):
        self.entries = {}

    @staticmethod
    def _tensors(val):
        if torch.is_tensor(val):
            yield val
        elif isinstance(val, (tuple, list)):
            for v in val:
                yield from DerivedCache._tensors(v)

    def clear(self):
        """Drops every entry (and the autograd graphs the entries carry)."""
        for e in self.entries.values():
            for i_ in e["ids"]:
                _GradSink.proxy_ids.pop(i_, None)
        self.entries = {}

    def get(self, name, params, extra, build, proxies=False):
        # Sharing a value WITH a graph between forward passes is only right when ONE backward pass follows them all (a second,
        # separate backward would find the shared part of the graph freed): that is the BPTT window, which says so with
        # `with bptt_window():`.  Everywhere else a grad-mode call builds its own value, exactly as before round 4; without grad
        # mode (sampling loops of TrainFlow.test / modelPred) there is no graph and the cache is always on.
        if torch.is_grad_enabled() and DerivedCache.window_depth == 0:
            return build()
        key = (tuple((p.data_ptr(), p._version) for p in params), PARAM_GENERATION[0], torch.is_grad_enabled(), extra)
        e = self.entries.get(name)
        if e is not None and e["key"] == key and not e["stale"][0]:
            return e["val"]
        if e is not None:
            for i_ in e["ids"]:
                _GradSink.proxy_ids.pop(i_, None)
        val = build()
        stale, ids = [False], set()
        for t in self._tensors(val):
            if t.requires_grad:
                t.register_hook(lambda g, s=stale: s.__setitem__(0, True))
                if proxies:
                    ids.add(t._cdata)
                    _GradSink.proxy_ids[t._cdata] = weakref.ref(t)
        if len(_GradSink.proxy_ids) > 4096:      # entries of caches that died with their model
            for i_ in [i_ for i_, r_ in _GradSink.proxy_ids.items() if r_() is None]:
                del _GradSink.proxy_ids[i_]
        self.entries[name] = {"key": key, "val": val, "stale": stale, "ids": ids}
        return val


def invalidate_derived(model=None):
    """Explicit invalidation of everything derived from parameter values (DerivedCache: folded ActNorm + PLU mixes, zero-padded
    weights).  The caches key on the parameters' data pointers, torch version counters and PARAM_GENERATION - a write that moves none
    of them (`p.data.mul_(..)`, weight surgery through `.data` inside a no-grad sampling loop, a kernel launched through ctypes) must
    be followed by this call.  model: also drop the entries held by its modules (frees the autograd graphs they carry - a hipGraph
    recording needs the AccumulateGrad nodes of earlier eager passes gone: they remember the stream they were created on)."""
    PARAM_GENERATION[0] += 1
    if model is not None:
        for m in model.modules():
            c = m.__dict__.get("_derived")
            if c is not None:
                c.clear()


class _GradSink:
    """Parameter gradients of the custom nodes collected over ONE backward pass instead of being handed to autograd one by one.

    A BPTT window runs every node T = 10 times on the same parameters, so autograd's AccumulateGrad adds ~900 parameter-sized
    tensors per time-step with one tiny launch each (rocprofv3 of the trainer's window, round 4: 540 one-block `add` launches per
    time-step, 1.8 ms of 52).  Inside `with fused_grad_accumulation():` the backward of every node in this file puts the gradients
    of its LEAF parameters here and returns None for them; on exit the T gradients of all parameters are summed with T - 1
    multi-tensor launches (`torch._foreach_add_`) and bound to `p.grad` (added to an existing one).  Same sums, in the order of
    the time-steps, as autograd's own accumulation."""
    active = None
    # TensorImpl id -> weak reference of the DerivedCache tensors registered as sink targets (non-leaf: flushed through autograd).  The id
    # alone is not enough: a cache dies with its model, and the address of a dead TensorImpl is handed to a later tensor - a plain set of
    # ids then declared unrelated derived tensors sink targets (their gradients went BOTH through the sink and through the main backward
    # pass: "backward through the graph a second time", seen only with several models in one process).
    proxy_ids = {}

    @staticmethod
    def is_proxy(t):
        r = _GradSink.proxy_ids.get(t._cdata)
        if r is None:
            return False
        o = r()
        return o is not None and o._cdata == t._cdata

    def __init__(self):
        self.items = {}      # TensorImpl id -> (parameter, [gradients in arrival order])

    def push(self, p, g):
        e = self.items.get(p._cdata)
        if e is None:
            self.items[p._cdata] = (p, [g])
        else:
            e[1].append(g)

    def flush(self):
        items = list(self.items.values())
        self.items = {}
        if not items:
            return
        with torch.no_grad():
            depth = max(len(gl) for _, gl in items)
            acc = [gl[0] if gl[0].is_contiguous() else gl[0].contiguous() for _, gl in items]
            for t in range(1, depth):
                idx = [i for i, (_, gl) in enumerate(items) if len(gl) > t]
                torch._foreach_add_([acc[i] for i in idx], [items[i][1][t] for i in idx])
            leaves = [(p, a) for (p, _), a in zip(items, acc) if p.is_leaf]
            old = [(p, a) for p, a in leaves if p.grad is not None]
            if old:
                torch._foreach_add_([p.grad for p, _ in old], [a for _, a in old])
            for p, a in leaves:
                if p.grad is None:
                    p.grad = a.view(p.shape) if a.shape != p.shape else a
        # derived tensors (DerivedCache proxies): their summed gradients go through the graph that built them, once
        der = [(p, a) for (p, _), a in zip(items, acc) if not p.is_leaf]
        if der:
            torch.autograd.backward([p for p, _ in der], [a.view(p.shape) if a.shape != p.shape else a for p, a in der])


class bptt_window:
    """Context of ONE BPTT window (reference trainFlowParallel.py:256-287): T forward passes on unchanged parameters followed by one
    backward pass.  Inside it the tensors derived from parameters alone are evaluated once (DerivedCache) and `backward(loss)` runs
    the backward pass with the parameter gradients summed by multi-tensor launches (fused_grad_accumulation).

        with tmg_ops.bptt_window() as win:
            for t in range(T): y, logp, states = model.sample(x[t], states); ...
            win.backward(loss)
    """

    def __enter__(self):
        DerivedCache.window_depth += 1
        return self

    def __exit__(self, et, ev, tb):
        DerivedCache.window_depth -= 1
        return False

    @staticmethod
    def backward(loss):
        with fused_grad_accumulation():
            loss.backward()


class fused_grad_accumulation:
    """Context for ONE backward pass (wrap `loss.backward()`): see _GradSink.  Not re-entrant; gradients reach `p.grad` on exit, i.e.
    before the gradient exchange / clipping / optimizer step.  Post-accumulate-grad hooks of the deferred parameters do not fire.
    The sink is process-wide (autograd evaluates the nodes on its own device thread, so a thread-local would not reach them): one
    training loop per process - the design's one process per GPU."""

    def __enter__(self):
        if _GradSink.active is not None:
            raise RuntimeError("fused_grad_accumulation is not re-entrant")
        _GradSink.active = _GradSink()
        return self

    def __exit__(self, et, ev, tb):
        sink, _GradSink.active = _GradSink.active, None
        if et is None:
            sink.flush()
        return False


def _defer(params, grads):
    """grads -> the tuple a node's backward returns for `params`: unchanged outside fused_grad_accumulation; inside it the gradients
    of leaf parameters go to the sink and None is returned in their place."""
    sink = _GradSink.active
    if sink is None:
        return tuple(grads)
    out = []
    for p, g in zip(params, grads):
        if g is not None and p is not None and p.requires_grad and (p.is_leaf or _GradSink.is_proxy(p)):
            sink.push(p, g)
            out.append(None)
        else:
            out.append(g)
    return tuple(out)


def _out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


class ConvFn(torch.autograd.Function):
    """y = [relu]((conv_k(pad(act(cat(inputs))), W) + b) * exp(clamp(kappa)))   (see tmg_conv_fwd)."""

    @staticmethod
    def forward(ctx, weight, bias, kappa, opts, *inputs):
        ksize, stride, relu_in, pad_rep, relu_out = opts[:5]
        inputs = tuple(t if t.stride(3) == 1 else t.contiguous() for t in inputs)
        B, Hin, Win, _ = inputs[0].shape
        Cout = weight.shape[0]
        Ho, Wo = _out_hw(Hin, Win, stride)
        out = empty((B, Ho, Wo, Cout), weight.device)
        if ksize == 3 and stride == 1 and kappa is None:
            H.conv3x3_auto(list(inputs), weight, Cout, [out], bias=bias, relu_in=relu_in, pad_rep=pad_rep, relu_out=relu_out)
        else:
            H.conv_fwd(list(inputs), H.conv_pack(weight, 0), Cout, ksize, stride, [out], bias=bias, kappa=kappa, relu_in=relu_in,
                       pad_rep=pad_rep, relu_out=relu_out)
        ctx.opts = opts
        ctx.n_in = len(inputs)
        ctx.has_bias = bias is not None
        ctx.has_kappa = kappa is not None
        ctx.save_for_backward(weight, bias, kappa, out if relu_out else None, *inputs)
        return out

    @staticmethod
    def backward(ctx, dout):
        ksize, stride, relu_in, pad_rep, relu_out = ctx.opts[:5]
        premasked = len(ctx.opts) > 5 and ctx.opts[5]
        weight, bias, kappa, out = ctx.saved_tensors[:4]
        inputs = ctx.saved_tensors[4:]
        if not H._pixel_linear(dout):       # (a channel slice of a wider gradient is addressed in place: pixel stride + offset)
            dout = dout.contiguous()
        if relu_out and not premasked:
            dy = torch.empty_like(dout)
            H.masked_add(dy, src=dout, ref=out)
        else:
            dy = dout
            if premasked and os.environ.get("TMG_CHECK_PREMASK"):
                leak = float((dout * (out <= 0)).abs().max())
                if leak != 0.0:
                    raise RuntimeError("ConvFn: _grad_premasked contract violated - the output gradient is non-zero (%.3e) where the "
                                       "ReLU output is zero: `out` has a consumer that does not mask its gradient" % leak)
        dW = db = dk = None
        if ctx.needs_input_grad[0] or ctx.has_kappa:
            dW = zeros_like(weight)
            db = zeros_like(bias) if ctx.has_bias else None
            if ctx.has_kappa:
                dk = zeros_like(kappa)
            # (weight gradients on a second stream beside the input-gradient kernels: measured three times - every weight gradient,
            # rounds 1 / 2; the wide levels' only, round 6, profiles/r6_ab_side_stream_wide_levels.txt - and slower each time)
            H.conv_wgrad(list(inputs), dy, dW, db, ksize, stride, kappa=kappa, relu_in=relu_in, pad_rep=pad_rep)
            if ctx.has_kappa:
                H.dkappa(weight, dW, bias if ctx.has_bias else weight[:0], db if ctx.has_bias else dW[:0], kappa, dk)
        dins = [None] * ctx.n_in
        if any(ctx.needs_input_grad[4:]):
            dins = [empty(t.shape, t.device) for t in inputs]
            if stride == 1:
                cin = sum(t.shape[3] for t in inputs)
                if ksize == 3 and kappa is None:
                    wpk_t = H.conv3x3_auto([dy], weight, cin, dins, dgrad=True)
                else:
                    wpk_t = H.conv_pack(weight, 1)
                    H.conv_fwd([dy], wpk_t, cin, ksize, 1, dins, kappa=kappa)
                if pad_rep and ksize == 3:
                    H.conv_rep_border_fix(dy, wpk_t if wpk_t is not None else H.conv_pack(weight, 1), dins, kappa=kappa)
            else:
                assert ctx.n_in == 1 and not ctx.has_kappa and not pad_rep
                Hin_, Win_ = inputs[0].shape[1], inputs[0].shape[2]
                if stride == 2 and ksize == 3 and Hin_ % 2 == 0 and Win_ % 2 == 0:
                    # stride-2 input gradient on the matrix cores: dx(i) = sum_k w[k] dy((i + 1 - k) / 2) over the even arguments
                    # = a stride-1 correlation with the flipped taps over dy spread onto the even positions of a zero grid
                    # (4x the minimal MFMA work, but these encoder convs have 8-32 channels: the scalar direct kernel spent
                    # 260 us per call at 0.12 TB/s on them)
                    up = empty((dy.shape[0], Hin_, Win_, dy.shape[3]), dy.device)
                    if not H.spread2(dy, up):
                        up.zero_()
                        up[:, ::2, ::2] = dy
                    H.conv_fwd([up], H.conv_pack(weight, 1), inputs[0].shape[3], ksize, 1, dins)
                else:
                    H.conv_dgrad_direct(dy, weight, dins[0], ksize, stride)
            if relu_in:
                for d, t in zip(dins, inputs):
                    H.masked_add(d, src=d, ref=t)
        return _defer((weight, bias, kappa), (dW, db, dk)) + (None,) + tuple(dins)


def conv(inputs, weight, bias=None, kappa=None, ksize=3, stride=1, relu_in=False, pad_rep=False, relu_out=False, _grad_premasked=False):
    """_grad_premasked (with relu_out) is PRIVATE to the ResidLSTMBlock -> CouplingTailFn(mode 1) pairing (nn/modules/convLSTM.py): the
    only consumer of the output is a node that applies relu to it and masks its input gradient by [out > 0], so the gradient arriving
    here is already zero wherever the output is and the backward pass skips its own mask pass - the same values, one full-tensor
    launch less.  A second consumer of `out` would get wrong gradients silently: TMG_CHECK_PREMASK=1 verifies the contract on every
    backward pass (one reduction + a host sync per call: a debugging switch)."""
    return ConvFn.apply(weight, bias, kappa, (ksize, stride, relu_in, pad_rep, relu_out, bool(_grad_premasked and relu_out)), *inputs)


class BNReLUConvFn(torch.autograd.Function):
    """y = conv3x3(relu(batchnorm(x)))  -- the encoder's dense layer (denseBlock.py:49-53), with the
    normalisation folded into the conv's input staging as a per-channel affine."""

    @staticmethod
    def forward(ctx, x, gamma, beta, weight, mean, rstd, a, bsh, training):
        # mean / rstd and the folded affine a = gamma*rstd, bsh = beta - mean*a come from bn_batch_stats (training: batch
        # moments, one fused kernel) or from the running moments (eval)
        x = x if x.stride(3) == 1 else x.contiguous()
        B, Hh, Ww, _ = x.shape
        Cout = weight.shape[0]
        out = empty((B, Hh, Ww, Cout), x.device)
        wpk = H.conv_pack(weight, 0)
        H.conv_fwd([x], wpk, Cout, 3, 1, [out], in_scale=a, in_shift=bsh, relu_in=True)
        ctx.training = training
        ctx.save_for_backward(x, gamma, weight, mean, rstd, a, bsh)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, gamma, weight, mean, rstd, a, bsh = ctx.saved_tensors
        dy = dout.contiguous()
        B, Hh, Ww, C = x.shape
        n = B * Hh * Ww
        dW = zeros_like(weight)
        H.conv_wgrad([x], dy, dW, None, 3, 1, in_scale=a, in_shift=bsh, relu_in=True)
        wpk_t = H.conv_pack(weight, 1)
        G = empty((B, Hh, Ww, C), x.device)
        H.conv_fwd([dy], wpk_t, C, 3, 1, [G])
        s = zeros((2, C), x.device)  # sums of du, du*xhat
        s0, s1 = s[0], s[1]
        H.chan_reduce(x, G, a, bsh, mean, rstd, s0, s1, 1)
        dgamma, dbeta = s1, s0
        dx = empty((B, Hh, Ww, C), x.device)
        if ctx.training:
            H.bn_bwd_apply(x, G, a, bsh, mean, rstd, gamma, s0, s1, dx, False, divisor=n)
        else:
            H.bn_bwd_apply(x, G, a, bsh, mean, rstd, gamma, None, None, dx, False)
        return (dx,) + _defer((gamma, None, weight), (dgamma, dbeta, dW)) + (None, None, None, None, None)


class DenseBlockFn(torch.autograd.Function):
    """All layers of an encoder dense block (reference denseBlock.py:69-100: x <- cat(x, conv3x3(relu(bn(x)))) per layer) as ONE node on
    ONE pre-sized buffer [B,H,W,c0 + sum(growth)]: every layer reads the channel prefix it sees and writes its new channels in place.
    The reference (and the per-layer path) re-concatenates the whole map per layer - on this device a `cat` launch per layer forward
    and a slice + add of a full-size gradient per layer backward; here the gradient of the buffer is accumulated in place
    (bn_bwd_apply with `accumulate`).  Arithmetic per layer = BNReLUConvFn's.

    inputs: x, the block's BatchNorm modules (running statistics are updated as nn.BatchNorm2d does), training flag, then per layer
    (gamma, beta, conv weight)."""

    @staticmethod
    def forward(ctx, x, bns, training, *params):
        L = len(bns)
        x = x if x.stride(3) == 1 else x.contiguous()
        B, Hh, Ww, c0 = x.shape
        growth = [params[3 * i + 2].shape[0] for i in range(L)]
        buf = empty((B, Hh, Ww, c0 + sum(growth)), x.device)
        H.masked_add(buf[..., :c0], src=x)
        # forward and input-gradient operands of all L layers in one launch per 16 (one pack launch per layer and direction otherwise)
        ws = [params[3 * i + 2].contiguous() for i in range(L)]
        packs = H.conv_pack_many([(w, 0) for w in ws] + [(w, 1) for w in ws])
        stats, use_batch, c = [], [], c0
        for i in range(L):
            gamma, beta, weight = params[3 * i:3 * i + 3]
            bn = bns[i]
            xin = buf[..., :c]
            use_batch.append(bool(training) or not bn.track_running_stats)
            if use_batch[-1]:
                mean, rstd, a, bsh = bn_batch_stats(xin, bn)
            else:
                mean = bn.running_mean
                rstd = torch.rsqrt(bn.running_var + bn.eps)
                a = gamma.detach() * rstd
                bsh = beta.detach() - mean * a
            H.conv_fwd([xin], packs[i], growth[i], 3, 1, [buf[..., c:c + growth[i]]], in_scale=a, in_shift=bsh, relu_in=True)
            stats.append((mean, rstd, a, bsh))
            c += growth[i]
        ctx.meta = (L, c0, growth, use_batch)
        ctx.stats = stats
        ctx.packs_t = packs[L:]
        ctx.save_for_backward(buf, *params)
        return buf

    @staticmethod
    def backward(ctx, dout):
        L, c0, growth, use_batch = ctx.meta
        if ctx.stats is None:
            raise RuntimeError("DenseBlockFn: the per-layer statistics were released by a previous backward pass "
                               "(a second backward through the same graph is not supported)")
        buf = ctx.saved_tensors[0]
        params = ctx.saved_tensors[1:]
        B, Hh, Ww, Ct = buf.shape
        n = B * Hh * Ww
        dbuf = dout.contiguous().clone()     # accumulated into in place below: never the caller's tensor
        grads = [None] * (3 * L)
        c = Ct
        for i in range(L - 1, -1, -1):
            gamma, beta, weight = params[3 * i:3 * i + 3]
            mean, rstd, a, bsh = ctx.stats[i]
            g = growth[i]
            c -= g
            xin, dy = buf[..., :c], dbuf[..., c:c + g]
            dW = zeros_like(weight)
            H.conv_wgrad([xin], dy, dW, None, 3, 1, in_scale=a, in_shift=bsh, relu_in=True)
            G = empty((B, Hh, Ww, c), buf.device)
            H.conv_fwd([dy], ctx.packs_t[i], c, 3, 1, [G])
            s = zeros((2, c), buf.device)   # sums of du, du*xhat
            H.chan_reduce(xin, G, a, bsh, mean, rstd, s[0], s[1], 1)
            if use_batch[i]:
                H.bn_bwd_apply(xin, G, a, bsh, mean, rstd, gamma, s[0], s[1], dbuf[..., :c], True, divisor=n)
            else:
                H.bn_bwd_apply(xin, G, a, bsh, mean, rstd, gamma, None, None, dbuf[..., :c], True)
            grads[3 * i:3 * i + 3] = [s[1], s[0], dW]
        ctx.stats = None
        ctx.packs_t = None
        return (dbuf[..., :c0], None, None) + _defer(params, grads)


def bn_batch_stats(x, bn):
    """Training-mode statistics of nn.BatchNorm2d `bn` on an NHWC tensor / channel-slice view: one-pass fp64 moments, then ONE kernel for mean, var, rstd, the folded affine and the momentum update of the running
    statistics (the ~15 element-wise torch ops this replaces were ~40 % of the step's small launches).
    -> (mean, rstd, a, bsh), each [C]."""
    B, Hh, Ww, C = x.shape
    n = B * Hh * Ww
    out = torch.empty((5, C), device=x.device)
    track = bn.track_running_stats
    mom = bn.momentum if bn.momentum is not None else 0.1
    with torch.no_grad():
        # one pass: sum and sum of squares in fp64 (no cancellation error in E[x^2] - E[x]^2), the activation is read once
        acc64 = zeros((4 * C,), x.device).view(torch.float64)     # [2][C] doubles out of the pooled zero buffer (256-byte aligned)
        H.chan_moments(x, acc64)
        nbt = bn.num_batches_tracked if (track and bn.num_batches_tracked is not None and bn.num_batches_tracked.device == x.device) else None
        H.bn_finalize64(acc64, bn.weight.detach(), bn.bias.detach(), bn.running_mean if track else None,
                        bn.running_var if track else None, out, n, bn.eps, mom, counter=nbt)
        if nbt is not None:
            track = False        # counted by the launch above
        if track and bn.num_batches_tracked is not None:
            bn.num_batches_tracked += 1
    return out[0], out[2], out[3], out[4]


def batch_moments(x):
    """Two-pass per-channel mean / biased variance over (B,H,W) of an NHWC tensor or channel-slice view."""
    B, Hh, Ww, C = x.shape
    n = B * Hh * Ww
    s0 = zeros(C, x.device)
    s1 = zeros(C, x.device)
    H.chan_reduce(x, None, None, None, None, None, s0, s1, 0)
    mean = s0 / n
    s0b = zeros(C, x.device)
    s1b = zeros(C, x.device)
    H.chan_reduce(x, None, mean, None, None, None, s0b, s1b, 0)
    return mean, s1b / n, n


class AffineFn(torch.autograd.Function):
    """Affine coupling on the second channel half + per-sample log-det (flowAffine.py:76-83 / :102-109)."""

    @staticmethod
    def forward(ctx, hh, x, reverse):
        x = x if x.stride(3) == 1 else x.contiguous()
        hh = hh.contiguous()
        B, Hh, Ww, C = x.shape
        ch = C // 2
        y = empty((B, Hh, Ww, C), x.device)
        H.masked_add(y[..., :ch], src=x[..., :ch])
        r = empty((B, Hh, Ww, ch), x.device)
        logdet = zeros(B, x.device)
        H.affine_apply(hh, x[..., ch:], y[..., ch:], r, logdet, reverse)
        ctx.reverse = reverse
        ctx.save_for_backward(r, x if reverse else y)
        return y, logdet

    @staticmethod
    def backward(ctx, dy, dld):
        r, ref = ctx.saved_tensors
        dy = dy.contiguous()
        B, Hh, Ww, C = dy.shape
        ch = C // 2
        dx = torch.empty_like(dy)
        H.masked_add(dx[..., :ch], src=dy[..., :ch])
        dhh = empty((B, Hh, Ww, C), dy.device)
        g = dld.contiguous() if dld is not None else None
        H.affine_bwd(dy[..., ch:], ref[..., ch:], r, g, dx[..., ch:], dhh, ctx.reverse)
        return dhh, dx, None


class LSTMPointwiseFn(torch.autograd.Function):
    """Gate activations and state update of the ConvLSTM cell (convLSTM.py:76-83)."""

    @staticmethod
    def forward(ctx, gates, c_prev):
        acts = gates.contiguous()       # read only; backward works on a copy
        B, Hh, Ww, R4 = acts.shape
        R = R4 // 4
        if c_prev is not None and c_prev.stride(3) != 1:
            c_prev = c_prev.contiguous()
        c_next = empty((B, Hh, Ww, R), acts.device)
        h_next = empty((B, Hh, Ww, R), acts.device)
        H.lstm_pointwise_fwd(acts, c_prev, c_next, h_next)
        ctx.has_c = c_prev is not None
        ctx.save_for_backward(acts, c_prev, c_next)
        return h_next, c_next

    @staticmethod
    def backward(ctx, dh, dc):
        acts, c_prev, c_next = ctx.saved_tensors
        dg = acts.clone()
        dc_prev = torch.empty_like(c_next)
        H.lstm_pointwise_bwd(dg, c_prev, c_next, dh.contiguous() if dh is not None else None,
                             dc.contiguous() if dc is not None else None, dc_prev)
        return dg, (dc_prev if ctx.has_c else None)


class ConvLSTMCellFn(torch.autograd.Function):
    """ConvLSTM cell as one node: gates = conv3x3(cat(inputs, h)) + b; i,f,o,g activations; c' = f c + i g; h' = o tanh(c')
    (reference convLSTM.py:72-85).  The 4R-wide gate tensor is kept as the conv wrote it (the activated gates are never
    stored: backward evaluates the activations again) and, in backward, overwritten in place by the pre-activation gradients, so
    the largest activation of the model exists once (no clones).  Consequently the node supports a single backward pass (no
    retain_graph double backward)."""

    @staticmethod
    def forward(ctx, weight, bias, h_cur, c_cur, *inputs):
        inputs = tuple(t if t.stride(3) == 1 else t.contiguous() for t in inputs)
        h_cur = h_cur if h_cur.stride(3) == 1 else h_cur.contiguous()
        if c_cur is not None and c_cur.stride(3) != 1:
            c_cur = c_cur.contiguous()
        B, Hh, Ww, _ = inputs[0].shape
        R4 = weight.shape[0]
        R = R4 // 4
        dev = weight.device
        gates = empty((B, Hh, Ww, R4), dev)
        segs = list(inputs) + [h_cur]
        # the widest contraction of the path (Cin + R -> 4R channels): Winograd F(2x2, 3x3) when the shape is in its envelope
        H.conv3x3_auto(segs, weight, R4, [gates], bias=bias)
        c_next = empty((B, Hh, Ww, R), dev)
        h_next = empty((B, Hh, Ww, R), dev)
        H.lstm_pointwise_fwd(gates, c_cur, c_next, h_next)
        ctx.n_in = len(inputs)
        ctx.has_c = c_cur is not None
        ctx.consumed = False
        ctx.save_for_backward(weight, bias, h_cur, c_cur, gates, c_next, *inputs)
        ctx.set_materialize_grads(False)     # an unused output (the cell state of the last time-step) sends None, not a zero tensor
        return h_next, c_next

    @staticmethod
    def backward(ctx, dh, dc):
        if ctx.consumed:
            raise RuntimeError("ConvLSTMCellFn: the gate buffer was consumed by a previous backward pass")
        ctx.consumed = True
        weight, bias, h_cur, c_cur, acts, c_next = ctx.saved_tensors[:6]
        inputs = ctx.saved_tensors[6:]
        # (weight, bias, h_cur, c_cur, *inputs): the previous cell state's gradient is only written when someone asks for it
        dc_prev = torch.empty_like(c_next) if (ctx.has_c and ctx.needs_input_grad[3]) else None
        H.lstm_pointwise_bwd(acts, c_cur, c_next, dh.contiguous() if dh is not None else None,
                             dc.contiguous() if dc is not None else None, dc_prev)
        dg = acts  # now the pre-activation gate gradients
        segs = list(inputs) + [h_cur]
        dW = zeros_like(weight)
        db = zeros_like(bias)
        nrest = sum(t.shape[3] for t in segs[:-1])
        if h_cur.shape[3] == 64 and 32 < nrest <= 48 and nrest % 4 == 0 and H.wino_wgrad_eligible(nrest, weight.shape[0]):
            # The Winograd weight-gradient kernel works on blocks of 64 (or 48) input channels: the 104 channels of the first level
            # as 64 + 64 carry 24 padding channels through the matrix cores.  Two launches - the recurrent state's 64 channels, and
            # (x1 | cond) as one 48-channel block - write disjoint column ranges of dW: 112 channels of work instead of 128.
            Cin = nrest + 64
            H.conv_wgrad(segs[:-1], dg, dW, db, 3, 1, cin_dst=Cin, cin_valid=nrest, ci_off0=0)
            H.conv_wgrad([h_cur], dg, dW, None, 3, 1, cin_dst=Cin, cin_valid=64, ci_off0=nrest)
        else:
            H.conv_wgrad(segs, dg, dW, db, 3, 1)
        # input gradients only for the channel prefix that needs them: the recurrent state of the first time-step of a
        # window (and any constant input) carries no gradient, which removes R of the Cin+R gradient channels
        need = [ctx.needs_input_grad[4 + i] for i in range(ctx.n_in)] + [ctx.needs_input_grad[2]]
        last = max([i for i, n in enumerate(need) if n], default=-1)
        dins = [None] * len(segs)
        if last >= 0:
            nch = sum(t.shape[3] for t in segs[:last + 1])
            dins[:last + 1] = [empty(t.shape, t.device) for t in segs[:last + 1]]
            H.conv3x3_auto([dg], weight, nch, dins[:last + 1], dgrad=True, nvalid=nch)
        return _defer((weight, bias), (dW, db)) + (dins[-1], dc_prev if ctx.has_c else None) + tuple(dins[:-1])


class GaussLogpFn(torch.autograd.Function):
    """log N(z2; mean, exp(lsd)) summed per sample, and eps = (z2-mean)/exp(lsd)  (flowUtils.py:176-192, :311)."""

    @staticmethod
    def forward(ctx, hz, z2, clip_mean, limits, want_eps):
        hz = hz.contiguous()
        z2 = z2 if z2.stride(3) == 1 else z2.contiguous()
        B = z2.shape[0]
        logp = zeros(B, z2.device)
        eps = empty(z2.shape, z2.device) if want_eps else None
        H.gauss_fwd(hz, z2, eps, logp, 0, clip_mean, limits)
        ctx.cfg = (clip_mean, limits)
        ctx.save_for_backward(hz, z2)
        ctx.mark_non_differentiable(*([eps] if want_eps else []))
        return logp, eps

    @staticmethod
    def backward(ctx, g, _geps):
        hz, z2 = ctx.saved_tensors
        clip_mean, limits = ctx.cfg
        dz2 = empty(z2.shape, z2.device)
        dhz = torch.empty_like(hz)
        H.gauss_bwd(hz, z2, None, g.contiguous(), dz2, dhz, 0, clip_mean, limits)
        return dhz, dz2, None, None, None


class GaussSampleFn(torch.autograd.Function):
    """z2 = mean + exp(lsd)*eps and its log-prob (flowUtils.py:194-209, :331-334)."""

    @staticmethod
    def forward(ctx, hz, eps, clip_mean, limits):
        hz = hz.contiguous()
        eps = eps.contiguous()
        B = eps.shape[0]
        logp = zeros(B, eps.device)
        z2 = empty(eps.shape, eps.device)
        H.gauss_fwd(hz, eps, z2, logp, 1, clip_mean, limits)
        ctx.cfg = (clip_mean, limits)
        ctx.save_for_backward(hz, eps)
        return z2, logp

    @staticmethod
    def backward(ctx, dz2, g):
        hz, eps = ctx.saved_tensors
        clip_mean, limits = ctx.cfg
        dhz = torch.empty_like(hz)
        H.gauss_bwd(hz, eps, dz2.contiguous() if dz2 is not None else None, g.contiguous() if g is not None else None, None, dhz, 1,
                    clip_mean, limits)
        return dhz, None, None, None


def latent_nonce(device):
    """Two int64 on `device` drawn from torch's generator of that device (ONE launch per model call): the key of the in-kernel Philox
    draws of every latent of the call (tmg_gauss_sample).  The latents therefore follow torch.manual_seed / get_rng_state /
    set_rng_state like torch.randn's would, and a hipGraph replay draws fresh ones (the generator's offset is graph-safe) - without a
    randn launch, an eps write and an eps read per level."""
    return torch.empty(2, dtype=torch.int64, device=device).random_()


def latent_nonces(device, k):
    """A [k, 2] int64 key table on `device` from ONE random_() launch: row m keys the in-kernel latent draws of member m of a folded
    ensemble call (TMGlow.sampleEnsemble, tmg_gauss_sample_keyed), as latent_nonce keys a single sample call."""
    return torch.empty((int(k), 2), dtype=torch.int64, device=device).random_()


class GaussDrawFn(torch.autograd.Function):
    """Split.reverse / GaussianDiag.sample on the HIP path as ONE launch: z2 = mean + exp(log-std) eps, written into the second half
    of the [B,h,w,2 Ch] tensor whose first half is z1 (the reference's torch.cat((z1, z2), 1), flowUtils.py:334; z1 None: the
    deepest prior, output [B,h,w,Ch]), with the log-prob per sample (:331-333).  eps given (reconstruct) or drawn in the kernel from
    (nonce, site) (sample, :206 / :328), or from a [K, 2] key table (table, site, rows_per_key): row b draws with key row
    b // rows_per_key (TMGlow.sampleEnsemble).  Gradients: d(hz) by tmg_gauss_bwd (mode 1), d(z1) = the first half of the output's
    gradient (a channel-slice view: no copy), none for eps."""

    @staticmethod
    def forward(ctx, hz, z1, eps, rng, clip_mean, limits):
        hz = hz if hz.stride(3) == 1 else hz.contiguous()
        B, Hh, Ww, C2 = hz.shape
        Ch = C2 // 2
        dev = hz.device
        if z1 is not None and z1.stride(3) != 1:
            z1 = z1.contiguous()
        out = empty((B, Hh, Ww, 2 * Ch if z1 is not None else Ch), dev)
        logp = zeros(B, dev)
        if eps is not None:
            eps = eps if eps.stride(3) == 1 else eps.contiguous()
            H.gauss_sample(hz, eps, z1, out, logp, clip_mean, limits)
        else:
            eps = empty((B, Hh, Ww, Ch), dev)
            if len(rng) == 3:
                table, site, rows_per_key = rng
                H.gauss_sample_keyed(hz, None, z1, out, logp, clip_mean, limits, table, rows_per_key, site=site, eps_out=eps)
            else:
                nonce, site = rng
                H.gauss_sample(hz, None, z1, out, logp, clip_mean, limits, eps_out=eps, nonce=nonce, site=site)
        ctx.cfg = (clip_mean, limits, Ch, z1 is not None)
        ctx.save_for_backward(hz, eps)
        ctx.set_materialize_grads(False)
        return out, logp

    @staticmethod
    def backward(ctx, dout, g):
        hz, eps = ctx.saved_tensors
        clip_mean, limits, Ch, has_z1 = ctx.cfg
        dhz = torch.empty_like(hz)
        dz2 = dz1 = None
        if dout is not None:
            dout = dout if dout.stride(3) == 1 else dout.contiguous()
            dz2 = dout[..., Ch:] if has_z1 else dout
            dz1 = dout[..., :Ch] if has_z1 else None
        H.gauss_bwd(hz, eps, dz2, g.contiguous() if g is not None else None, None, dhz, 1, clip_mean, limits)
        return dhz, dz1, None, None, None, None


class ReverseLossFn(torch.autograd.Function):
    """The benchmark loss of SURVEY 8-D, generative direction: mean(y^2) + mean(logdet) / (noc H W) as one reduction launch, its gradient
    as one element-wise launch (tmg_reverse_loss_*); y is the model's NCHW-shaped, channels-last output (any layout is accepted)."""

    @staticmethod
    def forward(ctx, y, logdet):
        H.check_act(y)
        yn = y.permute(0, 2, 3, 1)
        yn = yn if yn.is_contiguous() else yn.contiguous()
        ld = logdet.contiguous()
        n = yn.numel()
        loss = zeros(1, y.device)
        H.reverse_loss_fwd(yn, ld, loss, 1.0 / n, 1.0 / n)     # mean(ld) / (noc H W) = sum(ld) / (B noc H W) = sum(ld) / numel(y)
        ctx.save_for_backward(yn)
        ctx.B = ld.numel()
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        yn, = ctx.saved_tensors
        n = yn.numel()
        dyn = torch.empty_like(yn)
        dld = empty(ctx.B, yn.device)
        H.reverse_loss_bwd(yn, g.contiguous(), dyn, dld, 1.0 / n, 1.0 / n)
        return dyn.permute(0, 3, 1, 2), dld


def reverse_loss(y, logdet):
    """mean(y^2) + mean(logdet) / (noc H W) on the HIP path; tests/common.py::loss_reverse is the torch statement of it."""
    return ReverseLossFn.apply(y, logdet)


class SumTermsFn(torch.autograd.Function):
    """Sum of per-sample log-det terms ([B] vectors; one-element tensors are broadcast) in ONE launch - the reference adds them one `+`
    at a time (flowLSTMBlock.py:314-318, :345-359; tmGlow.py:438-440), ~25 one-block launches per step here.  Backward: the upstream
    gradient itself for a [B] term, its sum (one tiny launch, shared by all scalar terms of the node) for a broadcast one."""

    @staticmethod
    def forward(ctx, B, *terms):
        ts = [t.reshape(-1) if t.is_contiguous() else t.contiguous().reshape(-1) for t in terms]
        out = empty(B, ts[0].device)
        H.sum_terms(ts, out)
        ctx.meta = [(t.numel(), t.shape) for t in terms]
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gs = None
        outs = []
        for n, shape in ctx.meta:
            if n == g.numel() and len(shape) == 1:
                outs.append(g)
            elif n == 1:
                if gs is None:
                    gs = empty(1, g.device)
                    H.vec_sum(g, gs)
                outs.append(gs.view(shape))
            else:
                outs.append(g.view(shape))
        return (None,) + tuple(outs)


def sum_logdet(terms, B, device):
    """Sum of log-det contributions: python numbers and None are dropped (0), tensors of B elements or one element are summed by one
    launch per SUM_TERMS_MAX terms.  Returns 0. when nothing is left (the callers add it to a tensor or return it as is)."""
    ts = [t for t in terms if torch.is_tensor(t)]
    const = sum(float(t) for t in terms if t is not None and not torch.is_tensor(t))
    if const != 0.0:
        ts.append(torch.full((1,), const, device=device, dtype=torch.float32))
    if not ts:
        return 0.
    if len(ts) == 1 and ts[0].numel() == B and ts[0].dim() == 1:
        return ts[0]
    while len(ts) > 1 or ts[0].numel() != B:
        head, ts = ts[:H.SUM_TERMS_MAX], ts[H.SUM_TERMS_MAX:]
        ts.insert(0, SumTermsFn.apply(B, *head))
        if len(ts) == 1:
            break
    return ts[0]


class CheckerFn(torch.autograd.Function):
    """Checker squeeze (to_small) / un-squeeze (flowUtils.py:99-145)."""

    @staticmethod
    def forward(ctx, x, to_small):
        x = x if x.stride(3) == 1 else x.contiguous()
        B, Hh, Ww, C = x.shape
        if to_small:
            assert Hh % 2 == 0 and Ww % 2 == 0
            y = empty((B, Hh // 2, Ww // 2, 4 * C), x.device)
        else:
            assert C >= 4 and C % 4 == 0
            y = empty((B, Hh * 2, Ww * 2, C // 4), x.device)
        H.checker(x, y, to_small)
        ctx.to_small = to_small
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        B, Hh, Ww, C = dy.shape
        if ctx.to_small:
            dx = empty((B, Hh * 2, Ww * 2, C // 4), dy.device)
        else:
            dx = empty((B, Hh // 2, Ww // 2, 4 * C), dy.device)
        H.checker(dy, dx, not ctx.to_small)
        return dx, None


class PadHalvesFn(torch.autograd.Function):
    """compact [B,H,W,2 ch] <-> zero-padded halves [x1 | 0.. | x2 | 0..] (LSTMFLowBlock's layout for channel halves that are not a
    multiple of 4): one launch each way, its own adjoint with the direction swapped (the reference has no counterpart: it works on
    the un-padded tensors, flowAffine.py:73 / :98)."""

    @staticmethod
    def forward(ctx, x, ch, pad, to_padded):
        x = x if x.stride(3) == 1 else x.contiguous()
        B, Hh, Ww, _ = x.shape
        y = empty((B, Hh, Ww, 2 * (ch + pad) if to_padded else 2 * ch), x.device)
        H.pad_halves(x, y, ch, pad, to_padded)
        ctx.cfg = (ch, pad, to_padded)
        return y

    @staticmethod
    def backward(ctx, dy):
        ch, pad, to_padded = ctx.cfg
        dy = dy if dy.stride(3) == 1 else dy.contiguous()
        B, Hh, Ww, _ = dy.shape
        dx = empty((B, Hh, Ww, 2 * ch if to_padded else 2 * (ch + pad)), dy.device)
        H.pad_halves(dy, dx, ch, pad, not to_padded)
        return dx, None, None, None


class UpsampleFn(torch.autograd.Function):
    """Bilinear align_corners=True up-sampling by an integer factor (misc.py:34-35)."""

    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous()
        B, Hh, Ww, C = x.shape
        ho, wo = int(math.floor(Hh * scale)), int(math.floor(Ww * scale))
        y = empty((B, ho, wo, C), x.device)
        H.upsample_fwd(x, y)
        ctx.in_shape = (B, Hh, Ww, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        dx = empty(ctx.in_shape, dy.device)
        H.upsample_bwd(dy.contiguous(), dx)
        return dx, None


class CouplingTailFn(torch.autograd.Function):
    """Coupling network + affine apply as ONE autograd node with a hand-written backward:
        t0 = cat(nn inputs);  d1 = c1(relu(t0));  d2 = c1(relu(t0|d1));  hh = ZeroConv(relu(t0|d1|d2))
        y = [x1 | affine(x2; hh)],  logdet[b]
    (reference flowAffine.py:73-83 / :98-109 and :189-198 / :227-236).
    The two growth-1 layers run on the vector ALUs (tmg_c1_fwd / tmg_dense2_bwd), the zero-conv on the matrix
    cores; the concatenations are never built: the kernels read x1 / cond / D as segments, D being a 4-channel
    buffer (2 used) so every segment stays 16-byte aligned; weights are consumed in their native layout.
    Saved for backward: x, cond/feat, D, r, y -- not hh.

    mode 0: nn inputs = (x[..., :C/2], cond)      -- AffineCouplingLayer
    mode 1: nn inputs = (feat,)                   -- LSTMAffineCouplingLayer (feat = ResidLSTMBlock output)
    """

    @staticmethod
    def forward(ctx, x, aux, w1, w2, wz, bz, kappa, reverse, mode):
        x = x if x.stride(3) == 1 else x.contiguous()
        aux = aux if aux.stride(3) == 1 else aux.contiguous()
        B, Hh, Ww, C = x.shape
        ch = C // 2
        dev = x.device
        nn_in = [x[..., :ch], aux] if mode == 0 else [aux]
        cin = sum(t.shape[3] for t in nn_in)
        w1, w2, wz = w1.contiguous(), w2.contiguous(), wz.contiguous()
        D = empty((B, Hh, Ww, 4), dev)
        H.c1_fwd(nn_in, w1, D[..., 0:1], relu_in=True, fill4=True)   # writes (d1, 0, 0, 0)
        H.c1_fwd(nn_in + [D], w2, D[..., 1:2], relu_in=True, w_rows=cin + 1)
        hh = empty((B, Hh, Ww, C), dev)
        H.conv_fwd(nn_in + [D], H.conv_pack(wz, 0, cin + 4), C, 3, 1, [hh], bias=bz, kappa=kappa, relu_in=True, pad_rep=True)
        y = empty((B, Hh, Ww, C), dev)
        r = empty((B, Hh, Ww, ch), dev)
        logdet = zeros(B, dev)
        H.affine_apply(hh, x[..., ch:], y[..., ch:], r, logdet, reverse, x1=x[..., :ch], y1=y[..., :ch])   # pass-through half in the same launch
        ctx.reverse, ctx.mode, ctx.cin = reverse, mode, cin
        ctx.save_for_backward(x, aux, D, r, y, w1, w2, wz, bz, kappa)
        return y, logdet

    @staticmethod
    def backward(ctx, dy, dld):
        x, aux, D, r, y, w1, w2, wz, bz, kappa = ctx.saved_tensors
        reverse, mode, cin = ctx.reverse, ctx.mode, ctx.cin
        dy = dy.contiguous()
        B, Hh, Ww, C = dy.shape
        ch = C // 2
        dev = dy.device
        nn_in = [x[..., :ch], aux] if mode == 0 else [aux]
        # 1. affine
        dx = empty((B, Hh, Ww, C), dev)
        dhh = empty((B, Hh, Ww, C), dev)
        g = dld.contiguous() if dld is not None else None
        H.affine_bwd(dy[..., ch:], (x if reverse else y)[..., ch:], r, g, dx[..., ch:], dhh, reverse)
        # one zero-filled buffer for every parameter gradient of this node
        dw1, dw2, dwz, dbz, dk = carve(dev, (1, cin, 3, 3), (1, cin + 1, 3, 3), (C, cin + 2, 3, 3), (C,), kappa.shape)
        # 2. zero-conv weight / bias / scale gradients
        H.conv_wgrad(nn_in + [D], dhh, dwz, dbz, 3, 1, kappa=kappa, relu_in=True, pad_rep=True, cin_dst=cin + 2)
        H.dkappa(wz, dwz, bz, dbz, kappa, dk)
        G = [empty(t.shape, dev) for t in nn_in]
        GD = empty((B, Hh, Ww, 4), dev)
        wz_t = H.conv_pack(wz, 1, cin + 4)
        H.conv_fwd([dhh], wz_t, cin + 4, 3, 1, G + [GD], kappa=kappa)
        H.conv_rep_border_fix(dhh, wz_t, G + [GD], kappa=kappa)
        # 3. both growth-1 layers, ReLU masks and the concat adjoint in one pass over the network input
        if mode == 0:
            H.dense2_bwd(nn_in + [D], w1, w2, dw1, dw2, GD, D, G, [dx[..., :ch], G[1]], cin, add0=dy[..., :ch], rows1=cin, rows2=cin + 1)
            daux = G[1]
        else:
            H.dense2_bwd(nn_in + [D], w1, w2, dw1, dw2, GD, D, G, [G[0]], cin, rows1=cin, rows2=cin + 1)
            H.masked_add(dx[..., :ch], src=dy[..., :ch])
            daux = G[0]
        return (dx, daux) + _defer((w1, w2, wz, bz, kappa), (dw1, dw2, dwz, dbz, dk)) + (None, None)


# Arithmetic of the 1x1 channel mixes (ActNorm folded into the invertible 1x1 conv, glowConv.py:193-194 / :219-220):
# "f32" (default) = fp32 MFMA; "f16" = fp16 operands, fp32 accumulation (tmg_mix_f16), forward and input gradient - the variant
# BASELINE.json configs[4] names.  Explicit opt-in: set_mix_precision("f16") or TMG_MIX_F16=1.  Round 6: "f16" applies wherever the
# mix is a LAUNCH OF ITS OWN - the LSTM coupling block of every level, every layer of a level wider than 128 channels (cfg5's 256),
# the density direction's per-layer mixes.  Inside the fused coupling kernels of the generative direction (cpl_fwd / cpl_bwd at
# 16 / 32 channels, mix32<AFF> at 64 / 128) the mix is a second MFMA contraction on the coupling's accumulator registers and stays
# fp32: rounds 2-5 switched those kernels OFF under "f16" and ran the per-op chain instead, which is why the fp16 line was SLOWER
# (0.89-0.94x).  The kernels are bandwidth-bound on fp32 activations either way (8 C bytes per pixel): 2-byte operands cannot buy more
# than the conversion costs (profiles/r6_mix_f16_vs_f32.txt).  Weight gradients stay fp32 in both modes.  The
# deviation of "f16" from "f32" is reported by tests/test_model_parity.py, separately from the fp32 parity tolerances.
_MIX_PRECISION = "f16" if os.environ.get("TMG_MIX_F16") else "f32"


def set_mix_precision(kind):
    global _MIX_PRECISION
    if kind not in ("f32", "f16"):
        raise ValueError("mix precision must be 'f32' or 'f16', got %r" % (kind,))
    _MIX_PRECISION = kind


def mix_precision():
    return _MIX_PRECISION


# Recompute-from-output ("memory-free") backward of the plain coupling layers (invertibility of the reference's
# flowAffine.py:85-109 / flowLSTMBlock.py:323-361).  Off by default: it trades time for capacity.
_RECOMPUTE = [bool(os.environ.get("TMG_RECOMPUTE"))]


def set_recompute(on):
    """True: the level nodes of the narrow flow levels (C <= 32, generative direction) keep NO per-layer activations - backward rebuilds
    every layer's input from its output (inverse channel mix -> coupling network -> x2 = (y2 + shift) e^{sg}) - so that a 10-step BPTT
    window's memory is no longer ~2 C + 4 floats per pixel, layer and time-step.  Slower per step (one more forward pass through those
    layers inside backward); same gradients up to fp32 rounding of the reconstruction."""
    _RECOMPUTE[0] = bool(on)


def recompute():
    return _RECOMPUTE[0]


def set_winograd_precision(kind):
    """Arithmetic of the wide Winograd contractions (ConvLSTM gate conv, level-wide conditioning conv, out-conv input gradient):
    "f32" = fp32 MFMA (default); "bf16x3" = the bf16 matrix pipe at fp32 accuracy (tmg_hip.conv_wino_fwd3; opt-in, round 5)."""
    H.set_winograd_precision(kind)


def winograd_precision():
    return H.winograd_precision()


def _mix16_ok(C):
    return _MIX_PRECISION == "f16" and C % 4 == 0 and C <= 256


def _mix_fwd(x, Wk, bk, packed=None):
    """y = Wk x + bk per pixel (ActNorm folded into the invertible 1x1 conv).  packed: Wk already in operand order."""
    C = Wk.shape[0]
    y = empty(x.shape, x.device)
    if _mix16_ok(C):
        H.mix_f16(x, Wk.contiguous(), bk, y)
        return y
    if x.stride(3) == 1 and H.mix_f32(x, Wk.contiguous(), bk, y):
        return y
    H.conv_fwd([x], packed if packed is not None else H.conv_pack(Wk.reshape(C, C, 1, 1), 0), C, 1, 1, [y], bias=bk)
    return y


class MixFn(torch.autograd.Function):
    """y = W x + b per pixel as one node in the selected mix precision (used by the blocks outside the level-fused node)."""

    @staticmethod
    def forward(ctx, x, W, b):
        x = x if x.stride(3) == 1 else x.contiguous()
        ctx.save_for_backward(x, W)
        ctx.has_b = b is not None
        return _mix_fwd(x, W.detach(), b.detach() if b is not None else None)

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        C = W.shape[0]
        dW = zeros_like(W)
        db = zeros(C, W.device)
        dx = _mix_bwd(x, dy, W, dW, db)
        return dx, dW, (db if ctx.has_b else None)


def _mix_dgrad(dy, Wk, packed_t=None):
    """Input gradient of _mix_fwd."""
    C = Wk.shape[0]
    dx = empty(dy.shape, dy.device)
    if _mix16_ok(C):
        H.mix_f16(dy, Wk.contiguous(), None, dx, transposed=True)
    elif not H.mix_f32(dy, Wk.contiguous(), None, dx, transposed=True):
        H.conv_fwd([dy], packed_t if packed_t is not None else H.conv_pack(Wk.reshape(C, C, 1, 1), 1), C, 1, 1, [dx])
    return dx


def _mix_bwd(x, dy, Wk, dWk, dbk):
    """Input gradient of _mix_fwd (returned) and weight / bias gradients (accumulated into dWk [C,C], dbk [C])."""
    dx = _mix_dgrad(dy, Wk)
    H.conv_wgrad([x], dy, dWk, dbk, 1, 1)
    return dx


# One flow level as LevelCouplingFn sees it (built once per forward pass and carried on ctx); w1s .. kps: (w1, w2, wz, bz, kappa) per layer
_Level = collections.namedtuple("_Level", "NL NLp C ch Cc cin reverse fuse split rec w1s w2s wzs bzs kps")
# What the per-layer steps of LevelCouplingFn.backward share (see there)
_LevelBwd = collections.namedtuple("_LevelBwd", "g Wm PZt PMt DH DD quad_last grouped zc_kw wg_in mix_wg dWz dBz dW1 dW2 dWm dbm DDp")


def _level(wts, C, Cc, reverse):
    NL = len(wts) // 5
    ch = C // 2
    fuse = 8 <= C <= 32 and ch % 4 == 0 and all(w.is_contiguous() for w in wts)     # narrow levels: see LevelCouplingFn._fwd_fused
    # Split-halves layout (round 4; generative direction on the levels whose per-layer kernels are bandwidth-bound): between
    # the layers of the node an activation lives as TWO [B,h,w,C/2] tensors (x1, x2) instead of one [B,h,w,C].  The kernels
    # that read x1 alone - growth layers, their backward, three weight gradients - then use every byte of the lines they
    # fetch (a 64-byte pixel of the 16-channel level shares its 128-byte line with the neighbour's other half), and the fused
    # coupling kernel's x1 patch loads and x2 epilogue loads no longer pull each other's half-used lines through L2 twice.
    # The node's input and output stay single tensors (addressed as two channel-slice views).
    split = fuse and reverse and C in (16, 32)
    # Recompute mode (set_recompute; narrow levels, generative direction - where ~80 % of the per-layer activations of the model
    # live): nothing per layer is kept; backward rebuilds layer k's input from its output (see _rebuild)
    rec = _RECOMPUTE[0] and fuse and reverse and C <= 64
    return _Level(NL, (NL + 3) // 4 * 4, C, ch, Cc, ch + Cc, reverse, fuse, split, rec,
                  wts[0::5], wts[1::5], wts[2::5], wts[3::5], wts[4::5])


class LevelCouplingFn(torch.autograd.Function):
    """All NL non-LSTM coupling blocks of one flow level (reference flowLSTMBlock.py:260-270: layers 1..K-1) as ONE
    autograd node with a hand-written backward.

    Besides removing ~100 autograd nodes per level, the node restructures the arithmetic around one observation:
    every coupling network of the level sees the SAME conditioning map, and a convolution is linear in its input
    channels, so conv(relu(cat(x1, cond, d))) = conv_x(relu(x1, d)) + conv_c(relu(cond)).  The cond parts of all NL
    zero-convs (and of the 2*NL growth-1 layers) are therefore computed ONCE per level as a single wide contraction
    (N = NL*C output channels: the regime where the fp32 MFMA kernel runs at >100 TFLOP/s) and injected into the
    per-layer kernels as an additive input; per-layer kernels only touch x1 | D (C/2+4 channels instead of C/2+Cc+4).
    Backward mirrors it: per-layer kernels produce the x1 / D gradients and stash exp(kappa)*dhh and (dd1, dd2) in
    level-wide buffers; after the last layer ONE input-gradient contraction gives d(cond) (no 16-fold accumulation)
    and ONE weight-gradient contraction writes the cond slices of all NL weight gradients in place.

    inputs: x [B,h,w,C], cond [B,h,w,Cc], Wm [NL,C,C], bm [NL,C] (folded ActNorm + 1x1 per layer, built by
    LSTMFLowBlock._level_mix with autograd), reverse, then (w1, w2, wz, bz, kappa) per layer in layer order.
    outputs: y, logdet [B] (sum of the NL coupling log-dets).

    L: the level (_Level); S: what the steps of backward share (_LevelBwd).  A per-layer step is a call of its own: the layer's tensors
    are unreferenced when it returns, before the next layer's buffers are allocated.
    """

    @staticmethod
    def _cond_parts(L, cond, Wcat):
        """The conditioning map's share of all NL zero convs (Hc) and of the 2 NL growth layers (Dc; dc_of(k) = layer k's two addends)."""
        bhw, dev = cond.shape[:3], cond.device
        Wzc, Wdc = Wcat[:L.NL * L.C], Wcat[L.NL * L.C:]
        Hc = empty(bhw + (L.NL * L.C,), dev)
        H.conv3x3_auto([cond], Wzc, L.NL * L.C, [Hc], relu_in=True, pad_rep=True)
        Dc = empty(bhw + (2 * L.NLp,), dev)
        H.conv_fwd([cond], H.conv_pack(Wdc, 0), 2 * L.NLp, 3, 1, [Dc], relu_in=True)
        if math.prod(bhw) >= int(os.environ.get("TMG_LAYER_PLANES_MIN", 1 << 17)):
            # large images: one float2 plane per layer (every layer reads its addends for every pixel - out of the interleaved
            # tensor that is a full cache line per pixel, more than the growth kernels' real input)
            Dc = H.layer_planes(Dc)
            dc_of = lambda k: (Dc[k][..., 0:1], Dc[k][..., 1:2])  # noqa: E731
        else:
            dc_of = lambda k: (Dc[..., 2 * k:2 * k + 1], Dc[..., 2 * k + 1:2 * k + 2])  # noqa: E731
        return Hc, Dc, dc_of

    @staticmethod
    def _level_operands(L, dev):
        """(Wz [NL,C,cin+2,3,3] = stack of the zero-conv weights, Wcat = [Wzc ; Wdc] with Wzc [NL C,Cc,3,3] the conditioning columns
        of all zero convs and Wdc [2 NLp,Cc,3,3] those of the growth layers - output channel 2k / 2k+1 = growth layer 1 / 2 of coupling
        layer k: a layer's two addends share one cache line of Dc -, Bz [NL,C], Kp [NL]) through tmg_level_pack: one launch reading the
        modules' tensors through a device pointer table (round 5: ~10 stack / slice-copy / cat launches per level and direction)."""
        NL, NLp, C, ch, Cc, cin = L[:6]
        layers = list(zip(L.w1s, L.w2s, L.wzs, L.bzs, L.kps))
        Wz = empty((NL, C, cin + 2, 3, 3), dev)
        Wcat = empty((NL * C + 2 * NLp, Cc, 3, 3), dev)
        Bz = empty((NL, C), dev)
        Kp = empty(NL, dev)
        if all(w.is_contiguous() and w.dtype == torch.float32 for ws in layers for w in ws) and os.environ.get("TMG_NO_LEVEL_PACK") is None:
            tab = H._segment_table([[w.data_ptr() for w in ws] for ws in layers], dev)
            H.level_pack(tab, Wz, Wcat, Bz, Kp, NL, NLp, C, ch, Cc)
            return Wz, Wcat, Bz, Kp
        torch.stack(L.wzs, out=Wz)
        Wcat[:NL * C] = Wz[:, :, ch:cin].reshape(NL * C, Cc, 3, 3)
        Wdc = Wcat[NL * C:].view(NLp, 2, Cc, 3, 3)
        Wdc[NL:].zero_()
        Wdc[:NL, 0] = torch.stack(L.w1s)[:, 0, ch:cin]
        Wdc[:NL, 1] = torch.stack(L.w2s)[:, 0, ch:cin]
        torch.stack(L.bzs, out=Bz)
        torch.stack([kp.reshape(()) for kp in L.kps], out=Kp)
        return Wz, Wcat, Bz, Kp

    @staticmethod
    def _growth(L, k, x1, dc_of):
        """D = (d1, d2, 0, 0) [B,h,w,4]: both growth-1 layers of layer k in one launch (the conditioning parts arrive as add operands)."""
        D = empty(x1.shape[:3] + (4,), x1.device)
        add1, add2 = dc_of(k)
        H.c1x2_fwd([x1], L.w1s[k], L.w2s[k], D, w_rows=L.ch, w2_d1_row=L.cin, add1=add1, add2=add2)
        return D

    @staticmethod
    def _fwd_fused(L, k, cur, Wm, bm, PM, Hc, dc_of, logdet):
        """Layer k of a narrow level -> (its output, what backward keeps of it): zero conv, coupling, log-det and - in the generative
        direction - the following channel mix are ONE launch (tmg_coupling_fwd) after the growth layers' launch."""
        C, ch, reverse = L.C, L.ch, L.reverse
        bhw, dev = Hc.shape[:3], Hc.device
        tin = cur if reverse else _mix_fwd(cur, Wm[k], bm[k], PM[k])
        t1 = H._halves(tin)[0]
        D = LevelCouplingFn._growth(L, k, t1, dc_of)
        if L.split and k != 0:     # (k = 0 is the node's last layer in this direction: its output is the node's)
            out = (empty(bhw + (ch,), dev), empty(bhw + (ch,), dev))
        else:
            out = empty(bhw + (C,), dev)
        r = empty(bhw + (ch,), dev)
        y2 = empty(bhw + (ch,), dev) if reverse else None
        ok = H.coupling_fwd(tin, out, r, y2, D, Hc[..., k * C:(k + 1) * C], L.wzs[k], L.bzs[k], L.kps[k], Wm[k] if reverse else None,
                            bm[k] if reverse else None, logdet, reverse, L.cin)
        assert ok
        if L.rec:
            return out, None
        # the coupling output y: reverse -> (x1 of the input, y2) as two segments (never materialised), forward -> out
        return out, ((tin, D, r, [t1, y2]) if reverse else (tin, D, r, out, cur))

    @staticmethod
    def _fwd_wide(L, k, cur, Wm, bm, PM, PZ, Hc, dc_of, logdet, mixaff):
        """Layer k of a wide level -> (its output, what backward keeps of it): one launch per op."""
        C, ch, reverse = L.C, L.ch, L.reverse
        bhw, dev = Hc.shape[:3], Hc.device
        tin = cur if reverse else _mix_fwd(cur, Wm[k], bm[k], PM[k])
        x1 = tin[..., :ch]
        if ch % 4 == 0:
            D = LevelCouplingFn._growth(L, k, x1, dc_of)
        else:
            D = empty(bhw + (4,), dev)
            add1, add2 = dc_of(k)
            H.c1_fwd([x1], L.w1s[k], D[..., 0:1], relu_in=True, w_rows=ch, fill4=True, add=add1)
            H.c1_fwd([x1, D], L.w2s[k], D[..., 1:2], relu_in=True, w_rows=ch + 1, w_split=ch, w_gap=L.Cc, add=add2)
        hh = empty(bhw + (C,), dev)
        H.conv_fwd([x1, D], PZ[k], C, 3, 1, [hh], bias=L.bzs[k], kappa=L.kps[k], relu_in=True, pad_rep=True, add=Hc[..., k * C:(k + 1) * C])
        r = empty(bhw + (ch,), dev)
        if mixaff:
            # 64- / 128-channel levels, generative direction: coupling + trailing mix in ONE launch (the coupling is evaluated on
            # the mix kernel's way in); the coupling output is kept as (x1 of the input, y2), never as a [.., C] tensor
            y2 = empty(bhw + (ch,), dev)
            out = empty(bhw + (C,), dev)
            if H.mix_affine_fwd(tin, hh, Wm[k], bm[k], out, r, y2, logdet):
                return out, (tin, D, r, [x1, y2])
        y = empty(bhw + (C,), dev)
        H.affine_apply(hh, tin[..., ch:], y[..., ch:], r, logdet, reverse, x1=x1, y1=y[..., :ch])
        return (_mix_fwd(y, Wm[k], bm[k], PM[k]) if reverse else y), (tin, D, r, y) + (() if reverse else (cur,))

    @staticmethod
    def forward(ctx, x, cond, Wm, bm, reverse, *wts):
        x = x if x.stride(3) == 1 else x.contiguous()
        cond = cond.contiguous()
        L = _level(wts, x.shape[3], cond.shape[3], reverse)
        NL, C, ch = L.NL, L.C, L.ch
        dev = x.device
        # parameter-side operands of the whole level (parameter-sized copies, no autograd inside a Function): ONE gather launch
        Wz, Wcat, Bz, Kp = LevelCouplingFn._level_operands(L, dev)
        Hc, Dc, dc_of = LevelCouplingFn._cond_parts(L, cond, Wcat)
        logdet = zeros(x.shape[0], dev)
        # operand packing of every layer's weights in two launches per level instead of two per layer
        PZ = H.conv_pack_batched(Wz, 0, ch + 4, (ch + 2, ch, L.Cc))
        PM = H.conv_pack_batched(Wm.reshape(NL, C, C, 1, 1), 0)
        mixaff = (reverse and C in (64, 128) and Wm.is_contiguous() and bm.is_contiguous()
                  and os.environ.get("TMG_NO_MIX_AFFINE") is None)
        saved = [None] * NL
        cur = x
        for k in (range(NL - 1, -1, -1) if reverse else range(NL)):
            if L.fuse:
                cur, saved[k] = LevelCouplingFn._fwd_fused(L, k, cur, Wm, bm, PM, Hc, dc_of, logdet)
            else:
                cur, saved[k] = LevelCouplingFn._fwd_wide(L, k, cur, Wm, bm, PM, PZ, Hc, dc_of, logdet, mixaff)
        del Hc, Dc
        # the per-layer activations are module-owned buffers freed layer by layer during backward, hence a plain attribute
        # instead of save_for_backward; the node hands out a VIEW of its last buffer, so the returned tensor (which owns the
        # grad_fn -> ctx reference) is not itself an element of `saved`: no reference cycle when backward never runs
        ctx.saved = saved
        ctx.rec_out = cur if L.rec else None      # (recompute mode: the node's own output buffer is all that backward starts from)
        ctx.level = L
        ctx.save_for_backward(cond, Wm, bm, Wz, Wcat, Bz, Kp, *wts)
        return cur.view(cur.shape), logdet

    @staticmethod
    def _rebuild(L, R, k):
        """Recompute mode: layer k's activations (tin, D, r, y) from its output R[-1].  The generative layer k maps tin = [x1 | x2] to
        out = Wm_k [x1; y2] + bm_k with y2 = x2 e^{-sg} - shift and (shift, sg) functions of x1 and the conditioning map alone
        (flowAffine.py:102-109, glowConv.py:207-222).  So from out:
          [x1; y2] = Wm_k^-1 (out - bm_k)                       one 1x1 mix with the inverse (tmg_mat_inverse: fp64, rounded once)
          D        = growth layers of x1                         tmg_c1x2_fwd, as in the forward pass
          x2       = (y2 + shift) e^{sg},  r                     tmg_coupling_fwd in its density-direction form, no trailing mix
        and the layer's input is the previous layer's output: R[-1] on return.  The rest of R: the conditioning shares Hc / Dc of the
        level, evaluated again, the inverse mixes and a log-det nobody reads."""
        Hc, dc_of, Winv, binv, ld_dummy, out = R
        C, ch = L.C, L.ch
        u = _mix_fwd(out, Winv[k], binv[k])
        t1 = u[..., :ch]
        D = LevelCouplingFn._growth(L, k, t1, dc_of)
        tin = empty(u.shape, u.device)
        r = empty(t1.shape, u.device)
        ok = H.coupling_fwd(u, tin, r, None, D, Hc[..., k * C:(k + 1) * C], L.wzs[k], L.bzs[k], L.kps[k], None, None, ld_dummy, False, L.cin)
        assert ok
        R[-1] = tin
        return tin, D, r, [t1, u[..., ch:]]

    @staticmethod
    def _zero_conv_wgrad(L, S, k, x1D, now=False):
        """Weight / bias gradient of layer k's zero conv (its x1 | D columns; upstream = the layer's slice of DH): one launch, or -
        grouped, unless `now` - the inputs recorded for the level's grouped launch, whose per-layer fallback this is too."""
        if S.grouped and not now:
            S.wg_in[k] = x1D
        else:
            H.conv_wgrad(x1D, S.DH[..., k * L.C:(k + 1) * L.C], S.dWz[k], S.dBz[k], 3, 1, **S.zc_kw)

    @staticmethod
    def _mix_wgrad(L, S, k, x, dy, now=False):
        """Weight / bias gradient of layer k's 1x1 mix (x: its input, a tensor or channel segments; dy: the upstream gradient, a tensor
        or two halves): one launch, or - grouped, unless `now` - the pair recorded for the level's grouped launch."""
        x = x if isinstance(x, list) else [x]
        if S.grouped and not now:
            S.mix_wg[k] = (x, dy)
        else:
            H.conv_wgrad(x, dy if torch.is_tensor(dy) else torch.cat(list(dy), 3), S.dWm[k], S.dbm[k], 1, 1)

    @staticmethod
    def _layer_mix_bwd(L, S, k, x, dy):
        """Backward of layer k's 1x1 mix on its own: the input gradient (returned), then the weight gradient (now or recorded)."""
        dx = _mix_dgrad(dy, S.Wm[k], S.PMt[k])
        LevelCouplingFn._mix_wgrad(L, S, k, x, dy)
        return dx

    @staticmethod
    def _growth_bwd(L, S, k, x1, D, G0, GD, dt1, add0):
        """Both growth-1 layers' backward, ReLU masks and the concat adjoint of layer k in one launch: dt1 (the first half of the
        layer-input gradient) = add0 (the pass-through half of the coupling's gradient) + G0 + the growth layers' share; (dd1, dd2)
        go to the layer's channels of DD; the x1 | d1 weight-gradient rows here unless the level's grouped launch writes them.
        G0 None: dt1 already holds add0 + [x1 > 0] G0 and GD the mask bits (the coupling backward's summed form): read and completed
        in place."""
        ch = L.ch
        dW1, dW2 = (None, None) if S.grouped else (S.dW1[k], S.dW2[k])
        summed = G0 is None
        if S.DDp is not None:     # large levels: the layer's own float2 plane (pixel stride 2)
            dd1, dd2, quad = S.DDp[k][..., 0:1], S.DDp[k][..., 1:2], False
        else:
            dd1, dd2, quad = S.DD[..., 2 * k:2 * k + 1], S.DD[..., 2 * k + 1:2 * k + 2], S.quad_last and k == L.NL - 1
        H.dense2_bwd([x1, D], L.w1s[k], L.w2s[k], dW1, dW2, GD, D, [dt1 if summed else G0], [dt1], ch, add0=None if summed else add0,
                     rows1=ch, rows2=ch + 1, split2=ch, gap2=L.Cc, dd1=dd1, dd2=dd2, dd_quad=quad, g0_masked=summed)

    @staticmethod
    def _bwd_fused_generative(L, S, k, dcur, tin, D, r, y):
        """Narrow level, generative direction (coupling -> mix) -> gradient w.r.t. the layer's input.
        One launch: mix input gradient -> coupling backward -> zero-conv input gradient (exact replicate adjoint)."""
        C, ch = L.C, L.ch
        bhw, dev = D.shape[:3], D.device
        if L.split and k != L.NL - 1:    # gradient w.r.t. a layer input that lives as two halves: the same layout
            dtin = (empty(bhw + (ch,), dev), empty(bhw + (ch,), dev))
        else:                            # (k = NL - 1: the node's own input gradient)
            dtin = empty(bhw + (C,), dev)
        # (the summed form - no G0 tensor - needs the growth backward without weight gradients: the grouped level)
        G0, GD = None if S.grouped else empty(bhw + (ch,), dev), empty(bhw + (4,), dev)
        dhh = S.DH[..., k * C:(k + 1) * C]
        x1, x2 = H._halves(tin)
        dt1 = H._halves(dtin)[0]
        ok = H.coupling_bwd(dcur, x2, r, S.g, S.Wm[k].contiguous(), L.wzs[k], L.kps[k], dhh, dtin, G0, GD, L.cin,
                            x1=x1 if G0 is None else None)
        assert ok
        LevelCouplingFn._zero_conv_wgrad(L, S, k, [x1, D])
        LevelCouplingFn._mix_wgrad(L, S, k, y, dcur)
        LevelCouplingFn._growth_bwd(L, S, k, x1, D, G0, GD, dt1, dt1)
        return dtin

    @staticmethod
    def _bwd_fused_density(L, S, k, dcur, tin, D, r, y, xin):
        """Narrow level, density direction (mix -> coupling) -> gradient w.r.t. the layer's input.
        Coupling backward + zero-conv input gradient in one launch (tmg_coupling_bwd in its `fwd` mode: the gradient arrives at the
        coupling output itself), then the growth layers' backward, then the input gradient of the leading mix (round 4: this
        direction ran affine_bwd + conv dgrad + border fold per layer before)."""
        C, ch = L.C, L.ch
        bhw, dev = D.shape[:3], D.device
        dtin = empty(bhw + (C,), dev)
        G0, GD = None if S.grouped else empty(bhw + (ch,), dev), empty(bhw + (4,), dev)
        dhh = S.DH[..., k * C:(k + 1) * C]
        x1, dt1 = tin[..., :ch], dtin[..., :ch]
        ok = H.coupling_bwd(dcur, y[..., ch:], r, S.g, S.Wm[k].contiguous(), L.wzs[k], L.kps[k], dhh, dtin, G0, GD, L.cin, fwd=True,
                            x1=x1 if G0 is None else None)
        assert ok
        LevelCouplingFn._zero_conv_wgrad(L, S, k, [x1, D])
        LevelCouplingFn._growth_bwd(L, S, k, x1, D, G0, GD, dt1, dt1)
        return LevelCouplingFn._layer_mix_bwd(L, S, k, xin, dtin)

    @staticmethod
    def _bwd_wide(L, S, k, dcur, tin, D, r, y, xin=None):
        """Wide level, either direction -> gradient w.r.t. the layer's input: one launch per op."""
        C, ch, reverse = L.C, L.ch, L.reverse
        bhw, dev = D.shape[:3], D.device
        dtin = empty(bhw + (C,), dev)        # grad w.r.t. the tail input
        dhh = S.DH[..., k * C:(k + 1) * C]
        add0 = None
        if reverse and isinstance(y, list) and C in (64, 128):
            # the forward pass took the fused coupling + mix launch: its backward in one launch too (mix input gradient with the
            # coupling's backward on the way out); dto1 = the pass-through half of the gradient, completed by dense2_bwd below
            dto1 = empty(bhw + (ch,), dev)
            if H.mix_affine_bwd(dcur, S.Wm[k].contiguous(), r, tin[..., ch:], S.g, L.kps[k], dto1, dtin[..., ch:], dhh):
                add0 = dto1
                LevelCouplingFn._mix_wgrad(L, S, k, y, dcur)
        if add0 is None:
            dto = LevelCouplingFn._layer_mix_bwd(L, S, k, y, dcur) if reverse else dcur   # grad w.r.t. the tail output y
            H.affine_bwd(dto[..., ch:], (tin if reverse else y)[..., ch:], r, S.g, dtin[..., ch:], dhh, reverse, kappa=L.kps[k])
            add0 = dto[..., :ch]
        x1 = tin[..., :ch]
        LevelCouplingFn._zero_conv_wgrad(L, S, k, [x1, D])
        G0, GD = empty(bhw + (ch,), dev), empty(bhw + (4,), dev)
        wt = S.PZt[k]
        H.conv_fwd([dhh], wt, ch + 4, 3, 1, [G0, GD])
        H.conv_rep_border_fix(dhh, wt, [G0, GD])
        LevelCouplingFn._growth_bwd(L, S, k, x1, D, G0, GD, dtin[..., :ch], add0)
        return dtin if reverse else LevelCouplingFn._layer_mix_bwd(L, S, k, xin, dtin)

    @staticmethod
    def _activations(L, R, saved, k):
        """Layer k's (tin, D, r, y[, xin]) for its backward step: stored (and released from `saved` here), or rebuilt from its output."""
        if R is not None:
            return LevelCouplingFn._rebuild(L, R, k)
        acts, saved[k] = saved[k], None
        return acts

    @staticmethod
    def _grouped_wgrads(L, S):
        """The level's grouped weight-gradient launches with their per-layer fallbacks -> tmpX (the growth layers' rows, for _finish)."""
        NL, C, ch = L.NL, L.C, L.ch
        if not H.conv_wgrad_grouped(S.wg_in, S.DH, C, S.dWz, S.dBz, 3, 1, **S.zc_kw):
            for k in range(NL):
                LevelCouplingFn._zero_conv_wgrad(L, S, k, S.wg_in[k], now=True)
        # x1 | d1 rows of the growth-layer weight gradients: same inputs, dy = this layer's (dd1, dd2, 0, 0) quad; row 0 of the
        # result belongs to w1, row 1 to w2 (its column ch is the d1 input)
        tmpX = zeros((NL, 4, ch + 4, 3, 3), S.DH.device)
        if S.DDp is not None:     # every group reads its own plane
            if os.environ.get("TMG_NO_THIN_WGRAD") is not None or not H._launched(
                    H.conv_wgrad_thin_grouped(S.wg_in, S.DDp, 2, tmpX, relu_in=True, dy_planes=True), "tmg_conv_wgrad_thin_grouped"):
                for k in range(NL):
                    H.conv_wgrad(S.wg_in[k], S.DDp[k], tmpX[k][:2], None, 3, 1, relu_in=True)
        elif not H.conv_wgrad_grouped(S.wg_in, S.DD, 2, tmpX, None, 3, 1, relu_in=True):
            for k in range(NL):
                H.conv_wgrad(S.wg_in[k], S.DD[..., 2 * k:2 * k + 2], tmpX[k][:2], None, 3, 1, relu_in=True)
        S.wg_in.clear()
        # the 1x1 mix weight gradients of all layers: same trick, every group with its own upstream gradient tensor
        gdy = [g_ for _, g_ in S.mix_wg]
        if any(not torch.is_tensor(g_) for g_ in gdy):      # split-halves layout: every group's upstream gradient as two halves
            gdy = [H._halves(g_) for g_ in gdy]
        if not H.conv_wgrad_grouped([a for a, _ in S.mix_wg], None, C, S.dWm.view(NL, C, C, 1, 1), S.dbm, 1, 1, group_dy=gdy):
            for k in range(NL):
                LevelCouplingFn._mix_wgrad(L, S, k, *S.mix_wg[k], now=True)
        S.mix_wg.clear()
        return tmpX

    @staticmethod
    def _cond_bwd(L, S, cond, Wcat):
        """Conditioning side of the whole level: one input-gradient pass (-> Gc = d(cond)), the conditioning columns of the zero-conv
        weight gradients into dWz, those of the growth layers -> tmpC for level_finish."""
        NL, NLp, C, ch, Cc, cin = L[:6]
        dev = cond.device
        Gc = empty(cond.shape, dev)
        # zero-conv part (dy = DH) and growth-layer part (dy = DD) of d(cond) as ONE contraction over [DH | DD] (K = NL (C + 4)): the
        # padding mode of the forward convs does not enter the interior of an input gradient, the replicate fold below adds the ring
        # terms of the zero convs alone (operand of Wzc by itself)
        # (Wcat = [Wzc ; Wdc]: rows NL C + 2k / + 2k+1 are the cond columns of w1_k / w2_k - Wdc's own layout)
        H.conv3x3_auto([S.DH, S.DD], Wcat, Cc, [Gc], dgrad=True)
        H.conv_rep_border_fix(S.DH, H.conv_pack(Wcat[:NL * C], 1), [Gc])
        H.masked_add(Gc, src=Gc, ref=cond)
        H.conv_wgrad([cond], S.DH, S.dWz, None, 3, 1, relu_in=True, pad_rep=True, cin_dst=cin + 2, cin_valid=Cc, ci_off0=ch)
        tmpC = zeros((NLp, 2, Cc, 3, 3), dev)  # one launch for both growth layers of all layers
        H.conv_wgrad([cond], S.DD, tmpC.view(2 * NLp, Cc, 3, 3), None, 3, 1, relu_in=True)
        return Gc, tmpC

    @staticmethod
    def _finish(L, S, Wz, Bz, Kp, tmpX, tmpC):
        """One launch: rows of tmpX / tmpC -> dW1 / dW2, and d(kappa_k) = <wz_k, dwz_k> + <bz_k, dbz_k> inside the clamp range
        (homogeneity of the zero conv in (W, b); the two inner products nearly cancel for small kappa gradients: fp64 sums)."""
        dK = empty(L.NL, Kp.device)
        H.level_finish(Wz, S.dWz, Bz, S.dBz, Kp, tmpX, tmpC, S.dW1, S.dW2, dK, zeros(4 * L.NL, Kp.device), L.ch, L.Cc)
        return dK

    @staticmethod
    def backward(ctx, dy, dld):
        L = ctx.level
        NL, NLp, C, ch, Cc, cin = L[:6]
        cond, Wm, bm, Wz, Wcat, Bz, Kp = ctx.saved_tensors[:7]
        wts = ctx.saved_tensors[7:]
        saved = ctx.saved
        if saved is None:
            raise RuntimeError("LevelCouplingFn: the saved activations were released by a previous backward pass "
                               "(a second backward through the same graph is not supported)")
        ctx.saved = None
        dy = dy.contiguous()
        bhw, dev = dy.shape[:3], dy.device
        g = dld.contiguous() if dld is not None else None
        # stacked native-layout parameter gradients of the whole level, one zero fill; dWz first: 16-byte aligned slices (tmg_level_finish)
        dWz, dW1, dW2, dBz, dWm, dbm = carve(dev, (NL, C, cin + 2, 3, 3), (NL, 1, cin, 3, 3), (NL, 1, cin + 1, 3, 3), (NL, C), (NL, C, C),
                                             (NL, C))
        DH = empty(bhw + (NL * C,), dev)     # exp(kappa_k) * dhh_k, all layers
        # masked gradients w.r.t. the growth channels, COMPACT: channels 2k, 2k + 1 = (dd1_k, dd2_k), 2 NLp channels (round 4: the
        # quad layout (dd1, dd2, 0, 0) per layer made the level-wide conditioning contractions below carry 2 NL zero channels - the
        # weight gradient w.r.t. the conditioning columns 60 output channels for 30, the conditioning input gradient K = NL (C + 4)).
        # Written whole by the per-layer backward kernels (8 bytes per pixel and layer; the LAST layer writes a (dd1, dd2, 0, 0) quad
        # when there is ONE padding layer, which zeroes its two channels; more padding layers are filled): no zero fill at NL = 15
        # Large levels (the forward direction's threshold, _cond_parts): one float2 plane per layer instead - a layer's 8 bytes per pixel
        # are then whole lines of its plane, not a fragment of every 128-byte pixel of the interleaved stash, for its writer and for the
        # grouped growth-row weight gradients; one re-interleaving launch (padding channels zeroed) in front of the conditioning side
        DDp = None
        if math.prod(bhw) >= int(os.environ.get("TMG_LAYER_PLANES_MIN", 1 << 17)):
            DDp, DD = empty((NL,) + bhw + (2,), dev), None
        else:
            DD = empty(bhw + (2 * NLp,), dev)
        quad_last = NLp - NL == 1        # (NL = 15 in the reference's models: one padding layer, zeroed by the last layer's quad store)
        if DD is not None and NLp - NL > 1:
            DD[..., 2 * NL:].zero_()
        # The NL zero-conv weight gradients (x1 | D part) are independent of each other once DH holds every layer's
        # exp(kappa)*dhh: they run as ONE grouped launch after the loop (a few microseconds of MFMA work each otherwise,
        # dominated by launch / pipeline-fill).  Their inputs stay alive until then (NL * C floats per pixel).
        grouped = NL > 1 and ch + 4 <= 132
        PZt = H.conv_pack_batched(Wz, 1, ch + 4, (ch + 2, ch, Cc))          # input-gradient operands of all layers: one launch
        PMt = H.conv_pack_batched(Wm.reshape(NL, C, C, 1, 1), 1)
        zc_kw = dict(relu_in=True, pad_rep=True, cin_dst=cin + 2, cin_valid=ch + 2, ci_split=ch, ci_off0=0, ci_off1=Cc)
        # wg_in[k] = [x1, D] of layer k's zero conv; mix_wg[k] = (input, upstream gradient) of its 1x1 mix
        S = _LevelBwd(g, Wm, PZt, PMt, DH, DD, quad_last, grouped, zc_kw, [None] * NL, [None] * NL if grouped else None, dWz, dBz, dW1, dW2,
                      dWm, dbm, DDp)
        R = None
        if ctx.rec_out is not None:     # recompute mode: see _rebuild
            Hc_r, Dc_r, dc_of_r = LevelCouplingFn._cond_parts(L, cond, Wcat)
            Winv, binv = H.mat_inverse(Wm, bm)
            R = [Hc_r, dc_of_r, Winv, binv, zeros(bhw[0], dev), ctx.rec_out]
        ctx.rec_out = None
        if not L.fuse:
            step = LevelCouplingFn._bwd_wide
        else:
            step = LevelCouplingFn._bwd_fused_generative if L.reverse else LevelCouplingFn._bwd_fused_density
        dcur = dy
        for k in (range(NL) if L.reverse else range(NL - 1, -1, -1)):
            dcur = step(L, S, k, dcur, *LevelCouplingFn._activations(L, R, saved, k))
        tmpX = LevelCouplingFn._grouped_wgrads(L, S) if grouped else None
        if DDp is not None:
            S = S._replace(DD=H.layer_unplanes(DDp, 2 * NLp), DDp=None)
        Gc, tmpC = LevelCouplingFn._cond_bwd(L, S, cond, Wcat)
        dK = LevelCouplingFn._finish(L, S, Wz, Bz, Kp, tmpX, tmpC)
        grads = []
        for k in range(NL):
            grads += [dW1[k], dW2[k], dWz[k], dBz[k], dK[k].reshape(L.kps[k].shape)]
        return (dcur, Gc, dWm, dbm, None) + _defer(wts, grads)


class LevelMixFoldFn(torch.autograd.Function):
    """ActNorm + PLU folding of all K layers of a level (W = P L U, then the ActNorm scale / shift) as one node: two launches per
    level (tmg_lu_fold_fwd / _bwd) instead of ~70 tiny torch launches.  Inputs after the meta tuple: per layer l, u, log_s, ActNorm
    weight, ActNorm bias (the module's own tensors, read through a device pointer table).  Outputs Wm [K,C,C], bm [K,C], ld [1] and
    the same mixes once more as (first K-1 layers, last layer) views: a caller that consumes the head as one slice and the tail on its
    own (LSTMFLowBlock) hands their gradients back as two tensors, read in place by the backward launch - slicing Wm under autograd
    instead costs a zero fill, a copy and an add of a full-size gradient per slice.  Use either Wm / bm or the split views."""

    @staticmethod
    def forward(ctx, meta, *params):
        tab, sign_s, perm, iperm, reverse, sgn, hw, K, C = meta
        dev = sign_s.device
        W = torch.empty((K, C, C), device=dev, dtype=torch.float64)     # P L U in fp64, kept for the backward launch
        Wm = empty((K, C, C), dev)
        bm = empty((K, C), dev)
        ld = empty(1, dev)
        H.lu_fold_fwd(tab, sign_s, perm, iperm, W, Wm, bm, ld, reverse, sgn, hw)
        ctx.meta = meta
        ctx.shapes = [t.shape if t is not None else None for t in params]
        ctx.save_for_backward(W, *[t for t in params if t is not None])      # params: kept alive (and version-checked) for the pointer table
        ctx.set_materialize_grads(False)
        return Wm, bm, ld, Wm[:K - 1], bm[:K - 1], Wm[K - 1], bm[K - 1]

    @staticmethod
    def backward(ctx, dWm, dbm, dld, dWh, dbh, dWt, dbt):
        tab, sign_s, perm, iperm, reverse, sgn, hw, K, C = ctx.meta
        W = ctx.saved_tensors[0]
        dev = W.device
        dl = empty((K, C, C), dev)
        du = empty((K, C, C), dev)
        dlogs = empty((K, C), dev)
        da = empty((K, C), dev)
        db = empty((K, C), dev)
        split = dWm is None and dbm is None and dWt is not None and (dWh is not None or K == 1) and (dbt is None) == (dbh is None or K == 1)
        if split:
            dWm, dbm, dWt, dbt = (None if t is None else t.contiguous() for t in (dWh, dbh, dWt, dbt))
        else:
            # general case (rare): assemble full-size gradients from whatever arrived
            full = zeros((K, C, C), dev) if dWm is None else dWm.clone()
            fb = zeros((K, C), dev) if dbm is None else dbm.clone()
            if dWh is not None:
                full[:K - 1] += dWh
            if dWt is not None:
                full[K - 1] += dWt
            if dbh is not None:
                fb[:K - 1] += dbh
            if dbt is not None:
                fb[K - 1] += dbt
            dWm, dbm, dWt, dbt = full, fb, None, None
        H.lu_fold_bwd(tab, sign_s, perm, iperm, W, dWm, dbm, dld.contiguous() if dld is not None else None, dl, du, dlogs, da, db,
                      reverse, sgn, hw, dWm_tail=dWt, dbm_tail=dbt)
        grads = []
        for k in range(K):
            sh = ctx.shapes[5 * k:5 * k + 5]
            grads += [dl[k], du[k], dlogs[k].view(sh[2]), da[k].view(sh[3]) if sh[3] is not None else None,
                      db[k].view(sh[4]) if sh[4] is not None else None]
        live = iter(ctx.saved_tensors[1:])
        params = [next(live) if sh is not None else None for sh in ctx.shapes]
        return (None,) + _defer(params, grads)


class LeadingChannelsFn(torch.autograd.Function):
    """x -> (x, x[..., :n]) as two autograd outputs for a tensor whose leading channels feed one branch (the ConvLSTM block of the LSTM
    coupling layer, flowAffine.py:199-205) while the whole tensor feeds another.  A plain slice makes autograd zero-fill a full-size
    gradient, copy the branch gradient in and add the two full-size tensors; here the branch gradient is added in place into the
    leading channels of the whole-tensor gradient (a fresh buffer owned by the producing node): one half-size launch."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.C = n, x.shape[3]
        ctx.set_materialize_grads(False)
        return x.view(x.shape), x[..., :n]

    @staticmethod
    def backward(ctx, dx, d1):
        if d1 is None:
            return dx, None
        if dx is None:   # the whole-tensor output took no part in the loss
            dx = torch.zeros(d1.shape[:3] + (ctx.C,), device=d1.device, dtype=d1.dtype)
        dx[..., :ctx.n] += d1
        return dx, None


class EnsembleFeed:
    """The feeding protocol of the Ensemble* accumulators: S members of B cases of [C, H, W] over Tk steps.  Members are fed in
    order (m0 = 0 first), whole members per chunk, every step's chunks before the next step's; the step's last chunk is the one that
    scores it.  Every accumulator folds in this one order, which is what makes its outputs bit-reproducible for every chunking.

    Host bookkeeping only: no device, no kernel.  An accumulator's add() is open_chunk, its own launches, close_chunk; its
    finalize() starts with finalize_guard.  C = None accepts any 2..4 channels (EnsembleSpectrum reads channels 0 and 1 only);
    time = None is the variant whose add() has no time argument (EnsembleTimeSpectrum: every fed step counts)."""

    def __init__(self, members, B, C, Hh, Ww, steps):
        self.S, self.B, self.H, self.W, self.Tk = int(members), int(B), int(Hh), int(Ww), int(steps)
        self.C = None if C is None else int(C)
        self._n = 0             # members fed for the current step
        self._step = 0          # the step being filled
        self._t = [0] * self.S  # timed steps every member has been fed for
        self._timed = []        # the steps whose last chunk came with time=True

    def open_chunk(self, y, m0, time=True, target=None, required=False):
        """The checks of a chunk y (API-shaped [k*B, C, H, W], rows member-major) that holds the step's members m0 .. m0 + k - 1:
        shape, target (required: None is an error; else optional, or absent when the add() has none to pass), order, time.
        -> (yn, tn, k, t_before, last): the channels-last views of y and of the target (None without one), the timed steps these
        members hold so far (None when time is None) and whether the chunk is the step's last."""
        yn = y.permute(0, 2, 3, 1)
        kB = yn.shape[0]
        if self.C is None:
            if kB % self.B or tuple(yn.shape[1:3]) != (self.H, self.W) or not 2 <= yn.shape[3] <= 4:
                raise ValueError("chunk shape %s does not hold whole members of [%d, 2..4, %d, %d]" % (tuple(y.shape), self.B, self.H, self.W))
        elif (time is None and kB < 1) or kB % self.B or tuple(yn.shape[1:]) != (self.H, self.W, self.C):
            raise ValueError("chunk shape %s does not hold whole members of [%d, %d, %d, %d]" % (tuple(y.shape), self.B, self.C, self.H, self.W))
        if (required and target is None) or (target is not None and tuple(target.shape) != (self.B, self.C, self.H, self.W)):
            raise ValueError("target shape %s is not [%d, %d, %d, %d]" % (None if target is None else tuple(target.shape), self.B, self.C,
                                                                          self.H, self.W))
        k = kB // self.B
        if m0 != self._n or m0 + k > self.S or self._step >= self.Tk:
            raise ValueError("members must be fed in order, every step's chunks before the next step's")
        t_before = None if time is None else self._t[m0]
        if time and any(self._t[m] != t_before for m in range(m0, m0 + k)):
            raise ValueError("members of one chunk hold different numbers of time steps")
        return yn, None if target is None else target.permute(0, 2, 3, 1), k, t_before, m0 + k == self.S

    def close_chunk(self, m0, k, time, last):
        """Count the chunk open_chunk accepted, after its launches."""
        if time:
            for m in range(m0, m0 + k):
                self._t[m] += 1
            if last:
                self._timed.append(self._step)
        self._n = 0 if last else self._n + k
        self._step += 1 if last else 0

    def finalize_guard(self, timed=True):
        """Every step is fed -> the number of steps fed with time=True (timed=False, the variant without a time argument: Tk)."""
        if not timed:
            if self._step != self.Tk or self._n != 0:
                raise RuntimeError("%d of %d steps fed" % (self._step, self.Tk))
            return self.Tk
        if self._step != self.Tk:
            raise RuntimeError("%d of %d steps folded" % (self._step, self.Tk))
        T = self._t[0]
        if T < 1 or any(t != T for t in self._t) or len(self._timed) != T:
            raise RuntimeError("no time statistics: no step was folded with time=True")
        return T


def _on_device(yn, tn=None):
    """The device checks of a chunk and its target, where an add() makes them itself: after open_chunk, before its launches."""
    H.check_device(yn)
    if tn is not None:
        H.check_act(tn)
        H.check_device(tn)


def _ens_channels(noun, C, why=""):
    if not (2 <= C <= 4):
        raise ValueError("%s need 2 <= C <= 4 channels%s, got %d" % (noun, why, C))


def _ens_members(noun, members):
    if not (1 <= int(members) <= SCORES_MAX_MEMBERS):
        raise ValueError("%s need 1 <= members <= %d, got %d" % (noun, SCORES_MAX_MEMBERS, int(members)))


def _ens_tables(C, reason, out_std, out_mu=None):
    """The first C entries of out_std (finite, strictly positive) and, when given, out_mu (finite) -> (sd, mu): fp32 CPU tensors, mu
    None without out_mu."""
    sd = torch.as_tensor(out_std, dtype=torch.float32).detach().reshape(-1)[:C].cpu()
    mu = None if out_mu is None else torch.as_tensor(out_mu, dtype=torch.float32).detach().reshape(-1)[:C].cpu()
    if mu is None and sd.numel() != C:
        raise ValueError("out_std needs %d entries, got %d" % (C, sd.numel()))
    if mu is not None and (sd.numel() != C or mu.numel() != C):
        raise ValueError("out_mu / out_std need %d entries, got %d / %d" % (C, mu.numel(), sd.numel()))
    if not bool((torch.isfinite(sd) & (sd > 0)).all()):
        raise ValueError("out_std must be finite and strictly positive (%s), got %s" % (reason, sd.tolist()))
    if mu is not None and not bool(torch.isfinite(mu).all()):
        raise ValueError("out_mu must be finite, got %s" % mu.tolist())
    return sd, mu


def _ens_u(u, B, C, reason):
    """u (finite, strictly positive) -> [B, C] fp32 CPU tensor, or None for 1."""
    if u is None:
        return None
    u = torch.as_tensor(u, dtype=torch.float32).detach().reshape(B, C).cpu()
    if not bool((torch.isfinite(u) & (u > 0)).all()):
        raise ValueError("u must be finite and strictly positive (%s)" % reason)
    return u


def _ens_device(noun, device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("%s run on the HIP path: device %s is not a GPU (there is no CPU path)" % (noun, dev))
    return dev


def _ens_scale(sd, u, B, dtype):
    """a[b, c] = u[b, c] out_std[c] (u None: 1), formed in dtype from the fp32 factors -> [B, C] CPU tensor."""
    sd = sd.to(dtype).view(1, -1)
    return (sd.expand(B, sd.shape[1]) if u is None else u.to(dtype) * sd).contiguous()


def _ens_directions(entries):
    """(channel, value, ">" | "<") entries -> the kernels' (channel, 1 for ">" else 0) list."""
    return [(int(e[0]), 1 if e[2] == ">" else 0) for e in entries]


_KEEPS_ORDER = "u * out_std > 0 keeps the members' order"


class EnsembleStats(EnsembleFeed):
    """On-device statistics over the members of sampled roll-outs of B cases (tmg_ens_accum / tmg_ens_time_finalize): for every kept
    step the mean and population standard deviation (ddof 0, as np.std) over the members of each un-normalised channel
    yh = u[b, c] (out_std[c] y + out_mu[c]) and of the velocity magnitude sqrt(yh0^2 + yh1^2); per member the time mean and RMS
    fluctuation of each channel over the steps folded with time=True, and their mean / std over the members.

    Feed every step's members in chunks of whole members, in member order (m0 = 0 first), each step's chunks before the next step's.
    Outputs (device tensors): mean, std [B, Tk, C, H, W]; mag_mean, mag_std [B, Tk, H, W]; finalize() adds time_mean_mean,
    time_mean_std, time_rms_mean, time_rms_std [B, C, H, W].

    grid=(dx, dy) adds the turbulence statistics (tmg_ens_turb_accum / tmg_ens_turb_finalize) of the velocity (channels 0, 1) on a
    grid of cell size dx along W, dy along H: vort_mean, vort_std [B, Tk, H, W], the members' mean / population std per kept step of the
    vorticity w = dv/dx - du/dy (3x3 first-derivative stencil of pc/, zero padding); finalize() adds time_uv_mean, time_uv_std (each
    member's Reynolds shear stress <u'v'> over the time window), time_tke_mean, time_tke_std (its 0.5 (<u'u'> + <v'v'>)) and
    time_vort_mean, time_vort_std (its time-mean vorticity), all [B, H, W].  The other outputs do not depend on grid."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=None):
        _ens_channels("ensemble statistics", C, " (the magnitude is formed from channels 0 and 1)")
        if grid is not None:
            grid = tuple(float(g) for g in grid)
            if len(grid) != 2 or not all(math.isfinite(g) and g > 0 for g in grid):
                raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %s" % (grid,))
        dev = _ens_device("ensemble statistics", device)
        self.grid = grid
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        HW = self.H * self.W
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu = torch.as_tensor(out_mu, **f32).reshape(-1)[:C].contiguous()
        self.sd = torch.as_tensor(out_std, **f32).reshape(-1)[:C].contiguous()
        if self.mu.numel() != C or self.sd.numel() != C:
            raise ValueError("out_mu / out_std need %d entries, got %d / %d" % (C, self.mu.numel(), self.sd.numel()))
        self.u = None if u is None else torch.as_tensor(u, **f32).reshape(B, C).contiguous()
        self.step_state = torch.empty((2, B, C + 1, HW), **f32)
        self.time_state = torch.empty((2, self.S, B, C, HW), **f32)
        self.out = {"mean": torch.empty((B, self.Tk, C, Hh, Ww), **f32), "std": torch.empty((B, self.Tk, C, Hh, Ww), **f32),
                    "mag_mean": torch.empty((B, self.Tk, Hh, Ww), **f32), "mag_std": torch.empty((B, self.Tk, Hh, Ww), **f32)}
        if grid is not None:
            self.vort_state = torch.empty((2, B, HW), **f32)                 # the step's (mean, M2) of the vorticity
            self.turb_state = torch.empty((2, self.S, B, HW), **f32)         # per member: time co-moment of (u, v), time-mean vorticity
            self.out.update(vort_mean=torch.empty((B, self.Tk, Hh, Ww), **f32), vort_std=torch.empty((B, self.Tk, Hh, Ww), **f32))

    def add(self, y, m0, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major)."""
        yn, _, k, t_before, last = self.open_chunk(y, m0, time)    # the device checks are the wrappers'
        HW = self.H * self.W
        o = self.out
        t = self._step
        flags = (1 if time else 0) | (2 if last else 0)
        if self.grid is not None:   # before ens_accum: it reads the members' time means as they stand after t_before steps
            H.ens_turb_accum(yn, self.u, self.mu, self.sd, self.time_state[0], self.vort_state[0], self.vort_state[1], self.turb_state[0],
                             self.turb_state[1], (o["vort_mean"][:, t], o["vort_std"][:, t]) if last else None, self.Tk * HW, self.grid, k,
                             self._n, m0, t_before, flags)
        outs = (o["mean"][:, t], o["std"][:, t], o["mag_mean"][:, t], o["mag_std"][:, t]) if last else None
        H.ens_accum(yn, self.u, self.mu, self.sd, self.step_state[0], self.step_state[1], self.time_state[0], self.time_state[1], outs,
                    (self.Tk * self.C * HW, self.Tk * HW), k, self._n, m0, t_before, flags)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time statistics cover the steps folded with time=True."""
        T = self.finalize_guard()
        shp = (self.B, self.C, self.H, self.W)
        names = ("time_mean_mean", "time_mean_std", "time_rms_mean", "time_rms_std")
        for n in names:
            self.out[n] = empty(shp, self.step_state.device)
        H.ens_time_finalize(self.time_state[0], self.time_state[1], *[self.out[n] for n in names], self.S, self.B, self.H * self.W,
                            self.C, T)
        if self.grid is not None:
            names = ("time_uv_mean", "time_uv_std", "time_tke_mean", "time_tke_std", "time_vort_mean", "time_vort_std")
            for n in names:
                self.out[n] = empty((self.B, self.H, self.W), self.step_state.device)
            H.ens_turb_finalize(self.time_state[1], self.turb_state[0], self.turb_state[1], [self.out[n] for n in names], self.S, self.B,
                                self.H * self.W, self.C, T)
        return self.out


SCORES_MAX_MEMBERS = 1024


class EnsembleScores(EnsembleFeed):
    """On-device calibration scores of sampled roll-outs of B cases against the target (tmg_ens_score_store / tmg_ens_score_step).
    For case b, kept step t, channel c and pixel p, with the members x_1..x_S (raw normalised model outputs), the normalised target
    y, a = u[b, c] out_std[c] > 0 and the un-normalised xh = u (out_std x + out_mu), yh likewise:
      crps      = (1/S) sum_m |xh_m - yh| - (1 / (2 S^2)) sum_m sum_n |xh_m - xh_n|       the ensemble CRPS
      crps_fair = the same with 1 / (2 S (S - 1)) on the pair term (S = 1: crps)
      rank      = #{m : x_m < y}, strict: a member equal to the target is not below it
    out_mu cancels in every term and a > 0 keeps the order, so the kernels work on the raw values and multiply by a once; out_mu is
    not an input.  rank_hist[b, t, c, r] counts the pixels of rank r = 0..S.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is scored.
    Outputs (device tensors): crps, crps_fair [B, Tk, C, H, W]; rank_hist [B, Tk, C, S + 1] int64; finalize() adds time_crps,
    time_crps_fair [B, C, H, W] (running means over the steps folded with time=True) and time_rank_hist [B, C, S + 1] int64 (the sum
    of rank_hist over those steps)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_std, u=None):
        noun, why = "ensemble scores", "the scores scale with u * out_std"
        _ens_channels(noun, C)
        _ens_members(noun, members)
        sd, _ = _ens_tables(C, why, out_std)
        u = _ens_u(u, B, C, why)
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        HW = self.H * self.W
        f32 = dict(device=dev, dtype=torch.float32)
        self.scale = _ens_scale(sd, u, self.B, torch.float32).to(dev)
        self.xs = torch.empty((self.S, self.B, C, HW), **f32)
        self.time_state = torch.empty((2, self.B, C, HW), **f32)
        self.hist = torch.zeros((self.B, self.Tk, C, self.S + 1), device=dev, dtype=torch.int32)
        self.out = {"crps": torch.empty((self.B, self.Tk, C, Hh, Ww), **f32), "crps_fair": torch.empty((self.B, self.Tk, C, Hh, Ww), **f32)}

    def add(self, y, m0, target, time=True):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk scores the step against its target."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        H.ens_score_store(yn, self.xs, k, m0)
        if last:
            HW = self.H * self.W
            t = self._step
            o = self.out
            H.ens_score_step(self.xs, tn, self.scale, o["crps"][:, t], o["crps_fair"][:, t], self.hist[:, t],
                             (self.time_state[0], self.time_state[1]), (self.Tk * self.C * HW, self.Tk * self.C * (self.S + 1)),
                             t_before, 1 if time else 0)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time statistics cover the steps folded with time=True."""
        self.finalize_guard()
        shp = (self.B, self.C, self.H, self.W)
        self.out["rank_hist"] = self.hist.to(torch.int64)
        self.out["time_crps"] = self.time_state[0].view(shp)
        self.out["time_crps_fair"] = self.time_state[1].view(shp)
        self.out["time_rank_hist"] = self.out["rank_hist"][:, self._timed].sum(dim=1)
        return self.out


def quantile_levels(S, levels):
    """The host level table of EnsembleQuantiles, numpy's method="linear" in fp64: for every probability q of `levels` the virtual
    index h = q (S - 1), lo = min(floor(h), S - 1), hi = min(lo + 1, S - 1) and the weight w = float32(h - lo), so that the quantile is
    x_(lo) + w (x_(hi) - x_(lo)) over the order statistics x_(0) <= .. <= x_(S-1).  -> (lo, hi, w): int64, int64, float32 arrays."""
    import numpy as np
    S = int(S)
    q = np.asarray(levels, dtype=np.float64).reshape(-1)
    if S < 1 or not bool(np.all(np.isfinite(q) & (q >= 0) & (q <= 1))):
        raise ValueError("quantile levels must be finite and in [0, 1] and S >= 1, got S=%d, levels=%s" % (S, q.tolist()))
    h = q * (S - 1)
    lo = np.minimum(np.floor(h), S - 1).astype(np.int64)
    hi = np.minimum(lo + 1, S - 1)
    return lo, hi, (h - lo).astype(np.float32)


QUANT_MAX_LEVELS = 8
QUANT_MAX_EXCEED = 4


def quantile_args(levels, exceed, C):
    """The checks of EnsembleQuantiles' levels and exceed arguments for C channels -> (levels as floats, exceed as tuples)."""
    lv = [float(q) for q in levels]
    if not (1 <= len(lv) <= QUANT_MAX_LEVELS) or not all(math.isfinite(q) and 0.0 <= q <= 1.0 for q in lv):
        raise ValueError("levels must be 1 to %d finite probabilities in [0, 1], got %s" % (QUANT_MAX_LEVELS, lv))
    ex = [tuple(e) for e in exceed]
    if len(ex) > QUANT_MAX_EXCEED:
        raise ValueError("exceed takes at most %d entries, got %d" % (QUANT_MAX_EXCEED, len(ex)))
    for e in ex:
        if len(e) != 3 or isinstance(e[0], bool) or not isinstance(e[0], numbers.Integral) or not 0 <= e[0] < C \
                or e[2] not in (">", "<") or isinstance(e[1], bool) or not isinstance(e[1], numbers.Real) or not math.isfinite(e[1]):
            raise ValueError("exceed entries are (channel in 0..%d, finite value, '>' or '<'), got %r" % (C - 1, e))
    return lv, ex


def raw_thresholds(entries, B, C, mu, sd, u=None):
    """The raw thresholds of the entries (channel, value, direction) for B cases: thr[b, k] = (value / u[b, c] - out_mu[c]) / out_std[c]
    in fp64, rounded once to fp32 (mu, sd: [C] fp32 CPU tensors, u: [B, C] fp32 CPU tensor or None for 1).  With u out_std > 0,
    comparing raw normalised values with thr is comparing physical values with `value`.  -> [B, K] fp32 CPU tensor."""
    scd = torch.ones(B, C, dtype=torch.float64) if u is None else u.double()
    thr = torch.stack([(float(e[1]) / scd[:, e[0]] - mu.double()[e[0]]) / sd.double()[e[0]] for e in entries], 1)
    return thr.to(torch.float32)


class EnsembleQuantiles(EnsembleFeed):
    """On-device prediction intervals of sampled roll-outs of B cases (tmg_ens_score_store / tmg_ens_quant_step): per case b, kept
    step t, channel c and pixel p the quantiles of the S members at the probability `levels` (numpy's method="linear": exact order
    statistics, ties broken by member index, then one fp32 interpolation, see quantile_levels), un-normalised as
    u[b, c] (out_std[c] q + out_mu[c]); and for every entry (channel, value, ">" | "<") of `exceed` the share of the members of that
    channel whose un-normalised value is strictly above / below `value` (physical units; (0, 0.0, "<") is the reverse-flow
    probability).  u out_std > 0 keeps the order, so the kernel selects on the raw normalised values and compares them with the
    thresholds (value / u - out_mu) / out_std, formed in fp64 and rounded once.  Non-finite members are not supported: the outputs
    of a pixel that holds one are unspecified.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's.  The target is optional, but given for every step or for none; the last chunk's is the one used.
    Outputs (device tensors): quant [B, Tk, Q, C, H, W]; exceed_prob [B, Tk, K, H, W] (K > 0); finalize() adds, over the steps folded
    with time=True (Tn of them), time_quant [B, Q, C, H, W] (the running mean of quant), with a target time_below_count int64 (the
    steps whose normalised target was strictly under the normalised quantile) and below_frac = time_below_count / Tn, with K > 0
    time_exceed_count [B, K, H, W] int64 (member counts summed over the steps) and time_exceed_prob = count / (S Tn); and levels [Q]
    float64 as given."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, levels=(0.05, 0.5, 0.95), exceed=()):
        noun = "ensemble quantiles"
        _ens_channels(noun, C)
        if int(steps) < 1:
            raise ValueError("%s need steps >= 1, got %d" % (noun, int(steps)))
        lv, ex = quantile_args(levels, exceed, C)
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.levels = lv
        self.lo, self.hi, self.w = quantile_levels(self.S, lv)
        self.Q, self.K = len(lv), len(ex)
        HW = self.H * self.W
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).contiguous()
        self.xs = torch.empty((self.S, self.B, C, HW), **f32)
        self.tquant = torch.empty((self.B, self.Q, C, HW), **f32)
        self.tbelow = torch.empty((self.B, self.Q, C, HW), device=dev, dtype=torch.int32)
        self.out = {"quant": torch.empty((self.B, self.Tk, self.Q, C, Hh, Ww), **f32)}
        self.ex = _ens_directions(ex)
        self.thr = self.texceed = None
        if self.K:
            self.thr = raw_thresholds(ex, self.B, C, mu, sd, u).to(dev).contiguous()
            self.texceed = torch.empty((self.B, self.K, HW), device=dev, dtype=torch.int32)
            self.out["exceed_prob"] = torch.empty((self.B, self.Tk, self.K, Hh, Ww), **f32)
        self._scored = None   # whether the steps come with a target: the first step decides

    def add(self, y, m0, target=None, time=True):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule, or None.  The
        step's last chunk selects the step's quantiles."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target)
        _on_device(yn, tn)
        if last:
            if self._scored is None:
                self._scored = tn is not None
            if self._scored != (tn is not None):
                raise ValueError("the target is given for every step or for none")
        H.ens_score_store(yn, self.xs, k, m0)
        if last:
            HW = self.H * self.W
            t = self._step
            o = self.out
            H.ens_quant_step(self.xs, tn, self.u, self.mu, self.sd, self.lo, self.hi, self.w, self.thr, self.ex, o["quant"][:, t],
                             o["exceed_prob"][:, t] if self.K else None, (self.tquant, self.tbelow, self.texceed),
                             (self.Tk * self.Q * self.C * HW, self.Tk * self.K * HW), t_before, (1 if time else 0) | (2 if tn is not None else 0))
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        T = self.finalize_guard()
        shp = (self.B, self.Q, self.C, self.H, self.W)
        o = self.out
        o["time_quant"] = self.tquant.view(shp)
        if self._scored:
            o["time_below_count"] = self.tbelow.view(shp).to(torch.int64)
            o["below_frac"] = (o["time_below_count"].double() / float(T)).to(torch.float32)
        if self.K:
            o["time_exceed_count"] = self.texceed.view(self.B, self.K, self.H, self.W).to(torch.int64)
            o["time_exceed_prob"] = (o["time_exceed_count"].double() / (float(self.S) * float(T))).to(torch.float32)
        o["levels"] = torch.tensor(self.levels, dtype=torch.float64)
        return o


EVENT_MAX_EVENTS = QUANT_MAX_EXCEED
EVENT_MAX_SCALES = 8
EVENT_MAX_WIDTH = 33
EVENT_DEFAULT_SCALES = (1, 3, 5, 9, 17, 33)


def event_args(events, scales, C):
    """The checks of EnsembleEvents' events and scales arguments for C channels.  events: the rules and messages of quantile_args'
    exceed entries (channel in 0..C-1, finite value, '>' or '<'; at most 4), and at least one of them.  scales: 1 to 8 distinct odd
    integers in 1..33 (no bools, no floats); the first offending entry is named.  -> (events as tuples, scales as a tuple of ints)."""
    _, ev = quantile_args((0.5,), events, C)
    if len(ev) < 1:
        raise ValueError("events needs at least one entry (channel, value, '>' or '<')")
    sc = list(scales)
    if not (1 <= len(sc) <= EVENT_MAX_SCALES):
        raise ValueError("scales takes 1 to %d neighbourhood widths, got %d" % (EVENT_MAX_SCALES, len(sc)))
    for i, w in enumerate(sc):
        if isinstance(w, bool) or not isinstance(w, numbers.Integral) or not 1 <= w <= EVENT_MAX_WIDTH or w % 2 != 1:
            raise ValueError("scales are odd integers in 1..%d, got %r" % (EVENT_MAX_WIDTH, w))
        if w in sc[:i]:
            raise ValueError("scales must be distinct, got %r twice" % (w,))
    return ev, tuple(int(w) for w in sc)


def event_table_scores(cnt, hit, S):
    """The scores of reliability tables (cnt, hit: int64 CPU tensors [..., S + 1]; bin j holds the pixels with j of S members in the
    event, hit those of them at which the target is in the event), in fp64 -> dict of fp64 tensors [...] and, for obs_freq / the
    ROC curve, [..., S + 1] / [..., S + 2].  N = sum cnt.  Empty bins add nothing; roc_area is NaN without an event or a non-event."""
    S = int(S)
    j = torch.arange(S + 1, dtype=torch.int64)
    N = cnt.sum(-1)
    nd = N.double()
    num = (cnt * (j * j) - 2 * S * (hit * j) + S * S * hit).sum(-1)           # exact: S^2 N < 2^63
    out = {"brier": num.double() / (float(S * S) * nd)}
    nh = hit.sum(-1)
    ob = nh.double() / nd
    out["base_rate"] = ob
    out["fcst_rate"] = (cnt * j).sum(-1).double() / (float(S) * nd)
    c, h = cnt.double(), hit.double()
    full = cnt > 0
    oj = torch.where(full, h / torch.where(full, c, torch.ones_like(c)), torch.zeros_like(c))
    fj = j.double() / float(S)
    out["brier_rel"] = (c * (fj - oj) ** 2).sum(-1) / nd
    out["brier_res"] = (c * (oj - ob.unsqueeze(-1)) ** 2).sum(-1) / nd
    out["brier_unc"] = ob * (1.0 - ob)
    out["obs_freq"] = torch.where(full, oj, torch.full_like(oj, float("nan")))
    # the rule "yes when n >= j", j = 0..S+1: the sums over the bins i >= j, then a zero
    tail = lambda v: torch.cat([v.flip(-1).cumsum(-1).flip(-1), torch.zeros_like(v[..., :1])], -1)     # noqa: E731
    hr = tail(hit).double() / nh.double().unsqueeze(-1)
    fr = tail(cnt - hit).double() / (N - nh).double().unsqueeze(-1)
    out["roc_hit_rate"], out["roc_false_rate"] = hr, fr
    out["roc_area"] = ((fr[..., :-1] - fr[..., 1:]) * (hr[..., :-1] + hr[..., 1:])).sum(-1) * 0.5
    return out


def event_fss(raw, S):
    """The fractions skill score of the raw sums raw [..., 3] = (A, Bx, Cc) (int64 CPU tensor): 1 - (A - 2 S Bx + S^2 Cc) /
    (A + S^2 Cc), the integers exact, one fp64 division; NaN when the denominator is 0.  -> fp64 [...]."""
    S = int(S)
    A, Bx, Cc = raw[..., 0], raw[..., 1], raw[..., 2]
    return 1.0 - (A - 2 * S * Bx + S * S * Cc).double() / (A + S * S * Cc).double()


EVENT_STEP_KEYS = ("brier", "brier_rel", "brier_res", "brier_unc", "base_rate", "fcst_rate", "roc_area")
EVENT_TIME_KEYS = ("brier", "brier_rel", "brier_res", "brier_unc", "base_rate", "roc_area")


class EnsembleEvents(EnsembleFeed):
    """On-device probabilistic event verification of sampled roll-outs of B cases against the target (tmg_ens_event_count /
    tmg_ens_event_step).  An event k is (channel, value, ">" | "<"), strict, in physical units ((0, 0.0, "<") is reverse flow); it
    is decided on the raw normalised values against the raw threshold of raw_thresholds (u out_std > 0 keeps the order).  Per case b,
    kept step t, event k and pixel p: n = the number of the S members in the event (the forecast probability is n / S) and o = 1
    when the target is in it.  rel_count[j] counts the pixels with n = j and rel_hit[j] those of them with o = 1; the Brier score,
    its Murphy decomposition (brier = brier_rel - brier_res + brier_unc, exact here because the forecast takes only S + 1 values),
    base_rate, fcst_rate and the ROC area (the rule "yes when n >= j"; NaN without an event or a non-event) are formed from the two
    tables on the host in fp64 and rounded once.  For every odd width w of `scales`, with Nf / No the sums of n / o over the w x w box
    centred on a pixel (zeros outside the field), fss_raw = (sum Nf^2, sum Nf No, sum No^2) and fss = 1 - (A - 2 S Bx + S^2 Cc) /
    (A + S^2 Cc), the fractions skill score of Roberts & Lean (2008); NaN when the denominator is 0.

    The counts fold chunk by chunk: no member buffer [S][..] is kept.  The device memory of this class is O(B K HW) (the counts and
    four running sums per pixel, int32) plus the tables, not O(S B C HW).

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each
    step's chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is used.
    Outputs (device tensors): rel_count, rel_hit [B, Tk, K, S + 1] int64; brier, brier_rel, brier_res, brier_unc, base_rate,
    fcst_rate, roc_area [B, Tk, K]; fss_raw [B, Tk, K, NS, 3] int64; fss [B, Tk, K, NS]; finalize() adds, over the steps folded with
    time=True (Tn of them), time_rel_count, time_rel_hit [B, K, S + 1] int64 (the tables summed: pooled over steps and pixels),
    time_rel_obs_freq [B, K, S + 1] (NaN in empty bins), time_roc_hit_rate, time_roc_false_rate [B, K, S + 2], time_brier,
    time_brier_rel, time_brier_res, time_brier_unc, time_base_rate, time_roc_area [B, K] (the same formulas on the summed tables),
    time_fss [B, K, NS] (from the summed raw sums, not a mean of ratios), time_fss_uniform = 0.5 + time_base_rate / 2 [B, K],
    time_event_count, time_obs_count [B, K, H, W] int64 (sum_t n, sum_t o), time_brier_map [B, K, H, W] = (sum n^2 - 2 S sum n o +
    S^2 sum o) / (S^2 Tn), and event_scales [NS] int64 as given."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, events=((0, 0.0, "<"),), scales=EVENT_DEFAULT_SCALES):
        noun = "ensemble events"
        _ens_channels(noun, C)
        if int(steps) < 1:
            raise ValueError("%s need steps >= 1, got %d" % (noun, int(steps)))
        ev, sc = event_args(events, scales, C)
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        S, Tk, HW, wmax = int(members), int(steps), int(Hh) * int(Ww), max(sc)
        if int(B) < 1 or HW < 1:
            raise ValueError("%s need B, H, W >= 1, got %d, %d, %d" % (noun, B, Hh, Ww))
        if S * S * Tk >= 2 ** 31:
            raise ValueError("S^2 Tk = %d^2 * %d does not stay under 2^31 (the int32 per-pixel sums)" % (S, Tk))
        if S * S * wmax ** 4 * HW * Tk >= 2 ** 63:
            raise ValueError("S^2 w_max^4 HW Tk = %d^2 * %d^4 * %d * %d does not stay under 2^63 (the int64 raw sums)" % (S, wmax, HW, Tk))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.events, self.scales = ev, sc
        self.K, self.NS = len(ev), len(sc)
        self.ev = _ens_directions(ev)
        self.thr = raw_thresholds(ev, self.B, C, mu, sd, u).to(dev).contiguous()
        self.plan = H.ens_event_plan(S, self.B, self.H, self.W, self.K, sc)
        i32 = dict(device=dev, dtype=torch.int32)
        self.cnt = torch.empty((self.B, self.K, HW), **i32)
        self.tsum = torch.empty((4, self.B, self.K, HW), **i32)
        self.rel = torch.empty((2, self.B, Tk, self.K, S + 1), **i32)
        self.fss_raw = torch.empty((self.B, Tk, self.K, self.NS, 3), device=dev, dtype=torch.int64)

    def add(self, y, m0, target, time=True):
        """Count the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk verifies the step against its target."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        H.ens_event_count(yn, self.thr, self.ev, self.cnt, self.S, k, m0)
        if last:
            t = self._step
            H.ens_event_step(self.cnt, tn, self.thr, self.ev, self.scales, self.rel[0, :, t], self.rel[1, :, t], self.fss_raw[:, t],
                             self.tsum, (self.Tk * self.K * (self.S + 1), self.Tk * self.K * self.NS * 3), self.S, t_before,
                             1 if time else 0)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        T = self.finalize_guard()
        dev, S = self.rel.device, self.S
        f32 = lambda v: v.to(torch.float32).to(dev)                            # noqa: E731
        rel = self.rel.to(torch.int64)
        o = {"rel_count": rel[0], "rel_hit": rel[1], "fss_raw": self.fss_raw}
        hc, hh, hraw = rel[0].cpu(), rel[1].cpu(), self.fss_raw.cpu()
        sc = event_table_scores(hc, hh, S)
        for key in EVENT_STEP_KEYS:
            o[key] = f32(sc[key])
        o["fss"] = f32(event_fss(hraw, S))
        tc, th, traw = hc[:, self._timed].sum(1), hh[:, self._timed].sum(1), hraw[:, self._timed].sum(1)
        o["time_rel_count"], o["time_rel_hit"] = tc.to(dev), th.to(dev)
        sc = event_table_scores(tc, th, S)
        o["time_rel_obs_freq"] = f32(sc["obs_freq"])
        o["time_roc_hit_rate"], o["time_roc_false_rate"] = f32(sc["roc_hit_rate"]), f32(sc["roc_false_rate"])
        for key in EVENT_TIME_KEYS:
            o["time_" + key] = f32(sc[key])
        o["time_fss_uniform"] = f32(0.5 + sc["base_rate"] / 2)
        o["time_fss"] = f32(event_fss(traw, S))
        shp = (self.B, self.K, self.H, self.W)
        ts = self.tsum.to(torch.int64)
        o["time_event_count"], o["time_obs_count"] = ts[0].view(shp), ts[1].view(shp)
        o["time_brier_map"] = ((ts[2] - 2 * S * ts[3] + S * S * ts[1]).double() / float(S * S * T)).to(torch.float32).view(shp)
        o["event_scales"] = torch.tensor(self.scales, dtype=torch.int64)
        return o


SPELL_MAX_LEN = 64
SPELL_MAX_STEPS = 32767
SPELL_MAX_CASES = 65535
SPELL_TABLE_KEYS = ("spell_hist", "spell_len", "spell_cens", "spell_cens_len")
SPELL_MAP_KEYS = ("time_in_count", "time_spell_count", "time_longest_sum", "time_longest_max", "target_in_count", "target_spell_count",
                  "target_longest")


def spell_args(events, max_len, C):
    """The checks of EnsembleSpells' events and max_len arguments for C channels.  events: event_args' rules and messages (channel in
    0..C-1, finite value, '>' or '<'; 1 to 4 of them).  max_len: the number of length bins L, an integer in 1..64 (no bools, no
    floats).  -> (events as tuples, L)."""
    ev, _ = event_args(events, (1,), C)
    if isinstance(max_len, bool) or not isinstance(max_len, numbers.Integral) or not 1 <= max_len <= SPELL_MAX_LEN:
        raise ValueError("max_len is an integer in 1..%d (the length bins), got %r" % (SPELL_MAX_LEN, max_len))
    return ev, int(max_len)


def spell_outputs(hist, length, cens, cens_len, S, Tn, HW):
    """The duration statistics of the run tables of S members and the target (row S) over a window of Tn steps of HW pixels: hist
    [..., S + 1, 2, L] (the complete runs by length, the last bin open), length [..., S + 1, 2] (the sum of their lengths), cens,
    cens_len [..., S + 1, 2, 3] (the numbers and length sums of the left, right and both runs), int64 CPU tensors; the axis of 2 is
    the polarity (0 gaps, 1 spells).  Host only, integers in int64 and ratios in fp64, every float rounded to fp32 once.  -> dict:
      spell_mean [..., S + 1, 2]          length / sum(hist): the mean complete duration, NaN without a complete run
      spell_survival [..., S + 1, 2, L]   entry j - 1: the share of the complete runs of length >= j
      spell_p11, spell_p01 [..., S + 1]   n11 / (n11 + n10) and n01 / (n01 + n00), the step-to-step persistence and onset
                                          probabilities of the two-state chain, the transition counts from the tables' identities
                                          (n11 = t_in - n_s, n01 = n_s - left_1 - both_1, n10 = n_s - right_1 - both_1, n00 alike
                                          from the gaps); NaN on an empty denominator
      spell_markov_mean [..., S + 1]      1 / (1 - p11) = (n11 + n10) / n10: the mean spell a chain of this persistence would have
      spell_w1 [..., S, 2], spell_w1_pooled [..., 2]   the Wasserstein-1 distance over the bin index between a member's (all members'
                                          pooled) length distribution and the target's; NaN when either is empty
      spell_mean_below, spell_mean_equal, spell_mean_valid [..., 2] int64   the members with at least one complete run (valid) whose
                                          mean duration is strictly below / equal to the target's, by the integer products
                                          len_m cnt_T against len_T cnt_m: the exact rank of the target's persistence; below and
                                          equal are 0 when the target has no complete run."""
    S, Tn, HW = int(S), int(Tn), int(HW)
    hist, length, cens, cens_len = (torch.as_tensor(v) for v in (hist, length, cens, cens_len))
    lead = tuple(hist.shape[:-3])
    if S < 1 or Tn < 2 or HW < 1 or hist.dim() < 3 or tuple(hist.shape[-3:-1]) != (S + 1, 2) or hist.shape[-1] < 1 \
            or any(v.dtype != torch.int64 for v in (hist, length, cens, cens_len)) or tuple(length.shape) != lead + (S + 1, 2) \
            or tuple(cens.shape) != lead + (S + 1, 2, 3) or tuple(cens_len.shape) != lead + (S + 1, 2, 3):
        raise ValueError("spell_outputs takes int64 tables [..., %d, 2, L], [..., %d, 2] and two of [..., %d, 2, 3], got %s, %s, %s, %s"
                         % (S + 1, S + 1, S + 1, tuple(hist.shape), tuple(length.shape), tuple(cens.shape), tuple(cens_len.shape)))
    if Tn * HW >= 2 ** 31:
        raise ValueError("Tn HW = %d * %d does not stay under 2^31 (the int64 products of the duration ranks)" % (Tn, HW))
    hist, length, cens, cens_len = hist.cpu(), length.cpu(), cens.cpu(), cens_len.cpu()
    f32 = lambda v: v.to(torch.float32)                                        # noqa: E731
    n = hist.sum(-1)
    nd = n.double()
    o = {"spell_mean": f32(length.double() / nd)}
    o["spell_survival"] = f32(hist.flip(-1).cumsum(-1).flip(-1).double() / nd.unsqueeze(-1))
    runs, tlen = n + cens.sum(-1), length + cens_len.sum(-1)                   # every run of the polarity and the steps it covers
    n11, n00 = tlen[..., 1] - runs[..., 1], tlen[..., 0] - runs[..., 0]
    n01 = runs[..., 1] - cens[..., 1, 0] - cens[..., 1, 2]
    n10 = runs[..., 1] - cens[..., 1, 1] - cens[..., 1, 2]
    o["spell_p11"] = f32(n11.double() / (n11 + n10).double())
    o["spell_p01"] = f32(n01.double() / (n01 + n00).double())
    o["spell_markov_mean"] = f32((n11 + n10).double() / n10.double())
    cdf = lambda h: h.cumsum(-1).double() / h.sum(-1, keepdim=True).double()   # noqa: E731
    ct = cdf(hist[..., S, :, :])
    o["spell_w1"] = f32((cdf(hist[..., :S, :, :]) - ct.unsqueeze(-3)).abs().sum(-1))
    o["spell_w1_pooled"] = f32((cdf(hist[..., :S, :, :].sum(-3)) - ct).abs().sum(-1))
    lm, cm = length[..., :S, :], n[..., :S, :]
    lt, ctg = length[..., S, :].unsqueeze(-2), n[..., S, :].unsqueeze(-2)
    ok = (cm > 0) & (ctg > 0)
    o["spell_mean_below"] = (ok & (lm * ctg < lt * cm)).sum(-2)
    o["spell_mean_equal"] = (ok & (lm * ctg == lt * cm)).sum(-2)
    o["spell_mean_valid"] = (cm > 0).sum(-2)
    return o


class EnsembleSpells(EnsembleFeed):
    """On-device event durations of sampled roll-outs of B cases and of the target along a time window (tmg_ens_spell_step /
    tmg_ens_spell_finalize): how long a pixel stays in an event and out of it.  An event k is (channel, value, ">" | "<"), strict, in
    physical units ((0, 0.0, "<") is reverse flow), decided on the raw normalised values against raw_thresholds (u out_std > 0 keeps
    the order); a value that compares false (NaN, an infinity on the wrong side) is in no event.  Rows 0 .. S - 1 are the members,
    row S is the target.  Per row, case, event and pixel the indicator series e_0 .. e_{Tn-1} splits into runs, maximal stretches of
    equal value: polarity 1 is a spell, 0 a gap.  A run is complete (it starts after step 0 and ends before step Tn - 1), left
    (holds step 0), right (holds step Tn - 1) or both (the whole window); the three censored classes are kept apart, their true
    length being unknown, and never enter a histogram.  Bin j - 1 of the L = max_len bins holds the complete runs of length j, the
    last bin those of length >= L.

    `steps` is Tn >= 2: only the steps of the window are fed.  Limits: 1 <= members <= 1024, B <= 65535, Tn <= 32767 (the 15-bit
    run length of the state word), S Tn < 2^31 and Tn HW < 2^31.  Device memory: the state, one int32 word per (row, case, event,
    pixel), (S + 1) B K HW 4 bytes, which max_state_bytes bounds (default 2^31); seven int32 maps, 28 B K HW bytes; the tables,
    16 B K (S + 1) (L + 7) bytes.  No member buffer [S][..][C] is kept: a chunk is read straight from its NHWC rows.

    Feeding protocol of EnsembleFeed without a time argument: every step's members in chunks of whole members, in member order
    (m0 = 0 first), each step's chunks before the next step's; every chunk comes with the step's target, and the last chunk's is
    the one that is used.  finalize() returns, per (case, event, row, polarity) and pooled over the pixels, int64 on the device:
    spell_hist [B, K, S + 1, 2, L], spell_len [B, K, S + 1, 2], spell_cens, spell_cens_len [B, K, S + 1, 2, 3] (left, right, both);
    spell_outputs' keys (fp32 / int64); the maps [B, K, H, W] int64 time_in_count (sum over members and steps of e_t),
    time_spell_count (sum over members of the polarity-1 runs of any class), time_longest_sum, time_longest_max (sum and maximum over
    the members of each member's longest spell of any class, 0 without one), target_in_count, target_spell_count, target_longest;
    time_longest_mean = time_longest_sum / S, time_mean_duration = time_in_count / time_spell_count and target_mean_duration =
    target_in_count / target_spell_count (fp32, NaN where the count is 0); and spell_bins [L] int64 = 1 .. L."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, events=((0, 0.0, "<"),), max_len=32,
                 max_state_bytes=2 ** 31):
        noun = "ensemble spells"
        _ens_channels(noun, C)
        if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or int(steps) < 2:
            raise ValueError("%s need steps >= 2 (the time window), got %r" % (noun, steps))
        ev, L = spell_args(events, max_len, C)
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        S, Tn, HW, K = int(members), int(steps), int(Hh) * int(Ww), len(ev)
        if int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need B, H, W >= 1, got %d, %d, %d" % (noun, B, Hh, Ww))
        if int(B) > SPELL_MAX_CASES:
            raise ValueError("%s take at most %d cases, got %d" % (noun, SPELL_MAX_CASES, int(B)))
        if Tn > SPELL_MAX_STEPS:
            raise ValueError("steps = %d exceeds %d (the 15-bit run length of the state word)" % (Tn, SPELL_MAX_STEPS))
        if S * Tn >= 2 ** 31:
            raise ValueError("S Tn = %d * %d does not stay under 2^31 (the int32 per-pixel maps)" % (S, Tn))
        if Tn * HW >= 2 ** 31:
            raise ValueError("Tn HW = %d * %d does not stay under 2^31 (the int64 products of the duration ranks)" % (Tn, HW))
        nbytes = (S + 1) * int(B) * K * HW * 4
        if nbytes > int(max_state_bytes):
            raise ValueError("the state buffer (S + 1) B K HW 4 = (%d + 1) * %d * %d * %d * 4 = %d bytes exceeds max_state_bytes = %d"
                             % (S, int(B), K, HW, nbytes, int(max_state_bytes)))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.Tn, self.L, self.K = self.Tk, L, K
        self.events = ev
        self.ev = _ens_directions(ev)
        self.thr = raw_thresholds(ev, self.B, C, mu, sd, u).to(dev).contiguous()
        self.plan = H.ens_spell_plan(S, self.B, HW, K, L, Tn)
        self.state = torch.empty((S + 1, self.B, K, HW), device=dev, dtype=torch.int32)
        self.table = torch.empty((self.B, K, S + 1, 2, L + 7), device=dev, dtype=torch.int64)
        self.maps = torch.empty((H.SPELL_MAPS, self.B, K, HW), device=dev, dtype=torch.int32)
        self.out = None

    def add(self, y, m0, target):
        """Advance the runs of the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last
        view is an NHWC channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride
        rule.  The step's last chunk advances the target's runs as row S."""
        yn, tn, k, _, last = self.open_chunk(y, m0, None, target, required=True)
        _on_device(yn, tn)
        t = self._step
        H.ens_spell_step(yn, self.thr, self.ev, self.state, self.table, self.maps, self.S, k, m0, self.Tn, t)
        if last:
            H.ens_spell_step(tn, self.thr, self.ev, self.state, self.table, self.maps, self.S, 1, self.S, self.Tn, t)
        self.close_chunk(m0, k, None, last)

    def finalize(self):
        """-> dict of the outputs: the tables and maps on the device, spell_outputs' keys formed on the host."""
        self.finalize_guard(timed=False)
        if self.out is None:
            H.ens_spell_finalize(self.state, self.table, self.maps, self.Tn)
            dev, S, L = self.table.device, self.S, self.L
            tab = self.table
            raw = (tab[..., :L].contiguous(), tab[..., L].contiguous(), tab[..., L + 1:L + 4].contiguous(), tab[..., L + 4:L + 7].contiguous())
            o = dict(zip(SPELL_TABLE_KEYS, raw))
            for key, v in spell_outputs(*[v.cpu() for v in raw], S, self.Tn, self.H * self.W).items():
                o[key] = v.to(dev)
            maps = self.maps.to(torch.int64).view(H.SPELL_MAPS, self.B, self.K, self.H, self.W)
            for i, key in enumerate(SPELL_MAP_KEYS):
                o[key] = maps[i]
            ratio = lambda a, b: (a.double() / b.double()).to(torch.float32)   # noqa: E731  (0 / 0: NaN)
            o["time_longest_mean"] = (o["time_longest_sum"].double() / float(S)).to(torch.float32)
            o["time_mean_duration"] = ratio(o["time_in_count"], o["time_spell_count"])
            o["target_mean_duration"] = ratio(o["target_in_count"], o["target_spell_count"])
            o["spell_bins"] = torch.arange(1, L + 1, dtype=torch.int64)
            self.out = o
        return self.out


ISCALE_MAX_LEVELS = 6
ISCALE_RAW_KEYS = ("iscale_member_raw", "iscale_target_raw", "iscale_ens_raw")
ISCALE_FLOAT_KEYS = ("iscale_mse", "iscale_skill", "iscale_energy", "iscale_energy_bias", "iscale_brier", "iscale_brier_skill",
                     "iscale_spread", "iscale_spread_skill")


def iscale_args(events, levels, C, H, W):
    """The checks of EnsembleIntensityScale's events and levels arguments for C channels of [H, W].  events: event_args' rules and
    messages (channel in 0..C-1, finite value, '>' or '<'; 1 to 4 of them).  levels: the number of Haar levels L, an integer in 1..6
    (no bools, no floats), or None for max(1, min(6, floor(log2(min(H, W))))).  -> (events as tuples, L)."""
    ev, _ = event_args(events, (1,), C)
    if levels is None:
        if int(H) < 1 or int(W) < 1:
            raise ValueError("levels=None needs H, W >= 1, got %d, %d" % (H, W))
        return ev, max(1, min(ISCALE_MAX_LEVELS, min(int(H), int(W)).bit_length() - 1))
    if isinstance(levels, bool) or not isinstance(levels, numbers.Integral) or not 1 <= levels <= ISCALE_MAX_LEVELS:
        raise ValueError("levels is an integer in 1..%d (the Haar levels) or None, got %r" % (ISCALE_MAX_LEVELS, levels))
    return ev, int(levels)


def _iscale_energy(Q):
    """Q [..., L + 1] int64 level sums -> the integer numerators [..., L + 1] of the component energies and their divisors [L + 1]:
    (4 Q[c-1] - Q[c]) over 4^c for the Haar components c = 1..L, Q[L] over 4^L for the remainder."""
    L = Q.shape[-1] - 1
    num = torch.cat([4 * Q[..., :L] - Q[..., 1:], Q[..., L:]], -1)
    den = torch.tensor([4 ** c for c in range(1, L + 1)] + [4 ** L], dtype=torch.int64)
    return num, den


def iscale_outputs(member_raw, target_raw, ens_raw, S, HW, steps=1):
    """The intensity-scale scores of the raw block sums of S members over `steps` steps of HW pixels (pooled: the sums of the steps'
    tables): member_raw [..., S, L + 1, 2] = (A, X), target_raw [..., L + 1] = Cc, ens_raw [..., L + 1, 2] = (AN, XN), int64 CPU
    tensors, level l = 0..L last but one.  Host only: every integer combination is exact in int64 (S HW steps < 2^31), every output
    is one fp64 division (for the skills, subtracted from 1) rounded to fp32 once.  With N = HW steps, D = A - 2 X + Cc the level
    sums of a member's error I_m - o, DN = AN - 2 S XN + S^2 Cc those of n - S o, SP = S sum_m A - AN, and E_c(Q) the component
    energy (4 Q[c-1] - Q[c]) / 4^c for c = 1..L, Q[L] / 4^L for the remainder (components last, L + 1 of them; they sum to Q[0])
    -> dict:
      iscale_mse [..., S, L + 1]          E_c(D) / N: they sum to the member's share of mismatched pixels
      iscale_skill [..., S, L + 1]        1 - (L + 1) mse_c / (f + o - 2 f o), f = A[0] / N and o = Cc[0] / N the event rates of the
                                          member and the target; NaN when the random forecast's error is 0
      iscale_energy [..., S + 1, L + 1]   E_c(A[m]) / N, and E_c(Cc) / N as row S
      iscale_energy_bias [..., S, L + 1]  (Ef - Eo) / (Ef + Eo); NaN when both are 0
      iscale_brier [..., L + 1]           E_c(DN) / (S^2 N): they sum to the Brier score
      iscale_brier_skill [..., L + 1]     1 - (L + 1) brier_c / (mean p^2 + o - 2 mean p o) with p = n / S; NaN when that is 0
      iscale_spread [..., L + 1]          E_c(SP) / (S^2 N) >= 0: the mean member mse minus iscale_brier
      iscale_spread_skill [..., L + 1]    spread over brier; NaN at 0 / 0."""
    S, HW, steps = int(S), int(HW), int(steps)
    member_raw, target_raw, ens_raw = (torch.as_tensor(v) for v in (member_raw, target_raw, ens_raw))
    lead = tuple(target_raw.shape[:-1])
    L = target_raw.shape[-1] - 1 if target_raw.dim() >= 1 else 0
    if S < 1 or HW < 1 or steps < 1 or L < 1 or any(v.dtype != torch.int64 for v in (member_raw, target_raw, ens_raw)) \
            or tuple(member_raw.shape) != lead + (S, L + 1, 2) or tuple(ens_raw.shape) != lead + (L + 1, 2):
        raise ValueError("iscale_outputs takes int64 tables [..., %d, L + 1, 2], [..., L + 1] and [..., L + 1, 2] with L >= 1, got %s, %s, %s"
                         % (S, tuple(member_raw.shape), tuple(target_raw.shape), tuple(ens_raw.shape)))
    N = HW * steps
    if S * N >= 2 ** 31:
        raise ValueError("S HW steps = %d * %d does not stay under 2^31 (the int64 products of the skill scores)" % (S, N))
    member_raw, target_raw, ens_raw = member_raw.cpu(), target_raw.cpu(), ens_raw.cpu()
    A, X, Cc = member_raw[..., 0], member_raw[..., 1], target_raw.unsqueeze(-2)
    AN, XN = ens_raw[..., 0], ens_raw[..., 1]
    ratio = lambda a, b: (a.double() / b.double()).to(torch.float32)          # noqa: E731  (one division; 0 / 0: NaN)
    eD, den = _iscale_energy(A - 2 * X + Cc)
    eA, _ = _iscale_energy(A)
    eC, _ = _iscale_energy(Cc)
    eDN, _ = _iscale_energy(AN - 2 * S * XN + S * S * target_raw)
    eSP, _ = _iscale_energy(S * A.sum(-2) - AN)
    A0, C0 = A[..., :1], Cc[..., :1]
    rnd = A0 * N + C0 * N - 2 * A0 * C0                                        # N^2 (f + o - 2 f o)
    P1 = A[..., 0].sum(-1, keepdim=True)                                       # sum n, as I^2 = I
    rnb = AN[..., :1] * N + S * S * target_raw[..., :1] * N - 2 * S * P1 * target_raw[..., :1]     # S^2 N^2 (mean p^2 + o - 2 mean p o)
    o = {"iscale_mse": ratio(eD, den * N)}
    # 1 - (L + 1) N E_c / (4^c rnd): exact integers, multiplied in fp64 (N^2-sized products would leave int64), one division
    skill = lambda e, r: (1.0 - (e.double() * float((L + 1) * N)) / (den.double() * r.double())).to(torch.float32)   # noqa: E731
    o["iscale_skill"] = skill(eD, rnd)
    o["iscale_energy"] = ratio(torch.cat([eA, eC], -2), den * N)
    o["iscale_energy_bias"] = ratio(eA - eC, eA + eC)
    o["iscale_brier"] = ratio(eDN, den * (S * S * N))
    o["iscale_brier_skill"] = skill(eDN, rnb)
    o["iscale_spread"] = ratio(eSP, den * (S * S * N))
    o["iscale_spread_skill"] = ratio(eSP, eDN)
    return o


class EnsembleIntensityScale(EnsembleFeed):
    """On-device intensity-scale verification of sampled roll-outs of B cases against the target (tmg_ens_iscale_chunk /
    tmg_ens_iscale_step): at which spatial scale the error of an event forecast sits (Casati, Ross & Stephenson 2004; Casati 2010).
    An event k is (channel, value, ">" | "<"), strict, in physical units ((0, 0.0, "<") is reverse flow), decided on the raw
    normalised values against raw_thresholds (u out_std > 0 keeps the order); a value that compares false (NaN, an infinity on the
    wrong side) is in no event.  Per case, kept step, event and pixel I_m is member m's indicator, o the target's, n = sum_m I_m.  The
    blocks of level l = 0..L (L = levels, 1..6; None: max(1, min(6, floor(log2(min(H, W)))))) are the 2^l x 2^l squares aligned at
    pixel (0, 0), the field counting as zero outside H x W.  The device forms the integer sums over the blocks of a level of squared
    and multiplied block counts, (A, X) per member, Cc of the target, (AN, XN) of n; iscale_outputs turns them into the energies of
    the orthogonal Haar components of block size 2, 4, .., 2^L and of the coarse remainder, of every member's binary error and of
    the probability error n / S - o, whose components sum to EnsembleEvents' brier exactly.

    The counts fold chunk by chunk and a chunk is read straight from its NHWC rows: no member buffer [S][..] is kept.  The device
    memory of this class is O(B K HW) (the count n per pixel, int32, 4 B K HW bytes) plus the tables, 8 Tk B K (L + 1) (2 S + 3)
    bytes.  Limits: members <= 1024, B <= 65535, S^2 4^L H_pad W_pad < 2^63 with H, W padded to multiples of 64, and
    S HW Tk < 2^31 (the int64 products of the skill scores).

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target (the target's indicator enters X of every member).
    finalize() returns, with L + 1 levels or components last: iscale_member_raw [B, Tk, K, S, L + 1, 2], iscale_target_raw [B, Tk,
    K, L + 1], iscale_ens_raw [B, Tk, K, L + 1, 2] int64 on the device; iscale_outputs' keys per step, [B, Tk, K, ...] fp32; time_
    of every key, [B, K, ...], from the raw sums summed over the steps folded with time=True (Tn of them) with N = HW Tn: the
    standard aggregation, not a mean of ratios; and iscale_blocks [L + 1] int64, the block sizes 2 .. 2^L, then 0 for the remainder."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, events=((0, 0.0, "<"),), levels=None):
        noun = "ensemble intensity scales"
        _ens_channels(noun, C)
        if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or int(steps) < 1:
            raise ValueError("%s need steps >= 1, got %r" % (noun, steps))
        if int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need B, H, W >= 1, got %d, %d, %d" % (noun, B, Hh, Ww))
        ev, L = iscale_args(events, levels, C, Hh, Ww)
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        S, Tk, HW, K = int(members), int(steps), int(Hh) * int(Ww), len(ev)
        if int(B) > SPELL_MAX_CASES:
            raise ValueError("%s take at most %d cases, got %d" % (noun, SPELL_MAX_CASES, int(B)))
        pad = (-(-int(Hh) // 64) * 64) * (-(-int(Ww) // 64) * 64)
        if S * S * 4 ** L * pad >= 2 ** 63:
            raise ValueError("S^2 4^L H_pad W_pad = %d^2 * 4^%d * %d does not stay under 2^63 (the int64 raw sums)" % (S, L, pad))
        if S * HW * Tk >= 2 ** 31:
            raise ValueError("S HW Tk = %d * %d * %d does not stay under 2^31 (the int64 products of the skill scores)" % (S, HW, Tk))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.L, self.K = L, K
        self.events = ev
        self.ev = _ens_directions(ev)
        self.thr = raw_thresholds(ev, self.B, C, mu, sd, u).to(dev).contiguous()
        self.plan = H.ens_iscale_plan(S, self.B, self.H, self.W, K, L)
        i64 = dict(device=dev, dtype=torch.int64)
        self.cnt = torch.empty((self.B, K, HW), device=dev, dtype=torch.int32)
        self.member = torch.empty((Tk, self.B, K, S, L + 1, 2), **i64)
        self.target = torch.empty((Tk, self.B, K, L + 1), **i64)
        self.ens = torch.empty((Tk, self.B, K, L + 1, 2), **i64)

    def add(self, y, m0, target, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        first chunk zeroes the step's tables, its last chunk forms the sums of the ensemble count."""
        yn, tn, k, _, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        t = self._step
        H.ens_iscale_chunk(yn, tn, self.thr, self.ev, self.cnt, self.member[t], self.target[t], self.ens[t], self.S, k, m0)
        if last:
            H.ens_iscale_step(self.cnt, tn, self.thr, self.ev, self.ens[t], self.S)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        T = self.finalize_guard()
        dev, S, HW = self.member.device, self.S, self.H * self.W
        raw = [v.transpose(0, 1).contiguous() for v in (self.member, self.target, self.ens)]
        o = dict(zip(ISCALE_RAW_KEYS, raw))
        host = [v.cpu() for v in raw]
        for key, v in iscale_outputs(*host, S, HW).items():
            o[key] = v.to(dev)
        timed = [v[:, self._timed].sum(1) for v in host]
        for key, v in zip(ISCALE_RAW_KEYS, timed):
            o["time_" + key] = v.to(dev)
        for key, v in iscale_outputs(*timed, S, HW, T).items():
            o["time_" + key] = v.to(dev)
        o["iscale_blocks"] = torch.tensor([2 ** c for c in range(1, self.L + 1)] + [0], dtype=torch.int64)
        return o


MINK_MAX_FIELDS = 4
MINK_MAX_LEVELS = 32
MINK_CURVES = ("count", "edges", "euler4", "euler8")       # the four integer curves, in the order of the [.., 4, J] outputs
MINK_L1_CURVES = ("area", "perimeter", "euler4", "euler8")  # the four curves of mink_l1
MINK_INT_KEYS = ("mink_edges", "mink_euler4", "mink_euler8", "mink_below", "mink_equal")
MINK_FLOAT_KEYS = ("mink_area", "mink_perimeter", "mink_euler4_density", "mink_euler8_density", "mink_mean", "mink_std", "mink_l1")


def mink_args(fields, thresholds, C):
    """The checks of EnsembleMorphology's fields and thresholds arguments for C channels.  fields: 1 to 4 distinct channel indices in
    0..C-1 (no bools, no floats).  thresholds: per field a sequence of J strictly ascending finite values in physical units, 1 <= J <=
    32, the same J for every field.  -> (fields as a tuple of ints, the ladder as a tuple of F tuples of J floats)."""
    try:
        fl = list(fields)
    except TypeError:
        raise ValueError("fields is a sequence of channel indices, got %r" % (fields,))
    if not 1 <= len(fl) <= MINK_MAX_FIELDS:
        raise ValueError("fields takes 1 to %d channels, got %d" % (MINK_MAX_FIELDS, len(fl)))
    for i, c in enumerate(fl):
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= c < C:
            raise ValueError("fields are channel indices in 0..%d, got %r" % (C - 1, c))
        if c in fl[:i]:
            raise ValueError("fields must be distinct, got %r twice" % (c,))
    try:
        th = [list(t) for t in thresholds]
    except TypeError:
        raise ValueError("thresholds holds one sequence of values per field, got %r" % (thresholds,))
    if len(th) != len(fl):
        raise ValueError("thresholds holds one ladder per field: %d fields, %d ladders" % (len(fl), len(th)))
    J = len(th[0])
    if not 1 <= J <= MINK_MAX_LEVELS:
        raise ValueError("a ladder holds 1 to %d levels, got %d" % (MINK_MAX_LEVELS, J))
    for t in th:
        if len(t) != J:
            raise ValueError("every field takes the same number of levels, got %d and %d" % (J, len(t)))
        for j, v in enumerate(t):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError("thresholds are finite numbers, got %r" % (v,))
            if j and not t[j - 1] < v:
                raise ValueError("a ladder is strictly ascending, got %r after %r" % (v, t[j - 1]))
    return tuple(int(c) for c in fl), tuple(tuple(float(v) for v in t) for t in th)


def mink_raw_ladder(levels, fields, mu, sd, u=None):
    """The raw ladder of the physical one by raw_thresholds' rule, per case: levels [B, F, J] fp64 CPU tensor, fields the F channels,
    mu, sd [C] fp32 CPU tensors, u [B, C] fp32 CPU tensor or None for 1 -> thr[b, f, j] = (levels / u[b, c] - out_mu[c]) / out_std[c]
    in fp64, rounded once to fp32.  u out_std > 0 keeps the order; rounding may make neighbours equal."""
    ch = list(fields)
    B = levels.shape[0]
    scd = torch.ones(B, mu.numel(), dtype=torch.float64) if u is None else u.double()
    thr = (levels.double() / scd[:, ch].unsqueeze(-1) - mu.double()[ch].view(1, -1, 1)) / sd.double()[ch].view(1, -1, 1)
    return thr.to(torch.float32)


def mink_curves(raw):
    """raw [..., J, 5] int64 (N, Nh, Nv, Nq, Nd) -> the four integer curves [..., 4, J] of MINK_CURVES: N, edges = 4 N - 2 Nh - 2 Nv,
    chi4 = N - Nh - Nv + Nq, chi8 = chi4 - Nd."""
    N, Nh, Nv, Nq, Nd = raw.unbind(-1)
    chi4 = N - Nh - Nv + Nq
    return torch.stack([N, 4 * N - 2 * Nh - 2 * Nv, chi4, chi4 - Nd], -2)


def mink_outputs(raw, S, H, W, grid, steps=1, levels=None):
    """The Minkowski functionals of the raw excursion-set counts of S members and the target over `steps` steps of H x W pixels
    (pooled: the sums of the steps' tables): raw [..., S + 1, J, 5] int64 = (N, Nh, Nv, Nq, Nd), rows the members then the target,
    grid = (dx along W, dy along H).  Host only: every integer combination is exact in int64, every float output is formed in fp64
    and rounded to fp32 once.  With P = H W steps pixels and A = P dx dy the area -> dict:
      mink_area [..., S + 1, J]             N / P: the share of the field above the level
      mink_perimeter [..., S + 1, J]        (dy (2 N - 2 Nh) + dx (2 N - 2 Nv)) / A: boundary length per unit area, border included
      mink_edges [..., S + 1, J] int64      4 N - 2 Nh - 2 Nv: exposed unit edges
      mink_euler4, mink_euler8 [..., S + 1, J] int64   N - Nh - Nv + Nq (4-connected pieces minus 8-connected holes) and that minus
                                            Nd (8-connected pieces minus 4-connected holes)
      mink_euler4_density, mink_euler8_density [..., S + 1, J]   over A
      mink_mean, mink_std [..., 4, J]       mean and population std over the members of the integer curves MINK_CURVES (N, edges,
                                            chi4, chi8)
      mink_below, mink_equal [..., 4, J] int64   the members whose curve lies strictly below / equals the target's: the exact rank
                                            of the target within the ensemble, formed on the integers
      mink_l1 [..., S, 4]                   with levels (the physical ladder, broadcastable to [..., J]): the trapezoid integral over
                                            the ladder of |member - target| of MINK_L1_CURVES: area, perimeter and the two Euler
                                            densities as above; 0 when J = 1."""
    S, Hh, Ww, steps = int(S), int(H), int(W), int(steps)
    raw = torch.as_tensor(raw)
    if S < 1 or Hh < 1 or Ww < 1 or steps < 1 or raw.dtype != torch.int64 or raw.dim() < 3 or raw.shape[-3] != S + 1 or raw.shape[-1] != 5 \
            or raw.shape[-2] < 1:
        raise ValueError("mink_outputs takes an int64 table [..., %d, J, 5] with J >= 1 and S, H, W, steps >= 1, got %s %s"
                         % (S + 1, raw.dtype, tuple(raw.shape)))
    dx, dy = float(grid[0]), float(grid[1])
    if not (math.isfinite(dx) and math.isfinite(dy) and dx > 0 and dy > 0):
        raise ValueError("grid = (dx, dy) is finite and positive, got %r" % (grid,))
    raw = raw.cpu()
    P = Hh * Ww * steps
    A = float(P) * dx * dy
    f32 = lambda v: v.to(torch.float32)                                       # noqa: E731
    length = lambda t: dy * (2 * t[..., 0] - 2 * t[..., 1]).double() + dx * (2 * t[..., 0] - 2 * t[..., 2]).double()   # noqa: E731
    cur = mink_curves(raw)                                                    # [..., S + 1, 4, J]
    o = {"mink_area": f32(raw[..., 0].double() / float(P)), "mink_perimeter": f32(length(raw) / A),
         "mink_edges": cur[..., 1, :].contiguous(), "mink_euler4": cur[..., 2, :].contiguous(), "mink_euler8": cur[..., 3, :].contiguous()}
    o["mink_euler4_density"] = f32(o["mink_euler4"].double() / A)
    o["mink_euler8_density"] = f32(o["mink_euler8"].double() / A)
    mem, tg = cur[..., :S, :, :], cur[..., S:, :, :]
    md = mem.double()
    mean = md.mean(-3, keepdim=True)
    o["mink_mean"] = f32(mean.squeeze(-3))
    o["mink_std"] = f32(((md - mean) ** 2).mean(-3).sqrt())
    o["mink_below"] = (mem < tg).sum(-3)
    o["mink_equal"] = (mem == tg).sum(-3)
    if levels is not None:
        lv = torch.as_tensor(levels, dtype=torch.float64).cpu()
        J = raw.shape[-2]
        if lv.shape[-1] != J:
            raise ValueError("levels holds %d values per ladder, the table %d" % (lv.shape[-1], J))
        dr = raw[..., :S, :, :] - raw[..., S:, :, :]                          # exact integer differences [..., S, J, 5]
        dc = (mem - tg).abs().double()
        d = torch.stack([dc[..., 0, :] / float(P), length(dr).abs() / A, dc[..., 2, :] / A, dc[..., 3, :] / A], -2)   # [..., S, 4, J]
        wdt = (lv[..., 1:] - lv[..., :-1]).unsqueeze(-2).unsqueeze(-2)
        o["mink_l1"] = f32((0.5 * (d[..., 1:] + d[..., :-1]) * wdt).sum(-1))
    return o


class EnsembleMorphology(EnsembleFeed):
    """On-device excursion-set morphology of sampled roll-outs of B cases and of the target (tmg_ens_mink_chunk): the three Minkowski
    functionals of the sets {x > level} of a field as the level moves up a ladder: how much area lies above the level, how long
    its boundary is, and how many pieces and holes it has (the Euler characteristic, the "genus curve").  fields: 1 to 4 distinct
    channels.  thresholds: per field J (1..32) strictly ascending physical values, [F][J] for all cases or [B, F, J] per case; they
    are decided on the raw normalised values against the raw ladder of raw_thresholds' rule (u out_std > 0 keeps the order; rounding
    may make neighbours equal).  The rank of a pixel is the number of levels strictly below its value: NaN and -Inf have rank 0,
    +Inf rank J; the set of level j holds the pixels of rank > j.  Rows are the S members, then the target as row S.  Per row, case,
    kept step, field and level the device counts the pixels in the set (N), the horizontal and vertical neighbour pairs with both in
    (Nh, Nv), the 2 x 2 quads with all four in (Nq) and those with exactly a diagonal pair in (Nd), inside the field only;
    mink_outputs forms the functionals on the host.  grid = (dx along W, dy along H).

    A chunk is read straight from its NHWC rows, once for all fields and levels: no member buffer, no per-pixel state.  The device
    memory of this class is the tables, 40 Tk B F (S + 1) J bytes.  Limits: members <= 1024, B <= 65535, H W < 2^31 - 256.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target (the step's first chunk counts it).
    finalize() returns mink_raw [B, Tk, F, S + 1, J, 5] int64 on the device; mink_outputs' keys per step, [B, Tk, F, ...]; time_ of
    every key, [B, F, ...], from the raw sums summed over the steps folded with time=True (Tn of them) with H W Tn pixels as the
    area: the standard aggregation, not a mean of ratios; and mink_levels [B, F, J] float64, the physical ladder."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, fields=(0,), thresholds=((0.0,),), grid=(1.0, 1.0)):
        noun = "ensemble morphology"
        _ens_channels(noun, C)
        if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or int(steps) < 1:
            raise ValueError("%s needs steps >= 1, got %r" % (noun, steps))
        if int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s needs B, H, W >= 1, got %d, %d, %d" % (noun, B, Hh, Ww))
        if int(B) > SPELL_MAX_CASES:
            raise ValueError("%s takes at most %d cases, got %d" % (noun, SPELL_MAX_CASES, int(B)))
        if int(Hh) * int(Ww) >= 2 ** 31 - 256:
            raise ValueError("%s needs H W < 2^31 - 256, got %d x %d" % (noun, Hh, Ww))
        if isinstance(thresholds, torch.Tensor) and thresholds.dim() == 3:     # a ladder per case
            if thresholds.shape[0] != int(B):
                raise ValueError("thresholds per case are [%d, F, J], got %s" % (int(B), tuple(thresholds.shape)))
            rows = [mink_args(fields, t.tolist(), C) for t in thresholds.detach().double().cpu()]
            fl, lv = rows[0][0], torch.tensor([r[1] for r in rows], dtype=torch.float64)
        else:
            fl, th = mink_args(fields, thresholds.tolist() if isinstance(thresholds, torch.Tensor) else thresholds, C)
            lv = torch.tensor(th, dtype=torch.float64).unsqueeze(0).repeat(int(B), 1, 1)
        dx, dy = float(grid[0]), float(grid[1])
        if len(grid) != 2 or not (math.isfinite(dx) and math.isfinite(dy) and dx > 0 and dy > 0):
            raise ValueError("grid = (dx, dy) is finite and positive, got %r" % (grid,))
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.fields, self.levels, self.grid = fl, lv, (dx, dy)
        self.F, self.J = len(fl), lv.shape[2]
        self.thr = mink_raw_ladder(lv, fl, mu, sd, u).to(dev).contiguous()
        self.plan = H.ens_mink_plan(self.S, self.B, self.H, self.W, self.F, self.J)
        self.table = torch.empty((self.Tk, self.B, self.F, self.S + 1, self.J, 5), device=dev, dtype=torch.int64)

    def add(self, y, m0, target, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        first chunk zeroes the step's table and counts the target's row."""
        yn, tn, k, _, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        H.ens_mink_chunk(yn, tn, self.thr, self.fields, self.table[self._step], self.S, k, m0)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        T = self.finalize_guard()
        dev, S = self.table.device, self.S
        raw = self.table.transpose(0, 1).contiguous()
        o = {"mink_raw": raw}
        host = raw.cpu()
        for key, v in mink_outputs(host, S, self.H, self.W, self.grid, 1, self.levels.unsqueeze(1)).items():
            o[key] = v.to(dev)
        timed = host[:, self._timed].sum(1)
        o["time_mink_raw"] = timed.to(dev)
        for key, v in mink_outputs(timed, S, self.H, self.W, self.grid, T, self.levels).items():
            o["time_" + key] = v.to(dev)
        o["mink_levels"] = self.levels.clone()
        return o


DIST_MAX_CUTOFF = 255
DIST_MAX_SIDE = 4096
DIST_MAX_QUANTILES = 8
DIST_INF = 1 << 30
DIST_PAIR = ("nA", "nO", "nAO", "sOA1", "sOA2", "sAO1", "sAO2", "sD1", "sD2", "hOA", "hAO")    # the last axis of dist_pair_raw
DIST_SUMMARY = ("dist_med_miss", "dist_med_false", "dist_med", "dist_hausdorff", "dist_baddeley", "dist_csi")   # dist_mean / dist_std
DIST_FLOAT_KEYS = ("dist_med_miss", "dist_med_false", "dist_rms_miss", "dist_rms_false", "dist_med", "dist_hausdorff_miss",
                   "dist_hausdorff_false", "dist_hausdorff", "dist_hausdorff_q", "dist_baddeley", "dist_baddeley1", "dist_csi",
                   "dist_mean", "dist_std")


def dist_args(events, cutoff, quantiles, C, H, W):
    """The checks of EnsembleDistance's events, cutoff and quantiles arguments for C channels of [H, W].  events: event_args' rules
    and messages (channel in 0..C-1, finite value, '>' or '<'; 1 to 4 of them).  cutoff: the distance c in whole pixels at which the
    fixed-point distances saturate, an integer in 1..255 (no bools, no floats), or None for max(1, min(255, max(H, W) // 4)).
    quantiles: 1 to 8 probabilities in (0, 1] (no bools) of the partial Hausdorff distance.  -> (events as tuples, c, quantiles as a
    tuple of floats)."""
    ev, _ = event_args(events, (1,), C)
    if cutoff is None:
        if int(H) < 1 or int(W) < 1:
            raise ValueError("cutoff=None needs H, W >= 1, got %d, %d" % (H, W))
        c = max(1, min(DIST_MAX_CUTOFF, max(int(H), int(W)) // 4))
    elif isinstance(cutoff, bool) or not isinstance(cutoff, numbers.Integral) or not 1 <= cutoff <= DIST_MAX_CUTOFF:
        raise ValueError("cutoff is an integer in 1..%d (whole pixels) or None, got %r" % (DIST_MAX_CUTOFF, cutoff))
    else:
        c = int(cutoff)
    try:
        ql = list(quantiles)
    except TypeError:
        raise ValueError("quantiles is a sequence of probabilities, got %r" % (quantiles,))
    if not 1 <= len(ql) <= DIST_MAX_QUANTILES:
        raise ValueError("quantiles takes 1 to %d probabilities, got %d" % (DIST_MAX_QUANTILES, len(ql)))
    for q in ql:
        if isinstance(q, bool) or not isinstance(q, numbers.Real) or not 0.0 < q <= 1.0:
            raise ValueError("quantiles are probabilities in (0, 1], got %r" % (q,))
    return ev, c, tuple(float(q) for q in ql)


def dist_outputs(pair_raw, hist_raw, S, H, W, cutoff, quantiles, steps=1):
    """The distance-map scores of the raw sums of S members over `steps` steps of H x W pixels (pooled: sums added, maxima maxed):
    pair_raw [..., S, 11] = DIST_PAIR, hist_raw [..., S, 2, c + 1], int64, c = cutoff.  Host only: every float output is formed in
    fp64 from the integers and rounded to fp32 once.  Distances are in pixels.  A is a member's event set, O the target's -> dict:
      dist_med_miss [..., S]        sOA1 / (256 nO): the mean distance from the target's event pixels to the member's set (how far
                                    the misses are), distances cut at c; NaN when O is empty
      dist_med_false [..., S]       sAO1 / (256 nA): from the member's event pixels to the target's set (the false alarms); NaN when
                                    A is empty
      dist_rms_miss, dist_rms_false sqrt(sOA2 / nO) / 256 and sqrt(sAO2 / nA) / 256, NaN alike
      dist_med [..., S]             max(dist_med_miss, dist_med_false): the modified Hausdorff distance of Dubuisson & Jain; NaN
                                    when either is
      dist_hausdorff_miss, dist_hausdorff_false, dist_hausdorff [..., S]   sqrt(hOA), sqrt(hAO) and the larger: the directed and
                                    the symmetric Hausdorff distance, uncut; 0 when both sets are empty, inf when exactly one is (or
                                    when a pooled step had one set empty against a non-empty other)
      dist_hausdorff_q [..., S, 2, NQ]   the partial Hausdorff distance in whole pixels, miss then false: the smallest bin j whose
                                    cumulative count reaches ceil(q n), formed on the integers (c stands for "c or more"); NaN for
                                    an empty set
      dist_baddeley [..., S]        sqrt(sD2 / (H W steps)) / 256: Baddeley's delta with p = 2 and the cutoff transform min(d, c)
      dist_baddeley1 [..., S]       sD1 / (256 H W steps): the same with p = 1
      dist_csi [..., S]             nAO / (nA + nO - nAO): the critical success index, NaN when both sets are empty
      dist_mean, dist_std [..., 6]  mean and population std over the members of DIST_SUMMARY, non-finite values dropped; NaN
                                    when none is left
      dist_valid [..., 6] int64     the members kept."""
    import fractions
    S, Hh, Ww, steps = int(S), int(H), int(W), int(steps)
    pair_raw, hist_raw = torch.as_tensor(pair_raw), torch.as_tensor(hist_raw)
    _, c, ql = dist_args(((0, 0.0, "<"),), cutoff, quantiles, 2, Hh, Ww)
    if S < 1 or Hh < 1 or Ww < 1 or steps < 1 or pair_raw.dtype != torch.int64 or hist_raw.dtype != torch.int64 or pair_raw.dim() < 2 \
            or tuple(pair_raw.shape[-2:]) != (S, len(DIST_PAIR)) or tuple(hist_raw.shape) != tuple(pair_raw.shape[:-1]) + (2, c + 1):
        raise ValueError("dist_outputs takes int64 tables [..., %d, %d] and [..., %d, 2, %d] and S, H, W, steps >= 1, got %s %s and %s %s"
                         % (S, len(DIST_PAIR), S, c + 1, pair_raw.dtype, tuple(pair_raw.shape), hist_raw.dtype, tuple(hist_raw.shape)))
    pair, hist = pair_raw.cpu(), hist_raw.cpu()
    nA, nO, nAO, sOA1, sOA2, sAO1, sAO2, sD1, sD2, hOA, hAO = (v.double() for v in pair.unbind(-1))
    P = float(Hh * Ww * steps)
    o = {"dist_med_miss": sOA1 / (256.0 * nO), "dist_med_false": sAO1 / (256.0 * nA),
         "dist_rms_miss": (sOA2 / nO).sqrt() / 256.0, "dist_rms_false": (sAO2 / nA).sqrt() / 256.0}
    o["dist_med"] = torch.maximum(o["dist_med_miss"], o["dist_med_false"])
    noA, noO = pair[..., 0] == 0, pair[..., 1] == 0
    inf, zero = torch.full_like(nA, float("inf")), torch.zeros_like(nA)

    def directed(h):
        v = torch.where(h >= float(DIST_INF), inf, h.clamp(min=0.0).sqrt())
        return torch.where(noA & noO, zero, torch.where(noA | noO, inf, v))
    o["dist_hausdorff_miss"], o["dist_hausdorff_false"] = directed(hOA), directed(hAO)
    o["dist_hausdorff"] = torch.maximum(o["dist_hausdorff_miss"], o["dist_hausdorff_false"])
    # the quantiles: ceil(q n) in exact rational arithmetic on the integer n, then a count of the bins whose cumulative sum is short
    cum = hist.cumsum(-1)
    n = cum[..., -1]
    hq = []
    for q in ql:
        fq = fractions.Fraction(q)
        need = torch.tensor([-((-int(v) * fq.numerator) // fq.denominator) for v in n.reshape(-1).tolist()], dtype=torch.int64).reshape(n.shape)
        j = (cum < need.unsqueeze(-1)).sum(-1).double()
        hq.append(torch.where(n > 0, j, torch.full_like(j, float("nan"))))
    o["dist_hausdorff_q"] = torch.stack(hq, -1)
    o["dist_baddeley"] = (sD2 / P).sqrt() / 256.0
    o["dist_baddeley1"] = sD1 / (256.0 * P)
    o["dist_csi"] = nAO / (nA + nO - nAO)
    stack = torch.stack([o[k] for k in DIST_SUMMARY], -1)                       # [..., S, 6]
    ok = torch.isfinite(stack)
    cnt = ok.sum(-2)
    val = torch.where(ok, stack, torch.zeros_like(stack))
    mean = val.sum(-2) / cnt.double()                                          # 0 / 0: NaN
    dev = torch.where(ok, stack - mean.unsqueeze(-2), torch.zeros_like(stack))
    o["dist_mean"] = mean
    o["dist_std"] = ((dev * dev).sum(-2) / cnt.double()).sqrt()
    o = {k: v.to(torch.float32) for k, v in o.items()}
    o["dist_valid"] = cnt.to(torch.int64)
    return o


def dist_pool(pair_raw, hist_raw, dim):
    """The tables of several steps pooled along `dim`: sums added, the two maxima (hOA, hAO) maxed, so that a -1 (an empty set)
    stays only when every step's is -1 -> (pair, hist)."""
    pair = torch.cat([pair_raw[..., :9].sum(dim), pair_raw[..., 9:].max(dim).values], -1)
    return pair, hist_raw.sum(dim)


class EnsembleDistance(EnsembleFeed):
    """On-device distance-map verification of sampled roll-outs of B cases against the target (tmg_ens_edt_chunk / tmg_ens_edt_step):
    how far a member's event set lies from the target's, which overlap, neighbourhood, scale and morphology scores do not say (a
    bubble drawn six pixels downstream and one a quarter of the domain away both have zero overlap).  An event k is (channel, value,
    ">" | "<"), strict, in physical units ((0, 0.0, "<") is reverse flow), decided on the raw normalised values against
    raw_thresholds (u out_std > 0 keeps the order); a value that compares false (NaN, an infinity on the wrong side) is in no event.
    Per case, kept step and event, A is a member's event set and O the target's.  The device forms the exact squared Euclidean
    distance d2_A(p) of every pixel to A (an integer, in pixels, over the whole field, INF = 2^30 for an empty set), likewise d2_O,
    and from them, with the fixed-point distance w = 256 c if d2 >= c^2 else isqrt(65536 d2) (floor(256 d), c = cutoff in 1..255
    pixels, None: max(1, min(255, max(H, W) // 4))), the eleven integers DIST_PAIR per member, two histograms of the whole-pixel
    distances and per-pixel sums; dist_outputs forms the mean error distance, the Hausdorff distances, their quantiles, Baddeley's
    delta and the critical success index on the host.  Everything the device forms is an integer: bitwise the same for every
    chunking and run.

    A chunk is read straight from its NHWC rows.  The device memory of this class: the indicator words, 8 (S + 1) B K H ceil(W / 64)
    bytes; the target's map and the step's member sum, 4 B K HW bytes each; the two time maps, 8 B K HW bytes each; the set sizes,
    4 B K (S + 1) bytes; and the tables, 8 Tk B K S (11 + 2 (c + 1)) bytes.  Limits: members <= 1024, B <= 65535, H, W <= 4096,
    H W < 2^31 - 256.  Not supported: anisotropic metrics (pixels are the unit, as for the FSS widths and the Haar blocks), periodic
    domains, Pratt's figure of merit, distances finer than 1 / 256 pixel.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target (the step's first chunk forms its distance map).
    finalize() returns dist_pair_raw [B, Tk, K, S, 11] and dist_hist_raw [B, Tk, K, S, 2, c + 1] int64 on the device; dist_outputs'
    keys per step, [B, Tk, K, ...]; time_ of every key, [B, K, ...], from the raw sums pooled over the steps folded with time=True (Tn
    of them: sums added, maxima maxed, H W Tn pixels as the area: the standard aggregation, not a mean of ratios);
    time_dist_member_sum and time_dist_target_sum [B, K, H, W] int64, the sums over those steps (and the members) of w_A(p) and of
    w_O(p); time_dist_mean_map = member_sum / (256 S Tn), the ensemble's mean distance from the pixel to the event, and
    time_dist_bias_map = that minus target_sum / (256 Tn), positive where the ensemble keeps the event farther from the pixel than
    the target does; dist_cutoff (int64 scalar) and dist_quantiles [NQ] float64."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, events=((0, 0.0, "<"),), cutoff=None,
                 quantiles=(0.5, 0.75, 0.9)):
        noun = "ensemble distance maps"
        _ens_channels(noun, C)
        if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or int(steps) < 1:
            raise ValueError("%s need steps >= 1, got %r" % (noun, steps))
        if int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need B, H, W >= 1, got %d, %d, %d" % (noun, B, Hh, Ww))
        ev, c, ql = dist_args(events, cutoff, quantiles, C, Hh, Ww)
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        if int(B) > SPELL_MAX_CASES:
            raise ValueError("%s take at most %d cases, got %d" % (noun, SPELL_MAX_CASES, int(B)))
        if int(Hh) > DIST_MAX_SIDE or int(Ww) > DIST_MAX_SIDE:
            raise ValueError("%s need H, W <= %d, got %d x %d" % (noun, DIST_MAX_SIDE, Hh, Ww))
        if int(Hh) * int(Ww) >= 2 ** 31 - 256:
            raise ValueError("%s need H W < 2^31 - 256, got %d x %d" % (noun, Hh, Ww))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        S, Tk, HW, K = self.S, self.Tk, self.H * self.W, len(ev)
        self.K, self.cutoff, self.quantiles = K, c, ql
        self.events = ev
        self.ev = _ens_directions(ev)
        self.thr = raw_thresholds(ev, self.B, C, mu, sd, u).to(dev).contiguous()
        self.plan = H.ens_edt_plan(S, self.B, self.H, self.W, K, c)
        i32, i64 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.int64)
        self.scratch = torch.empty((S + 1, self.B, K, self.H, self.plan["strips"]), **i64)
        self.count = torch.empty((self.B, K, S + 1), **i32)
        self.dmap = torch.empty((self.B, K, HW), **i32)
        self.msum = torch.empty((self.B, K, HW), **i32)
        self.pair = torch.empty((Tk, self.B, K, S, len(DIST_PAIR)), **i64)
        self.hist = torch.empty((Tk, self.B, K, S, 2, c + 1), **i64)
        self.tmem = torch.zeros((self.B, K, HW), **i64)
        self.ttgt = torch.zeros((self.B, K, HW), **i64)

    def add(self, y, m0, target, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        first chunk presets the step's tables and forms the target's distance map; its last chunk, with time=True, folds the step
        into the time maps."""
        yn, tn, k, _, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        t = self._step
        H.ens_edt_chunk(yn, tn, self.thr, self.ev, self.scratch, self.count, self.dmap, self.msum, self.pair[t], self.hist[t], self.S, k, m0)
        if last and time:
            H.ens_edt_step(self.msum, self.dmap, self.tmem, self.ttgt, self.H, self.W, self.cutoff)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        T = self.finalize_guard()
        dev, S = self.pair.device, self.S
        pair, hist = self.pair.transpose(0, 1).contiguous(), self.hist.transpose(0, 1).contiguous()
        o = {"dist_pair_raw": pair, "dist_hist_raw": hist}
        hp, hh = pair.cpu(), hist.cpu()
        for key, v in dist_outputs(hp, hh, S, self.H, self.W, self.cutoff, self.quantiles).items():
            o[key] = v.to(dev)
        tp, th = dist_pool(hp[:, self._timed], hh[:, self._timed], 1)
        o["time_dist_pair_raw"], o["time_dist_hist_raw"] = tp.to(dev), th.to(dev)
        for key, v in dist_outputs(tp, th, S, self.H, self.W, self.cutoff, self.quantiles, T).items():
            o["time_" + key] = v.to(dev)
        shp = (self.B, self.K, self.H, self.W)
        o["time_dist_member_sum"], o["time_dist_target_sum"] = self.tmem.view(shp), self.ttgt.view(shp)
        mean = self.tmem.view(shp).double() / (256.0 * S * T)
        o["time_dist_mean_map"] = mean.to(torch.float32)
        o["time_dist_bias_map"] = (mean - self.ttgt.view(shp).double() / (256.0 * T)).to(torch.float32)
        o["dist_cutoff"] = torch.tensor(self.cutoff, dtype=torch.int64)
        o["dist_quantiles"] = torch.tensor(self.quantiles, dtype=torch.float64)
        return o


PDF_MAX_FIELDS = 8
PDF_MAX_BINS = 128
PDF_MAX_JOINT_BINS = 32
PDF_MAX_PAIRS = 2
PDF_MAX_REGIONS = 4
PDF_ALIASES = {"ux": 0, "uy": 1, "p": 2}
PDF_DERIVED = H.PDF_KINDS                                                      # "speed", "vort", "div" -> the kernel's kind codes


def _pdf_kind(f, C):
    """A field entry -> the kernel's kind code, or None."""
    if isinstance(f, str):
        k = PDF_ALIASES.get(f, PDF_DERIVED.get(f))
        return k if k is not None and (k >= 4 or k < C) else None
    if isinstance(f, bool) or not isinstance(f, numbers.Integral) or not 0 <= f < C:
        return None
    return int(f)


def pdf_args(fields, bins, ranges, joint, joint_bins, regions, grid, B, C, Hh, Ww):
    """The checks of EnsemblePdfs' arguments for B cases of C channels of [Hh, Ww]; the first offending entry is named.
    fields: 1 to 8 entries, each a channel 0..C-1 (aliases "ux", "uy", "p"), "speed", "vort" or "div"; the derived ones need
    grid = (dx, dy), two positive finite cell sizes.  bins: 1..128 (no bools, no floats); joint_bins: 1..32.  ranges: one finite
    (lo, hi), lo < hi, per field, or an array [B, F, 2].  joint: up to 2 pairs of distinct listed fields (an entry names the first field of its kind in the list).  regions: None (the whole
    field) or 1 to 4 integer boxes (x0, x1, y0, y1), half open, non-empty, inside the field.
    -> (kinds, nb, ranges as an fp64 CPU tensor [B, F, 2], pairs as field indices, nbj, regions as tuples of ints, grid or None)."""
    fl = list(fields)
    if not (1 <= len(fl) <= PDF_MAX_FIELDS):
        raise ValueError("fields takes 1 to %d entries, got %d" % (PDF_MAX_FIELDS, len(fl)))
    kinds = []
    for f in fl:
        k = _pdf_kind(f, C)
        if k is None:
            raise ValueError("fields are channels in 0..%d (\"ux\", \"uy\", \"p\" for 0, 1, 2), \"speed\", \"vort\" or \"div\", got %r" % (C - 1, f))
        kinds.append(k)
    F = len(kinds)
    for name, v, top in (("bins", bins, PDF_MAX_BINS), ("joint_bins", joint_bins, PDF_MAX_JOINT_BINS)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= top:
            raise ValueError("%s is an integer in 1..%d, got %r" % (name, top, v))
    if any(k >= 4 for k in kinds):
        if grid is None:
            raise ValueError("the derived field %r needs grid=(dx, dy)" % (fl[[k >= 4 for k in kinds].index(True)],))
    if grid is not None:
        grid = tuple(float(g) for g in grid)
        if len(grid) != 2 or not all(math.isfinite(g) and g > 0 for g in grid):
            raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %s" % (grid,))
    if ranges is None:
        raise ValueError("ranges needs one (lo, hi) per field, or an array [B, F, 2]")
    rg = torch.as_tensor(ranges, dtype=torch.float64).detach().cpu()
    if tuple(rg.shape) == (F, 2):
        rg = rg.unsqueeze(0).expand(B, F, 2)
    if tuple(rg.shape) != (B, F, 2):
        raise ValueError("ranges needs one (lo, hi) per field, or an array [%d, %d, 2], got shape %s" % (B, F, tuple(rg.shape)))
    rg = rg.contiguous()
    for b in range(B):
        for f in range(F):
            lo, hi = float(rg[b, f, 0]), float(rg[b, f, 1])
            if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
                raise ValueError("ranges are finite (lo, hi) with lo < hi, got (%r, %r) for field %r of case %d" % (lo, hi, fl[f], b))
    jl = [tuple(pr) for pr in joint]
    if len(jl) > PDF_MAX_PAIRS:
        raise ValueError("joint takes at most %d pairs, got %d" % (PDF_MAX_PAIRS, len(jl)))
    pairs = []
    for pr in jl:
        ks = [_pdf_kind(f, C) for f in pr] if len(pr) == 2 else [None]
        if any(k is None or k not in kinds for k in ks) or ks[0] == ks[1]:
            raise ValueError("joint entries are pairs of distinct listed fields, got %r" % (pr,))
        pairs.append((kinds.index(ks[0]), kinds.index(ks[1])))
    if regions is None:
        regs = [(0, int(Ww), 0, int(Hh))]
    else:
        regs = [tuple(r) for r in regions]
        if not (1 <= len(regs) <= PDF_MAX_REGIONS):
            raise ValueError("regions takes 1 to %d boxes, got %d" % (PDF_MAX_REGIONS, len(regs)))
        for r in regs:
            if len(r) != 4 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in r) \
                    or not (0 <= r[0] < r[1] <= Ww and 0 <= r[2] < r[3] <= Hh):
                raise ValueError("regions are integer boxes (x0, x1, y0, y1), half open, non-empty and inside the %d x %d field, got %r"
                                 % (Hh, Ww, r))
        regs = [tuple(int(v) for v in r) for r in regs]
    return kinds, int(bins), rg, pairs, int(joint_bins), regs, grid


def pdf_edge_tables(kinds, ranges, n, mu, sd, u=None, centered=False):
    """The edges of n uniform bins per case and field: E_j = lo + j (hi - lo) / n in fp64 (physical), and the device table in fp64
    rounded once to fp32: a channel field (E_j / u[b, c] - mu[c]) / sd[c], with a centre E_j / (u[b, c] sd[c]); a derived field E_j
    itself (ranges: [B, F, 2] fp64, mu, sd: [C] fp32 CPU tensors, u: [B, C] fp32 CPU tensor or None for 1).  Edges that are not
    strictly increasing after rounding are a ValueError.  -> (E [B, F, n + 1] fp64, e [B, F, n + 1] fp32), CPU tensors."""
    B, F = ranges.shape[:2]
    j = torch.arange(n + 1, dtype=torch.float64)
    lo, hi = ranges[..., 0:1], ranges[..., 1:2]
    E = lo + j * (hi - lo) / n
    e = E.clone()
    scd = torch.ones(B, mu.numel(), dtype=torch.float64) if u is None else u.double()
    for f, k in enumerate(kinds):
        if k < 4:
            e[:, f] = E[:, f] / (scd[:, k:k + 1] * sd.double()[k]) if centered else (E[:, f] / scd[:, k:k + 1] - mu.double()[k]) / sd.double()[k]
    e = e.to(torch.float32)
    bad = (e[..., 1:] <= e[..., :-1]).any(-1).nonzero()
    if bad.numel():
        raise ValueError("the edges of field %d of case %d are not strictly increasing after rounding to fp32: [%r, %r] in %d bins"
                         % (int(bad[0, 1]), int(bad[0, 0]), float(ranges[bad[0, 0], bad[0, 1], 0]), float(ranges[bad[0, 0], bad[0, 1], 1]), n))
    return E, e


def pdf_density(cnt, h):
    """cnt [..., nb + 2] int64 (under- and overflow first and last), h the bin width broadcastable to [..., 1] -> the density of the
    inner bins [..., nb] in fp64: inner count / (all counts h), so that what is out of range is missing from the integral; NaN
    without a sample."""
    return cnt[..., 1:-1].double() / (cnt.sum(-1, keepdim=True).double() * h)


def pdf_w1(p, q, h):
    """The Wasserstein-1 distance between the distributions of the counts p, q [..., nb + 2] int64 with each bin's mass at its
    centre (the under- and overflow masses one width outside): h sum_{j=0}^{nb} |F_j - G_j| with F, G the cumulative shares, in fp64;
    h broadcastable to [...].  NaN when either holds no sample."""
    F = p.cumsum(-1)[..., :-1].double() / p.sum(-1, keepdim=True).double()
    G = q.cumsum(-1)[..., :-1].double() / q.sum(-1, keepdim=True).double()
    return (F - G).abs().sum(-1) * h


def pdf_js(p, q):
    """The Jensen-Shannon divergence in bits between the distributions of the counts p, q [..., n] int64, 0 log 0 = 0: in [0, 1];
    NaN when either holds no sample.  fp64."""
    P = p.double() / p.sum(-1, keepdim=True).double()
    Q = q.double() / q.sum(-1, keepdim=True).double()
    M = 0.5 * (P + Q)
    one = torch.ones_like(M)
    kl = lambda A: torch.where(A > 0, A * torch.log2(torch.where(A > 0, A, one) / torch.where(A > 0, M, one)), torch.zeros_like(A))   # noqa: E731
    out = 0.5 * (kl(P).sum(-1) + kl(Q).sum(-1))
    return torch.where(torch.isnan(P.sum(-1) + Q.sum(-1)), torch.full_like(out, float("nan")), out)


class EnsemblePdfs(EnsembleFeed):
    """On-device probability densities of the flow quantities pooled over regions of the flow, for sampled roll-outs of B cases and
    for the target (tmg_ens_pdf_count).  fields: up to 8 of a channel 0..C-1 ("ux", "uy", "p" for 0, 1, 2), "speed", "vort", "div"
    (the derived ones on grid = (dx, dy): the 3x3 stencil of pc/ with zero padding at the field border, every fp32 operation rounded
    on its own).  Each field has `bins` uniform bins over its physical range (lo, hi) of `ranges` (per field, or [B, F, 2] per case)
    plus an underflow and an overflow bin; a value on an edge belongs to the bin above.  A channel field is binned on its raw
    normalised value against the edges (E / u - out_mu) / out_std (u out_std > 0 keeps the order: no rounding); center [B, C, H, W]
    (physical) subtracts c_raw = float32((center / u - out_mu) / out_std) first, one rounded fp32 subtraction, against the edges
    E / (u out_std): fluctuations about a given mean flow.  joint: up to 2 pairs of listed fields with joint_bins bins per axis over
    the same ranges; the first field indexes the rows.  regions: up to 4 pixel boxes (x0, x1, y0, y1), half open, x along W; they
    may overlap; default the whole field.  Non-finite members are not supported.

    The counts fold chunk by chunk by integer adds: no member buffer is kept, and every integer output is bitwise reproducible and
    independent of the chunking.  The target goes through the same kernel as a one-member chunk into planes of its own.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is used.
    Outputs of finalize() (device tensors; Tn steps folded with time=True, nb = bins, nbj = joint_bins):
      pdf_count, target_count [B, Tk, R, F, nb + 2] int64; joint_count, target_joint_count [B, Tk, R, P, nbj + 2, nbj + 2] int64
      time_member_count [B, S, R, F, nb + 2], time_count (its sum over the members), time_target_count [B, R, F, nb + 2],
      time_joint_count, time_target_joint_count [B, R, P, nbj + 2, nbj + 2] int64
      pdf, target_pdf [B, Tk, R, F, nb]: inner count / (all counts * bin width); time_pdf, time_target_pdf [B, R, F, nb] (pooled);
      time_pdf_mean, time_pdf_std: mean / population std over the members of each member's own time-pooled density
      w1, js [B, Tk, R, F], time_w1, time_js [B, R, F]: Wasserstein-1 (physical units) and Jensen-Shannon divergence (bits, over
      the nb + 2 bins) of the pooled ensemble against the target; time_member_w1 [B, S, R, F]; time_joint_js [B, R, P]
      (formed on the host in fp64 from the integers, rounded once; NaN for a distribution without samples)
      pdf_edges [B, F, nb + 1], joint_edges [B, P, 2, nbj + 1], pdf_ranges [B, F, 2] fp64 physical; pdf_fields, pdf_joint,
      pdf_regions as given."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, fields=("ux", "uy"), bins=64, ranges=None, joint=(),
                 joint_bins=32, regions=None, grid=None, center=None):
        noun = "ensemble pdfs"
        _ens_channels(noun, C)
        if int(steps) < 1:
            raise ValueError("%s need steps >= 1, got %d" % (noun, int(steps)))
        if int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need B, H, W >= 1, got %d, %d, %d" % (noun, B, Hh, Ww))
        kinds, nb, rg, pairs, nbj, regs, grid = pdf_args(fields, bins, ranges, joint, joint_bins, regions, grid, int(B), C, int(Hh), int(Ww))
        _ens_members(noun, members)
        sd, mu = _ens_tables(C, _KEEPS_ORDER, out_std, out_mu)
        u = _ens_u(u, B, C, _KEEPS_ORDER)
        S, Tk, HW = int(members), int(steps), int(Hh) * int(Ww)
        for name, v in (("S H W", S * HW), ("Tk H W", Tk * HW), ("S Tk H W", S * Tk * HW)):
            if v >= 2 ** 31:
                raise ValueError("%s = %d does not stay under 2^31 (the int32 counts)" % (name, v))
        cen = None
        if center is not None:
            cen = torch.as_tensor(center, dtype=torch.float32).detach().cpu()
            if tuple(cen.shape) != (int(B), C, int(Hh), int(Ww)) or not bool(torch.isfinite(cen).all()):
                raise ValueError("center is a finite array [%d, %d, %d, %d] in physical units, got shape %s" % (B, C, Hh, Ww, tuple(cen.shape)))
            scd = torch.ones(int(B), C, dtype=torch.float64) if u is None else u.double()
            cen = ((cen.double() / scd.view(int(B), C, 1, 1) - mu.double().view(1, C, 1, 1)) / sd.double().view(1, C, 1, 1)).to(torch.float32)
        self.E, e = pdf_edge_tables(kinds, rg, nb, mu, sd, u, cen is not None)
        jk = [kinds[i] for pr in pairs for i in pr]
        jr = rg[:, [i for pr in pairs for i in pr]] if pairs else rg[:, :0]
        self.JE, je = pdf_edge_tables(jk, jr, nbj, mu, sd, u, cen is not None)
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.fields, self.joint, self.regions = tuple(fields), tuple(tuple(pr) for pr in joint), tuple(regs)
        self.kinds, self.pairs, self.nb, self.nbj, self.grid = kinds, pairs, nb, nbj, grid
        self.F, self.P, self.R = len(kinds), len(pairs), len(regs)
        self.ranges = rg
        self.e, self.je = e.to(dev).contiguous(), je.to(dev).contiguous()
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).contiguous()
        self.cen = None if cen is None else cen.reshape(self.B, C, HW).to(dev).contiguous()
        self.derived = any(k >= 4 for k in kinds)
        self.plan = H.ens_pdf_plan(1, self.B, self.H, self.W, self.F, nb, self.P, nbj, self.R, self.derived)
        i32 = dict(device=dev, dtype=torch.int32)
        jb = (nbj + 2) ** 2
        # [0]: the ensemble's planes, [1]: the target's (a one-member ensemble: S = 1)
        self.cnt = torch.empty((2, self.B, Tk, self.R, self.F, nb + 2), **i32)
        self.jnt = torch.empty((2, self.B, Tk, self.R, self.P, jb), **i32)
        self.mt = (torch.empty((self.B, S, self.R, self.F, nb + 2), **i32), torch.empty((self.B, 1, self.R, self.F, nb + 2), **i32))
        self.tj = torch.empty((2, self.B, self.R, self.P, jb), **i32)

    def _count(self, which, yn, S, k, m0, t, timed):
        marg, jb = self.R * self.F * (self.nb + 2), self.R * self.P * (self.nbj + 2) ** 2
        H.ens_pdf_count(yn, self.u, self.mu, self.sd, self.cen, self.e, self.je if self.P else None, self.kinds, self.pairs, self.regions,
                        self.cnt[which, :, t], self.jnt[which, :, t] if self.P else None, self.mt[which], self.tj[which] if self.P else None,
                        (self.Tk * marg, self.Tk * jb), self.grid, S, k, m0, self.nb, self.nbj, 1 if timed else 0)

    def add(self, y, m0, target, time=True):
        """Bin the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        first chunk zeroes the step's planes (the first timed one the time planes), the last chunk bins the target."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        t = self._step
        if m0 == 0:
            self.cnt[:, :, t].zero_()
            self.jnt[:, :, t].zero_()
            if time and t_before == 0:
                self.mt[0].zero_()
                self.mt[1].zero_()
                self.tj.zero_()
        self._count(0, yn, self.S, k, m0, t, time)
        if last:
            self._count(1, tn, 1, 1, 0, t, time)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        self.finalize_guard()
        dev = self.cnt.device
        f32 = lambda v: v.to(torch.float32).to(dev)                            # noqa: E731
        nj = self.nbj + 2
        cnt, jnt = self.cnt.cpu().to(torch.int64), self.jnt.cpu().to(torch.int64)
        mt, tmt, tj = self.mt[0].cpu().to(torch.int64), self.mt[1].cpu().to(torch.int64)[:, 0], self.tj.cpu().to(torch.int64)
        ints = {"pdf_count": cnt[0], "target_count": cnt[1], "joint_count": jnt[0].view(self.B, self.Tk, self.R, self.P, nj, nj),
                "target_joint_count": jnt[1].view(self.B, self.Tk, self.R, self.P, nj, nj), "time_member_count": mt,
                "time_count": mt.sum(1), "time_target_count": tmt, "time_joint_count": tj[0].view(self.B, self.R, self.P, nj, nj),
                "time_target_joint_count": tj[1].view(self.B, self.R, self.P, nj, nj)}
        o = {key: v.to(dev) for key, v in ints.items()}
        h = (self.ranges[..., 1] - self.ranges[..., 0]) / self.nb                # [B, F] fp64
        h5, h4 = h.view(self.B, 1, 1, self.F, 1), h.view(self.B, 1, self.F, 1)
        o["pdf"], o["target_pdf"] = f32(pdf_density(cnt[0], h5)), f32(pdf_density(cnt[1], h5))
        tc = ints["time_count"]
        o["time_pdf"], o["time_target_pdf"] = f32(pdf_density(tc, h4)), f32(pdf_density(tmt, h4))
        dm = pdf_density(mt, h5)                                               # [B, S, R, F, nb]
        o["time_pdf_mean"], o["time_pdf_std"] = f32(dm.mean(1)), f32(dm.std(1, unbiased=False))
        o["w1"], o["js"] = f32(pdf_w1(cnt[0], cnt[1], h5[..., 0])), f32(pdf_js(cnt[0], cnt[1]))
        o["time_w1"], o["time_js"] = f32(pdf_w1(tc, tmt, h4[..., 0])), f32(pdf_js(tc, tmt))
        o["time_member_w1"] = f32(pdf_w1(mt, tmt.unsqueeze(1), h5[..., 0]))
        o["time_joint_js"] = f32(pdf_js(tj[0], tj[1]))
        o["pdf_edges"], o["joint_edges"] = self.E, self.JE.view(self.B, self.P, 2, self.nbj + 1)
        o["pdf_ranges"] = self.ranges
        o["pdf_fields"], o["pdf_joint"], o["pdf_regions"] = self.fields, self.joint, self.regions
        return o


def energy_groups(groups, C):
    """The checks of EnsembleEnergy's groups argument for C channels: non-empty tuples of distinct channels in 0..C-1, every channel in
    at most one group -> the groups as a tuple of tuples of ints."""
    try:
        gs = tuple(tuple(g) for g in groups)
    except TypeError:
        raise ValueError("groups must be tuples of channels, got %r" % (groups,))
    seen = set()
    if not gs:
        raise ValueError("groups must hold at least one group of channels, got %r" % (groups,))
    for g in gs:
        if not g:
            raise ValueError("groups must be non-empty tuples of channels, got %r" % (groups,))
        for ch in g:
            if isinstance(ch, bool) or not isinstance(ch, numbers.Integral) or not 0 <= ch < C or int(ch) in seen:
                raise ValueError("groups hold distinct channels in 0..%d, each in at most one group, got %r" % (C - 1, groups))
            seen.add(int(ch))
    return tuple(tuple(int(ch) for ch in g) for g in gs)


ENERGY_STEP_KEYS = ("energy_score", "energy_score_fair", "target_dist_mean", "pair_dist_mean", "nearest_dist")


class EnsembleEnergy(EnsembleFeed):
    """On-device energy score and member distances of sampled roll-outs of B cases against the target (tmg_ens_score_store /
    tmg_ens_gram_step): the score of every member as ONE vector over the pixels, which no per-pixel score can see.  For case b and
    kept step t, with the rows x_0..x_{S-1} (raw normalised members) and x_S = y (the normalised target), a_c = u[b, c] out_std[c] > 0
    and the channel groups g (tuples of channels that share a unit; default for 3 channels ((0, 1), (2,)): velocity and pressure):
      d2_g[m, n] = sum_{c in g} a_c^2 sum_p (x_m - x_n)^2,  dist = sqrt(d2)            the distance of two fields in physical units
      target_dist_mean = (1/S) sum_{m<S} dist[m, S],  pair_dist_mean = (2/S^2) sum_{m<n<S} dist[m, n]
      energy_score = target_dist_mean - pair_dist_mean / 2; energy_score_fair: 1 / (S (S - 1)) for 1 / S^2 (S = 1: the pair term is 0)
      medoid = argmin_{m<S} sum_{n<S} dist[m, n],  nearest = argmin_{m<S} dist[m, S] (ties: the lowest member), nearest_dist
    out_mu cancels in every term and is not an input.  The kernels form d2 from the Gram matrix of the rows centred about the members'
    mean (csrc/tmg_gram.hip), on the fp32 matrix pipe.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is scored.
    Outputs (device tensors, Gn groups): energy_score, energy_score_fair, target_dist_mean, pair_dist_mean, nearest_dist [B, Tk, Gn]
    float32; medoid, nearest [B, Tk, Gn] int64; finalize() adds, over the steps folded with time=True, time_energy_score,
    time_energy_score_fair [B, Gn] (the means of the per-step scores), traj_dist2 [B, Gn, S + 1, S + 1] (the sum of d2: the squared
    distance between whole roll-outs, space and time as one vector; symmetric, zero diagonal, the target last), traj_energy_score,
    traj_energy_score_fair [B, Gn] and traj_medoid, traj_nearest [B, Gn] int64 (the same formulas on sqrt(traj_dist2))."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_std, u=None, groups=None):
        noun, why = "ensemble energy scores", "the distances scale with u * out_std"
        _ens_channels(noun, C)
        _ens_members(noun, members)
        sd, _ = _ens_tables(C, why, out_std)
        u = _ens_u(u, B, C, why)
        if groups is None:
            groups = ((0, 1), (2,)) if C == 3 else (tuple(range(C)),)
        self.groups = energy_groups(groups, C)
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        HW = self.H * self.W
        Gn = len(self.groups)
        f32 = dict(device=dev, dtype=torch.float32)
        # a_c^2 = (u out_std)^2 in fp64 from the fp32 factors, rounded once
        a = _ens_scale(sd, u, self.B, torch.float64)
        self.a2 = (a * a).to(torch.float32).to(dev).contiguous()
        self.plan = H.ens_gram_plan(self.S, self.B, C, HW)
        self.xs = torch.empty((self.S, self.B, C, HW), **f32)
        self.r = torch.empty((self.B, C, HW), **f32)
        self.ws = torch.empty((self.plan["ws"],), **f32)
        self.traj = torch.empty((self.B, Gn, self.S + 1, self.S + 1), **f32)
        self.outf = torch.empty((5, self.B, self.Tk, Gn), **f32)
        self.outi = torch.empty((2, self.B, self.Tk, Gn), device=dev, dtype=torch.int64)
        self.out = dict(zip(ENERGY_STEP_KEYS, self.outf))
        self.out["medoid"], self.out["nearest"] = self.outi[0], self.outi[1]

    def add(self, y, m0, target, time=True):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk scores the step against its target."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        H.ens_score_store(yn, self.xs, k, m0)
        if last:
            H.ens_gram_step(self.xs, tn, self.a2, self.groups, self.r, self.ws, self.traj, self.outf, self.outi, self._step, t_before,
                            1 if time else 0)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time statistics cover the steps folded with time=True."""
        self.finalize_guard()
        o = self.out
        Gn = len(self.groups)
        tf = torch.empty((5, self.B, Gn), device=self.traj.device, dtype=torch.float32)
        ti = torch.empty((2, self.B, Gn), device=self.traj.device, dtype=torch.int64)
        H.ens_gram_traj(self.traj, tf, ti)
        o["traj_dist2"] = self.traj
        o["traj_energy_score"], o["traj_energy_score_fair"] = tf[0], tf[1]
        o["traj_medoid"], o["traj_nearest"] = ti[0], ti[1]
        o["time_energy_score"] = o["energy_score"][:, self._timed].double().mean(dim=1).to(torch.float32)
        o["time_energy_score_fair"] = o["energy_score_fair"][:, self._timed].double().mean(dim=1).to(torch.float32)
        return o


def fieldrank_hist(below, equal, S):
    """The rank histogram of a target whose pre-rank lies above `below` members and ties with `equal` of them, over the steps of
    dim 1: below, equal [B, Tn, G] integer tensors with 0 <= below, 0 <= equal, below + equal <= S -> [B, G, S + 1] float64.  Step
    n adds 1 / (equal + 1) to every bin below .. below + equal: the expectation of random tie-breaking, which is deterministic.  The
    steps are added in order, one elementwise fp64 addition each; every histogram sums to Tn.  Host work: no device is needed."""
    S = int(S)
    below, equal = torch.as_tensor(below).to(torch.int64).cpu(), torch.as_tensor(equal).to(torch.int64).cpu()
    if S < 1 or below.dim() != 3 or below.shape != equal.shape:
        raise ValueError("fieldrank_hist takes below and equal of one shape [B, Tn, G] and S >= 1, got %s, %s, S=%d"
                         % (tuple(below.shape), tuple(equal.shape), S))
    if below.numel() and (int(below.min()) < 0 or int(equal.min()) < 0 or int((below + equal).max()) > S):
        raise ValueError("fieldrank_hist needs 0 <= below, 0 <= equal and below + equal <= S = %d" % S)
    B, Tn, G = below.shape
    bins = torch.arange(S + 1, dtype=torch.int64).view(1, 1, S + 1)
    hist = torch.zeros((B, G, S + 1), dtype=torch.float64)
    for n in range(Tn):
        lo, k = below[:, n].unsqueeze(-1), equal[:, n].unsqueeze(-1)
        hist += ((bins >= lo) & (bins <= lo + k)).to(torch.float64) / (k + 1).to(torch.float64)
    return hist


def _fieldrank_of_target(pre):
    """pre [.., S + 1] int64, the target last -> (below, equal): the members whose pre-rank is under / equal to the target's."""
    return (pre[..., :-1] < pre[..., -1:]).sum(-1), (pre[..., :-1] == pre[..., -1:]).sum(-1)


def _fieldrank_median(pre):
    """pre [.., S + 1] int64 -> the member m < S with the largest pre-rank, the smallest index on ties."""
    m = pre[..., :-1]
    S = m.shape[-1]
    idx = torch.arange(S, dtype=torch.int64).expand(m.shape)
    return torch.where(m == m.max(-1, keepdim=True).values, idx, torch.full_like(idx, S)).min(-1).values


def fieldrank_outputs(pre_raw, outside_count, time_outside_count, groups, timed):
    """The host side of EnsembleFieldRanks.finalize(): the device's integer sums pre_raw [B, Tk, C, S + 1, 2], outside_count
    [B, Tk, C] and time_outside_count [B, C, H, W] (int64 CPU tensors), the channel groups and the list of timed steps -> the dict
    of outputs of the class docstring.  int64 and fp64 only; no device is needed."""
    raw = pre_raw
    B, Tk, C, R, _ = raw.shape
    timed = [int(t) for t in timed]
    if raw.dtype != torch.int64 or raw.dim() != 5 or raw.shape[4] != 2 or R < 2 or tuple(outside_count.shape) != (B, Tk, C) \
            or time_outside_count.dim() != 4 or tuple(time_outside_count.shape[:2]) != (B, C) or not timed \
            or any(not 0 <= t < Tk for t in timed):
        raise ValueError("fieldrank_outputs: pre_raw %s, outside_count %s, time_outside_count %s, timed %s do not fit"
                         % (tuple(raw.shape), tuple(outside_count.shape), tuple(time_outside_count.shape), timed))
    groups = energy_groups(groups, C)
    HW = time_outside_count.shape[2] * time_outside_count.shape[3]
    o = {"pre_raw": raw, "outside_count": outside_count, "outside_frac": outside_count.double() / float(HW),
         "time_outside_count": time_outside_count, "time_outside_frac": time_outside_count.double() / float(len(timed))}
    for j, kind in enumerate(("avg", "depth")):
        pre = torch.stack([raw[..., j][:, :, list(g)].sum(dim=2) for g in groups], dim=2)                 # [B, Tk, Gn, S + 1]
        o[kind + "_prerank"] = pre
        o[kind + "_rank_below"], o[kind + "_rank_equal"] = _fieldrank_of_target(pre)
        o[kind + "_rank_hist"] = fieldrank_hist(o[kind + "_rank_below"][:, timed], o[kind + "_rank_equal"][:, timed], R - 1)
        traj = pre[:, timed].sum(dim=1)
        o["traj_" + kind + "_prerank"] = traj
        o["traj_" + kind + "_rank_below"], o["traj_" + kind + "_rank_equal"] = _fieldrank_of_target(traj)
    o["depth_median"] = _fieldrank_median(o["depth_prerank"])
    o["traj_depth_median"] = _fieldrank_median(o["traj_depth_prerank"])
    return o


class EnsembleFieldRanks(EnsembleFeed):
    """On-device multivariate rank histograms of sampled roll-outs of B cases against the target (tmg_ens_score_store /
    tmg_ens_frank_step): whether the spread of whole FIELDS is right, which a per-pixel rank histogram cannot see and a score (one
    number) cannot separate from bias.  The average-rank and band-depth histograms of Thorarinsdottir, Scheuerer & Heinz (2016); the
    depth is the modified band depth of Lopez-Pintado & Romo (2009).  For case b, kept step t, channel c and pixel p, with the rows
    x_0..x_{S-1} (raw normalised members) and x_S (the normalised target), for row i over the S other rows j != i:
      lt = #{j : x_j < x_i}, eq = #{j : x_j == x_i}, gt = S - lt - eq
      A_i(p) = 2 lt + eq                              the average-rank term (twice the mid-rank minus a constant)
      D_i(p) = C(S,2) - C(lt,2) - C(gt,2)             the band-depth term: the pairs of other rows whose closed band holds x_i
      O(p)   = [lt_S == S or gt_S == S]               the target lies strictly outside the members' range
    It takes no out_mu, out_std or u: ranks do not change under x -> u (out_std x + out_mu) with u out_std > 0, so the kernel
    compares the raw values, and the channels of a group are combined as sums of integers, without any choice of norm or scale.
    The device sums A, D and O over the pixels in int64; everything else is host work on these small integer tensors, in int64 or
    fp64.  With the channel groups g (tuples of channels; default ((0, 1), (2,)): velocity and pressure) the pre-rank of row i is
    the sum over the group's channels; the field rank of the target is below = #{m < S : pre_m < pre_S}, equal = #{m < S : pre_m ==
    pre_S}.  A low average rank: the target field lies under the members; a low depth rank: the target is the most outlying row.
    A U-shaped average-rank histogram, or a depth-rank histogram piled at its low end, means under-dispersion.
    Non-finite rows are not supported: the outputs of a pixel that holds one are unspecified.  At most 1024 members.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is ranked.
    Outputs of finalize() (CPU tensors; Gn groups, Tn the steps folded with time=True, int64 unless stated):
      pre_raw [B, Tk, C, S + 1, 2]          sum_p A_i(p), sum_p D_i(p) per channel, the target last
      outside_count [B, Tk, C], outside_frac = outside_count / HW float64 (a calibrated continuous ensemble gives 2 / (S + 1))
      time_outside_count [B, C, H, W]       O(p) summed over the timed steps; time_outside_frac = count / Tn float64
      avg_prerank, depth_prerank [B, Tk, Gn, S + 1]
      avg_rank_below, avg_rank_equal, depth_rank_below, depth_rank_equal [B, Tk, Gn]
      avg_rank_hist, depth_rank_hist [B, Gn, S + 1] float64: fieldrank_hist over the timed steps; each sums to Tn
      traj_avg_prerank, traj_depth_prerank [B, Gn, S + 1]: the pre-ranks summed over the timed steps (a pre-rank is additive over
      pixels, so this is the pre-rank of the roll-out as one vector); traj_avg_rank_below, traj_avg_rank_equal,
      traj_depth_rank_below, traj_depth_rank_equal [B, Gn]
      depth_median [B, Tk, Gn], traj_depth_median [B, Gn]: the member with the largest depth pre-rank (the functional median),
      the smallest index on ties."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, groups=((0, 1), (2,))):
        noun = "ensemble field ranks"
        _ens_channels(noun, C)
        _ens_members(noun, members)
        if int(steps) < 1 or int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need B, H, W, steps >= 1, got %d, %d, %d, %d" % (noun, int(B), int(Hh), int(Ww), int(steps)))
        self.groups = energy_groups(groups, C)
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        HW = self.H * self.W
        self.plan = H.ens_frank_plan(self.S, self.B, C, HW)
        # rows 0 .. S - 1: the members; row S: the target, stored by the same kernel as a one-member chunk
        self.xs = torch.empty((self.S + 1, self.B, C, HW), device=dev, dtype=torch.float32)
        self.ws = torch.empty((self.plan["ws_words"],), device=dev, dtype=torch.int32)
        self.tout = torch.empty((self.B, C, HW), device=dev, dtype=torch.int32)
        self.pre_raw = torch.empty((self.B, self.Tk, C, self.S + 1, 2), device=dev, dtype=torch.int64)
        self.outside = torch.empty((self.B, self.Tk, C), device=dev, dtype=torch.int64)

    def add(self, y, m0, target, time=True):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk stores its target as the last row and ranks the step."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        H.ens_score_store(yn, self.xs[:self.S], k, m0)
        if last:
            H.ens_score_store(tn, self.xs[self.S:], 1, 0)                      # row S, through its one-row view
            H.ens_frank_step(self.xs, self.ws, self.pre_raw, self.outside, self.tout, self._step, t_before, 1 if time else 0)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs (CPU tensors); the histograms, the roll-out ranks and the time_ outputs cover the steps folded
        with time=True."""
        self.finalize_guard()
        return fieldrank_outputs(self.pre_raw.cpu(), self.outside.cpu(), self.tout.view(self.B, self.C, self.H, self.W).to(torch.int64).cpu(),
                                 self.groups, self._timed)


POD_MAX_MODES = 16


def pod_channels(channels, C):
    """The checks of the POD's channels argument for C channels: 1 to 4 distinct channels in 0..C-1 -> a tuple of ints."""
    try:
        chs = tuple(channels)
    except TypeError:
        raise ValueError("channels must be a tuple of channels, got %r" % (channels,))
    if not 1 <= len(chs) <= 4:
        raise ValueError("channels must hold 1 to 4 channels, got %r" % (channels,))
    for ch in chs:
        if isinstance(ch, bool) or not isinstance(ch, numbers.Integral) or not 0 <= ch < C:
            raise ValueError("channels hold distinct channels in 0..%d, got %r" % (C - 1, channels))
    if len(set(int(ch) for ch in chs)) != len(chs):
        raise ValueError("channels hold distinct channels in 0..%d, got %r" % (C - 1, channels))
    return tuple(int(ch) for ch in chs)


def pod_basis(series, a, channels, K, name="pod_basis", case0=0):
    """The POD basis of a target series by the method of snapshots, in fp64 plain torch on the series' device (once per mini-batch:
    not the hot path).  series [B, Tn, C, H, W]: the normalised target at the Tn kept steps; a [B, C]: the scales u out_std > 0;
    channels: the Cg distinct channels of the inner product <f, g> = (1 / HW) sum_{c in channels} sum_p f_c g_c; 1 <= K <= 16 modes,
    K <= Tn - 1 (the centred snapshots have rank at most Tn - 1), Tn >= 2.  With m the time mean and d_j = a_c (x_j - m):
      R[j, j'] = <d_j, d_j'> / Tn = sum_k lam_k v_k[j] v_k[j'], lam_0 >= lam_1 >= ..; every v_k with its entry of largest magnitude
      positive (the first such entry on a tie); psi_k = sum_j v_k[j] d_j / sqrt(Tn lam_k): <psi_k, psi_l> = delta_kl, RMS 1
    -> (m [B, Cg, H, W], psi [B, K, Cg, H, W], lam [B, K], lam_total [B] = trace R, target_coef [B, Tn, K] = <d_j, psi_k> =
    sqrt(Tn lam_k) v_k[j]), all fp64.  A mode with lam_k <= 1e-12 lam_0, or lam_0 == 0 (at most 2^-80 of the un-centred energy <a x, a x>,
    what the rounding of the mean leaves of a constant series), raises (a constant target has no modes);
    name and case0 (the cases before this batch) only word that message."""
    series = torch.as_tensor(series)
    if series.dim() != 5:
        raise ValueError("the series is [B, Tn, C, H, W], got shape %s" % (tuple(series.shape),))
    B, Tn, C, Hh, Ww = series.shape
    chs = pod_channels(channels, C)
    if isinstance(K, bool) or not isinstance(K, numbers.Integral) or not 1 <= K <= POD_MAX_MODES:
        raise ValueError("the POD keeps 1 <= modes <= %d, got %r" % (POD_MAX_MODES, K))
    if Tn < 2:
        raise ValueError("the POD needs at least 2 snapshots, got %d" % Tn)
    if K > Tn - 1:
        raise ValueError("%d centred snapshots have rank at most %d: modes = %d is too many" % (Tn, Tn - 1, K))
    a = torch.as_tensor(a, dtype=torch.float64).to(series.device).reshape(B, C)[:, list(chs)]
    if not bool((torch.isfinite(a) & (a > 0)).all()):
        raise ValueError("the scales a = u out_std must be finite and strictly positive")
    x = series[:, :, list(chs)].double()
    if not bool(torch.isfinite(x).all()):
        raise ValueError("the series must be finite")
    m = x.mean(1)
    d = (a.view(B, 1, -1, 1, 1) * (x - m.unsqueeze(1))).reshape(B, Tn, -1)   # [B, Tn, Cg HW]
    HW = Hh * Ww
    R = d @ d.transpose(1, 2) / (HW * Tn)
    lam_total = torch.diagonal(R, dim1=1, dim2=2).sum(1)
    w, v = torch.linalg.eigh(R)                                              # ascending
    lam = w.flip(1)[:, :K]
    v = v.flip(2)[:, :, :K]                                                  # [B, Tn, K]: column k is v_k
    # lam_0 == 0 as fp64 sees it: below the rounding of the mean, (2^-40)^2 of the un-centred energy <a x, a x>
    floor = 2.0 ** -80 * ((a.view(B, 1, -1, 1, 1) * x) ** 2).reshape(B, -1).sum(1, keepdim=True) / (HW * Tn)
    bad = (lam <= 1e-12 * lam[:, :1]) | (lam[:, :1] <= floor)
    if bool(bad.any()):
        b, k = [int(i) for i in bad.nonzero()[0]]
        raise ValueError("%s: mode %d of the target of case %d carries no energy (lam = %r, lam_0 = %r): a constant target has no "
                         "modes; keep fewer" % (name, k, case0 + b, float(lam[b, k]), float(lam[b, 0])))
    top = v.abs().argmax(1, keepdim=True)                                    # the first entry of largest magnitude
    sgn = torch.where(torch.gather(v, 1, top) < 0, -1.0, 1.0).to(v.dtype)
    v = v * sgn
    amp = torch.sqrt(Tn * lam)                                               # [B, K]
    psi = (v.transpose(1, 2) @ d) / amp.unsqueeze(2)                         # [B, K, Cg HW]
    return m, psi.reshape(B, K, len(chs), Hh, Ww), lam, lam_total, v * amp.unsqueeze(1)


def _pod_time(coef, en):
    """coef [.., T, K], en [.., T] fp64 over the timed steps -> the time aggregates of EnsembleModes (fp64)."""
    mean = coef.mean(-2)
    dev = coef - mean.unsqueeze(-2)
    energy = (coef * coef).mean(-2)
    cov = dev.transpose(-1, -2) @ dev / coef.shape[-2]
    fl = en.mean(-1)
    cap = energy.sum(-1)
    return {"time_mode_energy": energy, "time_mode_mean": mean, "time_coef_cov": cov, "time_captured_frac": cap / fl,
            "time_resid_energy": fl - cap}


class EnsembleModes(EnsembleFeed):
    """On-device projection of sampled roll-outs of B cases, and of the target, on given POD modes of the target (tmg_ens_pod_project):
    do the members hold the reference's coherent structures, with the right energy and the right dynamics?  Given per case the mean
    planes `mean` [B, Cg, H, W] (normalised) and the modes `basis` [B, K, Cg, H, W] (K <= 16; pod_basis builds both from the target
    series; any finite tables are accepted and rounded to fp32 once), a_c = u[b, c] out_std[c] > 0 and the inner product
    <f, g> = (1 / HW) sum_{c in channels} sum_p f_c g_c, for every row x (a member, or the step's target):
      d = fl(a_c fl(x - mean))                              the fluctuation in physical units, two fp32 roundings
      coef[k] = <d, basis_k>,  fluct_energy = <d, d>        fp32 sums on the device (the modes on the matrix pipe), / HW in fp64
    A member's coefficients need no other member: the kernel reads the chunk's rows in place and no member buffer is kept; the pixel
    slicing of the sums depends on the field alone, so every output is bitwise the same for every chunking and ensemble size.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is projected.
    Outputs (device tensors): coef [B, S, Tk, K], fluct_energy [B, S, Tk], target_coef [B, Tk, K], target_fluct_energy [B, Tk]
    float32; finalize() adds, over the steps folded with time=True (formed in fp64 from the outputs above, rounded once):
      time_mode_energy [B, S, K]      mean_t coef^2: each member's energy in the target's mode k; compare with the target's
      time_mode_mean [B, S, K]        mean_t coef: the member's mean-flow error as mode k sees it
      time_coef_cov [B, S, K, K]      mean_t (coef - mean)(coef - mean)^T: off-diagonals show structures rotated inside the subspace
      time_captured_frac [B, S]       sum_k time_mode_energy / mean_t fluct_energy
      time_resid_energy [B, S]        mean_t fluct_energy - sum_k time_mode_energy: what the K modes do not hold
      target_time_* [B, ..]           the same of the target's row; for pod_basis' tables over the same steps
                                      target_time_mode_energy is lam_k and target_time_captured_frac is sum_k lam_k / lam_total
      mode_energy_ratio_mean, mode_energy_ratio_std [B, K]   mean / population std over the members of time_mode_energy / lam_k,
                                      lam the attribute `lam` [B, K] (pod_basis' energies, set by whoever built the tables); None,
                                      the default: target_time_mode_energy, which is lam_k as this kernel measures it
    and the entries of the attribute `extra` (a dict, empty by default) as they are."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_std, u=None, channels=(0, 1), mean=None, basis=None):
        noun, why = "ensemble modes", "the fluctuations scale with u * out_std"
        _ens_channels(noun, C)
        _ens_members(noun, members)
        sd, _ = _ens_tables(C, why, out_std)
        u = _ens_u(u, B, C, why)
        self.channels = pod_channels(channels, C)
        Cg = len(self.channels)
        if int(steps) < 1 or int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need steps, B, H, W >= 1, got %d, %d, %d, %d" % (noun, steps, B, Hh, Ww))
        if mean is None or basis is None:
            raise ValueError("%s need the tables mean [B, Cg, H, W] and basis [B, K, Cg, H, W] (pod_basis builds them)" % noun)
        mean, basis = torch.as_tensor(mean).detach(), torch.as_tensor(basis).detach()
        if tuple(mean.shape) != (int(B), Cg, int(Hh), int(Ww)) or not bool(torch.isfinite(mean).all()):
            raise ValueError("mean is a finite array [%d, %d, %d, %d], got shape %s" % (B, Cg, Hh, Ww, tuple(mean.shape)))
        if (basis.dim() != 5 or not 1 <= basis.shape[1] <= POD_MAX_MODES or tuple(basis.shape[:1] + basis.shape[2:]) != tuple(mean.shape)
                or not bool(torch.isfinite(basis).all())):
            raise ValueError("basis is a finite array [%d, 1..%d, %d, %d, %d], got shape %s" % (B, POD_MAX_MODES, Cg, Hh, Ww, tuple(basis.shape)))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        HW, K = self.H * self.W, int(basis.shape[1])
        self.K = K
        f32 = dict(device=dev, dtype=torch.float32)
        # a_c = u out_std in fp64 from the fp32 factors, rounded once; the tables rounded once
        self.a = _ens_scale(sd, u, self.B, torch.float64)[:, list(self.channels)].to(torch.float32).to(dev).contiguous()
        self.m = mean.to(torch.float32).reshape(self.B, Cg, HW).to(dev).contiguous()
        self.psi = basis.to(torch.float32).reshape(self.B, K, Cg, HW).to(dev).contiguous()
        self.plan = H.ens_pod_plan(self.S, self.B, Cg, HW, K)
        self.ws = torch.empty((self.plan["ws"],), **f32) if self.plan["ws"] else None
        self.coef_raw = torch.empty((self.B, self.S, self.Tk, K), **f32)
        self.en_raw = torch.empty((self.B, self.S, self.Tk), **f32)
        self.tcoef_raw = torch.empty((self.B, self.Tk, K), **f32)
        self.ten_raw = torch.empty((self.B, self.Tk), **f32)
        self.extra = {}
        self.lam = None

    def add(self, y, m0, target, time=True):
        """Project the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk projects the target as one more row."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        t, S, Tk, K = self._step, self.S, self.Tk, self.K
        H.ens_pod_project(yn, self.channels, self.a, self.m, self.psi, self.ws, self.coef_raw[:, m0:, t], self.en_raw[:, m0:, t],
                          (S * Tk * K, Tk * K, S * Tk, Tk), k)
        if last:
            H.ens_pod_project(tn, self.channels, self.a, self.m, self.psi, self.ws, self.tcoef_raw[:, t], self.ten_raw[:, t],
                              (Tk * K, 0, Tk, 0), 1)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time aggregates cover the steps folded with time=True."""
        self.finalize_guard()
        dev = self.coef_raw.device
        hw = float(self.H * self.W)
        f32 = lambda v: v.to(torch.float32)                                   # noqa: E731
        # the host divides the raw sums by HW in fp64 and rounds once
        o = {"coef": f32(self.coef_raw.double() / hw), "fluct_energy": f32(self.en_raw.double() / hw),
             "target_coef": f32(self.tcoef_raw.double() / hw), "target_fluct_energy": f32(self.ten_raw.double() / hw)}
        tm = _pod_time(o["coef"][:, :, self._timed].double().cpu(), o["fluct_energy"][:, :, self._timed].double().cpu())
        tt = _pod_time(o["target_coef"][:, self._timed].double().cpu(), o["target_fluct_energy"][:, self._timed].double().cpu())
        lam = tt["time_mode_energy"] if self.lam is None else torch.as_tensor(self.lam, dtype=torch.float64).cpu().reshape(self.B, self.K)
        ratio = tm["time_mode_energy"] / lam.unsqueeze(1)
        for key, v in tm.items():
            o[key] = f32(v).to(dev)
        for key, v in tt.items():
            o["target_" + key] = f32(v).to(dev)
        o["mode_energy_ratio_mean"], o["mode_energy_ratio_std"] = f32(ratio.mean(1)).to(dev), f32(ratio.std(1, unbiased=False)).to(dev)
        o.update(self.extra)
        return o


PHASE_BINS = (4, 8, 16, 32)


def phase_args(pair, bins, min_amp, K=None):
    """The checks of the phase arguments: pair two distinct mode indices >= 0 (below K when given), bins one of 4, 8, 16, 32,
    min_amp finite and >= 0 -> (pair, bins, min_amp) as ints and a float."""
    try:
        pr = tuple(pair)
    except TypeError:
        raise ValueError("pair must hold two modes, got %r" % (pair,))
    if len(pr) != 2 or any(isinstance(p, bool) or not isinstance(p, numbers.Integral) or p < 0 for p in pr):
        raise ValueError("pair must hold two mode indices >= 0, got %r" % (pair,))
    if pr[0] == pr[1]:
        raise ValueError("pair must hold two different modes, got %r" % (pair,))
    if K is not None and max(pr) + 1 > K:
        raise ValueError("pair %r needs modes >= %d, got %d" % (tuple(pr), max(pr) + 1, K))
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral) or bins not in PHASE_BINS:
        raise ValueError("bins must be one of %s, got %r" % (PHASE_BINS, bins))
    if isinstance(min_amp, bool) or not isinstance(min_amp, numbers.Real) or not 0 <= float(min_amp) < float("inf"):
        raise ValueError("min_amp must be finite and >= 0, got %r" % (min_amp,))
    return (int(pr[0]), int(pr[1])), int(bins), float(min_amp)


def phase_table(bins, min_amp):
    """The 8 host floats of tmg_ens_phase_label: the gate thr = 2 min_amp^2 and the tangents tan(2 pi q / bins), q = 1 .. bins / 4 - 1,
    each formed in fp64 and rounded to fp32 once (unused entries 0) -> a list of Python floats that are exact fp32 values."""
    r32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))   # noqa: E731
    tab = [r32(2.0 * float(min_amp) * float(min_amp))]
    tab += [r32(math.tan(2.0 * math.pi * q / bins)) for q in range(1, bins // 4)]
    return tab + [0.0] * (8 - len(tab))


def _phase_fields(cnt, raw, C):
    """cnt [B, NB] (fp64 counts), raw [B, NB, Q, P] (fp64 raw sums, Q = 2 C + 1) -> the phase fields and the triple decomposition
    about the target's mean (fp64): dev [B, NB, C, P] = sum d / n, var [B, NB, C, P], uv [B, NB, P] (NaN where n = 0), coh_var,
    incoh_var [B, C, P], coh_uv, incoh_uv [B, P], coh_tke_frac [B], coh [B, NB, C, P] = dev - sum_k w_k dev_k (NaN where n = 0)."""
    nan = float("nan")
    n = cnt.view(cnt.shape + (1, 1))
    has = n > 0
    safe = torch.where(has, n, torch.ones_like(n))
    ex = raw / safe
    dev, sq, xy = ex[:, :, :C], ex[:, :, C:2 * C], ex[:, :, 2 * C]
    var = sq - dev * dev
    uv = xy - dev[:, :, 0] * dev[:, :, 1]
    tot = cnt.sum(1)
    w = (cnt / torch.where(tot > 0, tot, torch.ones_like(tot)).unsqueeze(1)).view(n.shape)   # 0 for an empty sector
    mbar = (w * dev).sum(1, keepdim=True)
    coh = dev - mbar
    o = {"coh_var": (w * coh * coh).sum(1), "incoh_var": (w * var).sum(1), "coh_uv": (w[:, :, 0] * coh[:, :, 0] * coh[:, :, 1]).sum(1),
         "incoh_uv": (w[:, :, 0] * uv).sum(1)}
    num = o["coh_var"][:, :2].sum((1, 2))
    o["coh_tke_frac"] = num / (num + o["incoh_var"][:, :2].sum((1, 2)))
    none = (tot <= 0)
    for key in ("coh_var", "incoh_var", "coh_uv", "incoh_uv", "coh_tke_frac"):
        o[key] = torch.where(none.view((-1,) + (1,) * (o[key].dim() - 1)), torch.full_like(o[key], nan), o[key])
    fill = lambda v, h: torch.where(h, v, torch.full_like(v, nan))           # noqa: E731
    o["dev"], o["var"], o["uv"], o["coh"] = fill(dev, has), fill(var, has), fill(uv, has[:, :, 0]), fill(coh, has)
    return o


class EnsemblePhase(EnsembleFeed):
    """On-device phase averages of sampled roll-outs of B cases, and of the target, on the shedding phase (tmg_ens_phase_label /
    tmg_ens_phase_accum): the triple decomposition u = U + u~ + u' of Reynolds & Hussain.  At a given phase of the cycle, do the
    members put the vortices where the reference puts them, and how much of the Reynolds stress is organised motion?

    `modes` is a ready EnsembleModes of the same feed that this accumulator drives: add() calls modes.add() first, so the projection
    runs once, through tmg_ens_pod_project.  The phase of a row is the angle of (x, y) = (coef_i / sqrt(lam_i), coef_j / sqrt(lam_j)),
    (i, j) = pair, lam [B, 2] the pair's energies: on the device x = fl(g_i raw_i) with g = 1 / (HW sqrt(lam)) formed in fp64 and
    rounded once.  A row with fl(fl(x x) + fl(y y)) < fl(2 min_amp^2) is skipped (label -1; a clean limit cycle has x^2 + y^2 = 2);
    else its label is the sector 0 .. bins - 1 of the angle counted from the positive x axis towards positive y.  A point exactly on
    an edge belongs to the higher sector; (0, 0) with min_amp = 0 is sector 0.  No transcendental runs on the device and every
    operation is rounded on its own, so the labels equal a float32 numpy mirror bit for bit.

    `mean` [B, C, H, W] is the target's time mean in normalised units for all C channels; with a_c = u[b, c] out_std[c] every labelled
    row adds d_c = fl(a_c fl(x_c - mean_c)), d_c^2 and d_0 d_1 to the fp32 sums of its sector (centred on the target's mean, so that
    E[d^2] - E[d]^2 does not cancel).  The additions into one element run steps in order, members in order for every chunking: the
    outputs are bitwise reproducible.  The attribute `mean_phys` [B, C, H, W] (fp64; None, the default: a mean from the fp32 tables, an
    output mean of zero) is the physical mean that phase_mean is counted from; whoever built the tables sets it.

    Feeding protocol of EnsembleFeed, with the step's target on every chunk.  Every kept step is labelled; only steps with time=True
    are accumulated.  finalize() returns modes.finalize()'s dict plus (n_k the rows of sector k, all formed in fp64 on the host from
    the raw sums and the labels, rounded once; NaN where a sector is empty, empty sectors left out of every aggregate):
      phase_bin [B, S, Tk], target_phase_bin [B, Tk] int32     the labels, -1 for a skipped row
      phase_count [B, NB], member_phase_count [B, S, NB], target_phase_count [B, NB] int64, over the timed steps; phase_skipped,
      target_phase_skipped [B]
      phase_mean [B, NB, C, H, W]     mean_phys + sum d / n_k: the phase average <u>_k
      phase_var [B, NB, C, H, W]      sum d^2 / n_k - (sum d / n_k)^2: the incoherent <u'_c u'_c>_k
      phase_uv [B, NB, H, W]          the incoherent <u'_0 u'_1>_k
      coh_var [B, C, H, W], coh_uv [B, H, W]        sum_k w_k (M_k - M)^2 and the same cross product, w_k = n_k / sum n, M = sum w_k M_k
      incoh_var [B, C, H, W], incoh_uv [B, H, W]    sum_k w_k phase_var_k, sum_k w_k phase_uv_k
      coh_tke_frac [B]                channels 0 and 1: sum_p coh_var / sum_p (coh_var + incoh_var)
      target_*                        each of the fields above for the target's rows
      phase_mean_rmse [B, NB, C]      RMS over the pixels of phase_mean - target_phase_mean
      coh_corr [B, NB]                sum (M_k - M)(T_k - T) / sqrt(sum (M_k - M)^2 sum (T_k - T)^2) over channels 0, 1 and the pixels
      phase_speed [B, S], target_phase_speed [B]    the mean increment of atan2(y, x), from the returned coef and lam in fp64, between
                                      consecutive timed steps, wrapped to (-pi, pi], radians per kept step (NaN with one timed step)
      phase_edges [NB + 1]            the sector angles 2 pi k / NB, float64 on the host."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_std, u=None, modes=None, pair=(0, 1), bins=8, min_amp=0.25, mean=None,
                 lam=None):
        noun, why = "ensemble phase averages", "the fluctuations scale with u * out_std"
        _ens_channels(noun, C)
        _ens_members(noun, members)
        sd, _ = _ens_tables(C, why, out_std)
        u = _ens_u(u, B, C, why)
        if int(steps) < 1 or int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s need steps, B, H, W >= 1, got %d, %d, %d, %d" % (noun, steps, B, Hh, Ww))
        if not isinstance(modes, EnsembleModes):
            raise ValueError("%s need modes, a ready EnsembleModes of the same feed" % noun)
        if (modes.S, modes.B, modes.C, modes.H, modes.W, modes.Tk) != (int(members), int(B), int(C), int(Hh), int(Ww), int(steps)):
            raise ValueError("modes is an EnsembleModes of another feed: %s" % ((modes.S, modes.B, modes.C, modes.H, modes.W, modes.Tk),))
        self.pair, self.NB, self.min_amp = phase_args(pair, bins, min_amp, modes.K)
        if mean is None or lam is None:
            raise ValueError("%s need the tables mean [B, C, H, W] and lam [B, 2]" % noun)
        mean, lam = torch.as_tensor(mean).detach(), torch.as_tensor(lam).detach().double().cpu()
        if tuple(mean.shape) != (int(B), int(C), int(Hh), int(Ww)) or not bool(torch.isfinite(mean).all()):
            raise ValueError("mean is a finite array [%d, %d, %d, %d], got shape %s" % (B, C, Hh, Ww, tuple(mean.shape)))
        if tuple(lam.shape) != (int(B), 2) or not bool((torch.isfinite(lam) & (lam > 0)).all()):
            raise ValueError("lam is a finite, strictly positive array [%d, 2], got shape %s" % (B, tuple(lam.shape)))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        HW, NB = self.H * self.W, self.NB
        self.modes, self.lam = modes, lam
        f32 = dict(device=dev, dtype=torch.float32)
        # a_c = u out_std in fp64 from the fp32 factors, rounded once; the tables rounded once
        self.a = _ens_scale(sd, u, self.B, torch.float64).to(torch.float32).to(dev).contiguous()
        self.m = mean.to(torch.float32).reshape(self.B, self.C, HW).to(dev).contiguous()
        self.g = (1.0 / (HW * torch.sqrt(lam))).to(torch.float32).to(dev).contiguous()
        self.tab = phase_table(NB, self.min_amp)
        self.plan = H.ens_phase_plan(self.S, self.B, self.C, HW, NB)
        Q = 2 * self.C + 1
        self.acc = torch.zeros((self.B, NB, Q, HW), **f32)
        self.tacc = torch.zeros((self.B, NB, Q, HW), **f32)
        self.label = torch.full((self.B, self.S, self.Tk), -1, device=dev, dtype=torch.int32)
        self.tlabel = torch.full((self.B, self.Tk), -1, device=dev, dtype=torch.int32)
        self.mean_phys = None

    def add(self, y, m0, target, time=True):
        """Project (modes.add) and label the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose
        channels-last view is an NHWC channel-slice; rows member-major) and, with time=True, add them to their sectors; target: the
        step's normalised target [B, C, H, W] under the same stride rule.  The step's last chunk labels and adds the target's row."""
        self.modes.add(y, m0, target, time=time)
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        t, S, Tk, K, B, NB = self._step, self.S, self.Tk, self.modes.K, self.B, self.NB
        lab, ls = self.label[:, m0:, t], (S * Tk, Tk)
        H.ens_phase_label(self.modes.coef_raw[:, m0:, t], (S * Tk * K, Tk * K), self.pair, self.g, self.tab, lab, ls, k, B, NB)
        if time:
            H.ens_phase_accum(yn, lab, ls, self.a, self.m, self.acc, k)
        if last:
            tlab, tls = self.tlabel[:, t], (Tk, 0)
            H.ens_phase_label(self.modes.tcoef_raw[:, t], (Tk * K, 0), self.pair, self.g, self.tab, tlab, tls, 1, B, NB)
            if time:
                H.ens_phase_accum(tn, tlab, tls, self.a, self.m, self.tacc, 1)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the counts, fields and speeds cover the steps folded with time=True."""
        self.finalize_guard()
        o = self.modes.finalize()
        dev = self.acc.device
        B, S, C, NB, Hh, Ww = self.B, self.S, self.C, self.NB, self.H, self.W
        f32 = lambda v: v.to(torch.float32).to(dev)                           # noqa: E731
        lab, tlab = self.label.cpu().long(), self.tlabel.cpu().long()
        o["phase_bin"], o["target_phase_bin"] = self.label.clone(), self.tlabel.clone()
        lt, tlt = lab[:, :, self._timed], tlab[:, self._timed]
        sectors = torch.arange(NB).view(1, 1, 1, NB)
        mcount = (lt.unsqueeze(-1) == sectors).sum(2)                            # [B, S, NB]
        tcount = (tlt.unsqueeze(-1) == sectors[0]).sum(1)                        # [B, NB]
        count = mcount.sum(1)
        o["member_phase_count"], o["phase_count"], o["target_phase_count"] = mcount.to(dev), count.to(dev), tcount.to(dev)
        o["phase_skipped"], o["target_phase_skipped"] = (lt < 0).sum((1, 2)).to(dev), (tlt < 0).sum(1).to(dev)
        mp = (self.a.double().cpu().view(B, C, 1, 1) * self.m.double().cpu().view(B, C, Hh, Ww) if self.mean_phys is None
              else torch.as_tensor(self.mean_phys).detach().double().cpu().reshape(B, C, Hh, Ww))
        fe = _phase_fields(count.double(), self.acc.double().cpu(), C)
        ft = _phase_fields(tcount.double(), self.tacc.double().cpu(), C)
        for pre, f in (("", fe), ("target_", ft)):
            o[pre + "phase_mean"] = f32((mp.view(B, 1, C, -1) + f["dev"]).view(B, NB, C, Hh, Ww))
            o[pre + "phase_var"] = f32(f["var"].view(B, NB, C, Hh, Ww))
            o[pre + "phase_uv"] = f32(f["uv"].view(B, NB, Hh, Ww))
            for key in ("coh_var", "incoh_var"):
                o[pre + key] = f32(f[key].view(B, C, Hh, Ww))
            for key in ("coh_uv", "incoh_uv"):
                o[pre + key] = f32(f[key].view(B, Hh, Ww))
            o[pre + "coh_tke_frac"] = f32(f["coh_tke_frac"])
        diff = fe["dev"] - ft["dev"]                                             # mean_phys cancels
        o["phase_mean_rmse"] = f32(torch.sqrt((diff * diff).mean(-1)))
        ce, ct = fe["coh"][:, :, :2].reshape(B, NB, -1), ft["coh"][:, :, :2].reshape(B, NB, -1)
        o["coh_corr"] = f32((ce * ct).sum(-1) / torch.sqrt((ce * ce).sum(-1) * (ct * ct).sum(-1)))
        sl = torch.sqrt(self.lam)                                                # [B, 2]
        i, j = self.pair

        def speed(coef, s):
            """coef [.., T, K] fp64 over the timed steps, s [.., 1, 2] -> the mean wrapped increment of the angle."""
            if coef.shape[-2] < 2:
                return torch.full(coef.shape[:-2], float("nan"), dtype=torch.float64)
            th = torch.atan2(coef[..., j] / s[..., 1], coef[..., i] / s[..., 0])
            dth = th[..., 1:] - th[..., :-1]
            dth = dth - 2 * math.pi * torch.ceil((dth - math.pi) / (2 * math.pi))
            return dth.mean(-1)

        o["phase_speed"] = f32(speed(o["coef"][:, :, self._timed].double().cpu(), sl.view(B, 1, 1, 2)))
        o["target_phase_speed"] = f32(speed(o["target_coef"][:, self._timed].double().cpu(), sl.view(B, 1, 2)))
        o["phase_edges"] = 2 * math.pi * torch.arange(NB + 1, dtype=torch.float64) / NB   # (a host table)
        return o


BUDGET_TERMS = ("conv", "prod", "turb", "pres", "visc", "diss", "resid")
BUDGET_PLANES = 14


def budget_args(C, Hh, Ww, grid, nu, rho):
    """The checks of the budget arguments: C == 3 (the pressure is needed), H, W >= 3 (the stencils need neighbours), grid two
    positive finite sizes, nu >= 0 and rho > 0, both finite -> (dx, dy, nu, rho) as floats."""
    real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))   # noqa: E731
    if int(C) != 3:
        raise ValueError("the TKE budget needs C == 3 channels (ux, uy, p: the pressure diffusion reads p), got %d" % int(C))
    if int(Hh) < 3 or int(Ww) < 3:
        raise ValueError("the TKE budget needs H, W >= 3 (the stencils have no neighbours otherwise), got %d x %d" % (int(Hh), int(Ww)))
    try:
        g = tuple(grid)
    except TypeError:
        raise ValueError("grid must hold (dx, dy), got %r" % (grid,))
    if len(g) != 2 or not all(real(v) and float(v) > 0 for v in g):
        raise ValueError("grid must hold two positive finite sizes (dx, dy), got %r" % (grid,))
    if not real(nu) or float(nu) < 0:
        raise ValueError("nu must be finite and >= 0, got %r" % (nu,))
    if not real(rho) or float(rho) <= 0:
        raise ValueError("rho must be finite and > 0, got %r" % (rho,))
    return float(g[0]), float(g[1]), float(nu), float(rho)


class EnsembleBudget(EnsembleFeed):
    """On-device budget of the turbulent kinetic energy k = 1/2 <u'_i u'_i> of sampled roll-outs of B cases, and of the target
    (tmg_ens_budget_accum / tmg_ens_budget_terms): is the kinetic energy of the fluctuations produced, transported and dissipated
    where the reference simulation produces, transports and dissipates it?

    Rows are the S members plus the target as row S.  A row's fluctuation about the TARGET's time mean is d_c = fl(a_c fl(y_c - m_c)),
    c = (ux, uy, p), a = u * out_std (formed in fp64, rounded once), m = `mean` [B, 3, H, W] in normalised units (None: 0).  Every
    timed step adds 14 fp32 quantities per row and pixel to the state `raw` [S + 1, B, 14, HW]: d_u, d_v, d_p; d_u^2, d_u d_v, d_v^2;
    d_u^3, d_u^2 d_v, d_u d_v^2, d_v^3; d_p d_u, d_p d_v; (Sx d_u)^2 + (Sx d_v)^2; (Sy d_u)^2 + (Sy d_v)^2, with the un-scaled 3x3
    first-derivative stencils of pc/ (zero outside the field): Sx f = (f[h-1,w+1] - f[h-1,w-1]) + 2 (f[h,w+1] - f[h,w-1]) +
    (f[h+1,w+1] - f[h+1,w-1]), Sy with h and w exchanged, d/dx = Sx / (8 dx), d/dy = Sy / (8 dy).  An element of raw is touched by one
    thread once per step: the state is bitwise reproducible, independent of the chunking, and needs no memset (the first timed step
    stores).  It takes 14 * 4 bytes per element of [S + 1, B, HW].

    finalize() forms, in fp64 on the device, each row's central moments about its OWN mean from raw by the shift formulas (T timed
    steps, D_c = raw_c / T: uu = raw_3 / T - D_u^2, .., gx = raw_12 / T - (Sx D_u)^2 - (Sx D_v)^2), k = (uu + vv) / 2, the absolute
    mean velocity U = M_u + D_u, V = M_v + D_v (M = a m + u out_mu, the target's physical mean, in fp64 from the fp32 tables) and
    the seven terms of budget_terms, signed as they enter dk/dt:
      conv  = -(U dk/dx + V dk/dy)                       prod = -(uu dU/dx + uv (dU/dy + dV/dx) + vv dV/dy)
      turb  = -1/2 (d(uuu + uvv)/dx + d(uuv + vvv)/dy)   pres = -(1 / rho) (d pu/dx + d pv/dy)
      visc  = nu ((k[h,w+1] - 2 k + k[h,w-1]) / dx^2 + (k[h+1,w] - 2 k + k[h-1,w]) / dy^2)
      diss  = -nu (gx / (64 dx^2) + gy / (64 dy^2))     a sink
      resid = the sum of the six: what a resolved two-dimensional budget over a finite window does not close (-dk/dt of the window,
              sub-grid dissipation, out-of-plane terms); it is a term of the budget, not an error.
    Every term is NaN on the one-pixel frame of the field, where the stencils have no neighbours.

    Feeding protocol of EnsembleFeed, with the step's target on every chunk; a step fed with time=False launches nothing.
    finalize() -> dict:
      budget_mean, budget_std [B, 7, H, W]     Welford mean / population std (ddof 0) over the members, in member order
      target_budget [B, 7, H, W]               the target's terms
      stress_mean, stress_std, target_stress [B, 3, H, W]    the same of (uu, uv, vv), on the whole field
      member_budget [B, S, 7, H, W]            every member's terms (per_member=True only)
      budget_terms                             the names of the seven terms."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), nu=0.0, rho=1.0, mean=None,
                 per_member=False):
        noun, why = "ensemble TKE budgets", "the fluctuations scale with u * out_std"
        _ens_members(noun, members)
        self.fl = budget_args(C, Hh, Ww, grid, nu, rho)
        sd, mu = _ens_tables(3, why, out_std, out_mu)
        u = _ens_u(u, B, 3, why)
        if int(steps) < 1 or int(B) < 1:
            raise ValueError("%s need steps, B >= 1, got %d, %d" % (noun, steps, B))
        if mean is not None:
            mean = torch.as_tensor(mean).detach()
            if tuple(mean.shape) != (int(B), 3, int(Hh), int(Ww)) or not bool(torch.isfinite(mean).all()):
                raise ValueError("mean is a finite array [%d, 3, %d, %d], got shape %s" % (B, Hh, Ww, tuple(mean.shape)))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, 3, Hh, Ww, steps)
        HW = self.H * self.W
        self.per_member = bool(per_member)
        self.a = _ens_scale(sd, u, self.B, torch.float64).to(torch.float32).to(dev).contiguous()
        self.m = None if mean is None else mean.to(torch.float32).reshape(self.B, 3, HW).to(dev).contiguous()
        # M = a m + u out_mu in fp64 from the fp32 tables (channels 0, 1)
        a64 = self.a.double().cpu()
        M = (_ens_scale(torch.ones(3), u, self.B, torch.float64) * mu.double().view(1, 3)).view(self.B, 3, 1).expand(self.B, 3, HW)
        if self.m is not None:
            M = M + a64.view(self.B, 3, 1) * self.m.double().cpu()
        self.M = M[:, :2].contiguous().to(dev)
        self.plan = H.ens_budget_plan(self.S, self.B, self.H, self.W)
        self.raw = torch.empty((self.S + 1, self.B, BUDGET_PLANES, HW), device=dev, dtype=torch.float32)

    def add(self, y, m0, target, time=True):
        """Add the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, 3, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, 3, H, W] under the same stride rule, added as
        row S with the step's last chunk.  A step fed with time=False launches nothing."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        if time:
            H.ens_budget_accum(yn, self.a, self.m, self.raw, k, m0, t_before)
            if last:
                H.ens_budget_accum(tn, self.a, self.m, self.raw, 1, self.S, t_before)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs over the steps folded with time=True."""
        T = self.finalize_guard()
        B, S, Hh, Ww = self.B, self.S, self.H, self.W
        HW, dev = Hh * Ww, self.raw.device
        outs = [torch.empty((B, n, HW), device=dev, dtype=torch.float32) for n in (7, 7, 7, 3, 3, 3)]
        mb = torch.empty((B, S, 7, HW), device=dev, dtype=torch.float32) if self.per_member else None
        H.ens_budget_terms(self.raw, self.M, self.fl, outs, mb, Hh, Ww, T)
        o = {}
        for key, t in zip(("budget_mean", "budget_std", "target_budget", "stress_mean", "stress_std", "target_stress"), outs):
            o[key] = t.view(B, t.shape[1], Hh, Ww)
        if mb is not None:
            o["member_budget"] = mb.view(B, S, 7, Hh, Ww)
        o["budget_terms"] = BUDGET_TERMS
        return o


TRANSPORT_MAX_SUBSTEPS = 8
TRANSPORT_MAX_BOXES = 4
TRANSPORT_FIELDS = ("ftle_mean", "ftle_std", "target_ftle", "ftle_count", "disp_mean", "disp_std", "target_disp", "alive_frac",
                    "target_alive", "res_time_mean", "res_time_std", "target_res_time", "end_err_mean", "end_spread")
TRANSPORT_MEMBER_FIELDS = ("member_ftle", "member_end", "member_exit")


def transport_args(seed_stride, seed_origin, substeps, boxes, C, Hh, Ww, grid, step_dt):
    """The checks and the defaults of the transport arguments, without a device: 2 <= C <= 4 (channels 0 and 1 are the velocity),
    H, W >= 2, grid two positive finite sizes (dx, dy), step_dt a positive finite time between two kept steps; seed_stride two
    integers (sy, sx) >= 1 (along H, along W); seed_origin two integers (oy, ox) >= 0 inside the field (None: (sy // 2, sx // 2));
    substeps an integer in 1 .. 8; boxes at most 4 tuples (h0, h1, w0, w1) of integers, inclusive, 0 <= h0 <= h1 <= H - 1 and
    0 <= w0 <= w1 <= W - 1.  H = W = None (the field is not known yet) skips the field's limits and returns Gh = Gw = None.
    -> (lattice, substeps, boxes, dx, dy, step_dt) with lattice = (Gh, Gw, oy, ox, sy, sx): the seeds are the pixels
    (oy + i sy, ox + j sx), i < Gh, j < Gw, every one of that lattice that lies inside the field."""
    real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))   # noqa: E731
    whole = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)                         # noqa: E731
    if not 2 <= int(C) <= 4:
        raise ValueError("the transport needs 2 <= C <= 4 channels (ux, uy first), got %d" % int(C))
    known = Hh is not None and Ww is not None
    if known and (int(Hh) < 2 or int(Ww) < 2):
        raise ValueError("the transport needs H, W >= 2 (one bilinear cell), got %d x %d" % (int(Hh), int(Ww)))
    try:
        g = tuple(grid)
    except TypeError:
        raise ValueError("grid must hold (dx, dy), got %r" % (grid,))
    if len(g) != 2 or not all(real(v) and float(v) > 0 for v in g):
        raise ValueError("grid must hold two positive finite sizes (dx, dy), got %r" % (grid,))
    if not real(step_dt) or float(step_dt) <= 0:
        raise ValueError("step_dt must be a positive finite time between two kept steps, got %r" % (step_dt,))
    try:
        st = tuple(seed_stride)
    except TypeError:
        raise ValueError("seed_stride must hold (sy, sx), got %r" % (seed_stride,))
    if len(st) != 2 or not all(whole(v) and int(v) >= 1 for v in st):
        raise ValueError("seed_stride must hold two integers (sy, sx) >= 1, got %r" % (seed_stride,))
    sy, sx = int(st[0]), int(st[1])
    if seed_origin is None:
        og = (sy // 2, sx // 2)
    else:
        try:
            og = tuple(seed_origin)
        except TypeError:
            raise ValueError("seed_origin must hold (oy, ox), got %r" % (seed_origin,))
        if len(og) != 2 or not all(whole(v) and int(v) >= 0 for v in og):
            raise ValueError("seed_origin must hold two integers (oy, ox) >= 0, got %r" % (seed_origin,))
    oy, ox = int(og[0]), int(og[1])
    if not whole(substeps) or not 1 <= int(substeps) <= TRANSPORT_MAX_SUBSTEPS:
        raise ValueError("substeps must be an integer in 1 .. %d, got %r" % (TRANSPORT_MAX_SUBSTEPS, substeps))
    try:
        bx = tuple(tuple(b) for b in boxes)
    except TypeError:
        raise ValueError("boxes must hold tuples (h0, h1, w0, w1), got %r" % (boxes,))
    if len(bx) > TRANSPORT_MAX_BOXES:
        raise ValueError("at most %d boxes, got %d" % (TRANSPORT_MAX_BOXES, len(bx)))
    for b in bx:
        if len(b) != 4 or not all(whole(v) for v in b) or not (0 <= b[0] <= b[1] and 0 <= b[2] <= b[3]):
            raise ValueError("a box is (h0, h1, w0, w1) in pixels, inclusive, 0 <= h0 <= h1 and 0 <= w0 <= w1, got %r" % (b,))
        if known and (b[1] > int(Hh) - 1 or b[3] > int(Ww) - 1):
            raise ValueError("box %r does not fit a %d x %d field" % (b, int(Hh), int(Ww)))
    bx = tuple(tuple(int(v) for v in b) for b in bx)
    Gh = Gw = None
    if known:
        if oy > int(Hh) - 1 or ox > int(Ww) - 1:
            raise ValueError("seed_origin %r is outside the %d x %d field" % ((oy, ox), int(Hh), int(Ww)))
        Gh, Gw = (int(Hh) - 1 - oy) // sy + 1, (int(Ww) - 1 - ox) // sx + 1
    return (Gh, Gw, oy, ox, sy, sx), int(substeps), bx, float(g[0]), float(g[1]), float(step_dt)


class EnsembleTransport(EnsembleFeed):
    """On-device Lagrangian transport of sampled roll-outs of B cases, and of the target (tmg_ens_lagr_advect / tmg_ens_lagr_store /
    tmg_ens_lagr_finalize): pathlines of a lattice of seed particles through every row's own velocity field, the forward finite-time
    Lyapunov exponent of the flow map (its ridges are the repelling Lagrangian coherent structures: Haller; Shadden, Lekien & Marsden
    2005), the residence time in pixel boxes, and the spread of a parcel's endpoint over the members against its error to the
    target's endpoint.

    Rows are the S members plus the target as row S.  Positions are in pixels: px along W, py along H, pixel (h, w) at (w, h); a
    position is inside when 0 <= px <= W - 1 and 0 <= py <= H - 1.  The velocity in pixels per kept step is fl(fl(a_c y_c) + o_c),
    c = (ux, uy), a = u out_std step_dt / d, o = u out_mu step_dt / d, d = (dx, dy) (formed in fp64 as ((u sd) step_dt) / d, rounded
    once), bilinear in space, linear in time between the previous timed step and the current one.  Seeds are the pixels
    (oy + i sy, ox + j sx).  The first timed step seeds every row's particles and stores its velocity planes; every later one runs
    one advection of `substeps` Heun steps (predictor x* = x + h k1, corrector x + h (k1 + k2) / 2, h = 1 / substeps) and then
    overwrites the planes: Tn timed steps give Tn - 1 advections over T_int = (Tn - 1) step_dt, and Tn >= 2 is needed.  A particle
    whose predictor or corrector leaves the field dies: it keeps its last inside position and the index of that advection
    (member_exit; -1 while alive).  At every timed step an alive particle inside box r adds 1 to its counter.  The operation order is
    stated in include/tmglow_hip_lagr.h; an element of the state is touched by one thread once per call: the state (pos
    [S + 1, B, 2, P], exit [S + 1, B, P], res [S + 1, B, R, P], prev [S + 1, B, 2, HW]) is bitwise reproducible, independent of the
    chunking, and needs no memset.

    Feeding protocol of EnsembleFeed, with the step's target on every chunk; a step fed with time=False launches nothing.
    finalize() -> dict (fields over the lattice [Gh, Gw]; mean / population std (ddof 0) by Welford over the members valid at the
    node, in member order, NaN where none is):
      ftle_mean, ftle_std, target_ftle [B, Gh, Gw]   ln(lam) / (2 T_int), lam the largest eigenvalue of C = F^T F, F the central
                                                     differences of the final physical positions (px dx, py dy) over the seeds'
                                                     physical spacing; valid where the node and its four lattice neighbours are
                                                     alive in that row (never on the lattice's frame)
      ftle_count [B, Gh, Gw] int32                   the members valid there
      disp_mean, disp_std, target_disp [B, 2, Gh, Gw]   final minus seed position (along x, along y), over the alive members
      alive_frac, target_alive [B, Gh, Gw]           the share of the members alive at the end; 1 / 0 for the target
      res_time_mean, res_time_std, target_res_time [B, R, Gh, Gw]   counter * step_dt over all members (only with boxes)
      end_err_mean [B, Gh, Gw]                       the mean, over the members alive together with the target, of the distance
                                                     between their endpoints
      end_spread [B, Gh, Gw]                         sqrt(var_x + var_y) of the alive members' endpoints about their mean; read it
                                                     beside end_err_mean: a calibrated ensemble has them of one size
      member_ftle [B, S, Gh, Gw], member_end [B, S, 2, Gh, Gw] (pixels), member_exit [B, S, Gh, Gw] int32   (per_member=True only)
      paths [B, S + 1, Tn, 2, Gh, Gw]                the positions in pixels after every timed step (keep_paths=True only; plain
                                                     copies of pos)
      transport_seeds [Gh, Gw, 2] int64 (h, w), transport_boxes, transport_time = T_int."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), step_dt=1.0, seed_stride=(2, 2),
                 seed_origin=None, substeps=1, boxes=(), per_member=False, keep_paths=False):
        noun, why = "ensemble transport diagnostics", "the velocity scales with u * out_std"
        _ens_members(noun, members)
        self.lattice, self.n, self.boxes, self.dx, self.dy, self.step_dt = transport_args(seed_stride, seed_origin, substeps, boxes, C,
                                                                                          Hh, Ww, grid, step_dt)
        sd, mu = _ens_tables(int(C), why, out_std, out_mu)
        u = _ens_u(u, B, int(C), why)
        if int(steps) < 2 or int(B) < 1:
            raise ValueError("%s need steps >= 2 and B >= 1, got %d, %d" % (noun, steps, B))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, int(C), Hh, Ww, steps)
        HW = self.H * self.W
        self.Gh, self.Gw = self.lattice[:2]
        self.P = self.Gh * self.Gw
        self.per_member, self.keep_paths = bool(per_member), bool(keep_paths)
        d = torch.tensor([self.dx, self.dy], dtype=torch.float64).view(1, 2)
        self.a = ((_ens_scale(sd, u, self.B, torch.float64)[:, :2] * self.step_dt) / d).to(torch.float32).to(dev).contiguous()
        self.o = ((_ens_scale(mu, u, self.B, torch.float64)[:, :2] * self.step_dt) / d).to(torch.float32).to(dev).contiguous()
        self.plan = H.ens_lagr_plan(self.S, self.B, self.H, self.W, self.P)
        R = self.S + 1
        self.pos = torch.empty((R, self.B, 2, self.P), device=dev, dtype=torch.float32)
        self.exit = torch.empty((R, self.B, self.P), device=dev, dtype=torch.int32)
        self.res = torch.empty((R, self.B, len(self.boxes), self.P), device=dev, dtype=torch.int32)
        self.prev = torch.empty((R, self.B, 2, HW), device=dev, dtype=torch.float32)
        self._paths = []

    def _feed(self, yn, k, row0, t_before):
        H.ens_lagr_advect(yn, self.a, self.o, self.prev, self.pos, self.exit, self.res, self.lattice, self.boxes, self.n, k, row0, t_before)
        H.ens_lagr_store(yn, self.a, self.o, self.prev, k, row0)             # after the advection: it reads what this overwrites

    def add(self, y, m0, target, time=True):
        """Advect the particles of the step's members m0 .. m0 + k - 1 through y (API-shaped [k*B, C, H, W], any strides whose
        channels-last view is an NHWC channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the
        same stride rule, advected as row S with the step's last chunk.  A step fed with time=False launches nothing."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        if time:
            self._feed(yn, k, m0, t_before)
            if last:
                self._feed(tn, 1, self.S, t_before)
                if self.keep_paths:
                    self._paths.append(self.pos.clone())
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs over the steps folded with time=True (at least two)."""
        T = self.finalize_guard()
        if T < 2:
            raise RuntimeError("the transport needs at least 2 timed steps (one advection), got %d" % T)
        B, S, P, Gh, Gw, nb = self.B, self.S, self.P, self.Gh, self.Gw, len(self.boxes)
        dev = self.pos.device
        T_int = (T - 1) * self.step_dt
        shapes = {"ftle_count": (B, P), "disp_mean": (B, 2, P), "disp_std": (B, 2, P), "target_disp": (B, 2, P),
                  "res_time_mean": (B, nb, P), "res_time_std": (B, nb, P), "target_res_time": (B, nb, P),
                  "member_ftle": (B, S, P), "member_end": (B, S, 2, P), "member_exit": (B, S, P)}
        outs = []
        for name in H.LAGR_OUTS:
            if (name in TRANSPORT_MEMBER_FIELDS and not self.per_member) or ("res_time" in name and nb == 0):
                outs.append(None)
            else:
                outs.append(torch.empty(shapes.get(name, (B, P)), device=dev,
                                        dtype=torch.int32 if name in H.LAGR_INT_OUTS else torch.float32))
        H.ens_lagr_finalize(self.pos, self.exit, self.res, (self.dx, self.dy, self.step_dt, T_int), outs, self.lattice, self.boxes,
                            self.H, self.W)
        o = {}
        for name, t in zip(H.LAGR_OUTS, outs):
            if t is not None:
                o[name] = t.view(tuple(t.shape[:-1]) + (Gh, Gw))
        if self.keep_paths:
            # [Tn, S + 1, B, 2, P] -> [B, S + 1, Tn, 2, Gh, Gw]
            o["paths"] = torch.stack(self._paths).permute(2, 1, 0, 3, 4).reshape(B, S + 1, T, 2, Gh, Gw).contiguous()
        _, _, oy, ox, sy, sx = self.lattice
        hh = (oy + sy * torch.arange(Gh)).view(Gh, 1).expand(Gh, Gw)
        ww = (ox + sx * torch.arange(Gw)).view(1, Gw).expand(Gh, Gw)
        o["transport_seeds"] = torch.stack((hh, ww), dim=-1).contiguous()
        o["transport_boxes"] = self.boxes
        o["transport_time"] = T_int
        return o


VORTEX_MAX_K = 256
VORTEX_MAX_CIRC_BINS = 32
VORTEX_AREA_BINS = 19
VORTEX_MAX_SIDE = 512


def vortex_args(threshold, qscale, min_area, max_vortices, circ_bins, circ_range, C, Hh, Ww, grid, B=None):
    """The checks and the defaults of the vortex census arguments, without a device: 2 <= C <= 4 (channels 0 and 1 are the velocity),
    3 <= H, W <= 512, grid two positive finite sizes (dx, dy); threshold None, one finite number >= 0 or one per case, in physical
    1/s^2; qscale None, one positive power of two or one per case; min_area an integer >= 1; max_vortices an integer in 1 .. 256;
    circ_bins an integer in 1 .. 32; circ_range None, one (lo, hi) with 0 <= lo < hi or one per case.  H = W = None (the field is not
    known yet) skips the field's limits; B = None the lengths of the per-case arrays.
    -> (thr, qs, min_area, K, nb, cr, dx, dy): thr, qs [B] and cr [B, 2] fp64 CPU tensors, or None where None was given."""
    real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))   # noqa: E731
    whole = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)                         # noqa: E731
    if not 2 <= int(C) <= 4:
        raise ValueError("the vortex census needs 2 <= C <= 4 channels (ux, uy first), got %d" % int(C))
    known = Hh is not None and Ww is not None
    if known and not (3 <= int(Hh) <= VORTEX_MAX_SIDE and 3 <= int(Ww) <= VORTEX_MAX_SIDE):
        raise ValueError("the vortex census needs 3 <= H, W <= %d, got %d x %d" % (VORTEX_MAX_SIDE, int(Hh), int(Ww)))
    try:
        g = tuple(grid)
    except TypeError:
        raise ValueError("grid must hold (dx, dy), got %r" % (grid,))
    if len(g) != 2 or not all(real(v) and float(v) > 0 for v in g):
        raise ValueError("grid must hold two positive finite sizes (dx, dy), got %r" % (grid,))

    def per_case(v, name, width, ok, rule):
        if v is None:
            return None
        try:
            t = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError("%s must be %s, got %r" % (name, rule, v))
        if t.dim() == width:
            t = t.unsqueeze(0).expand((1 if B is None else int(B),) + tuple(t.shape)).contiguous()
        if t.dim() != width + 1 or (width and t.shape[-1] != 2) or (B is not None and t.shape[0] != int(B)) or not bool(ok(t).all()):
            raise ValueError("%s must be %s, got %r" % (name, rule, v))
        return t

    thr = per_case(threshold, "threshold", 0, lambda t: torch.isfinite(t) & (t >= 0), "None, one finite number >= 0 or one per case")
    pow2 = lambda t: torch.isfinite(t) & (t > 0) & (torch.frexp(t.clamp(min=1e-300))[0] == 0.5) & (t >= 2.0 ** -100) & (t <= 2.0 ** 100)   # noqa: E731
    qs = per_case(qscale, "qscale", 0, pow2, "None, one positive power of two (2^-100 .. 2^100) or one per case")
    cr = per_case(circ_range, "circ_range", 1, lambda t: (torch.isfinite(t) & (t >= 0)) & (t[..., 1:] > t[..., :1]),
                  "None, one (lo, hi) with 0 <= lo < hi or one per case")
    if not whole(min_area) or int(min_area) < 1:
        raise ValueError("min_area must be an integer >= 1, got %r" % (min_area,))
    if not whole(max_vortices) or not 1 <= int(max_vortices) <= VORTEX_MAX_K:
        raise ValueError("max_vortices must be an integer in 1 .. %d, got %r" % (VORTEX_MAX_K, max_vortices))
    if not whole(circ_bins) or not 1 <= int(circ_bins) <= VORTEX_MAX_CIRC_BINS:
        raise ValueError("circ_bins must be an integer in 1 .. %d, got %r" % (VORTEX_MAX_CIRC_BINS, circ_bins))
    return thr, qs, int(min_area), int(max_vortices), int(circ_bins), cr, float(g[0]), float(g[1])


def vortex_defaults(tp, grid):
    """tp [B, T, 2.., H, W]: the physical target series at the timed steps -> (threshold, qscale) [B] fp64 (CPU), the defaults of the
    census: 0.2 times the population std, over the interior pixels and the steps, of ow = w^2 - sn^2 - ss^2 (the 0.2 sigma of
    Isern-Fontanet et al.), and 2^(20 - ceil(log2(max |w|))), so that the largest vorticity lands in (2^19, 2^20] fixed-point steps.
    Plain torch in fp64: this only chooses two numbers per case.  A target whose ow does not vary, or without vorticity, raises."""
    tp = tp.double()
    U, V = tp[:, :, 0], tp[:, :, 1]
    ddx = lambda q: 2 * q[..., 1:-1, 2:] + q[..., :-2, 2:] + q[..., 2:, 2:] - 2 * q[..., 1:-1, :-2] - q[..., :-2, :-2] - q[..., 2:, :-2]   # noqa: E731
    ddy = lambda q: 2 * q[..., 2:, 1:-1] + q[..., 2:, :-2] + q[..., 2:, 2:] - 2 * q[..., :-2, 1:-1] - q[..., :-2, :-2] - q[..., :-2, 2:]   # noqa: E731
    rdx, rdy = 0.125 / float(grid[0]), 0.125 / float(grid[1])
    ux, uy, vx, vy = ddx(U) * rdx, ddy(U) * rdy, ddx(V) * rdx, ddy(V) * rdy
    w, sn, ss = vx - uy, ux - vy, vx + uy
    ow = (w * w - sn * sn - ss * ss).reshape(tp.shape[0], -1)
    sig = ow.std(1, unbiased=False).cpu()
    wmax = w.abs().reshape(tp.shape[0], -1).max(1).values.cpu()
    bad = ~(torch.isfinite(sig) & (sig > 0) & torch.isfinite(wmax) & (wmax > 0))
    if bool(bad.any()):
        raise ValueError("the Okubo-Weiss field of the target of case %d does not vary (std %r, max |vorticity| %r): give threshold and "
                         "qscale" % (int(bad.nonzero()[0]), float(sig[bad][0]), float(wmax[bad][0])))
    return 0.2 * sig, torch.pow(2.0, 20.0 - torch.ceil(torch.log2(wmax)))


def _vortex_w1(p, q, h):
    """The Wasserstein-1 distance between the distributions of the counts p, q [..., nb] with each bin's mass at its centre:
    h sum_{j < nb - 1} |F_j - G_j|, F, G the cumulative shares, in fp64; NaN when either holds no sample."""
    F = p.cumsum(-1)[..., :-1].double() / p.sum(-1, keepdim=True).double()
    G = q.cumsum(-1)[..., :-1].double() / q.sum(-1, keepdim=True).double()
    out = (F - G).abs().sum(-1) * h
    return torch.where((p.sum(-1) > 0) & (q.sum(-1) > 0), out, torch.full_like(out, float("nan")))


def vortex_finalize(tab, found, S, Hh, Ww, dx, dy, qscale, nb, circ_range):
    """The statistics of the integer tables: tab [B, S + 1, T, K, 8] int64 (the target last), found [B, S + 1, T, 2] (CPU), qscale [B]
    fp64, circ_range [B, 2] fp64 or None -> dict of fp64 CPU tensors (EnsembleVortices.finalize documents them).  Plain torch."""
    B, R, T, K = tab.shape[:4]
    cell = dx * dy
    valid = tab[..., 0] >= 0
    n, sq = tab[..., 1], tab[..., 4]
    sgn = torch.stack((valid & (sq > 0), valid & (sq < 0)), dim=-1)                       # [B, R, T, K, 2]
    gamma = sq.double() * cell / qscale.view(B, 1, 1, 1)
    den = torch.where(sq != 0, sq, torch.ones_like(sq)).double()
    cx, cy = tab[..., 5].double() / den * dx, tab[..., 6].double() / den * dy              # physical centroids
    sd = sgn.double()
    o = {}
    per_row = {"count": found.double(), "area_frac": (n.double().unsqueeze(-1) * sd).sum(3) / float((Hh - 2) * (Ww - 2)),
               "circ_sum": (gamma.unsqueeze(-1) * sd).sum(3)}
    for key, v in per_row.items():                                                        # [B, R, T, 2]
        o[key + "_mean"], o[key + "_std"], o["target_" + key] = v[:, :S].mean(1), v[:, :S].std(1, unbiased=False), v[:, S]
    # the distributions, pooled over the timed steps
    abin = sum((n >= (1 << j)).long() for j in range(1, VORTEX_AREA_BINS))
    if circ_range is None:
        top = (gamma[:, S].abs() * valid[:, S].double()).reshape(B, -1).max(1).values
        circ_range = torch.stack((torch.zeros(B, dtype=torch.float64), torch.where(top > 0, 1.25 * top, torch.ones_like(top))), dim=1)
    lo, hi = circ_range[:, 0].view(B, 1, 1, 1), circ_range[:, 1].view(B, 1, 1, 1)
    cbin = torch.floor((gamma.abs() - lo) / (hi - lo) * nb).clamp(0, nb - 1).long()
    ah, ch = torch.zeros(B, R, 2, VORTEX_AREA_BINS, dtype=torch.int64), torch.zeros(B, R, 2, nb, dtype=torch.int64)
    for s in range(2):
        wgt = sgn[..., s].reshape(B, R, T * K).long()
        ah[:, :, s].scatter_add_(2, abin.reshape(B, R, T * K), wgt)
        ch[:, :, s].scatter_add_(2, cbin.reshape(B, R, T * K), wgt)
    o["area_hist"], o["circ_hist"] = ah, ch
    hc = ((circ_range[:, 1] - circ_range[:, 0]) / nb).view(B, 1)
    o["time_area_w1"] = _vortex_w1(ah[:, :S].sum(1), ah[:, S], 1.0)
    o["time_circ_w1"] = _vortex_w1(ch[:, :S].sum(1), ch[:, S], hc)
    o["time_member_circ_w1"] = _vortex_w1(ch[:, :S], ch[:, S:], hc.view(B, 1, 1))
    o["vortex_circ_edges"] = circ_range[:, :1] + (circ_range[:, 1:] - circ_range[:, :1]) * torch.arange(nb + 1, dtype=torch.float64).view(1, -1) / nb
    # object matching: every kept target vortex against the nearest kept vortex of its sign in every member
    nan = float("nan")
    md, mf = torch.full((B, T, 2), nan, dtype=torch.float64), torch.full((B, T, 2), nan, dtype=torch.float64)
    for t in range(T):
        for s in range(2):
            tm, mm = sgn[:, S, t, :, s], sgn[:, :S, t, :, s]                              # [B, K], [B, S, K]
            if not bool(tm.any()):
                continue
            ddx_ = cx[:, S, t].view(B, 1, K, 1) - cx[:, :S, t].view(B, S, 1, K)
            ddy_ = cy[:, S, t].view(B, 1, K, 1) - cy[:, :S, t].view(B, S, 1, K)
            D = torch.sqrt(ddx_ * ddx_ + ddy_ * ddy_).masked_fill(~mm.view(B, S, 1, K), float("inf"))
            dmin = D.min(-1).values                                                       # [B, S, K]
            has = mm.any(-1).view(B, S, 1)
            hit, miss = tm.view(B, 1, K) & has, tm.view(B, 1, K) & ~has
            nh, nm = hit.sum((1, 2)).double(), miss.sum((1, 2)).double()
            dsum = torch.where(hit, dmin, torch.zeros_like(dmin)).sum((1, 2))
            any_t = tm.any(-1)
            md[:, t, s] = torch.where(any_t & (nh > 0), dsum / nh.clamp(min=1), torch.full_like(dsum, nan))
            mf[:, t, s] = torch.where(any_t, nm / (nh + nm).clamp(min=1), torch.full_like(dsum, nan))
    o["match_dist_mean"], o["match_miss_frac"] = md, mf
    return o


class EnsembleVortices(EnsembleFeed):
    """On-device vortex census of sampled roll-outs of B cases, and of the target (tmg_ens_vortex_classify / tmg_ens_vortex_label /
    tmg_ens_vortex_census): how many vortices does a field hold, how big and how strong are they, where do they live, and are the
    target's vortices present in the members at the right place?  The Okubo-Weiss / Q-criterion census of McWilliams (1990) with the
    0.2 sigma threshold of Isern-Fontanet et al., and the object-based verification of meteorology (SAL, MODE).

    Rows are the S members plus the target as row S.  At every timed step a pixel of a row gets the class sign(w) when it is not on
    the one-pixel frame, ow = w^2 - sn^2 - ss^2 > threshold[b] (w the vorticity, sn and ss the strains, from the un-scaled 3x3 stencils
    of pc/ on u (out_std y + out_mu); w is bit for bit the `vort` of EnsemblePdfs), |qf| <= 2^31 and q != 0 with the fixed-point
    vorticity qf = fl(w qscale[b]), q = rint(qf); else 0.  An interior pixel whose ow is NaN or whose qf alone fails is counted in
    vortex_rejected.  A vortex is a maximal 4-connected set of pixels of one non-zero class; its label is its smallest linear index.
    Its measures are 8 int64 words (root, n, sum w, sum h, sum q, sum q w, sum q h, max |q|): exact and independent of any order.
    The table of a row, case and step holds the vortices with n >= min_area in increasing root order, the first K = max_vortices of
    them; vortex_found counts them all.  The operation order is stated in include/tmglow_hip_vortex.h.  The state (the tables, 64 K
    bytes per row, case and step, and two occupancy planes of 8 bytes per pixel and case) holds integers only: bitwise reproducible
    and independent of the chunking; the workspace (17 bytes per pixel of the largest chunk) is transient.

    threshold and qscale are one number or one per case (vortex_defaults gives the target's own); circ_range None: [0, 1.25 max |G|]
    of the target's table per case.  Feeding protocol of EnsembleFeed, with the step's target on every chunk; a step fed with
    time=False launches nothing.  finalize() raises RuntimeError when a labelling loop reached its trip bound (the status word);
    else -> dict (fp32 unless stated; mean / population std (ddof 0) over the members; the sign axis is (+, -); G = circulation):
      target_vortex_table [B, Tn, K, 8] int64           the target's tables; an empty slot is (-1, 0, ..)
      vortex_table [B, S + 1, Tn, K, 8] int64           every row's (per_member=True only)
      vortex_found [B, S + 1, Tn, 2] int32              the vortices with n >= min_area, before the truncation to K
      vortex_rejected [B, S + 1, Tn] int32, vortex_truncated [B] int64 (the tables of the case with found(+) + found(-) > K)
      count_mean, count_std, target_count [B, Tn, 2]    of vortex_found
      area_frac_mean, area_frac_std, target_area_frac   the share of the interior pixels in kept vortices
      circ_sum_mean, circ_sum_std, target_circ_sum      the sum of G = sum q dx dy / qscale over the kept vortices
      area_hist [B, S + 1, 2, 19] int64                 the kept vortices of all timed steps by floor(log2 n)
      circ_hist [B, S + 1, 2, circ_bins] int64          ... by |G| over circ_range (what lies outside goes to the end bins)
      time_area_w1, time_circ_w1 [B, 2]                 the Wasserstein-1 distance between the pooled members' distribution and the
                                                        target's (in bins of log2 n / in units of G); NaN when either is empty
      time_member_circ_w1 [B, S, 2]                     each member's against the target's
      core_prob, target_core_freq [B, 2, H, W]          the share of (member, step) / of steps at which the pixel lies in a vortex
                                                        with n >= min_area, truncated or not
      match_dist_mean [B, Tn, 2]                        the mean, over the members and the kept target vortices, of the physical
                                                        distance from the target vortex' w-weighted centroid (sum q w / sum q,
                                                        sum q h / sum q) to the nearest kept vortex of its sign in the member
      match_miss_frac [B, Tn, 2]                        the share of (member, target vortex) pairs without any vortex of that sign;
                                                        both NaN where the target has none
      vortex_threshold, vortex_qscale [B], vortex_circ_edges [B, circ_bins + 1] float64; vortex_args, the dict (min_area,
      max_vortices, circ_bins)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), threshold=None, qscale=None,
                 min_area=4, max_vortices=64, circ_bins=16, circ_range=None, per_member=False):
        noun, why = "ensemble vortex censuses", "the velocity scales with u * out_std"
        _ens_members(noun, members)
        thr, qs, self.min_area, self.K, self.nb, self.circ_range, self.dx, self.dy = vortex_args(
            threshold, qscale, min_area, max_vortices, circ_bins, circ_range, C, Hh, Ww, grid, B=int(B))
        if thr is None or qs is None:
            raise ValueError("%s need threshold and qscale: they come from the target's series (vortex_defaults), which an accumulator "
                             "does not see before it is fed" % noun)
        sd, mu = _ens_tables(int(C), why, out_std, out_mu)
        u = _ens_u(u, B, int(C), why)
        if int(steps) < 1 or int(B) < 1:
            raise ValueError("%s need steps, B >= 1, got %d, %d" % (noun, steps, B))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, int(C), Hh, Ww, steps)
        self.per_member = bool(per_member)
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).contiguous()
        self.thr = thr.to(torch.float32).to(dev).contiguous()
        self.qs = qs.to(torch.float32).to(dev).contiguous()
        R, HW = self.S + 1, self.H * self.W
        self.plan = H.ens_vortex_plan(1, self.S, self.B, self.H, self.W, self.K, self.Tk)
        self.table = torch.empty((self.Tk, R, self.B, self.K, H.VORTEX_WORDS), device=dev, dtype=torch.int64)
        self.found = torch.empty((self.Tk, R, self.B, 2), device=dev, dtype=torch.int32)
        self.rejected = torch.empty((self.Tk, R, self.B), device=dev, dtype=torch.int32)
        self.core = torch.zeros((2, self.B, 2, HW), device=dev, dtype=torch.int32)          # the members', the target's
        self.status = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.ws = None

    def reserve(self, k):
        """The workspace of chunks of up to k rows (17 bytes per pixel; grown when a larger chunk arrives; its content never matters)."""
        need = 17 * int(k) * self.B * self.H * self.W
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty((need,), device=self.table.device, dtype=torch.uint8)
        return self.ws

    def _planes(self, k):
        n, HW = k * self.B * self.H * self.W, self.H * self.W
        ws = self.reserve(k)
        i32 = lambda j: ws[4 * j * n:4 * (j + 1) * n].view(torch.int32).view(k * self.B, HW)   # noqa: E731
        return ws[:4 * n].view(torch.float32).view(k * self.B, HW), i32(1), i32(2), i32(3), ws[16 * n:17 * n].view(torch.int8).view(k * self.B, HW)

    def _feed(self, yn, k, row0, t, core):
        om, lab, area, slot, cls = self._planes(k)
        H.ens_vortex_classify(yn, self.u, self.mu, self.sd, self.thr, self.qs, om, cls, self.rejected[t, row0:row0 + k], (self.dx, self.dy), k)
        H.ens_vortex_label(cls, lab, self.status, self.H, self.W)
        H.ens_vortex_census(lab, cls, om, self.qs, area, slot, self.table[t, row0:row0 + k].view(k * self.B, self.K, H.VORTEX_WORDS),
                            self.found[t, row0:row0 + k].view(k * self.B, 2), core, self.H, self.W, k, self.min_area)

    def add(self, y, m0, target, time=True):
        """Take the census of the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last
        view is an NHWC channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride
        rule, taken as row S with the step's last chunk.  A step fed with time=False launches nothing."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        if time:
            self._feed(yn, k, m0, t_before, self.core[0])
            if last:
                self._feed(tn, 1, self.S, t_before, self.core[1])
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs over the steps folded with time=True."""
        T = self.finalize_guard()
        code = int(self.status.item())
        if code:
            raise RuntimeError("the vortex labelling reached a loop's trip bound (status %d): the labels are not to be trusted" % code)
        B, S, K, Hh, Ww = self.B, self.S, self.K, self.H, self.W
        tab = self.table[:T].permute(2, 1, 0, 3, 4).contiguous().cpu()                    # [B, S + 1, T, K, 8]
        found = self.found[:T].permute(2, 1, 0, 3).contiguous().cpu()
        qs64 = self.qs.double().cpu()
        f = vortex_finalize(tab, found, S, Hh, Ww, self.dx, self.dy, qs64, self.nb, self.circ_range)
        o = {key: (v if v.dtype == torch.int64 else v.to(torch.float32)) for key, v in f.items() if key != "vortex_circ_edges"}
        o["vortex_circ_edges"] = f["vortex_circ_edges"]
        o["target_vortex_table"] = tab[:, S].contiguous()
        if self.per_member:
            o["vortex_table"] = tab
        o["vortex_found"] = found
        o["vortex_rejected"] = self.rejected[:T].permute(2, 1, 0).contiguous().cpu()
        o["vortex_truncated"] = (found.long().sum(-1) > K).sum((1, 2))
        core = self.core.cpu().double().view(2, B, 2, Hh, Ww)
        o["core_prob"] = (core[0] / float(S * T)).to(torch.float32)
        o["target_core_freq"] = (core[1] / float(T)).to(torch.float32)
        o["vortex_threshold"], o["vortex_qscale"] = self.thr.double().cpu(), qs64
        o["vortex_args"] = dict(min_area=self.min_area, max_vortices=K, circ_bins=self.nb)
        return o


FLUX_WIDTHS = (3, 5, 9, 17, 33)
FLUX_MAX_WIDTHS = 8
FLUX_MAX_WIDTH = 33
FLUX_PLANES = 7


def flux_args(widths, C, Hh, Ww, grid):
    """The checks and the defaults of the flux arguments: 2 <= C <= 4 (channels 0 and 1 are read), H, W >= 5 (one valid pixel of
    width 3), grid two positive finite sizes; widths (None: FLUX_WIDTHS without those over min(H, W) - 2) at most 8 odd integers in
    3 .. 33, strictly increasing, none over min(H, W) - 2.  H = W = None (the field is not known yet) skips the field's limits.
    -> (widths, dx, dy)."""
    real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v))   # noqa: E731
    if not 2 <= int(C) <= 4:
        raise ValueError("the energy flux needs 2 <= C <= 4 channels (ux, uy first), got %d" % int(C))
    known = Hh is not None and Ww is not None
    if known and (int(Hh) < 5 or int(Ww) < 5):
        raise ValueError("the energy flux needs H, W >= 5 (a 3 x 3 box and the ring of the stencils), got %d x %d" % (int(Hh), int(Ww)))
    try:
        g = tuple(grid)
    except TypeError:
        raise ValueError("grid must hold (dx, dy), got %r" % (grid,))
    if len(g) != 2 or not all(real(v) and float(v) > 0 for v in g):
        raise ValueError("grid must hold two positive finite sizes (dx, dy), got %r" % (grid,))
    lim = min(int(Hh), int(Ww)) - 2 if known else FLUX_MAX_WIDTH
    if widths is None:
        ws = tuple(w for w in FLUX_WIDTHS if w <= lim)
    else:
        try:
            ws = tuple(widths)
        except TypeError:
            raise ValueError("widths must hold odd box widths in pixels, got %r" % (widths,))
        if not 1 <= len(ws) <= FLUX_MAX_WIDTHS:
            raise ValueError("widths must hold 1 .. %d box widths, got %d" % (FLUX_MAX_WIDTHS, len(ws)))
        if not all(isinstance(w, numbers.Integral) and not isinstance(w, bool) for w in ws):
            raise ValueError("widths must be integers, got %r" % (widths,))
        ws = tuple(int(w) for w in ws)
        if any(w < 3 or w > FLUX_MAX_WIDTH or w % 2 == 0 for w in ws):
            raise ValueError("widths must be odd and in 3 .. %d, got %r" % (FLUX_MAX_WIDTH, ws))
        if any(b <= a for a, b in zip(ws, ws[1:])):
            raise ValueError("widths must be strictly increasing, got %r" % (ws,))
        if ws[-1] > lim:
            raise ValueError("width %d does not fit a %s x %s field: a width is at most min(H, W) - 2 = %d" % (ws[-1], Hh, Ww, lim))
    return ws, float(g[0]), float(g[1])


def flux_factors(widths, dx, dy):
    """k [L, 2] fp64 (CPU): 1 / (8 dx N^3), 1 / (8 dy N^3), N = w^2: Pi = -(A kx + B ky) with the un-normalised sums A, B."""
    return torch.tensor([[1.0 / ((8.0 * d) * float((w * w) ** 3)) for d in (float(dx), float(dy))] for w in widths], dtype=torch.float64)


class EnsembleFlux(EnsembleFeed):
    """On-device scale-to-scale energy flux and sub-filter stresses of sampled roll-outs of B cases, and of the target
    (tmg_ens_flux_accum / tmg_ens_flux_terms): the coarse-graining analysis of Germano, Eyink and Aluie.  For a box filter of width
    l = w pixels, tau_ij(l) = bar(u_i u_j) - bar(u_i) bar(u_j) is the sub-filter stress and Pi_l(x, t) = -tau_ij d bar(u_i) / dx_j the
    local flux of energy across l: positive for a forward cascade, negative for backscatter.

    Rows are the S members plus the target as row S.  The filtered field of a row is f_c = fl(a_c y_c), c = (ux, uy), a = u * out_std
    (formed in fp64, rounded once); out_mu never enters: tau and the gradients of bar(u) are exactly invariant to a constant
    velocity, and leaving it out shrinks the cancellation.  For a width w, r = w // 2, N = w^2, the state holds un-normalised
    quantities (integers on integer data): the box sums Sg of f_u, f_v, f_u f_u, f_u f_v, f_v f_v (a row pass, then a column pass, both
    added from the centre outwards; no running window, no summed-area table), Q_ij = N Sg_ij - Sg_i Sg_j = N^2 tau_ij,
    A = Q_uu Sx Sg_u + Q_uv Sx Sg_v, B = Q_uv Sy Sg_u + Q_vv Sy Sg_v with the un-scaled 3x3 stencils of pc/ applied to the box sums of
    the eight neighbours, and Pi_s = -(A kx + B ky), kx = 1 / (8 dx N^3), ky = 1 / (8 dy N^3).  A pixel is valid for w when the box and
    the ring of the stencils lie inside the field, r + 1 <= h <= H - 2 - r and the same in w: no padding, no one-sided filter, NaN
    outside.  Every timed step adds 7 fp32 quantities per row, width and valid pixel to `raw` [S + 1, B, L, 7, HW]: A, B, Pi_s^2,
    [Pi_s < 0], Q_uu, Q_uv, Q_vv.  An element is touched by one thread once per call: the state is bitwise reproducible, independent of
    the chunking, and needs no memset (the first timed step stores; invalid pixels are neither written nor read).  It takes 28 L
    bytes per element of [S + 1, B, HW].

    finalize() forms, in fp64 on the device, per row and width: Pi = -(sum A kx + sum B ky) / T, the temporal std of Pi_s
    sqrt(max(sum Pi_s^2 / T - Pi^2, 0)), the backscatter fraction count / T, tau = sum Q / (N^2 T).

    Feeding protocol of EnsembleFeed, with the step's target on every chunk; a step fed with time=False launches nothing.
    finalize() -> dict:
      flux_mean, flux_std, target_flux [B, L, H, W]        Welford mean / population std (ddof 0) over the members, and the target's
      flux_tstd_mean, target_flux_tstd [B, L, H, W]        the same of the temporal std of Pi_s
      backscatter_mean, backscatter_std, target_backscatter [B, L, H, W]
      sgs_mean, sgs_std, target_sgs [B, L, 3, H, W]        the same of tau (uu, uv, vv)
      member_flux [B, S, L, H, W]                          every member's Pi (per_member=True only)
      flux_curve, sgs_energy_curve [B, S + 1, L]           per row, the target last: the mean over the width's valid region of Pi and
                                                           of (tau_uu + tau_vv) / 2 (fp64, partials folded in a fixed order)
      flux_widths [L], flux_lengths [L, 2]                 the widths in pixels and as lengths (w dx, w dy)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), widths=None, per_member=False):
        noun, why = "ensemble energy fluxes", "the filtered velocity scales with u * out_std"
        _ens_members(noun, members)
        self.widths, self.dx, self.dy = flux_args(widths, C, Hh, Ww, grid)
        sd, _mu = _ens_tables(int(C), why, out_std, out_mu)
        u = _ens_u(u, B, int(C), why)
        if int(steps) < 1 or int(B) < 1:
            raise ValueError("%s need steps, B >= 1, got %d, %d" % (noun, steps, B))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.per_member = bool(per_member)
        self.L = len(self.widths)
        self.a = _ens_scale(sd, u, self.B, torch.float64)[:, :2].to(torch.float32).to(dev).contiguous()
        k64 = flux_factors(self.widths, self.dx, self.dy)
        self.k64 = k64.to(dev)
        self.kk = k64.to(torch.float32).to(dev)
        self.plan = H.ens_flux_plan(self.S, self.B, self.H, self.W, self.widths)
        self.raw = torch.empty((self.S + 1, self.B, self.L, FLUX_PLANES, self.H * self.W), device=dev, dtype=torch.float32)

    def add(self, y, m0, target, time=True):
        """Add the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule, added as
        row S with the step's last chunk.  A step fed with time=False launches nothing."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        if time:
            H.ens_flux_accum(yn, self.a, self.kk, self.raw, self.widths, k, m0, t_before)
            if last:
                H.ens_flux_accum(tn, self.a, self.kk, self.raw, self.widths, 1, self.S, t_before)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs over the steps folded with time=True."""
        T = self.finalize_guard()
        B, S, L, Hh, Ww = self.B, self.S, self.L, self.H, self.W
        HW, dev = Hh * Ww, self.raw.device
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)   # noqa: E731
        outs = [new(B, L, HW) for _ in range(8)] + [new(B, L, 3, HW) for _ in range(3)]
        outs += [new(B, S, L, HW) if self.per_member else None, new(B, S + 1, L), new(B, S + 1, L)]
        H.ens_flux_terms(self.raw, self.k64, outs, self.widths, Hh, Ww, T)
        o = {}
        for key, t in zip(H.FLUX_OUTS, outs):
            if t is not None:
                o[key] = t if key.endswith("curve") else t.view(tuple(t.shape[:-1]) + (Hh, Ww))
        o["flux_widths"] = torch.tensor(self.widths, dtype=torch.int64)
        o["flux_lengths"] = torch.tensor([[w * self.dx, w * self.dy] for w in self.widths], dtype=torch.float64)
        return o


CORR_MAX_PROBES = 8
CORR_MAX_PAIRS = 4
CORR_MAX_LAGS = 8
CORR_MAX_LAG = 64


def corr_args(probes, pairs, lags, C, Hh, Ww):
    """The checks and the defaults of the two-point correlation arguments: C == 3; probes (None: the three pixels (H // 2, W // 4),
    (H // 2, W // 2), (H // 2, 3 W // 4)) at most 8 pixels (h, w) inside the field, duplicates allowed; pairs (None: ((0, 0), (1, 1)))
    at most 4 pairs (ci, cj) of channels in 0..2; lags (None: (0, 1, 2, 4)) at most 8 strictly increasing integers that start at 0
    and stay <= 64 -> (probes, pairs, lags) as tuples of ints."""
    whole = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Integral)   # noqa: E731
    if int(C) != 3:
        raise ValueError("two-point correlations need C == 3 channels (ux, uy, p), got %d" % int(C))
    Hh, Ww = int(Hh), int(Ww)
    if Hh < 1 or Ww < 1:
        raise ValueError("two-point correlations need H, W >= 1, got %d x %d" % (Hh, Ww))
    if probes is None:
        probes = ((Hh // 2, Ww // 4), (Hh // 2, Ww // 2), (Hh // 2, 3 * Ww // 4))
    if pairs is None:
        pairs = ((0, 0), (1, 1))
    if lags is None:
        lags = (0, 1, 2, 4)

    def table(v, name, width):
        try:
            rows = [tuple(r) if width else r for r in v]
        except TypeError:
            raise ValueError("%s must be a sequence%s, got %r" % (name, " of pairs of integers" if width else " of integers", v))
        if width and not all(len(r) == 2 and whole(r[0]) and whole(r[1]) for r in rows):
            raise ValueError("%s must hold pairs of integers, got %r" % (name, v))
        if not width and not all(whole(r) for r in rows):
            raise ValueError("%s must hold integers, got %r" % (name, v))
        return rows

    probes, pairs, lags = table(probes, "probes", 2), table(pairs, "pairs", 2), table(lags, "lags", 0)
    if not 1 <= len(probes) <= CORR_MAX_PROBES:
        raise ValueError("1 to %d probes, got %d" % (CORR_MAX_PROBES, len(probes)))
    if not 1 <= len(pairs) <= CORR_MAX_PAIRS:
        raise ValueError("1 to %d channel pairs, got %d" % (CORR_MAX_PAIRS, len(pairs)))
    if not 1 <= len(lags) <= CORR_MAX_LAGS:
        raise ValueError("1 to %d lags, got %d" % (CORR_MAX_LAGS, len(lags)))
    for h, w in probes:
        if not (0 <= h < Hh and 0 <= w < Ww):
            raise ValueError("probe (%d, %d) lies outside the %d x %d field" % (h, w, Hh, Ww))
    for ci, cj in pairs:
        if not (0 <= ci <= 2 and 0 <= cj <= 2):
            raise ValueError("pair (%d, %d): channels are 0..2" % (ci, cj))
    if lags[0] != 0 or any(b <= a for a, b in zip(lags, lags[1:])):
        raise ValueError("lags start at 0 and increase strictly (a negative lag: exchange ci and cj), got %r" % (lags,))
    if lags[-1] > CORR_MAX_LAG:
        raise ValueError("the largest lag is %d kept steps, got %d" % (CORR_MAX_LAG, lags[-1]))
    return (tuple((int(h), int(w)) for h, w in probes), tuple((int(a), int(b)) for a, b in pairs), tuple(int(v) for v in lags))


def corr_probe_stats(series, pairs, lags, T):
    """The probe's side of the Pearson coefficient, fp64 on the host (not the hot path): series [S + 1, B, steps, P, 3], the rows'
    fluctuations at the probes at the timed steps 0 .. T - 1 -> (pm, pv) [S + 1, B, P, Q, L] fp64 CPU tensors: the mean and the
    population variance (about that mean) of the first n_l = T - tau_l values of series[.., p, ci_q]; NaN where n_l < 1."""
    s = torch.as_tensor(series).detach().cpu().double()
    R, B, _, P, _ = s.shape
    pm = torch.full((R, B, P, len(pairs), len(lags)), float("nan"), dtype=torch.float64)
    pv = pm.clone()
    for q, (ci, _cj) in enumerate(pairs):
        for l, tau in enumerate(lags):
            n = int(T) - int(tau)
            if n >= 1:
                v = s[:, :, :n, :, ci]
                mean = v.sum(2) / n
                pm[:, :, :, q, l] = mean
                pv[:, :, :, q, l] = ((v - mean.unsqueeze(2)) ** 2).sum(2) / n
    return pm, pv


def corr_lengths(line, pos, step):
    """Integral length scales from a lag-0 correlation line through the probe, fp64 on the host: line [.., n] with the probe at index
    pos -> [.., 2] fp64 CPU tensor, towards growing and towards falling index.  With rho_i the value i pixels from the probe and k the
    first i >= 1 that is outside the line or has rho_i <= 0 or NaN: len = step (rho_0 / 2 + sum_{i = 1}^{k - 1} rho_i), the trapezoid
    to a zero at k."""
    a = torch.as_tensor(line).detach().cpu().double()
    pos = int(pos)
    out = torch.empty(tuple(a.shape[:-1]) + (2,), dtype=torch.float64)
    for d, seq in enumerate((a[..., pos + 1:], a[..., :pos].flip(-1))):
        alive = torch.cumprod((seq > 0).to(torch.int64), dim=-1) > 0          # (NaN > 0 is False)
        out[..., d] = float(step) * (a[..., pos] / 2.0 + torch.where(alive, seq, torch.zeros_like(seq)).sum(-1))
    return out


def corr_shift(line, pos):
    """The displacement in pixels of the maximum of a correlation line from the probe at index pos, fp64 on the host: line [.., n] ->
    [..] fp64 CPU tensor; refined by the parabola through the peak and its two neighbours when the peak is interior, all three are
    finite and the second difference is negative; NaN for an all-NaN line."""
    a = torch.as_tensor(line).detach().cpu().double()
    n = a.shape[-1]
    flat = a.reshape(-1, n)
    nan = torch.isnan(flat)
    k = torch.where(nan, torch.full_like(flat, -math.inf), flat).argmax(-1)
    at = lambda i: flat.gather(1, i.clamp(0, n - 1).unsqueeze(1)).squeeze(1)   # noqa: E731
    y0, ym, yp = at(k), at(k - 1), at(k + 1)
    den = (ym - 2.0 * y0) + yp
    ok = (k > 0) & (k < n - 1) & torch.isfinite(ym) & torch.isfinite(yp) & torch.isfinite(y0) & (den < 0)
    delta = torch.where(ok, 0.5 * (ym - yp) / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
    out = (k - int(pos)).double() + delta
    out[nan.all(-1)] = float("nan")
    return out.reshape(tuple(a.shape[:-1]))


class EnsembleCorrelation(EnsembleFeed):
    """On-device two-point space-time correlations of sampled roll-outs of B cases, and of the target, about probe points
    (tmg_ens_corr_probe / tmg_ens_corr_accum / tmg_ens_corr_finalize):

      R(x0; x, tau) = < u'_i(x0, t) u'_j(x, t + tau) >

    the size and shape of the structure that passes a chosen point (the integral length scales), where that structure is tau later,
    and from that displacement the convection velocity.

    Rows are the S members plus the target as row S.  A row's fluctuation about the TARGET's time mean is d_c = fl(a_c fl(y_c - m_c)),
    a = u * out_std (formed in fp64, rounded once), m = `mean` [B, 3, H, W] in normalised units (None: 0).  probes: P <= 8 pixels
    (h, w), pairs: Q <= 4 channel pairs (ci at the probe, cj in the field), lags: L <= 8 strictly increasing lags tau_l in timed
    steps, the first 0, the largest <= 64 (corr_args); J the sorted set of distinct cj.  t = 0, 1, .. numbers the timed steps; after T
    of them lag l has n_l = T - tau_l pairs (probe at t - tau_l, field at t).  State, fp32 on the device:
      series [S + 1, B, steps, P, 3]   every row's d at the probe pixels at every timed step
      raw [S + 1, B, NPL, HW], NPL = P Q L + 2 |J| L:  X[p,q,l] += fl(series[t - tau_l, p, ci_q] * d_{cj_q}(x, t)),  F[j,l] += d_j(x, t),
      G[j,l] += fl(d_j d_j), each plane at t >= tau_l only and stored instead of added at t == tau_l, so raw needs no memset; a lag
      with tau_l >= T leaves its planes unwritten and they are never read.
    The state takes NPL * 4 bytes per element of [S + 1, B, HW]: 40 planes, 160 bytes, at the defaults.  An element of raw is touched
    by one thread once per call: the state is bitwise reproducible and independent of the chunking.

    finalize() reads series back, forms on the host in fp64 the mean pm and the population variance pv of the probe's first n_l values
    (corr_probe_stats) and then, on the device in fp64, per (p, q, l) and row with n = n_l:
      mf = F / n,  vf = G / n - mf^2,  cov = X / n - pm mf,  rho = cov / sqrt(pv vf) when pv > 0 and vf > 0, else NaN
    the Pearson coefficient of the n paired samples, so |rho| <= 1 up to rounding.  Lags with n_l < 2 give NaN.

    Feeding protocol of EnsembleFeed, with the step's target on every chunk; a step fed with time=False launches nothing.
    finalize() -> dict:
      tp_cov_mean, tp_cov_std, tp_rho_mean, tp_rho_std [B, P, Q, L, H, W]   Welford mean / population std over the members
      target_tp_cov, target_tp_rho [B, P, Q, L, H, W]                      row S
      member_tp_rho [B, S, P, Q, L, H, W]                                  every member's rho (per_member=True only)
      tp_line_x [B, S + 1, P, Q, L, W], tp_line_y [B, S + 1, P, Q, L, H]    rho of every row on the probe's field row and column
      tp_len [B, S + 1, P, Q, 4]         integral lengths from the lag-0 lines in the directions (+x, -x, +y, -y) (corr_lengths with
                                         step = dx, dy of grid); tp_len_mean, tp_len_std [B, P, Q, 4] over the members, target_tp_len
      tp_shift [B, S + 1, P, Q, L, 2]    the displacement (along x, along y) in pixels of the maximum of each line (corr_shift)
      tp_speed [B, S + 1, P, Q, L, 2]    tp_shift * (dx, dy) / (tau_l step_dt), NaN at tau = 0; tp_speed_mean, tp_speed_std
                                         [B, P, Q, L, 2] over the members, target_tp_speed
      tp_probes, tp_pairs, tp_lags       the arguments as used.
    Not supported: probes off the pixel grid, pixel-box averages of probes, negative lags (exchange ci and cj), more than 8 probes,
    4 pairs or 8 lags or a lag over 64, the full two-point tensor, non-finite members."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), probes=None,
                 pairs=((0, 0), (1, 1)), lags=(0, 1, 2, 4), mean=None, per_member=False, step_dt=1.0):
        noun, why = "ensemble two-point correlations", "the fluctuations scale with u * out_std"
        _ens_members(noun, members)
        self.probes, self.pairs, self.lags = corr_args(probes, pairs, lags, C, Hh, Ww)
        real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(float(v)) and float(v) > 0   # noqa: E731
        try:
            g = tuple(grid)
        except TypeError:
            raise ValueError("grid must hold (dx, dy), got %r" % (grid,))
        if len(g) != 2 or not all(real(v) for v in g):
            raise ValueError("grid must hold two positive finite sizes (dx, dy), got %r" % (grid,))
        if not real(step_dt):
            raise ValueError("step_dt must be finite and > 0, got %r" % (step_dt,))
        self.grid, self.step_dt = (float(g[0]), float(g[1])), float(step_dt)
        sd, _mu = _ens_tables(3, why, out_std, out_mu)
        u = _ens_u(u, B, 3, why)
        if int(steps) < 1 or int(B) < 1:
            raise ValueError("%s need steps, B >= 1, got %d, %d" % (noun, steps, B))
        if mean is not None:
            mean = torch.as_tensor(mean).detach()
            if tuple(mean.shape) != (int(B), 3, int(Hh), int(Ww)) or not bool(torch.isfinite(mean).all()):
                raise ValueError("mean is a finite array [%d, 3, %d, %d], got shape %s" % (B, Hh, Ww, tuple(mean.shape)))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, 3, Hh, Ww, steps)
        HW = self.H * self.W
        self.per_member = bool(per_member)
        self.a = _ens_scale(sd, u, self.B, torch.float64).to(torch.float32).to(dev).contiguous()
        self.m = None if mean is None else mean.to(torch.float32).reshape(self.B, 3, HW).to(dev).contiguous()
        P, Q, L = len(self.probes), len(self.pairs), len(self.lags)
        self.plan = H.ens_corr_plan(self.S, self.B, self.H, self.W, P, Q, L, len(set(cj for _ci, cj in self.pairs)))
        self.series = torch.empty((self.S + 1, self.B, self.Tk, P, 3), device=dev, dtype=torch.float32)
        self.raw = torch.empty((self.S + 1, self.B, self.plan["planes"], HW), device=dev, dtype=torch.float32)

    def add(self, y, m0, target, time=True):
        """Add the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, 3, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, 3, H, W] under the same stride rule, added as
        row S with the step's last chunk.  A step fed with time=False launches nothing."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        if time:
            cfg = (self.probes, self.pairs, self.lags)
            H.ens_corr_probe(yn, self.a, self.m, self.series, *cfg, k, m0, t_before)
            H.ens_corr_accum(yn, self.a, self.m, self.series, self.raw, *cfg, k, m0, t_before)
            if last:
                H.ens_corr_probe(tn, self.a, self.m, self.series, *cfg, 1, self.S, t_before)
                H.ens_corr_accum(tn, self.a, self.m, self.series, self.raw, *cfg, 1, self.S, t_before)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs over the steps folded with time=True."""
        T = self.finalize_guard()
        B, S, Hh, Ww = self.B, self.S, self.H, self.W
        HW, dev = Hh * Ww, self.raw.device
        P, Q, L = len(self.probes), len(self.pairs), len(self.lags)
        pm, pv = corr_probe_stats(self.series[:, :, :T], self.pairs, self.lags, T)
        outs = [torch.empty((B, P, Q, L, HW), device=dev, dtype=torch.float32) for _ in range(6)]
        lines = [torch.empty((B, S + 1, P, Q, L, n), device=dev, dtype=torch.float32) for n in (Ww, Hh)]
        mr = torch.empty((B, S, P, Q, L, HW), device=dev, dtype=torch.float32) if self.per_member else None
        H.ens_corr_finalize(self.raw, pm.to(dev), pv.to(dev), outs, mr, lines, self.probes, self.pairs, self.lags, Hh, Ww, T)
        o = {}
        for key, t in zip(("tp_cov_mean", "tp_cov_std", "tp_rho_mean", "tp_rho_std", "target_tp_cov", "target_tp_rho"), outs):
            o[key] = t.view(B, P, Q, L, Hh, Ww)
        if mr is not None:
            o["member_tp_rho"] = mr.view(B, S, P, Q, L, Hh, Ww)
        o["tp_line_x"], o["tp_line_y"] = lines
        # the derived scalars, fp64 on the host from the lines
        lx, ly = lines[0].cpu().double(), lines[1].cpu().double()
        dx, dy = self.grid
        ln = torch.empty((B, S + 1, P, Q, 4), dtype=torch.float64)
        sh = torch.empty((B, S + 1, P, Q, L, 2), dtype=torch.float64)
        for p, (h0, w0) in enumerate(self.probes):
            ln[:, :, p, :, 0:2] = corr_lengths(lx[:, :, p, :, 0], w0, dx)
            ln[:, :, p, :, 2:4] = corr_lengths(ly[:, :, p, :, 0], h0, dy)
            sh[:, :, p, :, :, 0] = corr_shift(lx[:, :, p], w0)
            sh[:, :, p, :, :, 1] = corr_shift(ly[:, :, p], h0)
        tau = torch.tensor([float(v) if v > 0 else float("nan") for v in self.lags], dtype=torch.float64) * self.step_dt
        sp = sh * torch.tensor([dx, dy], dtype=torch.float64) / tau.view(L, 1)
        o["tp_len"], o["tp_len_mean"], o["tp_len_std"], o["target_tp_len"] = ln, ln[:, :S].mean(1), ln[:, :S].std(1, unbiased=False), ln[:, S]
        o["tp_shift"] = sh
        o["tp_speed"], o["tp_speed_mean"], o["tp_speed_std"], o["target_tp_speed"] = sp, sp[:, :S].mean(1), sp[:, :S].std(1, unbiased=False), sp[:, S]
        o["tp_probes"], o["tp_pairs"], o["tp_lags"] = self.probes, self.pairs, self.lags
        return o


STRUCTURE_MAX_LAGS = 16
STRUCTURE_MAX_LAG = 64


def structure_lags(lags, H, W):
    """The checks of EnsembleStructure's lags argument for an H x W field -> the lags as a tuple of (dx, dy) int pairs.  A lag is
    l = (dx, dy) in pixels, dx along W and dy along H, in canonical form: dx >= 0, and dy > 0 when dx == 0; 0 <= dx <= 64, |dy| <= 64,
    dx < W, |dy| < H; distinct, 1 <= L <= 16 of them.  None: (1, 0), (2, 0), .. in powers of two up to min(32, W // 2), then the same
    along H.  A lag that breaks a rule raises ValueError naming it."""
    H, W = int(H), int(W)
    if lags is None:
        lags = [(1 << k, 0) for k in range(6) if (1 << k) <= min(32, W // 2)] + [(0, 1 << k) for k in range(6) if (1 << k) <= min(32, H // 2)]
        if not lags:
            raise ValueError("lags: a %d x %d field holds no default lag" % (H, W))
    try:
        ls = [tuple(l) for l in lags]
    except TypeError:
        raise ValueError("lags must be (dx, dy) pairs, got %r" % (lags,))
    if not 1 <= len(ls) <= STRUCTURE_MAX_LAGS:
        raise ValueError("lags must hold 1 to %d (dx, dy) pairs, got %d" % (STRUCTURE_MAX_LAGS, len(ls)))
    seen = set()
    for l in ls:
        if len(l) != 2 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in l):
            raise ValueError("lag %r is not a pair of integers (dx, dy)" % (l,))
        dx, dy = int(l[0]), int(l[1])
        if dx < 0 or (dx == 0 and dy <= 0):
            raise ValueError("lag %r is not in canonical form: dx >= 0, and dy > 0 when dx == 0" % (l,))
        if dx > STRUCTURE_MAX_LAG or abs(dy) > STRUCTURE_MAX_LAG:
            raise ValueError("lag %r is beyond %d pixels" % (l, STRUCTURE_MAX_LAG))
        if dx >= W or abs(dy) >= H:
            raise ValueError("lag %r has no pair in a %d x %d field" % (l, H, W))
        if (dx, dy) in seen:
            raise ValueError("lag %r is listed twice" % (l,))
        seen.add((dx, dy))
    return tuple((int(l[0]), int(l[1])) for l in ls)


class EnsembleStructure(EnsembleFeed):
    """On-device structure functions and variogram score of sampled roll-outs of B cases against the target (tmg_ens_score_store /
    tmg_ens_sfun_step): the dependence between neighbouring pixels of one member.  Permute the members independently at every pixel
    and every per-pixel score stays bit-identical; the increments do not.

    Setting.  Case b, kept step t, channel c.  Rows x_0..x_{S-1} are the raw normalised members.  Row x_S = y is the normalised target.
    a_c = u[b,c] * out_std[c] > 0.  out_mu cancels and is not an input.
    Lags.  A lag is l = (dx, dy) in pixels, dx along W and dy along H.  Lags are in canonical form: dx >= 0, and dy > 0 when dx == 0.
    0 <= dx <= 64, |dy| <= 64, dx < W, |dy| < H.  Lags are distinct, with 1 <= L <= 16 of them.  The pairs of a lag are all pixels
    p = (i, j) for which p' = (i + dy, j + dx) lies in the field.  N_l = (H - |dy|) (W - dx) >= 1.  D_m(p) = x_m(p') - x_m(p).
    Raw moment sums.  Per row m = 0..S and lag: M_q[m] = sum_p D_m(p)^q for q = 2, 3, 4, in fp32.
    Raw variogram sum.  Per lag, of order 1/2: s_m(p) = sqrtf(|D_m(p)|); sbar(p) = (s_0 + .. + s_{S-1}, added sequentially in member
    order in fp32) * fl(1/S); V_l = sum_p (s_S(p) - sbar(p))^2.
    Physical outputs.  Formed from the raw sums in fp64 and rounded once to float32:
      sf2, sf3, sf4 [B, Tk, C, L, S+1] = a_c^q M_q / N_l, with the target's row last.
      sf2_mean, sf2_std [B, Tk, C, L]: mean and population std over the members, target excluded.
      vario_lag[b,t,c,l] = w_l a_c V_l / N_l.  vario_score[b,t,c] = sum_l vario_lag.  The weights w_l are positive and finite, default 1.
    Time statistics.  Over the steps folded with time=True, the raw sums are added up on the device: tmom [3, B, C, L, S+1] and
    tvar [B, C, L], one fp32 addition per step, written rather than read at the first timed step.
      time_sf2, time_sf3, time_sf4 [B, C, L, S+1] = a^q tmom / (T N_l).  time_skew = time_sf3 / time_sf2^1.5.
      time_flat = time_sf4 / time_sf2^2.  Both are 0 where time_sf2 == 0.  time_vario_lag [B, C, L] and time_vario_score [B, C].
    Lag outputs.  lags is int64 [L, 2].  lag_dist is float64 [L] = hypot(dx * grid_dx, dy * grid_dy).
    Not supported.  Non-finite members, as in EnsembleQuantiles.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is scored.  The raw
    device buffers: xs [S, B, C, HW], ws (the workspace), mom [Tk, 3, B, C, L, S+1] and vsum [Tk, B, C, L] (step t writes its own
    plane), tmom [3, B, C, L, S+1], tvar [B, C, L]."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_std, u=None, lags=None, weights=None, grid=(1.0, 1.0)):
        noun, why = "ensemble structure functions", "the increments scale with u * out_std"
        _ens_channels(noun, C)
        _ens_members(noun, members)
        sd, _ = _ens_tables(C, why, out_std)
        u = _ens_u(u, B, C, why)
        self.lags = structure_lags(lags, Hh, Ww)
        L = len(self.lags)
        if weights is None:
            w = torch.ones(L, dtype=torch.float64)
        else:
            w = torch.as_tensor(weights, dtype=torch.float64).detach().reshape(-1).cpu()
            if w.numel() != L or not bool((torch.isfinite(w) & (w > 0)).all()):
                raise ValueError("weights must be %d positive finite numbers, one per lag, got %r" % (L, weights))
        try:
            gx, gy = float(grid[0]), float(grid[1])
        except (TypeError, IndexError, ValueError):
            raise ValueError("grid must be the cell sizes (dx, dy), got %r" % (grid,))
        if not (0 < gx < float("inf") and 0 < gy < float("inf")):
            raise ValueError("grid must be positive finite cell sizes (dx, dy), got %r" % (grid,))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.L = L
        HW = self.H * self.W
        f32 = dict(device=dev, dtype=torch.float32)
        self.a = _ens_scale(sd, u, self.B, torch.float64)                    # fp64, host
        self.w = w
        self.lag_dist = torch.tensor([math.hypot(dx * gx, dy * gy) for dx, dy in self.lags], dtype=torch.float64)
        self.plan = H.ens_sfun_plan(self.S, self.B, C, self.H, self.W, self.lags)
        R = self.S + 1
        self.xs = torch.empty((self.S, self.B, C, HW), **f32)
        self.ws = torch.empty((self.plan["ws"],), **f32)
        self.mom = torch.empty((self.Tk, 3, self.B, C, L, R), **f32)
        self.vsum = torch.empty((self.Tk, self.B, C, L), **f32)
        self.tmom = torch.empty((3, self.B, C, L, R), **f32)
        self.tvar = torch.empty((self.B, C, L), **f32)

    def add(self, y, m0, target, time=True):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk forms the step's sums against its target."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        H.ens_score_store(yn, self.xs, k, m0)
        if last:
            H.ens_sfun_step(self.xs, tn, self.lags, self.ws, self.mom[self._step], self.vsum[self._step], self.tmom, self.tvar,
                            self.H, self.W, t_before, 1 if time else 0)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time statistics cover the steps folded with time=True."""
        T = self.finalize_guard()
        dev = self.mom.device
        f32 = torch.float32
        a = self.a.to(dev)                                                   # [B, C] fp64
        n = torch.tensor(self.plan["N"], dtype=torch.float64, device=dev)    # [L]
        w = self.w.to(dev)
        S = self.S
        o = {}
        mom = self.mom.double()                                              # [Tk, 3, B, C, L, R]
        sf = []
        for q in (2, 3, 4):
            v = (a ** q).view(1, self.B, self.C, 1, 1) * mom[:, q - 2] / n.view(1, 1, 1, -1, 1)
            sf.append(v.permute(1, 0, 2, 3, 4).contiguous())                 # [B, Tk, C, L, R]
            o["sf%d" % q] = sf[-1].to(f32)
        mem = sf[0][..., :S]
        mean = mem.mean(-1)
        o["sf2_mean"] = mean.to(f32)
        o["sf2_std"] = ((mem - mean.unsqueeze(-1)) ** 2).mean(-1).sqrt().to(f32)
        vl = (w.view(1, 1, 1, -1) * a.view(1, self.B, self.C, 1) * self.vsum.double() / n.view(1, 1, 1, -1)).permute(1, 0, 2, 3).contiguous()
        o["vario_lag"] = vl.to(f32)
        o["vario_score"] = vl.sum(-1).to(f32)
        tm = self.tmom.double()                                              # [3, B, C, L, R]
        ts = [(a ** q).view(self.B, self.C, 1, 1) * tm[q - 2] / (T * n.view(1, 1, -1, 1)) for q in (2, 3, 4)]
        for q in (2, 3, 4):
            o["time_sf%d" % q] = ts[q - 2].to(f32)
        nz = ts[0] != 0
        den = torch.where(nz, ts[0], torch.ones_like(ts[0]))
        o["time_skew"] = torch.where(nz, ts[1] / den ** 1.5, torch.zeros_like(den)).to(f32)
        o["time_flat"] = torch.where(nz, ts[2] / den ** 2, torch.zeros_like(den)).to(f32)
        tv = w.view(1, 1, -1) * a.view(self.B, self.C, 1) * self.tvar.double() / (T * n.view(1, 1, -1))
        o["time_vario_lag"] = tv.to(f32)
        o["time_vario_score"] = tv.sum(-1).to(f32)
        o["lags"] = torch.tensor(self.lags, dtype=torch.int64).reshape(-1, 2)
        o["lag_dist"] = self.lag_dist
        return o


def spectrum_bins(H_, W_, dx, dy):
    """The shell map of an H x W field on a grid of cell size dx along W, dy along H (fp64, host): signed mode numbers p' (p - H
    above H // 2), q' likewise, r = sqrt((p' Lmax / Ly)^2 + (q' Lmax / Lx)^2) with Lx = W dx, Ly = H dy, Lmax = max(Lx, Ly), shell
    s = floor(r + 0.5).  Returns (bins int32 [H, W], k float64 [NK]): NK = 1 + max s, k[s] = s 2 pi / Lmax.  Every mode is kept: the
    shells sum to 0.5 mean(|z|^2); shell 0 is the mean mode alone."""
    Hn, Wn = int(H_), int(W_)
    Lx, Ly = Wn * float(dx), Hn * float(dy)
    Lmax = max(Lx, Ly)
    p = torch.arange(Hn, dtype=torch.float64)
    q = torch.arange(Wn, dtype=torch.float64)
    p = torch.where(p <= Hn // 2, p, p - Hn) * (Lmax / Ly)
    q = torch.where(q <= Wn // 2, q, q - Wn) * (Lmax / Lx)
    r = torch.sqrt(p[:, None] ** 2 + q[None, :] ** 2)
    bins = torch.floor(r + 0.5).to(torch.int32)
    k = torch.arange(int(bins.max()) + 1, dtype=torch.float64) * (2.0 * math.pi / Lmax)
    return bins, k


def _spectrum_operand(N, window):
    """[2, N, N] fp32 (re, im): T[n][m] = w[n] exp(-2 pi i ((n m) mod N) / N), the argument reduced with integers, built in fp64 and
    rounded once.  w: the periodic Hann window over sqrt(mean(w^2)), or 1."""
    n = torch.arange(N, dtype=torch.int64)
    ang = ((n[:, None] * n[None, :]) % N).to(torch.float64) * (-2.0 * math.pi / N)
    w = torch.ones(N, dtype=torch.float64)
    if window == "hann":
        w = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n.to(torch.float64) / N)
        w = w / torch.sqrt(torch.mean(w * w))
    return torch.stack((w[:, None] * torch.cos(ang), w[:, None] * torch.sin(ang))).to(torch.float32).contiguous()


def _spectrum_lists(bins, NK):
    """Per 16-column tile of the bin map the tile's modes p * 16 + (q & 15) sorted by shell (stable) and the first list position of
    every shell: (perm int32 [W/16, 16 H], offs int32 [W/16, NK + 1]).  The column pass sums a shell in this order."""
    Hn, Wn = bins.shape
    tiles = bins.view(Hn, Wn // 16, 16).permute(1, 0, 2).reshape(Wn // 16, Hn * 16).to(torch.int64)
    perm = torch.argsort(tiles, dim=1, stable=True).to(torch.int32)
    offs = torch.zeros((Wn // 16, NK + 1), dtype=torch.int64)
    for t in range(Wn // 16):
        offs[t, 1:] = torch.cumsum(torch.bincount(tiles[t], minlength=NK), 0)
    return perm.contiguous(), offs.to(torch.int32).contiguous()


SPECTRUM_MAX_SHELLS = 8192


class EnsembleSpectrum(EnsembleFeed):
    """On-device shell-binned kinetic-energy spectra E(k) of sampled roll-outs of B cases (tmg_spec_rows / tmg_spec_cols /
    tmg_spec_accum / tmg_spec_finalize).  Per case, member and kept step: z = g (u + i v) from channels 0 and 1 of the un-normalised
    field yh = u[b, c] (out_std[c] y + out_mu[c]) (the pressure is ignored), g[y, x] = w_H[y] w_W[x] the periodic Hann window
    w_N[n] = 0.5 - 0.5 cos(2 pi n / N) over sqrt(mean(w_N^2)) (window=None: g = 1), Z = fft2(z), E2 = 0.5 |Z|^2 / (H W)^2, and
    E[s] the sum of E2 over shell s of spectrum_bins(H, W, dx, dy).  The transform is a dense DFT on the fp32 matrix pipe with the
    window folded into its operand matrices; H and W are multiples of 16 up to 512.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order, each step's chunks before
    the next step's.  y: API-shaped [k*B, C, H, W], 2 <= C <= 4.  Outputs (device tensors): spec_mean, spec_std [B, Tk, NK] (mean and
    population std over the members); finalize() adds time_spec_mean, time_spec_std [B, NK] (mean / std over the members of each
    member's time mean of E over the steps folded with time=True) and spec_k [NK] (float64, host: the shell centres s 2 pi / Lmax)."""

    def __init__(self, members, B, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), window="hann"):
        try:
            grid = tuple(float(g) for g in grid)
        except TypeError:
            raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %r" % (grid,)) from None
        if len(grid) != 2 or not all(math.isfinite(g) and g > 0 for g in grid):
            raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %s" % (grid,))
        if window not in ("hann", None):
            raise ValueError("window must be 'hann' or None, got %r" % (window,))
        Hh, Ww = int(Hh), int(Ww)
        if not all(16 <= n <= 512 and n % 16 == 0 for n in (Hh, Ww)):
            raise ValueError("spectra need H and W that are a multiple of 16 in [16, 512], got %d x %d" % (Hh, Ww))
        dev = _ens_device("ensemble spectra", device)
        bins, k = spectrum_bins(Hh, Ww, grid[0], grid[1])
        NK = k.numel()
        if NK > SPECTRUM_MAX_SHELLS:
            raise ValueError("grid %s gives %d shells on %d x %d modes, at most %d are supported" % (grid, NK, Hh, Ww, SPECTRUM_MAX_SHELLS))
        self.grid, self.window = grid, window
        EnsembleFeed.__init__(self, members, B, None, Hh, Ww, steps)
        self.NK = NK
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu = torch.as_tensor(out_mu, **f32).reshape(-1)[:2].contiguous()
        self.sd = torch.as_tensor(out_std, **f32).reshape(-1)[:2].contiguous()
        if self.mu.numel() != 2 or self.sd.numel() != 2:
            raise ValueError("out_mu / out_std need at least 2 entries, got %d / %d" % (self.mu.numel(), self.sd.numel()))
        self.u = None if u is None else torch.as_tensor(u, **f32).reshape(self.B, -1)[:, :2].contiguous()
        if self.u is not None and self.u.shape[1] != 2:
            raise ValueError("u needs at least 2 entries per case")
        self.k = k
        self.bins = bins                  # host: the device reads the shell lists derived from it
        perm, offs = _spectrum_lists(bins, NK)
        self.perm, self.offs = perm.to(dev), offs.to(dev)
        self.ft_w = _spectrum_operand(Ww, window).to(dev)
        self.ft_h = self.ft_w if Hh == Ww else _spectrum_operand(Hh, window).to(dev)
        self.step_state = torch.empty((2, self.B, NK), **f32)
        self.time_state = torch.empty((self.S, self.B, NK), **f32)
        self.out = {"spec_mean": torch.empty((self.B, self.Tk, NK), **f32), "spec_std": torch.empty((self.B, self.Tk, NK), **f32)}
        self._yw = self._part = None      # workspace of the largest chunk: the planar row transform, the tiles' partial spectra

    def add(self, y, m0, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major)."""
        yn, _, k, t_before, last = self.open_chunk(y, m0, time)
        _on_device(yn)
        kB = k * self.B
        QT = self.W // 16
        if self._yw is None or self._yw.numel() < 2 * kB * self.H * self.W:
            self._yw = torch.empty(2 * kB * self.H * self.W, device=self.step_state.device, dtype=torch.float32)
            self._part = torch.empty(kB * QT * self.NK, device=self.step_state.device, dtype=torch.float32)
        t = self._step
        flags = (1 if time else 0) | (2 if last else 0)
        H.spec_rows(yn, self.u, self.mu, self.sd, self.ft_w, self._yw, k)
        H.spec_cols(self.ft_h, self._yw, self.perm, self.offs, self._part, kB, self.H, self.W, self.NK)
        o = self.out
        H.spec_accum(self._part, self.step_state[0], self.step_state[1], self.time_state,
                     (o["spec_mean"][:, t], o["spec_std"][:, t]) if last else None, self.Tk * self.NK, k, self.B, self.NK, QT, self._n,
                     m0, t_before, flags)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time statistics cover the steps folded with time=True."""
        self.finalize_guard()
        for n in ("time_spec_mean", "time_spec_std"):
            self.out[n] = empty((self.B, self.NK), self.step_state.device)
        H.spec_finalize(self.time_state, self.out["time_spec_mean"], self.out["time_spec_std"], self.S, self.B, self.NK)
        self.out["spec_k"] = self.k
        return self.out


def xspec_args(C, Hh, Ww, grid, window, level):
    """The argument checks of the spectral skill (EnsembleSpectralSkill, utils.modelPredSpectralSkill), every failure a ValueError
    before any device work, in this order: C, H and W, grid, window, level, the number of shells -> (grid as floats, bins, k) with
    (bins, k) = spectrum_bins(H, W, dx, dy)."""
    if isinstance(C, bool) or not isinstance(C, numbers.Integral):
        raise ValueError("spectral skill needs an integer number of channels, got %r" % (C,))
    _ens_channels("spectral skill", C, " (the velocity is channels 0 and 1)")
    if any(isinstance(n, bool) or not isinstance(n, numbers.Integral) for n in (Hh, Ww)) \
            or not all(16 <= n <= 512 and n % 16 == 0 for n in (Hh, Ww)):
        raise ValueError("spectral skill needs H and W that are a multiple of 16 in [16, 512], got %r x %r" % (Hh, Ww))
    try:
        grid = tuple(float(g) for g in grid)
    except (TypeError, ValueError):
        raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %r" % (grid,)) from None
    if len(grid) != 2 or not all(math.isfinite(g) and g > 0 for g in grid):
        raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %s" % (grid,))
    if window not in ("hann", None):
        raise ValueError("window must be 'hann' or None, got %r" % (window,))
    if isinstance(level, bool) or not isinstance(level, numbers.Real) or not 0.0 < float(level) < 1.0:
        raise ValueError("level is the coherence that defines the cut-off wavenumber, a number in (0, 1), got %r" % (level,))
    bins, k = spectrum_bins(int(Hh), int(Ww), grid[0], grid[1])
    if k.numel() > SPECTRUM_MAX_SHELLS:
        raise ValueError("grid %s gives %d shells on %d x %d modes, at most %d are supported" % (grid, k.numel(), Hh, Ww, SPECTRUM_MAX_SHELLS))
    return grid, bins, k


XSPEC_RAW_KEYS = ("xs_target_power", "xs_sum", "xs_mean_field", "xs_time_member", "xs_time_target", "xs_time_mean_field")


def _xs_ratio(a, b):
    """a / b in fp64, NaN where b == 0 (an empty shell, or no power at all)."""
    ok = b != 0
    return torch.where(ok, a / torch.where(ok, b, torch.ones_like(b)), torch.full_like(b, float("nan")))


def _xs_forms(P, X, D, Pb, Xb, Db, PT, S, pre):
    """The derived spectra of one set of sums (fp64; P, X, D: the members' means): the issue's formulas, keys with prefix pre."""
    spread = D - Db
    arg = _xs_ratio((S + 1.0) / S * spread, Db)
    return {pre + "spec_corr": _xs_ratio(X, torch.sqrt(P * PT)), pre + "mean_field_corr": _xs_ratio(Xb, torch.sqrt(Pb * PT)),
            pre + "err_spec": D, pre + "mean_err_spec": Db, pre + "spread_spec": spread,
            pre + "spread_skill": torch.sqrt(torch.where(arg >= 0, arg, torch.full_like(arg, float("nan")))),
            pre + "power_ratio": _xs_ratio(P, PT), pre + "rel_err": _xs_ratio(D, PT)}


def _xs_cutoff(corr, k, level):
    """corr [..., NK] fp64 -> the cut-off wavenumber [...]: over the shells s >= 1 whose corr is finite, the first with corr < level;
    linearly interpolated in corr between the finite shell before it and itself, k of that shell when it is the first finite one,
    inf when no shell is under level."""
    flat = corr.reshape(-1, corr.shape[-1])
    out = torch.full((flat.shape[0],), float("inf"), dtype=torch.float64)
    kk = k.tolist()
    for r, row in enumerate(flat.tolist()):
        prev = None
        for s in range(1, len(row)):
            c = row[s]
            if not math.isfinite(c):
                continue
            if c < level:
                out[r] = kk[s] if prev is None else kk[prev] + (row[prev] - level) / (row[prev] - c) * (kk[s] - kk[prev])
                break
            prev = s
    return out.reshape(corr.shape[:-1])


def xspec_outputs(xs_target_power, xs_sum, xs_mean_field, xs_time_member, xs_time_target, xs_time_mean_field, S, k, level, timed):
    """The derived outputs of the spectral skill from its raw shell sums (XSPEC_RAW_KEYS; shapes as EnsembleSpectralSkill returns
    them): host fp64 work on CPU copies, no device.  S: the members; k [NK]: the shell centres; level: the coherence of the cut-off;
    timed: the number of timed steps, which turns the time sums into time means.  With Pm = xs_sum[:, :, 0] / S and likewise Xm, Dm,
    (P_bar, X_bar, D_bar) = xs_mean_field and P_T = xs_target_power -> dict of float64 CPU tensors:
      spec_corr = Xm / sqrt(Pm P_T), mean_field_corr = X_bar / sqrt(P_bar P_T), err_spec = Dm, mean_err_spec = D_bar,
      spread_spec = Dm - D_bar (the identity mean|Z_m - T|^2 = mean|Z_m - Zbar|^2 + |Zbar - T|^2 shifted by the target, which stays
      well-conditioned when the members track it; small negative values from rounding are returned as they are),
      spread_skill = sqrt((S + 1) / S spread_spec / D_bar) (near 1 for a calibrated ensemble: its square has the expectation
      (S - 1) / S there, spread_spec being the population variance; NaN where its argument is negative),
      power_ratio = Pm / P_T, rel_err = Dm / P_T (2 for a decorrelated member of the right energy)            all [N, Tk, NK]
      time_* of all of these [N, NK], from the time sums over `timed`
      time_member_corr [N, S, NK] and its mean and population std over the members time_corr_mean, time_corr_std [N, NK]
      cutoff_k [N, S + 1] (the mean field last): over the shells s >= 1 with a finite time correlation the first with corr < level,
      linearly interpolated in corr between the finite shell before it and itself, k[s] when it is the first, inf when there is
      none; cutoff_len = 2 pi / cutoff_k; cutoff_k_mean, cutoff_k_std [N] over the members, ignoring inf (NaN when all are inf)
      xs_k [NK].
    A ratio with a zero denominator is NaN (the empty shells of a stretched grid)."""
    f64 = lambda v: torch.as_tensor(v).detach().cpu().to(torch.float64)          # noqa: E731
    PT, sm, bar, tm, tT, tb = (f64(v) for v in (xs_target_power, xs_sum, xs_mean_field, xs_time_member, xs_time_target, xs_time_mean_field))
    k = f64(k).reshape(-1)
    S, Tn, NK = int(S), int(timed), k.numel()
    if S < 1 or Tn < 1:
        raise ValueError("xspec_outputs needs S >= 1 members and timed >= 1 steps, got %d and %d" % (S, Tn))
    if isinstance(level, bool) or not isinstance(level, numbers.Real) or not 0.0 < float(level) < 1.0:
        raise ValueError("level is a coherence in (0, 1), got %r" % (level,))
    if PT.dim() != 3 or PT.shape[2] != NK:
        raise ValueError("xs_target_power is [N, Tk, %d], got %s" % (NK, tuple(PT.shape)))
    N, Tk = PT.shape[:2]
    for name, v, shp in (("xs_sum", sm, (N, Tk, 3, NK)), ("xs_mean_field", bar, (N, Tk, 3, NK)), ("xs_time_member", tm, (N, S, 3, NK)),
                         ("xs_time_target", tT, (N, NK)), ("xs_time_mean_field", tb, (N, 3, NK))):
        if tuple(v.shape) != shp:
            raise ValueError("%s is %s, got %s" % (name, list(shp), tuple(v.shape)))
    o = _xs_forms(sm[:, :, 0] / S, sm[:, :, 1] / S, sm[:, :, 2] / S, bar[:, :, 0], bar[:, :, 1], bar[:, :, 2], PT, S, "")
    ms = tm.sum(1)                                                               # [N, 3, NK]: the members in member order
    o.update(_xs_forms(ms[:, 0] / S / Tn, ms[:, 1] / S / Tn, ms[:, 2] / S / Tn, tb[:, 0] / Tn, tb[:, 1] / Tn, tb[:, 2] / Tn, tT / Tn, S,
                       "time_"))
    mc = _xs_ratio(tm[:, :, 1], torch.sqrt(tm[:, :, 0] * tT.unsqueeze(1)))       # (the 1 / Tn of numerator and denominator cancel)
    o["time_member_corr"] = mc
    o["time_corr_mean"] = mc.mean(1)
    o["time_corr_std"] = mc.std(1, unbiased=False)
    bc = _xs_ratio(tb[:, 1], torch.sqrt(tb[:, 0] * tT))
    cut = _xs_cutoff(torch.cat((mc, bc.unsqueeze(1)), 1), k, float(level))
    o["cutoff_k"] = cut
    o["cutoff_len"] = 2.0 * math.pi / cut
    mem = cut[:, :S]
    fin = torch.isfinite(mem)
    cnt = fin.sum(1).to(torch.float64)
    mean = _xs_ratio(torch.where(fin, mem, torch.zeros_like(mem)).sum(1), cnt)
    o["cutoff_k_mean"] = mean
    o["cutoff_k_std"] = torch.sqrt(_xs_ratio(torch.where(fin, (mem - mean.unsqueeze(1)) ** 2, torch.zeros_like(mem)).sum(1), cnt))
    o["xs_k"] = k
    return o


class EnsembleSpectralSkill(EnsembleFeed):
    """On-device spectral skill of sampled roll-outs of B cases against the target (tmg_ens_xspec_prep / tmg_spec_rows /
    tmg_ens_xspec_cols / tmg_ens_xspec_accum): down to which scale does a member reproduce the target field itself, and from which
    scale on is it only statistically plausible.  Rows are the members m, the target T and the ensemble-mean field bar; per case and
    kept step
      f_c = u[b, c] (out_std[c] y_c + out_mu[c]) - M_c, c = 0, 1     M: the centre plane [B, 2, H, W] in physical units (fp32, one
                                                                     separate rounding); center=None: nothing is subtracted.  The
                                                                     mean flow is trivially coherent; the question is about the
                                                                     fluctuations
      z = g (f_0 + i f_1), Z = fft2(z)                               g: the separable periodic Hann window over its RMS, or 1 for
                                                                     window=None; the dense DFT of EnsembleSpectrum on the fp32
                                                                     matrix pipe, H and W multiples of 16 up to 512
      P = sc |Z|^2, X = sc Re(conj(Z) Z_T), D = sc |Z - Z_T|^2       sc = 0.5 / (H W)^2, D from the differences (P + P_T - 2 X
                                                                     cancels exactly where the members are good)
    summed over the shells of spectrum_bins(H, W, dx, dy); the shells are symmetric under k -> -k, so the shell sum of X is the
    vector co-spectrum Re sum(conj(U_m) U_T + conj(V_m) V_T).  fbar = (sum_m f_m) / S, the members added in member order, goes
    through the same transform as one more image per case.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's normalised target [B, C, H, W], which is transformed at m0 = 0.
    Raw outputs (device tensors, fp32; every sum in a fixed order, so they are bitwise equal for every chunking):
      xs_target_power [B, Tk, NK]      P_T
      xs_sum [B, Tk, 3, NK]            sum_m (P, X, D) in member order
      xs_mean_field [B, Tk, 3, NK]     (P_bar, X_bar, D_bar)
      xs_time_member [B, S, 3, NK], xs_time_target [B, NK], xs_time_mean_field [B, 3, NK]
                                       the sums over the steps folded with time=True, in step order (finalize())
    finalize() adds what xspec_outputs derives from them on the host in fp64 (float64 CPU tensors): spec_corr, mean_field_corr,
    err_spec, mean_err_spec, spread_spec, spread_skill, power_ratio, rel_err and their time_ forms, time_member_corr, time_corr_mean,
    time_corr_std, cutoff_k, cutoff_len, cutoff_k_mean, cutoff_k_std, xs_k.

    Not supported: a pressure or scalar coherence; quadrature and phase spectra (the imaginary part does not reduce to a phase under
    the shells' symmetry); per-member per-step outputs; coherence with the low-fidelity input, which lives on a different grid; pixel
    boxes; fields that are not multiples of 16; more than 1024 members; non-finite members (the outputs of an affected step are
    unspecified; there is no data-dependent addressing, so nothing can fault)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), window="hann", center=None,
                 level=0.5):
        noun = "spectral skill"
        grid, bins, k = xspec_args(C, Hh, Ww, grid, window, level)
        _ens_members(noun, members)
        if int(B) < 1 or int(steps) < 1:
            raise ValueError("%s needs B >= 1 cases and steps >= 1, got %d and %d" % (noun, int(B), int(steps)))
        sd, mu = _ens_tables(2, "the fields are un-normalised with it", out_std, out_mu)
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float32).detach().cpu()
            if u.numel() % int(B) or u.numel() // int(B) < 2:
                raise ValueError("u needs at least 2 entries per case")
            u = _ens_u(u.reshape(int(B), -1)[:, :2].contiguous(), int(B), 2, "the fields are scaled with it")
        if isinstance(center, str):
            raise ValueError("center is a plane [B, >= 2, H, W] or None (the target's time mean is utils.modelPredSpectralSkill's), got %r" % (center,))
        if center is not None:
            center = torch.as_tensor(center).detach()
            if center.dim() != 4 or center.shape[0] != int(B) or center.shape[1] < 2 or tuple(center.shape[2:]) != (int(Hh), int(Ww)):
                raise ValueError("center is a plane [B, >= 2, H, W] in physical units, got %s" % (tuple(center.shape),))
            center = center[:, :2].to(torch.float32)
            if not bool(torch.isfinite(center).all()):
                raise ValueError("center must be finite")
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.grid, self.window, self.level = grid, window, float(level)
        self.k, self.bins, self.NK = k, bins, k.numel()
        NK = self.NK
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).contiguous()
        self.cen = None if center is None else center.to(dev).contiguous()
        # the row pass runs on the field the prep kernel has formed: unit tables, no scale
        self.one, self.zero = torch.ones(2, **f32), torch.zeros(2, **f32)
        perm, offs = _spectrum_lists(bins, NK)
        self.perm, self.offs = perm.to(dev), offs.to(dev)
        self.ft_w = _spectrum_operand(self.W, window).to(dev)
        self.ft_h = self.ft_w if self.H == self.W else _spectrum_operand(self.H, window).to(dev)
        self.plan = H.ens_xspec_plan(1, self.B, self.H, self.W, NK)
        QT = self.W // 16
        self.fsum = torch.empty((self.B, self.H, self.W, 2), **f32)
        self.zt = torch.empty((2, self.B, self.H, self.W), **f32)
        self.part_t = torch.empty((self.B, QT, NK), **f32)
        self.part_b = torch.empty((self.B, QT, 3, NK), **f32)
        self.step_state = torch.empty((self.B, 3, NK), **f32)
        self.out = {"xs_target_power": torch.empty((self.B, self.Tk, NK), **f32), "xs_sum": torch.empty((self.B, self.Tk, 3, NK), **f32),
                    "xs_mean_field": torch.empty((self.B, self.Tk, 3, NK), **f32),
                    "xs_time_member": torch.empty((self.B, self.S, 3, NK), **f32), "xs_time_target": torch.empty((self.B, NK), **f32),
                    "xs_time_mean_field": torch.empty((self.B, 3, NK), **f32)}
        self._f = self._yw = self._part = None       # workspace of the largest chunk: the field, its row transform, the tiles' sums

    def _transform(self, n, cross, part):
        """Rows and columns of the n images at the front of the field buffer."""
        f = self._f[:n]
        H.spec_rows(f, None, self.zero, self.one, self.ft_w, self._yw, n // self.B)
        H.ens_xspec_cols(self.ft_h, self._yw, self.perm, self.offs, self.zt, part, n, self.B, self.H, self.W, self.NK, cross)

    def add(self, y, m0, target, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule, transformed
        at m0 = 0.  The step's last chunk also transforms the ensemble-mean field and writes the step's outputs."""
        yn, tn, k, t_before, last = self.open_chunk(y, m0, time, target, required=True)
        _on_device(yn, tn)
        kB = k * self.B
        QT = self.W // 16
        dev = self.fsum.device
        if self._f is None or self._f.shape[0] < kB:
            self._f = torch.empty((kB, self.H, self.W, 2), device=dev, dtype=torch.float32)
            self._yw = torch.empty(2 * kB * self.H * self.W, device=dev, dtype=torch.float32)
            self._part = torch.empty(kB * QT * 3 * self.NK, device=dev, dtype=torch.float32)
        if m0 == 0:
            H.ens_xspec_prep(tn, self.u, self.mu, self.sd, self.cen, self._f, self.fsum, 1, 0, self.S)
            self._transform(self.B, False, self.part_t)
        H.ens_xspec_prep(yn, self.u, self.mu, self.sd, self.cen, self._f, self.fsum, k, 1 if m0 == 0 else 2, self.S)
        self._transform(kB, True, self._part)
        if last:
            H.ens_xspec_prep(None, None, None, None, None, self._f, self.fsum, 1, 3, self.S)
            self._transform(self.B, True, self.part_b)
        o = self.out
        H.ens_xspec_accum(self._part, self.part_t, self.part_b, self.step_state, o["xs_target_power"], o["xs_sum"], o["xs_mean_field"],
                          o["xs_time_member"], o["xs_time_target"], o["xs_time_mean_field"], k, QT, self._step, self._n, m0, t_before,
                          (1 if time else 0) | (2 if last else 0))
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the raw sums (device) and of xspec_outputs' derived outputs (float64, CPU); the time forms cover the steps
        folded with time=True."""
        T = self.finalize_guard()
        o = dict(self.out)
        o.update(xspec_outputs(*[self.out[n] for n in XSPEC_RAW_KEYS], self.S, self.k, self.level, T))
        return o


LSPEC_AXES = ("x", "y")


def lspec_fields(C):
    """The names of the F = C + 2 planes of a line spectrum, in plane order: the C autospectra, then uv_co, uv_quad."""
    return tuple(("uu", "vv", "pp", "ss")[c] for c in range(C)) + ("uv_co", "uv_quad")


def lspec_args(C, Hh, Ww, grid, axis, window, members):
    """The argument checks of the line spectra (EnsembleLineSpectra, utils.modelPredLineSpectra), every failure a ValueError before
    any device work, in this order: channels, N, L, grid, axis, window, members.  N (the points of a line) and L (the lines) are read
    as for axis "x" (N = W, L = H) unless axis is "y" (N = H, L = W); an axis that is neither is reported at its turn.
    -> (grid as floats, N, L, d): d the cell size along the line (dx for "x", dy for "y")."""
    noun = "line spectra"
    if isinstance(C, bool) or not isinstance(C, numbers.Integral):
        raise ValueError("%s need an integer number of channels, got %r" % (noun, C))
    _ens_channels(noun, C, " (the co-spectrum is that of channels 0 and 1)")
    N, L = (Hh, Ww) if isinstance(axis, str) and axis == "y" else (Ww, Hh)
    if isinstance(N, bool) or not isinstance(N, numbers.Integral) or not (16 <= N <= 512 and N % 16 == 0):
        raise ValueError("%s need a line of N points, N a multiple of 16 in [16, 512], got %r" % (noun, N))
    if isinstance(L, bool) or not isinstance(L, numbers.Integral) or L < 1:
        raise ValueError("%s need L >= 1 lines, got %r" % (noun, L))
    try:
        grid = tuple(float(g) for g in grid)
    except (TypeError, ValueError):
        raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %r" % (grid,)) from None
    if len(grid) != 2 or not all(math.isfinite(g) and g > 0 for g in grid):
        raise ValueError("grid needs two positive finite cell sizes (dx, dy), got %s" % (grid,))
    if not isinstance(axis, str) or axis not in LSPEC_AXES:
        raise ValueError("axis must be 'x' (along W) or 'y' (along H), got %r" % (axis,))
    if window not in ("hann", None):
        raise ValueError("window must be 'hann' or None, got %r" % (window,))
    if isinstance(members, bool) or not isinstance(members, numbers.Integral):
        raise ValueError("%s need an integer number of members, got %r" % (noun, members))
    _ens_members(noun, members)
    return grid, int(N), int(L), grid[0] if axis == "x" else grid[1]


def _lspec_operand(N, window):
    """[2, N, NQP] fp32 (re, im) of the one-sided transform of a line of N points: op[n][q] = (w[n] / N) exp(-2 pi i ((q n) mod N) / N)
    for q = 0 .. N/2, the argument reduced with integers, built in fp64 and rounded once (_spectrum_operand's rule); the columns from
    NQ = N/2 + 1 up to NQP = 16 ceil(NQ / 16) are exactly zero.  w: the periodic Hann window over sqrt(mean(w^2)), or 1."""
    NQ = N // 2 + 1
    NQP = (NQ + 15) // 16 * 16
    n = torch.arange(N, dtype=torch.int64)
    q = torch.arange(NQ, dtype=torch.int64)
    ang = ((n[:, None] * q[None, :]) % N).to(torch.float64) * (-2.0 * math.pi / N)
    w = torch.ones(N, dtype=torch.float64)
    if window == "hann":
        w = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n.to(torch.float64) / N)
        w = w / torch.sqrt(torch.mean(w * w))
    w = (w / N)[:, None]
    op = torch.zeros((2, N, NQP), dtype=torch.float32)
    op[0, :, :NQ] = (w * torch.cos(ang)).to(torch.float32)
    op[1, :, :NQ] = (w * torch.sin(ang)).to(torch.float32)
    return op.contiguous()


def lspec_outputs(fluct, k, C):
    """The host-formed outputs of the line spectra from the ensemble-mean fluctuation planes fluct [B, F, L, NQ] (F = C + 2) and the
    wavenumbers k [NQ]: fp64 work on CPU copies, no device -> dict of float64 CPU tensors
      time_lspec_energy [B, F, L]        the sum over q (for an autospectrum: the line's windowed variance, by Parseval)
      time_lspec_centroid [B, C, L]      sum_{q >= 1} k Phi_cc / sum_{q >= 1} Phi_cc, NaN at 0 / 0
      time_lspec_coherence [B, L, NQ]    (co^2 + quad^2) / (Phi_00 Phi_11), NaN at 0 / 0."""
    P = torch.as_tensor(fluct).detach().cpu().to(torch.float64)
    k = torch.as_tensor(k).detach().cpu().to(torch.float64).reshape(-1)
    C = int(C)
    if P.dim() != 4 or P.shape[1] != C + 2 or P.shape[3] != k.numel():
        raise ValueError("fluct is [B, %d, L, %d], got %s" % (C + 2, k.numel(), tuple(P.shape)))
    A = P[:, :C, :, 1:]
    return {"time_lspec_energy": P.sum(-1), "time_lspec_centroid": _xs_ratio((A * k[1:]).sum(-1), A.sum(-1)),
            "time_lspec_coherence": _xs_ratio(P[:, C] ** 2 + P[:, C + 1] ** 2, P[:, 0] * P[:, 1])}


class EnsembleLineSpectra(EnsembleFeed):
    """On-device one-dimensional line spectra of sampled roll-outs of B cases (tmg_ens_lspec_chunk / tmg_ens_lspec_step /
    tmg_ens_lspec_finalize): the streamwise (or wall-normal) spectrum of u'u', v'v', p'p' and the u'v' co-spectrum at every line, the
    map k Phi(k, y) that says at which scales a member carries its Reynolds stress.  axis="x" transforms along W: the lines are the
    L = H rows, N = W, d = dx; axis="y" along H: the L = W columns, N = H, d = dy.  N is a multiple of 16 in 16..512, L >= 1 is free.
    Per case, member, kept step, channel c and line l, with yh = u[b, c] (out_std[c] y + out_mu[c]):
      X_c[l, q] = (1 / N) sum_n w[n] yh_c[l, n] exp(-2 pi i q n / N), q = 0 .. N/2 (NQ = N/2 + 1), w the periodic Hann window over its
      RMS (window=None: 1); a dense DFT on the fp32 matrix pipe with w / N folded into its operand
      planes (F = C + 2: lspec_fields): a_q |X_c|^2, then uv_co = a_q Re(X_0 conj X_1), uv_quad = a_q Im(X_0 conj X_1); a_q = 1 at
      q = 0 and q = N/2, else 2
      total spectrum of a step: the planes of X; mean-flow spectrum of a member: the planes of Xbar = mean_t X over the steps folded
      with time=True; fluctuation spectrum: Phi = a_q (1 / T) sum_t (X_t - Xbar) conj(Y_t - Ybar), a population moment as time_rms
      is, accumulated as a running mean and co-moment (Welford) in ONE pass, never as mean|X|^2 - |Xbar|^2.
    Parseval: sum_q Phi_cc[l, q] = mean_n w[n]^2 var_t(yh_c[l, n]).

    Feeding protocol of EnsembleFeed; add(y, m0, time=True) takes no target.  Device memory: the members' state takes
    4 (3 C + 2) S B L NQ bytes (44 S B L NQ at C = 3: 2 C floats of running mean and C + 2 of co-moments per member, line and mode),
    the partials of the largest chunk 4 k B ceil(L / 16) F NQ.  Every sum has a fixed order and the step's Welford over the members is
    sequential across chunks: all outputs are bitwise equal for every chunking.
    Outputs (device tensors, fp32): lspec_mean, lspec_std [B, Tk, F, NQ] (the line-averaged total spectra: mean and population std over
    the members); finalize() adds time_lspec_fluct_mean / _std and time_lspec_flow_mean / _std [B, F, L, NQ] (over the members), with
    per_member time_lspec_fluct_member [B, S, F, L, NQ], and from lspec_outputs on the host in fp64 time_lspec_energy [B, F, L],
    time_lspec_centroid [B, C, L], time_lspec_coherence [B, L, NQ]; lspec_k [NQ] (float64: 2 pi q / (N d)) and lspec_fields.

    Not supported: two-dimensional fluctuation spectra, wavenumber-frequency spectra, Welch segments, sizes off the 16 grid, a CPU
    path, non-finite members (the outputs they touch are unspecified; no address depends on the data)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, grid=(1.0, 1.0), axis="x", window="hann",
                 per_member=False):
        noun = "line spectra"
        grid, N, L, d = lspec_args(C, Hh, Ww, grid, axis, window, members)
        if int(B) < 1 or int(steps) < 1:
            raise ValueError("%s need B >= 1 cases and steps >= 1, got %d and %d" % (noun, int(B), int(steps)))
        sd, mu = _ens_tables(C, "the fields are un-normalised with it", out_std, out_mu)
        u = _ens_u(u, int(B), C, "the fields are scaled with it")
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.grid, self.axis, self.window, self.per_member = grid, axis, window, bool(per_member)
        self.N, self.L, self.NQ, self.F = N, L, N // 2 + 1, C + 2
        self.k = torch.arange(self.NQ, dtype=torch.float64) * (2.0 * math.pi / (N * d))
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).contiguous()
        self.op = _lspec_operand(N, window).to(dev)
        self.plan = H.ens_lspec_plan(1, self.S, self.B, C, L, N)
        self.mean_state = torch.empty((self.S, self.B, C, L, self.NQ, 2), **f32)
        self.comom_state = torch.empty((self.S, self.B, self.F, L, self.NQ), **f32)
        self.step_state = torch.empty((2, self.B, self.F, self.NQ), **f32)
        self.out = {"lspec_mean": torch.empty((self.B, self.Tk, self.F, self.NQ), **f32),
                    "lspec_std": torch.empty((self.B, self.Tk, self.F, self.NQ), **f32)}
        self._part = None                 # workspace of the largest chunk: the tiles' line sums

    def add(self, y, m0, time=True):
        """Fold the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major)."""
        yn, _, k, t_before, last = self.open_chunk(y, m0, time)
        _on_device(yn)
        need = k * self.plan["part_floats"]
        if self._part is None or self._part.numel() < need:
            self._part = torch.empty(need, device=self.step_state.device, dtype=torch.float32)
        H.ens_lspec_chunk(yn, self.u, self.mu, self.sd, self.op, self.mean_state, self.comom_state, self._part, self.S, k, m0, t_before,
                          bool(time), columns=self.axis == "y")
        H.ens_lspec_step(self._part, self.step_state, self.out["lspec_mean"], self.out["lspec_std"], k, self.L, self.N, self._n, self.S,
                         self._step, last)
        self.close_chunk(m0, k, time, last)

    def finalize(self):
        """-> dict of the outputs; the time statistics cover the steps folded with time=True."""
        T = self.finalize_guard()
        dev = self.step_state.device
        o = dict(self.out)
        names = ("time_lspec_fluct_mean", "time_lspec_fluct_std", "time_lspec_flow_mean", "time_lspec_flow_std")
        for n in names:
            o[n] = empty((self.B, self.F, self.L, self.NQ), dev)
        mem = empty((self.B, self.S, self.F, self.L, self.NQ), dev) if self.per_member else None
        H.ens_lspec_finalize(self.mean_state, self.comom_state, [o[n] for n in names], mem, T)
        if mem is not None:
            o["time_lspec_fluct_member"] = mem
        o.update(lspec_outputs(o["time_lspec_fluct_mean"], self.k, self.C))
        o["lspec_k"] = self.k
        o["lspec_fields"] = lspec_fields(self.C)
        return o


def _tspec_window(Tn, window):
    """fp64 [Tn]: the periodic Hann window w_n = 0.5 - 0.5 cos(2 pi n / Tn) over sqrt(mean(w^2)), or ones."""
    n = torch.arange(Tn, dtype=torch.float64)
    if window != "hann":
        return torch.ones(Tn, dtype=torch.float64)
    w = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / Tn)
    return w / torch.sqrt(torch.mean(w * w))


def _tspec_operand(Tn, NF, window):
    """The host-built constants of the temporal DFT, fp64 rounded once to fp32, the argument reduced with integers as (k n) mod Tn:
    tm [Tn, RP] (RP = 2 NF + 1 rounded up to 16): tm[n, k] = g_n cos(2 pi k n / Tn), tm[n, NF + k] = -g_n sin(2 pi k n / Tn),
    tm[n, 2 NF] = 1 (the plain sum that gives xbar), the padding columns zero; cst [3, NF] = (Re G_k, Im G_k, c_k / Tn^2) with
    G_k = sum_n g_n exp(-2 pi i k n / Tn) (parts below 1e-9 Tn, fp64 noise of a sum that vanishes, set to zero) and c_k = 1 at k = 0 and at the Nyquist bin of an even Tn, else 2."""
    Tn, NF = int(Tn), int(NF)
    R = 2 * NF + 1
    RP = (R + 15) // 16 * 16
    g = _tspec_window(Tn, window)
    n = torch.arange(Tn, dtype=torch.int64)
    k = torch.arange(NF, dtype=torch.int64)
    ang = ((n[:, None] * k[None, :]) % Tn).to(torch.float64) * (2.0 * math.pi / Tn)
    re, im = g[:, None] * torch.cos(ang), -g[:, None] * torch.sin(ang)
    tm = torch.zeros((Tn, RP), dtype=torch.float64)
    tm[:, :NF], tm[:, NF:2 * NF], tm[:, 2 * NF] = re, im, 1.0
    ck = torch.full((NF,), 2.0, dtype=torch.float64)
    ck[0] = 1.0
    if Tn % 2 == 0 and NF > Tn // 2:
        ck[Tn // 2] = 1.0
    G = torch.stack((re.sum(0), im.sum(0)))
    G[G.abs() < 1e-9 * Tn] = 0.0        # sums that vanish analytically (Hann: every k >= 2) hold fp64 rounding noise: exact zeros
    cst = torch.cat((G, (ck / float(Tn) ** 2)[None]))
    return tm.to(torch.float32).contiguous(), cst.to(torch.float32).contiguous()


TSPEC_BLOCK = 16      # steps per ring pass (csrc/tmg_tspec.hip)


class EnsembleTimeSpectrum(EnsembleFeed):
    """On-device temporal power spectra of sampled roll-outs of B cases (tmg_tspec_store / tmg_tspec_block / tmg_tspec_finalize).
    For case b, member m, channel c and pixel p, with xh_n = u[b, c] (out_std[c] y + out_mu[c]) at the fed steps n = 0 .. Tn - 1:
      xbar = mean_n xh_n
      g_n  = periodic Hann w_n = 0.5 - 0.5 cos(2 pi n / Tn) over sqrt(mean_n w_n^2)           (window=None: g_n = 1)
      d_n  = g_n (xh_n - xbar)
      X_k  = sum_n d_n exp(-2 pi i k n / Tn),   k = 0 .. NF - 1,   NF = min(nfreq, Tn // 2 + 1)
      P_k  = c_k |X_k|^2 / Tn^2,   c_k = 1 for k = 0 and (Tn even and k = Tn / 2), else 2
    so that sum_{k = 0}^{Tn // 2} P_k = mean_n d_n^2.  The average over the members plays the role of Welch's segment average.
    The steps are gathered 16 at a time in a planar ring and folded by a dense DFT on the fp32 matrix pipe; the state is
    (2 NF + 1 + 16) * 4 bytes per element of [members, B, C, H, W].  H and W are any positive sizes.

    `steps` is Tn: there are no per-step outputs, so only the steps of the time window are fed.  Feeding protocol of EnsembleFeed:
    every step's members in chunks of whole members, in member order (m0 = 0 first), each step's chunks before the next step's.
    finalize() returns psd_mean, psd_std [B, NF, C, H, W] (device; mean and population std of P_k over the members) and psd_freq [NF]
    (float64, host: k / (Tn dt), dt the time between two fed steps).

    Argument errors are ValueError in this order: C, steps, nfreq, window, dt, members, the entries of out_mu / out_std, the shape of
    u; a device that is not a GPU comes last (RuntimeError)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, nfreq=32, window="hann", dt=1.0):
        _ens_channels("temporal spectra", C)
        if int(steps) < 2:
            raise ValueError("temporal spectra need steps >= 2 (the window of the transform), got %d" % int(steps))
        if int(nfreq) < 1:
            raise ValueError("temporal spectra need nfreq >= 1, got %d" % int(nfreq))
        if window not in ("hann", None):
            raise ValueError("window must be 'hann' or None, got %r" % (window,))
        try:
            dt = float(dt)
        except (TypeError, ValueError):
            raise ValueError("dt needs a positive finite time between two fed steps, got %r" % (dt,)) from None
        if not (math.isfinite(dt) and dt > 0):
            raise ValueError("dt needs a positive finite time between two fed steps, got %r" % (dt,))
        if int(members) < 1 or int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("temporal spectra need members, B, H and W >= 1, got %d, %d, %d x %d" % (int(members), int(B), int(Hh), int(Ww)))
        mu = torch.as_tensor(out_mu, dtype=torch.float32).detach().reshape(-1)[:C].cpu()
        sd = torch.as_tensor(out_std, dtype=torch.float32).detach().reshape(-1)[:C].cpu()
        if mu.numel() != C or sd.numel() != C:
            raise ValueError("out_mu / out_std need %d entries, got %d / %d" % (C, mu.numel(), sd.numel()))
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float32).detach()
            if u.numel() != int(B) * C:
                raise ValueError("u needs %d x %d entries, got %d" % (int(B), C, u.numel()))
        dev = _ens_device("temporal spectra", device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.Tn = self.Tk
        self.NF = min(int(nfreq), self.Tn // 2 + 1)
        self.window, self.dt = window, dt
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).reshape(self.B, C).contiguous()
        tm, cst = _tspec_operand(self.Tn, self.NF, window)
        self.tm, self.cst = tm.to(dev), cst.to(dev)
        HW = self.H * self.W
        self.ring = torch.empty((TSPEC_BLOCK, self.S, self.B, C, HW), **f32)
        self.acc = torch.empty((2 * self.NF + 1, self.S, self.B, C, HW), **f32)
        self.freq = torch.arange(self.NF, dtype=torch.float64) / (self.Tn * dt)
        self.out = None

    def _fold(self, n0, nb):
        H.tspec_block(self.tm, self.ring, self.acc, self.Tn, self.NF, n0, nb, n0 == 0)

    def add(self, y, m0):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); the last chunk of every 16th step folds the ring into the accumulator."""
        yn, _, k, _, last = self.open_chunk(y, m0, None)
        _on_device(yn)
        H.tspec_store(yn, self.u, self.mu, self.sd, self.ring, k, m0, self._step % TSPEC_BLOCK)
        self.close_chunk(m0, k, None, last)
        if last and self._step % TSPEC_BLOCK == 0:
            self._fold(self._step - TSPEC_BLOCK, TSPEC_BLOCK)

    def finalize(self):
        """-> dict of psd_mean, psd_std (device) and psd_freq (host)."""
        self.finalize_guard(timed=False)
        if self.out is None:
            nb = self.Tn % TSPEC_BLOCK
            if nb:
                self._fold(self.Tn - nb, nb)
            shp = (self.B, self.NF, self.C, self.H, self.W)
            dev = self.acc.device
            self.out = {"psd_mean": empty(shp, dev), "psd_std": empty(shp, dev), "psd_freq": self.freq}
            H.tspec_finalize(self.acc, self.cst, self.out["psd_mean"], self.out["psd_std"], self.S, self.B, self.C, self.H * self.W,
                             self.NF, self.Tn)
        return self.out


SPOD_MAX_MEMBERS = 255
SPOD_MAX_BINS = 16
SPOD_MAX_MODES = 8
# Roundings of one csd_raw entry beside the plan's L + P (csrc/tmg_spod.hip): 3 per operand for the correction (xbar, xbar G, the
# subtraction), 1 for the final combine, 1 for the second-order terms.
SPOD_ROUNDINGS = 8


def spod_args(bins, modes, channels, Tn, C):
    """The checks of the SPOD arguments for a window of Tn steps and C channels, in this order: Tn >= 2; bins None (the bins
    1..min(16, Tn // 2)) or 1 to 16 strictly increasing integers in 1..Tn // 2; modes an integer in 1..8; channels 1 to C distinct
    channels in 0..C-1 in any order (pod_channels' rules) -> (bins, modes, channels) as tuples of ints and an int."""
    if isinstance(Tn, bool) or not isinstance(Tn, numbers.Integral) or Tn < 2:
        raise ValueError("the SPOD needs a window of Tn >= 2 steps, got %r" % (Tn,))
    Tn = int(Tn)
    if bins is None:
        bins = tuple(range(1, min(SPOD_MAX_BINS, Tn // 2) + 1))
    else:
        try:
            bins = tuple(bins)
        except TypeError:
            raise ValueError("bins must be None or a tuple of frequency bins, got %r" % (bins,)) from None
        if not 1 <= len(bins) <= SPOD_MAX_BINS:
            raise ValueError("bins must hold 1 to %d bins, got %d" % (SPOD_MAX_BINS, len(bins)))
        for k in bins:
            if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= Tn // 2:
                raise ValueError("bins hold integers in 1..%d (k = 0 is not offered), got %r" % (Tn // 2, bins))
        if any(b <= a for a, b in zip(bins, bins[1:])):
            raise ValueError("bins must be strictly increasing, got %r" % (bins,))
        bins = tuple(int(k) for k in bins)
    if isinstance(modes, bool) or not isinstance(modes, numbers.Integral) or not 1 <= modes <= SPOD_MAX_MODES:
        raise ValueError("the SPOD keeps 1 <= modes <= %d, got %r" % (SPOD_MAX_MODES, modes))
    return bins, int(modes), pod_channels(channels, C)


def _spod_phase(theta):
    """Every eigenvector (the columns of theta [.., S, J], complex) rotated so that its entry of largest modulus (ties: the lowest
    member) is real and positive."""
    top = theta.abs().argmax(-2, keepdim=True)
    v = torch.gather(theta, -2, top)
    mod = v.abs()
    rot = torch.where(mod > 0, v.conj() / torch.where(mod > 0, mod, torch.ones_like(mod)), torch.ones_like(v))
    out = theta * rot
    # the rotated entry is real by construction: drop the rounding residue of its imaginary part
    fix = torch.gather(out, -2, top)
    return out.scatter(-2, top, torch.complex(fix.real, torch.zeros_like(fix.real)))


def _spod_eig(A, J):
    """Hermitian A [.., n, n] complex128 -> (lam [.., min(J, n)] descending, theta [.., n, min(J, n)] with _spod_phase's convention)."""
    w, v = torch.linalg.eigh(A)
    j = min(J, A.shape[-1])
    return w.flip(-1)[..., :j], _spod_phase(v.flip(-1)[..., :j])


def spod_decompose(csd_raw, S, HW, kappa, J, cnt, loo=True):
    """The host step of the spectral POD, plain torch fp64 on the CPU (once per mini-batch: not the hot path).  csd_raw
    [B, NB, 2, R, R], R = S + 1 (the members, then the target): raw0 + i raw1 = M[m, n] = sum conj(X_m) X_n over the Cg HW elements;
    HW: the pixels of the inner product <f, g> = (1 / HW) sum conj(f) g; kappa [NB] (or a number): c_k / Tn^2; J: the modes kept;
    cnt: the counted roundings of one csd_raw entry.  Per case and bin:
      A = kappa M[:S, :S] / (S HW) = Theta Lambda Theta^H (torch.linalg.eigh, eigenvalues descending; every eigenvector rotated so that
      its entry of largest modulus, the lowest member on a tie, is real and positive)
      spod_energy [B, NB, J] = lambda_j (0 for j >= S), spod_total [B, NB] = trace A, spod_energy_frac = spod_energy / spod_total,
      captured = sum_j spod_energy_frac, member_mode_energy [B, NB, S, J] = S lambda_j |Theta_mj|^2
      spod_noise_floor [B, NB] = cnt 2^-24 spod_total: bounds ||dA||_F, so eigenvalues below it cannot be told from rounding (Weyl)
      weights w_mj = Theta_mj sqrt(kappa / (S lambda_j)): Phi_j = sum_m X_m w_mj has <Phi_i, Phi_j> = delta_ij
      target_coef [B, NB, J] complex128 = b_j = <Phi_j, X_S> = sqrt(kappa / (S lambda_j)) sum_n conj(Theta_nj) M[n, S] / HW
      target_mode_energy = kappa |b_j|^2, target_energy [B, NB] = kappa M[S, S] / HW, target_captured = sum_j target_mode_energy /
      target_energy
      csd [B, NB, R, R] complex128 = M / HW
    A mode with lambda_j <= spod_noise_floor, or j >= S, has NaN weights, target_coef and target_mode_energy and is left out of
    target_captured.  loo: loo_captured [B, NB, S], the share of member m's energy kappa M[m, m] / HW in the leading J modes (above
    their own floor) of the other S - 1 members, which costs S eigendecompositions per case and bin, and target_captured_rank
    [B, NB], the number of members whose loo_captured is strictly under target_captured; both NaN for S = 1, absent for loo=False.
    -> dict of CPU tensors (float64 / complex128) with the keys above and `weights` [B, NB, S, J] complex128, `valid` [B, NB, J] bool."""
    raw = torch.as_tensor(csd_raw).detach().to("cpu", torch.float64)
    S, HW, J = int(S), int(HW), int(J)
    if raw.dim() != 5 or raw.shape[2] != 2 or tuple(raw.shape[3:]) != (S + 1, S + 1):
        raise ValueError("csd_raw is [B, NB, 2, %d, %d], got shape %s" % (S + 1, S + 1, tuple(raw.shape)))
    B, NB = raw.shape[:2]
    kap = torch.as_tensor(kappa, dtype=torch.float64).reshape(-1)
    if kap.numel() not in (1, NB):
        raise ValueError("kappa holds one value per bin (%d), got %d" % (NB, kap.numel()))
    kap = kap.expand(NB).reshape(1, NB)
    M = torch.complex(raw[:, :, 0], raw[:, :, 1])
    nan = float("nan")
    A = kap.view(1, NB, 1, 1) * M[:, :, :S, :S] / (S * HW)
    lam_s, theta_s = _spod_eig(A, J)                                         # [B, NB, Js], [B, NB, S, Js]
    Js = lam_s.shape[-1]
    total = torch.diagonal(A, dim1=-2, dim2=-1).real.sum(-1)
    floor = float(cnt) * 2.0 ** -24 * total
    lam = torch.zeros((B, NB, J), dtype=torch.float64)
    lam[..., :Js] = lam_s
    valid = torch.zeros((B, NB, J), dtype=torch.bool)
    valid[..., :Js] = lam_s > floor.unsqueeze(-1)
    theta = torch.zeros((B, NB, S, J), dtype=torch.complex128)
    theta[..., :Js] = theta_s
    safe = torch.where(valid, lam, torch.ones_like(lam))
    scale = torch.sqrt(kap.view(1, NB, 1) / (S * safe))                      # [B, NB, J]
    cnan = torch.complex(torch.full_like(lam, nan), torch.full_like(lam, nan))
    w = torch.where(valid.unsqueeze(2), theta * scale.unsqueeze(2), cnan.unsqueeze(2).expand(B, NB, S, J))
    col = M[:, :, :S, S]                                                     # [B, NB, S]
    bj = scale * (theta.conj() * col.unsqueeze(-1)).sum(2) / HW
    tme = torch.where(valid, kap.view(1, NB, 1) * bj.abs() ** 2, torch.full_like(lam, nan))
    ten = kap * M[:, :, S, S].real / HW
    frac = lam / total.unsqueeze(-1)
    o = {"spod_energy": lam, "spod_total": total, "spod_energy_frac": frac, "captured": frac.sum(-1),
         "member_mode_energy": S * lam.unsqueeze(2) * theta.abs() ** 2, "spod_noise_floor": floor,
         "target_coef": torch.where(valid, bj, cnan), "target_mode_energy": tme, "target_energy": ten,
         "target_captured": torch.where(valid, tme, torch.zeros_like(tme)).sum(-1) / ten, "csd": M / HW, "weights": w, "valid": valid}
    if loo:
        if S == 1:
            o["loo_captured"] = torch.full((B, NB, 1), nan, dtype=torch.float64)
            o["target_captured_rank"] = torch.full((B, NB), nan, dtype=torch.float64)
        else:
            cap = torch.empty((B, NB, S), dtype=torch.float64)
            for m in range(S):
                rest = [n for n in range(S) if n != m]
                Ao = kap.view(1, NB, 1, 1) * M[:, :, rest][:, :, :, rest] / ((S - 1) * HW)
                lo, to = _spod_eig(Ao, J)
                fo = float(cnt) * 2.0 ** -24 * torch.diagonal(Ao, dim1=-2, dim2=-1).real.sum(-1)
                ok = lo > fo.unsqueeze(-1)
                so = torch.sqrt(kap.view(1, NB, 1) / ((S - 1) * torch.where(ok, lo, torch.ones_like(lo))))
                bo = so * (to.conj() * M[:, :, rest, m].unsqueeze(-1)).sum(2) / HW
                en = torch.where(ok, kap.view(1, NB, 1) * bo.abs() ** 2, torch.zeros_like(lo)).sum(-1)
                cap[:, :, m] = en / (kap * M[:, :, m, m].real / HW)
            o["loo_captured"] = cap
            o["target_captured_rank"] = (cap < o["target_captured"].unsqueeze(-1)).sum(-1).to(torch.float64)
    return o


class EnsembleSpod(EnsembleFeed):
    """On-device spectral POD (SPOD; Towne, Schmidt & Colonius 2018) of sampled roll-outs of B cases, the members standing where
    Welch's blocks stand: per frequency bin the modes that are coherent in space and time among the members, their energies, and whether
    the target's Fourier coefficient at that bin lies in the same subspace with the same energy (tmg_tspec_store / tmg_tspec_block,
    unchanged, then tmg_ens_spod_csd / tmg_ens_spod_modes).  The rows are the S members and, as row S, the target at the same steps.
    X_m(c, p) at bin k is EnsembleTimeSpectrum's coefficient of row m (un-normalised to physical units, mean removed, periodic Hann over
    its RMS or no window), <f, g> = (1 / HW) sum_{c in channels} sum_p conj(f) g and kappa_k = c_k / Tn^2.  The device forms
      csd_raw [B, NB, 2, R, R]: raw0 + i raw1 = M[m, n] = sum conj(X_m) X_n            (fp32 on the matrix pipe, R = S + 1)
    spod_decompose turns it into the energies and weights on the host in fp64, and the device synthesises
      spod_modes [B, NB, J, 2, Cg, H, W]: the real and imaginary parts of Phi_j = sum_m X_m w_mj, <Phi_i, Phi_j> = delta_ij
    from the members' rows alone.  A mode at or below spod_noise_floor, or with j >= S, is NaN.

    bins: None for 1..min(16, Tn // 2), else 1 to 16 strictly increasing bins in 1..Tn // 2 (k = 0 is not offered); modes: J in 1..8;
    channels: 1 to C distinct channels in any order; 1 <= members <= 255; 2 <= C <= 4; any H, W >= 1.  `steps` is Tn: only the steps
    of the time window are fed.  The state is EnsembleTimeSpectrum's, (2 NF + 1 + 16) * 4 bytes per element of [R, B, C, H W] with
    NF = max(bins) + 1: all C channels are kept although only those of `channels` are used.  loo=True adds loo_captured and
    target_captured_rank, host fp64 from M alone at the cost of S eigendecompositions per case and bin.

    Feeding protocol of EnsembleFeed: every step's members in chunks of whole members, in member order (m0 = 0 first), each step's
    chunks before the next step's; every chunk comes with the step's target, and the last chunk's is the one that is stored.
    finalize() returns csd_raw and spod_modes (device, float32) and, on the host in float64 / complex128, spod_decompose's keys
    (spod_energy, spod_total, spod_energy_frac, captured, member_mode_energy, spod_noise_floor, target_coef, target_mode_energy,
    target_energy, target_captured, csd, and with loo loo_captured, target_captured_rank), spod_bins [NB] int64 and spod_freq [NB]
    = k / (Tn dt).  The attribute `cnt` is the counted roundings of one csd_raw entry, plan L + P + 8.

    Argument errors are ValueError in this order: C, steps, bins, modes, channels, window, dt, members (and B, H, W), the entries of
    out_mu / out_std, the shape of u; a device that is not a GPU comes last (RuntimeError)."""

    def __init__(self, members, B, C, Hh, Ww, steps, device, out_mu, out_std, u=None, bins=None, modes=4, channels=(0, 1), window="hann",
                 dt=1.0, loo=True):
        noun = "the SPOD"
        _ens_channels(noun, C)
        if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or int(steps) < 2:
            raise ValueError("%s needs steps >= 2 (the window of the transform), got %r" % (noun, steps))
        self.bins, self.J, self.channels = spod_args(bins, modes, channels, int(steps), int(C))
        if window not in ("hann", None):
            raise ValueError("window must be 'hann' or None, got %r" % (window,))
        try:
            dt = float(dt)
        except (TypeError, ValueError):
            raise ValueError("dt needs a positive finite time between two fed steps, got %r" % (dt,)) from None
        if not (math.isfinite(dt) and dt > 0):
            raise ValueError("dt needs a positive finite time between two fed steps, got %r" % (dt,))
        if not 1 <= int(members) <= SPOD_MAX_MEMBERS or int(B) < 1 or int(Hh) < 1 or int(Ww) < 1:
            raise ValueError("%s needs 1 <= members <= %d and B, H, W >= 1, got %d, %d, %d x %d"
                             % (noun, SPOD_MAX_MEMBERS, int(members), int(B), int(Hh), int(Ww)))
        mu = torch.as_tensor(out_mu, dtype=torch.float32).detach().reshape(-1)[:C].cpu()
        sd = torch.as_tensor(out_std, dtype=torch.float32).detach().reshape(-1)[:C].cpu()
        if mu.numel() != C or sd.numel() != C:
            raise ValueError("out_mu / out_std need %d entries, got %d / %d" % (C, mu.numel(), sd.numel()))
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float32).detach()
            if u.numel() != int(B) * C:
                raise ValueError("u needs %d x %d entries, got %d" % (int(B), C, u.numel()))
        dev = _ens_device(noun, device)
        EnsembleFeed.__init__(self, members, B, C, Hh, Ww, steps)
        self.Tn = self.Tk
        self.R = self.S + 1
        self.NF = max(self.bins) + 1
        self.window, self.dt, self.loo = window, dt, bool(loo)
        f32 = dict(device=dev, dtype=torch.float32)
        self.mu, self.sd = mu.to(dev).contiguous(), sd.to(dev).contiguous()
        self.u = None if u is None else u.to(dev).reshape(self.B, C).contiguous()
        tm, cst = _tspec_operand(self.Tn, self.NF, window)
        self.tm, self.cst = tm.to(dev), cst.to(dev)
        ck = torch.full((len(self.bins),), 2.0, dtype=torch.float64)
        if self.Tn % 2 == 0:
            ck[torch.tensor(self.bins) == self.Tn // 2] = 1.0
        self.kappa = ck / float(self.Tn) ** 2
        HW = self.H * self.W
        self.ring = torch.empty((TSPEC_BLOCK, self.R, self.B, C, HW), **f32)
        self.acc = torch.empty((2 * self.NF + 1, self.R, self.B, C, HW), **f32)
        self.plan = H.ens_spod_plan(self.S, self.B, len(self.channels), HW, len(self.bins), self.acc)
        self.cnt = self.plan["L"] + self.plan["P"] + SPOD_ROUNDINGS
        self.ws = torch.empty((self.plan["ws"],), **f32)
        self.freq = torch.tensor(self.bins, dtype=torch.float64) / (self.Tn * dt)
        self.out = None

    def _fold(self, n0, nb):
        H.tspec_block(self.tm, self.ring, self.acc, self.Tn, self.NF, n0, nb, n0 == 0)

    def add(self, y, m0, target):
        """Store the step's members m0 .. m0 + k - 1 of y (API-shaped [k*B, C, H, W], any strides whose channels-last view is an NHWC
        channel-slice; rows member-major); target: the step's normalised target [B, C, H, W] under the same stride rule.  The step's
        last chunk stores the target as row S; the last chunk of every 16th step folds the ring into the accumulator."""
        yn, tn, k, _, last = self.open_chunk(y, m0, None, target, required=True)
        _on_device(yn, tn)
        slot = self._step % TSPEC_BLOCK
        H.tspec_store(yn, self.u, self.mu, self.sd, self.ring, k, m0, slot)
        if last:
            H.tspec_store(tn, self.u, self.mu, self.sd, self.ring, 1, self.S, slot)
        self.close_chunk(m0, k, None, last)
        if last and self._step % TSPEC_BLOCK == 0:
            self._fold(self._step - TSPEC_BLOCK, TSPEC_BLOCK)

    def finalize(self):
        """-> dict of the outputs: csd_raw and spod_modes on the device, the derived ones on the host."""
        self.finalize_guard(timed=False)
        if self.out is None:
            nb = self.Tn % TSPEC_BLOCK
            if nb:
                self._fold(self.Tn - nb, nb)
            dev = self.acc.device
            B, NB, J, S, Cg, HW = self.B, len(self.bins), self.J, self.S, len(self.channels), self.H * self.W
            raw = empty((B, NB, 2, self.R, self.R), dev)
            H.ens_spod_csd(self.acc, self.cst, self.bins, self.channels, self.ws, raw, self.Tn)
            o = spod_decompose(raw, S, HW, self.kappa, J, self.cnt, self.loo)
            w, valid = o.pop("weights"), o.pop("valid")
            # the operand of the synthesis, fp64 rounded once: row 2 j = [Re w_j | -Im w_j], row 2 j + 1 = [Im w_j | Re w_j]; a mode under
            # the floor gets zero weights and its NaN afterwards, not through the pipe
            w = torch.where(valid.unsqueeze(2), w, torch.zeros_like(w)).transpose(2, 3)   # [B, NB, J, S]
            SP = (S + 3) // 4 * 4
            wr = torch.zeros((B, NB, 16, 2 * SP), dtype=torch.float64)
            wr[:, :, 0:2 * J:2, :S], wr[:, :, 0:2 * J:2, SP:SP + S] = w.real, -w.imag
            wr[:, :, 1:2 * J:2, :S], wr[:, :, 1:2 * J:2, SP:SP + S] = w.imag, w.real
            modes = empty((B, NB, 2 * J, Cg, HW), dev)
            H.ens_spod_modes(self.acc, self.cst, self.bins, self.channels, wr.to(torch.float32).to(dev).contiguous(), modes, self.Tn)
            modes = modes.view(B, NB, J, 2, Cg, self.H, self.W)
            modes[(~valid).to(dev)] = float("nan")
            o.update({"csd_raw": raw, "spod_modes": modes, "spod_bins": torch.tensor(self.bins, dtype=torch.int64), "spod_freq": self.freq})
            self.out = o
        return self.out
