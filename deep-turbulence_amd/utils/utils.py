"""Workspace (checkpoint) files in the reference's on-disk format (reference
utils/utils.py:55-148): `<name><id>.zip` holding `torchModel<id>.pth` = {'epoch', 'state_dict', 'optimizer'} and
`args.json`.  A workspace written by either code base loads in the other (the state_dict schema is the reference's, see
tests/test_boundary_cpu.py)."""
import collections
import io
import json
import math
import numbers
import os
import zipfile
from types import SimpleNamespace

import torch

# run-specific arguments a loaded workspace must not overwrite (reference utils/utils.py:20)
PARAM_BLACKLIST = ['epoch_start', 'epochs', 'run_dir', 'ckpt_dir', 'pred_dir']


def _model_entry(file_id):
    return 'torchModel{:d}.pth'.format(file_id)


def saveWorkspace(args, model, optimizer, file_name="nsWorkspace", file_id=0):
    """Write `<args.ckpt_dir>/<file_name><file_id>.zip`.  Built in memory: nothing but the zip touches the disk."""
    blob = io.BytesIO()
    torch.save({'epoch': file_id, 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict()}, blob)
    arg_dict = {k: v for k, v in vars(args).items() if k != 'device'}
    path = os.path.join(args.ckpt_dir, '{}{:d}.zip'.format(file_name, file_id))
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as z:
        z.writestr(_model_entry(file_id), blob.getvalue())
        z.writestr('args.json', json.dumps(arg_dict, indent=4, default=str))
    return path


def loadWorkspace(args, file_dir, file_name="nsWorkspace", file_id=0):
    """-> (args, model_state_dict, optimizer_state_dict), or None when the zip does not exist (as the reference).
    Arguments stored in the workspace overwrite those of `args` except the PARAM_BLACKLIST ones.  Tensors are loaded on
    the host; `load_state_dict` moves them."""
    path = os.path.join(file_dir, '{}{:d}.zip'.format(file_name, file_id))
    if not os.path.isfile(path):
        print('[LoadWorkspace] Could not find workspace zip file: {}'.format(path))
        return None
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
        if 'args.json' in names:
            try:
                for key, val in json.loads(z.read('args.json').decode()).items():
                    if key not in PARAM_BLACKLIST:
                        setattr(args, key, val)
            except ValueError as e:  # a damaged args file does not block the weights (reference :130-132)
                print('[LoadWorkspace] Could not read args.json: {}'.format(e))
        if _model_entry(file_id) not in names:
            raise FileNotFoundError('{} holds no {}'.format(path, _model_entry(file_id)))
        state = torch.load(io.BytesIO(z.read(_model_entry(file_id))), map_location='cpu', weights_only=False)
    return args, state['state_dict'], state['optimizer']


def modelPred(args, model, testing_loader, log, samples=1, stride=1, tmax=1):
    """Roll the model out over the test set for post-processing (reference utils/utils.py:151-235, the plotting scripts'
    entry): `samples` independent roll-outs of `tmax` steps per test case, every `stride`-th step kept, everything
    un-normalised and scaled back by the case's inlet velocity u0 (velocities x u0, pressure x u0^2).

    Returns (ypred [samples, N, tmax // stride, C, H, W], ytarget [N, T, C, H, W], yinput [N, T, 3, h, w]) on the CPU.
    The recurrent states are re-anchored half-way to their seed states every 20 steps, as the reference does."""
    core = getattr(model, "module", model)
    core.eval()
    dev = torch.device(args.device) if getattr(args, "device", None) is not None else next(core.parameters()).device
    shp = (1, -1, 1, 1)
    in_std, in_mu = core.in_std.to(dev).view(shp), core.in_mu.to(dev).view(shp)
    out_std, out_mu = core.out_std.to(dev).view(shp), core.out_mu.to(dev).view(shp)
    nkeep = tmax // stride
    preds, targets, inputs = [], [], []
    with torch.no_grad():
        for mbIdx, (input0, target0, u0) in enumerate(testing_loader):
            log.log('Running mini-batch {:d}/{:d}'.format(mbIdx + 1, len(testing_loader)))
            u = u0.to(dev).view(-1, 1, 1, 1, 1)
            u = torch.cat((u, u, u ** 2), dim=2)                      # [N,1,3,1,1]: (ux, uy, p) scales
            inp = input0.to(dev)
            tgt = u * (out_std * target0.to(dev) + out_mu)
            inputs.append((u * (in_std * inp[:, :, :3] + in_mu)).cpu())
            targets.append(tgt.cpu())
            mb = torch.full((samples, inp.size(0), nkeep) + tuple(tgt.shape[2:]), 10000.0, device=dev, dtype=inp.dtype)
            for i in range(samples):
                log.log('Running sample {:d}.'.format(i))
                seeds = torch.LongTensor(inp.size(0)).random_(0, int(1e8))
                key = core.initLSTMStates(seeds, [tgt.size(-2), tgt.size(-1)], cache=False)
                h0 = [(h.clone(), c.clone()) for h, c in key]
                for tstep in range(tmax):
                    y0, _logp, h0 = core.sample(inp[:, tstep], h0)
                    if tstep % stride == 0 and tstep // stride < nkeep:
                        mb[i, :, tstep // stride] = u[:, 0] * (out_std * y0 + out_mu)
                    if tstep % 20 == 0:
                        h0 = [(0.5 * h + 0.5 * hk, 0.5 * c + 0.5 * ck) for (h, c), (hk, ck) in zip(h0, key)]
            log.log('Number of elements unset: {}'.format(int((mb > 10000).sum())))
            preds.append(mb.cpu())
    return torch.cat(preds, dim=1), torch.cat(targets, dim=0), torch.cat(inputs, dim=0)


# modelPredTurbulence's statistics of the target series <- the one-member EnsembleStats output that holds them
_TARGET_STATS = (("target_time_mean", "time_mean_mean"), ("target_time_rms", "time_rms_mean"), ("target_time_uv", "time_uv_mean"),
                 ("target_time_tke", "time_tke_mean"), ("target_time_vort", "time_vort_mean"))


def _pdf_target_fields(tp, kinds, grid):
    """tp [B, T, C, H, W] fp64 physical target -> per field of `kinds` (tmg_ops.EnsemblePdfs' codes) its values [B, T, H, W]: the
    channel itself, or speed / vort / div by the 3x3 stencil of pc/ with zero padding (plain torch: this only chooses ranges)."""
    U, V = tp[:, :, 0], tp[:, :, 1]
    pad = lambda a: torch.nn.functional.pad(a, (1, 1, 1, 1))                  # noqa: E731
    ddx = lambda q: 2 * q[..., 1:-1, 2:] + q[..., :-2, 2:] + q[..., 2:, 2:] - 2 * q[..., 1:-1, :-2] - q[..., :-2, :-2] - q[..., 2:, :-2]   # noqa: E731
    ddy = lambda q: 2 * q[..., 2:, 1:-1] + q[..., 2:, :-2] + q[..., 2:, 2:] - 2 * q[..., :-2, 1:-1] - q[..., :-2, :-2] - q[..., :-2, 2:]   # noqa: E731
    out = []
    for k in kinds:
        if k < 4:
            out.append(tp[:, :, k])
        elif k == 4:
            out.append(torch.sqrt(U * U + V * V))
        else:
            rdx, rdy = 0.125 / float(grid[0]), 0.125 / float(grid[1])
            pu, pv = pad(U), pad(V)
            out.append(ddx(pv) * rdx - ddy(pu) * rdy if k == 5 else ddx(pu) * rdx + ddy(pv) * rdy)
    return out


# One optional accumulator of _ensembleStats, built by a modelPred* wrapper.
#   make(mb, members, steps) -> the tmg_ops accumulator of one mini-batch.  mb holds what the constructors take: B, C, H, W, dev,
#       out_mu, out_std, u [B, C], grid (the statistics': None without turbulence), and for the PDFs' ranges and centre tgt (the
#       physical target series on the device) and case0 (the cases before this mini-batch)
#   target: add() takes the step's normalised target
#   window: fed only the kept steps from t_start on, by add(y, m0) without time= (the temporal spectrum), or by add(y, m0, target) when
#       the record also has target (the SPOD); finalized last
#   meta:   result keys that are returned once, not concatenated over the mini-batches
#   extra:  fixed results
#   tail:   (result key, source key) pairs read from a one-member accumulator of the same make that is fed the target series
_Acc = collections.namedtuple("_Acc", "make target window meta extra tail", defaults=(False, False, (), {}, ()))


def _pdf_factory(name, args, stride, t_start, pdfs):
    """The make of modelPredPdfs' record.  pdfs: the keywords of tmg_ops.EnsemblePdfs, with ranges None for the target's own and
    center "target" for its time mean, both over the kept steps from t_start on; arrays per case are cut to the mini-batch."""
    def make(mb, members, steps):
        import tmg_ops as ops
        kw = dict(pdfs)
        B, pgrid = mb.B, (args.dx, args.dy)
        kinds = ops.pdf_args(kw["fields"], kw["bins"], [(0.0, 1.0)] * len(kw["fields"]), kw["joint"], kw["joint_bins"], kw["regions"],
                             pgrid, B, mb.C, mb.H, mb.W)[0]
        # the target's physical series at the kept steps from t_start on, in fp64 (range and centre only: not the hot path)
        tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride].double()
        if isinstance(kw["center"], str):
            kw["center"] = tk.mean(1).float()
        elif kw["center"] is not None:
            kw["center"] = torch.as_tensor(kw["center"])[mb.case0:mb.case0 + B]
        if kw["ranges"] is not None and torch.as_tensor(kw["ranges"]).dim() == 3:
            kw["ranges"] = torch.as_tensor(kw["ranges"])[mb.case0:mb.case0 + B]
        if kw["ranges"] is None:
            cen = None if kw["center"] is None else kw["center"].to(mb.dev).float().double().unsqueeze(1)
            vals = _pdf_target_fields(tk, kinds, pgrid)
            rg = torch.zeros(B, len(kinds), 2, dtype=torch.float64)
            for f, (k, v) in enumerate(zip(kinds, vals)):
                if k < 4 and cen is not None:
                    v = v - cen[:, :, k]
                lo, hi = v.reshape(B, -1).min(1).values.cpu(), v.reshape(B, -1).max(1).values.cpu()
                if bool((hi <= lo).any()):
                    raise ValueError("%s: field %r of the target of case %d is constant (%r): give ranges"
                                     % (name, kw["fields"][f], mb.case0 + int((hi <= lo).nonzero()[0]), float(lo[(hi <= lo).nonzero()[0]])))
                rg[:, f, 0], rg[:, f, 1] = lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)
            kw["ranges"] = rg
        return ops.EnsemblePdfs(members, B, mb.C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=pgrid, **kw)
    return make


def _ensembleStats(name, args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, turbulence, accs=()):
    """The body of every modelPred* wrapper below: modelPred's roll-outs, folded chunk by chunk into an EnsembleStats (turbulence:
    with grid = (args.dx, args.dy)) and then, in list order, into the accumulators of `accs`, the wrapper's _Acc records.  No record
    draws from the host RNG or iterates the loader again: same seed draws in the same order, same folding, same re-anchoring, so that
    the keys two wrappers share hold identical values under the same host RNG state."""
    import tmg_ops as ops
    core = getattr(model, "module", model)
    core.eval()
    dev = torch.device(args.device) if getattr(args, "device", None) is not None else next(core.parameters()).device
    if dev.type != "cuda" or next(core.parameters()).device.type != "cuda":
        raise RuntimeError("%s runs on the HIP path: the model must live on a GPU (there is no CPU path)" % name)
    grid = (args.dx, args.dy) if turbulence else None
    samples, max_rows = int(samples), int(max_rows)
    nkeep = tmax // stride
    if samples < 1 or nkeep < 1:
        raise ValueError("%s needs samples >= 1 and tmax >= stride (samples=%d, tmax=%d, stride=%d)" % (name, samples, tmax, stride))
    if not 0 <= t_start < nkeep:
        raise ValueError("t_start=%d outside the %d kept steps" % (t_start, nkeep))
    if any(a.window for a in accs) and nkeep - t_start < 2:
        raise ValueError("%s needs at least 2 kept steps from t_start on, got %d (tmax=%d, stride=%d, t_start=%d)"
                         % (name, nkeep - t_start, tmax, stride, t_start))
    needs_series = any(a.target or a.window for a in accs)
    stats = _Acc(lambda mb, S, T: ops.EnsembleStats(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=mb.grid),
                 tail=_TARGET_STATS if turbulence else ())
    accs = [stats] + list(accs)
    tails = [a for a in accs if a.tail]
    shp = (1, -1, 1, 1)
    in_std, in_mu = core.in_std.to(dev).view(shp), core.in_mu.to(dev).view(shp)
    out_std, out_mu = core.out_std.to(dev), core.out_mu.to(dev)
    outs, targets, inputs, meta = {}, [], [], {}
    case0 = 0                                                                 # cases before this mini-batch
    with torch.no_grad():
        for mbIdx, (input0, target0, u0) in enumerate(testing_loader):
            log.log('Running mini-batch {:d}/{:d}'.format(mbIdx + 1, len(testing_loader)))
            u = u0.to(dev).view(-1, 1, 1, 1, 1)
            u = torch.cat((u, u, u ** 2), dim=2)                      # [N,1,3,1,1]: (ux, uy, p) scales
            inp = input0.to(dev)
            tgt = u * (out_std.view(shp) * target0.to(dev) + out_mu.view(shp))
            inputs.append((u * (in_std * inp[:, :, :3] + in_mu)).cpu())
            targets.append(tgt.cpu())
            B, C, Hh, Ww = inp.size(0), tgt.size(2), tgt.size(-2), tgt.size(-1)
            if C != 3:
                raise ValueError("%s scales (ux, uy, p) by (u0, u0, u0^2) as modelPred does: 3 target channels, got %d" % (name, C))
            short = "%s: the target series holds %d steps, kept step %d needs step %d" % (name, target0.size(1), nkeep - 1, (nkeep - 1) * stride)
            if needs_series and target0.size(1) <= (nkeep - 1) * stride:
                raise ValueError(short)
            keys = []
            for i in range(samples):                                   # modelPred's seed draws, member by member
                seeds = torch.LongTensor(B).random_(0, int(1e8))
                keys.append(core.initLSTMStates(seeds, [Hh, Ww], cache=False))
            per = max(1, max_rows // B)
            chunks = [(m0, min(per, samples - m0)) for m0 in range(0, samples, per)]
            # per chunk: the members' seed states stacked member-major, and the running states
            anchors = [[tuple(torch.cat([keys[m0 + j][lv][s] for j in range(k)]) for s in (0, 1)) for lv in range(len(keys[0]))]
                       for m0, k in chunks]
            states = [[(h.clone(), c.clone()) for h, c in a] for a in anchors]
            mb = SimpleNamespace(B=B, C=C, H=Hh, W=Ww, dev=dev, out_mu=out_mu, out_std=out_std, u=u.view(B, 3)[:, :C], grid=grid, tgt=tgt,
                                 case0=case0)
            live = [(a, a.make(mb, samples, nkeep - t_start if a.window else nkeep)) for a in accs]
            case0 += B
            tnorm = target0.to(dev) if any(a.target for a in accs) else None   # the normalised series; one step at a time goes channels-last
            for tstep in range(tmax):
                keep = tstep % stride == 0 and tstep // stride < nkeep
                timed = tstep // stride >= t_start
                tj = tnorm[:, tstep].contiguous(memory_format=torch.channels_last) if keep and tnorm is not None else None
                for ci, (m0, k) in enumerate(chunks):
                    y0, _logp, states[ci] = core.sampleEnsemble(inp[:, tstep], states[ci], k)
                    if keep:
                        for a, acc in live:
                            if a.window:
                                if timed:
                                    if a.target:
                                        acc.add(y0, m0, tj)
                                    else:
                                        acc.add(y0, m0)
                            elif a.target:
                                acc.add(y0, m0, tj, time=timed)
                            else:
                                acc.add(y0, m0, time=timed)
                    if tstep % 20 == 0:
                        states[ci] = [(0.5 * h + 0.5 * hk, 0.5 * c + 0.5 * ck) for (h, c), (hk, ck) in zip(states[ci], anchors[ci])]
            for a, acc in sorted(live, key=lambda p: p[0].window):    # list order, the windowed ones last
                for key, t in acc.finalize().items():
                    if key in a.meta:
                        meta[key] = t
                    else:
                        outs.setdefault(key, []).append(t.cpu())
            if tails:
                # the target series over the kept steps from t_start on through the same kernels: a one-member ensemble
                if target0.size(1) <= (nkeep - 1) * stride:
                    raise ValueError(short)
                tn = target0.to(dev)
                ones = [a.make(mb, 1, nkeep - t_start) for a in tails]
                for j in range(t_start, nkeep):
                    tj = tn[:, j * stride].contiguous(memory_format=torch.channels_last)
                    for acc in ones:
                        acc.add(tj, 0)
                for a, acc in zip(tails, ones):
                    tout = acc.finalize()
                    for key, src in a.tail:
                        outs.setdefault(key, []).append(tout[src].cpu())
    res = {key: torch.cat(v, dim=0) for key, v in outs.items()}
    res["target"] = torch.cat(targets, dim=0)
    res["input"] = torch.cat(inputs, dim=0)
    for a in accs:
        res.update(a.extra)
    res.update(meta)
    return res


def modelPredStats(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64):
    """Ensemble statistics of `samples` roll-outs per test case, computed on the device without forming modelPred's
    [samples, N, T, C, H, W] tensor.  The roll-outs are modelPred's: fresh seeds from random_(0, 1e8) drawn member by member in
    modelPred's order (cache=False), states re-anchored half-way to their seed states every 20 steps, fields un-normalised and scaled
    by the case's inlet velocity u0 (velocities x u0, pressure x u0^2), every `stride`-th of `tmax` steps kept.  The members are
    folded into TMGlow.sampleEnsemble calls of at most `max_rows` rows, each chunk holding whole members (one member per call when
    a batch alone exceeds max_rows).

    Returns a dict of CPU tensors:
      mean, std [N, Tk, C, H, W]        mean and population std (ddof 0) over the members, per kept step (Tk = tmax // stride)
      mag_mean, mag_std [N, Tk, H, W]   the same of the velocity magnitude sqrt(ux^2 + uy^2)
      time_mean_mean, time_mean_std     mean / std over the members of each member's time mean over the kept steps t_start..Tk-1
      time_rms_mean, time_rms_std       ... of each member's RMS fluctuation sqrt(mean_t (y - mean_t y)^2) over those steps
                                        (all four [N, C, H, W]; t_start indexes the kept steps)
      target [N, T, C, H, W], input [N, T, 3, h, w]   as modelPred returns them."""
    return _ensembleStats("modelPredStats", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False)


def modelPredTurbulence(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64):
    """modelPredStats plus the turbulence statistics of the velocity field (channels 0, 1) on the grid (args.dx along W, args.dy
    along H), still without forming modelPred's [samples, N, T, C, H, W] tensor.  Same roll-outs as modelPredStats: under the same
    host RNG state the keys both return are identical.

    Returns modelPredStats' dict plus (CPU tensors):
      vort_mean, vort_std [N, Tk, H, W]       mean / population std over the members of the vorticity w = dv/dx - du/dy (3x3
                                              first-derivative stencil of pc/, zero padding), per kept step
      time_uv_mean, time_uv_std [N, H, W]     mean / std over the members of each member's Reynolds shear stress <u'v'> over the
                                              kept steps t_start..Tk-1
      time_tke_mean, time_tke_std             ... of each member's turbulent kinetic energy 0.5 (<u'u'> + <v'v'>)
      time_vort_mean, time_vort_std           ... of each member's time-mean vorticity
      target_time_mean, target_time_rms [N, C, H, W], target_time_uv, target_time_tke, target_time_vort [N, H, W]
                                              the same time statistics of the target series over the same steps (target step
                                              j * stride for kept step j), through the same kernels as a one-member ensemble."""
    return _ensembleStats("modelPredTurbulence", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, True)


def modelPredSpectra(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, window="hann"):
    """modelPredTurbulence plus the shell-binned kinetic-energy spectra E(k) of the velocity field (channels 0, 1) on the grid
    (args.dx along W, args.dy along H), still without forming modelPred's [samples, N, T, C, H, W] tensor: the 2-D DFT of
    g (u + i v) of every member and kept step on the device (tmg_ops.EnsembleSpectrum; g: the periodic Hann window over its RMS, or 1
    for window=None), E2 = 0.5 |Z|^2 / (H W)^2 summed over the shells of tmg_ops.spectrum_bins, so that the shells of one field sum
    to 0.5 mean(g^2 (u^2 + v^2)).  H and W must be multiples of 16 up to 512.  Same roll-outs as modelPredTurbulence: under the same
    host RNG state the keys both return are identical.

    Returns modelPredTurbulence's dict plus (CPU tensors):
      spec_k [NK] float64                    the shell centres s 2 pi / max(W dx, H dy)
      spec_mean, spec_std [N, Tk, NK]        mean / population std over the members of E, per kept step
      time_spec_mean, time_spec_std [N, NK]  mean / std over the members of each member's time mean of E over the kept steps
                                             t_start..Tk-1
      target_spec [N, Tk - t_start, NK], target_time_spec [N, NK]
                                             E of the target series at those steps (target step j * stride for kept step j) and its
                                             time mean, through the same kernels as a one-member ensemble."""
    if window not in ("hann", None):
        raise ValueError("window must be 'hann' or None, got %r" % (window,))
    import tmg_ops as ops
    acc = _Acc(lambda mb, S, T: ops.EnsembleSpectrum(S, mb.B, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=mb.grid, window=window),
               meta=("spec_k",), tail=(("target_spec", "spec_mean"), ("target_time_spec", "time_spec_mean")))
    return _ensembleStats("modelPredSpectra", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, True, [acc])


def _xspec_factory(args, stride, t_start, window, center, level):
    """The make of modelPredSpectralSkill's record.  center "target": the target's time mean over the kept steps from t_start on,
    formed in fp64 on the physical target series and rounded once (as _pdf_factory); an array [N, >= 2, H, W] is cut to the
    mini-batch; None: no centre."""
    def make(mb, members, steps):
        import tmg_ops as ops
        cen = center
        if isinstance(cen, str):
            cen = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride].double().mean(1).float()
        elif cen is not None:
            cen = torch.as_tensor(cen)[mb.case0:mb.case0 + mb.B]
        return ops.EnsembleSpectralSkill(members, mb.B, mb.C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u,
                                         grid=(args.dx, args.dy), window=window, center=cen, level=level)
    return make


def modelPredSpectralSkill(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, window="hann",
                           center="target", level=0.5):
    """modelPredStats plus the spectral skill of the velocity field (channels 0, 1) against the target on the grid (args.dx along W,
    args.dy along H), still without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleSpectralSkill).  TM-Glow is
    a conditional generator: the low-fidelity input pins the large scales of a member, the small scales are invented.  The question
    here: down to which scale does a member reproduce the target field itself, and from which scale on is it only statistically
    plausible?  modelPredSpectra's E(k) holds magnitudes only (a member whose small scales hold the right energy in the wrong places
    has a perfect E(k)); crps, rank_hist, energy_score, fss and the field ranks verify in physical space with all scales mixed; and
    spread against error is reported per scale nowhere else.  The target of kept step j is series step j * stride; a series that is
    too short raises.  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.

    Per case, kept step and row (member m, target T, ensemble-mean field bar = the mean of the members' fields):
    f_c = yh_c - M_c (c = 0, 1; center "target": M is the target's time mean over the kept steps from t_start on, an array
    [N, >= 2, H, W]: that plane, None: nothing is subtracted; the mean flow is trivially coherent, the question is about the
    fluctuations), z = g (f_0 + i f_1) with g the periodic Hann window over its RMS (window=None: 1), Z = fft2(z), and per mode
    P = sc |Z|^2, X = sc Re(conj(Z) Z_T), D = sc |Z - Z_T|^2 with sc = 0.5 / (H W)^2, summed over the shells of
    tmg_ops.spectrum_bins.  H and W must be multiples of 16 up to 512.

    Returns modelPredStats' dict plus (CPU tensors; S = samples, kept steps t_start..Tk-1 are the timed ones):
      xs_target_power [N, Tk, NK], xs_sum, xs_mean_field [N, Tk, 3, NK], xs_time_member [N, S, 3, NK], xs_time_target [N, NK],
      xs_time_mean_field [N, 3, NK]      float32: the raw shell sums of P_T, of sum_m (P, X, D), of (P_bar, X_bar, D_bar), and their
                                         sums over the timed steps per member, for the target and for the mean field
      spec_corr, mean_field_corr [N, Tk, NK]
                                         float64 from here on: the spectral coherence with the target of the members (pooled:
                                         Xm / sqrt(Pm P_T)) and of the ensemble-mean field
      err_spec, mean_err_spec, spread_spec
                                         the members' mean error spectrum Dm, the mean field's D_bar, and Dm - D_bar
      spread_skill                       sqrt((S + 1) / S spread_spec / D_bar): 1 for a calibrated ensemble, per shell
      power_ratio, rel_err               Pm / P_T and Dm / P_T (2 for a decorrelated member of the right energy)
      time_spec_corr .. time_rel_err [N, NK]
                                         the same from the sums over the timed steps
      time_member_corr [N, S, NK], time_corr_mean, time_corr_std [N, NK]
                                         each member's coherence over the timed steps, its mean and population std over the members
      cutoff_k [N, S + 1], cutoff_len    the effective resolution: the wavenumber at which the time coherence first falls under
                                         `level` (members, the mean field last; interpolated between shells, inf when it never
                                         does), and 2 pi over it
      cutoff_k_mean, cutoff_k_std [N]    over the members, ignoring inf
      xs_k [NK]                          the shell centres s 2 pi / max(W dx, H dy).
    A ratio with a zero denominator is NaN (the empty shells of a stretched grid).

    Not supported: a pressure or scalar coherence; quadrature and phase spectra; per-member per-step outputs; coherence with the
    low-fidelity input, which lives on a different grid; pixel boxes; fields that are not multiples of 16; non-finite members (the
    outputs of an affected step are unspecified)."""
    import tmg_ops as ops
    if isinstance(center, str) and center != "target":
        raise ValueError("center is 'target', None or a plane [N, >= 2, H, W], got %r" % (center,))
    ops.xspec_args(3, 16, 16, (getattr(args, "dx", 1.0), getattr(args, "dy", 1.0)) if args is not None else (1.0, 1.0), window, level)
    acc = _Acc(_xspec_factory(args, stride, t_start, window, center, level), target=True, meta=("xs_k",))
    return _ensembleStats("modelPredSpectralSkill", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _lspec_log_distance(ens, tgt, C):
    """ens, tgt [N, F, L, NQ] -> [N, C, L] float64: the RMS over q = 1 .. NQ-1 of 10 log10(ens / tgt) of the C autospectra, NaN where
    either is not positive at any of those modes."""
    a, b = ens[:, :C, :, 1:].double(), tgt[:, :C, :, 1:].double()
    ok = (a > 0) & (b > 0)
    r = 10.0 * torch.log10(torch.where(ok, a, torch.ones_like(a)) / torch.where(ok, b, torch.ones_like(b)))
    d = torch.sqrt((r * r).mean(-1))
    return torch.where(ok.all(-1), d, torch.full_like(d, float("nan")))


def modelPredLineSpectra(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, axis="x", window="hann",
                         per_member=False):
    """modelPredTurbulence plus the one-dimensional line spectra of every channel at every line of the field, still without forming
    modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleLineSpectra): the spectrum of u'u', v'v', p'p' and the co-spectrum of
    u'v' along x at each height y (axis="x": lines are the rows, d = args.dx) or along y at each station x (axis="y": the columns,
    d = args.dy), of the fluctuations about each member's own time mean.  time_tke_* and time_uv_* give the integral over scales of
    what these resolve by scale; modelPredSpectra's E(k) includes the mean flow.  Same roll-outs as modelPredTurbulence: under the
    same host RNG state the keys both return are identical.

    Per case, member, kept step, channel c and line l: X_c[l, q] = (1 / N) sum_n w[n] yh_c[l, n] exp(-2 pi i q n / N), q = 0 .. N/2,
    w the periodic Hann window over its RMS (window=None: 1); planes (lspec_fields): a_q |X_c|^2 of the C channels, then
    uv_co = a_q Re(X_0 conj X_1) and uv_quad = a_q Im(X_0 conj X_1), a_q = 1 at q = 0 and N/2, else 2.  The line length must be a
    multiple of 16 in 16..512.  Kept steps t_start..Tk-1 are the timed ones (T of them).

    Returns modelPredTurbulence's dict plus (CPU tensors; F = C + 2, L lines, NQ = N/2 + 1):
      lspec_mean, lspec_std [N, Tk, F, NQ]           mean / population std over the members of the line-averaged planes of X, per
                                                     kept step (the total spectrum: mean flow included)
      time_lspec_fluct_mean, time_lspec_fluct_std [N, F, L, NQ]
                                                     ... of each member's fluctuation spectrum a_q (1 / T) sum_t (X_t - Xbar) conj(Y_t - Ybar)
                                                     (a population moment, as time_rms; one pass, Welford)
      time_lspec_flow_mean, time_lspec_flow_std      ... of the planes of each member's time-mean coefficient Xbar
      time_lspec_fluct_member [N, S, F, L, NQ]       every member's fluctuation spectrum (per_member=True only)
      time_lspec_energy [N, F, L], time_lspec_centroid [N, C, L], time_lspec_coherence [N, L, NQ]
                                                     float64, of time_lspec_fluct_mean: the sum over q; sum_{q>=1} k Phi / sum_{q>=1} Phi;
                                                     (co^2 + quad^2) / (Phi_00 Phi_11); NaN at 0 / 0
      target_lspec [N, T, F, NQ], target_time_lspec_fluct, target_time_lspec_flow [N, F, L, NQ]
                                                     the same of the target series at the timed steps (target step j * stride for
                                                     kept step j), through the same kernels as a one-member ensemble
      lspec_log_distance [N, C, L]                   float64: the RMS over q = 1..NQ-1 of 10 log10(time_lspec_fluct_mean /
                                                     target_time_lspec_fluct) of the autospectra, NaN where either is not positive
      lspec_k [NQ] float64 (2 pi q / (N d)), lspec_fields (the plane names).
    Not supported: two-dimensional fluctuation spectra, wavenumber-frequency spectra, Welch segments, sizes off the 16 grid."""
    import tmg_ops as ops
    grid = (getattr(args, "dx", 1.0), getattr(args, "dy", 1.0)) if args is not None else (1.0, 1.0)
    ops.lspec_args(3, 16, 16, grid, axis, window, int(samples) if int(samples) >= 1 else 1)
    acc = _Acc(lambda mb, S, T: ops.EnsembleLineSpectra(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=grid,
                                                        axis=axis, window=window, per_member=bool(per_member)),
               meta=("lspec_k", "lspec_fields"),
               tail=(("target_lspec", "lspec_mean"), ("target_time_lspec_fluct", "time_lspec_fluct_mean"),
                     ("target_time_lspec_flow", "time_lspec_flow_mean")))
    res = _ensembleStats("modelPredLineSpectra", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, True, [acc])
    res["lspec_log_distance"] = _lspec_log_distance(res["time_lspec_fluct_mean"], res["target_time_lspec_fluct"], 3)
    return res


def modelPredScores(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64):
    """modelPredStats plus the ensemble's calibration scores against the target the loader carries, still without forming modelPred's
    [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleScores).  The target of kept step j is series step j * stride.  Same roll-outs
    as modelPredStats: under the same host RNG state the keys both return are identical.

    Returns modelPredStats' dict plus (CPU tensors), with xh_1..xh_S the un-normalised members and yh the un-normalised target:
      crps [N, Tk, C, H, W]             the ensemble CRPS per pixel and kept step,
                                        (1/S) sum_m |xh_m - yh| - (1 / (2 S^2)) sum_m sum_n |xh_m - xh_n|
      crps_fair [N, Tk, C, H, W]        the same with 1 / (2 S (S - 1)) on the pair term (samples = 1: crps = |xh_1 - yh|)
      rank_hist [N, Tk, C, S + 1]       int64: the number of pixels whose target has rank r = #{m : xh_m < yh} (strict), r = 0..S
                                        (the Talagrand histogram; flat for a calibrated ensemble)
      time_crps, time_crps_fair [N, C, H, W]   the means of crps / crps_fair over the kept steps t_start..Tk-1
      time_rank_hist [N, C, S + 1]      int64: the sum of rank_hist over those steps."""
    import tmg_ops as ops
    acc = _Acc(lambda mb, S, T: ops.EnsembleScores(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_std, u=mb.u), target=True)
    return _ensembleStats("modelPredScores", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredTimeSpectra(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, nfreq=32, window="hann",
                         dt=None):
    """modelPredStats plus the temporal power spectra of every member's series at every pixel over the kept steps t_start..Tk-1
    (Tn = Tk - t_start >= 2 of them), still without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleTimeSpectrum):
    the frequency content of the roll-outs - shedding behind the cylinders, the flapping shear layer behind the step - beside the
    target's.  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.

    With xh_n the un-normalised value at kept step t_start + n, xbar its mean over the window, g the periodic Hann window over its
    RMS (window=None: 1), d_n = g_n (xh_n - xbar) and X_k = sum_n d_n exp(-2 pi i k n / Tn):
      P_k = c_k |X_k|^2 / Tn^2, k = 0 .. NF - 1, NF = min(nfreq, Tn // 2 + 1); c_k = 1 at k = 0 and at the Nyquist bin of an even Tn,
      else 2, so that the bins 0 .. Tn // 2 of one series sum to mean_n d_n^2.
    The average over the members stands where Welch's segment average stands for a single signal.

    Returns modelPredStats' dict plus (CPU tensors):
      psd_mean, psd_std [N, NF, C, H, W]   mean / population std over the members of P_k
      psd_freq [NF] float64                k / Tn, cycles per kept step, when dt is None; else k / (Tn stride dt) with dt the time
                                           between two model steps (the reference's args carry no time step)
      target_psd [N, NF, C, H, W]          P_k of the target series at steps j * stride, j = t_start..Tk-1, through the same kernels
                                           as a one-member ensemble; raises when the series is too short."""
    if window not in ("hann", None):
        raise ValueError("window must be 'hann' or None, got %r" % (window,))
    if int(nfreq) < 1:
        raise ValueError("nfreq must be >= 1, got %d" % int(nfreq))
    step_dt = 1.0 if dt is None else float(stride) * float(dt)
    if not (math.isfinite(step_dt) and step_dt > 0):
        raise ValueError("dt must be a positive finite time between two model steps, got %r" % (dt,))
    import tmg_ops as ops
    acc = _Acc(lambda mb, S, T: ops.EnsembleTimeSpectrum(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, nfreq=int(nfreq), window=window, dt=step_dt),
               window=True, meta=("psd_freq",), tail=(("target_psd", "psd_mean"),))
    return _ensembleStats("modelPredTimeSpectra", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredQuantiles(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, levels=(0.05, 0.5, 0.95),
                       exceed=()):
    """modelPredStats plus the ensemble's prediction band and exceedance probabilities per pixel, still without forming modelPred's
    [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleQuantiles): exact order statistics of the members, so the band is right where
    the members' marginals are skewed or bimodal (behind a bluff body) and mean +- k std is not.  The target of kept step j is series
    step j * stride; a series that is too short raises.  Channel scales (u0, u0, u0^2).  Same roll-outs as modelPredStats: under the
    same host RNG state the keys both return are identical.

    levels: 1 to 8 probabilities in [0, 1] (any order, duplicates allowed).  exceed: up to 4 tuples (channel, value, ">" | "<") with
    value in physical units; (0, 0.0, "<") is the reverse-flow probability P(ux < 0), which locates the recirculation and
    reattachment behind the step and the wake behind the cylinders.

    Returns modelPredStats' dict plus (CPU tensors), with Q levels, K thresholds, S = samples and Tn = Tk - t_start timed steps:
      quant [N, Tk, Q, C, H, W]         the un-normalised quantiles of the members per kept step (numpy's method="linear")
      time_quant [N, Q, C, H, W]        the mean of quant over the kept steps t_start..Tk-1
      time_below_count [N, Q, C, H, W]  int64: the number of those steps at which the target is strictly under the quantile
      below_frac [N, Q, C, H, W]        time_below_count / Tn
      exceed_prob [N, Tk, K, H, W]      the share of the members strictly above (">") / below ("<") the threshold, per kept step
      time_exceed_count [N, K, H, W]    int64: the member counts summed over those steps
      time_exceed_prob [N, K, H, W]     time_exceed_count / (S Tn)                       (the three exceed keys only when K > 0)
      levels [Q] float64                the levels as given.

    What below_frac should be.  For a calibrated ensemble the target is exchangeable with the members, so it falls under the order
    statistic x_(r) (r = 0..S-1) with probability P(y < x_(r)) = (r + 1) / (S + 1) - not r / (S - 1).  A level that falls on a member
    (w = 0 in tmg_ops.quantile_levels, rank lo) should therefore show below_frac near (lo + 1) / (S + 1), not q: the median of S = 5
    members gives 0.5, but level 0 gives 1 / 6 and level 1 gives 5 / 6.  A level between two members is approximately the linear
    interpolation ((lo + 1) + w) / (S + 1) of its two neighbours."""
    import tmg_ops as ops
    levels, exceed = (tuple(v) for v in ops.quantile_args(levels, exceed, 3))
    acc = _Acc(lambda mb, S, T: ops.EnsembleQuantiles(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, levels=levels, exceed=exceed), target=True,
               meta=("levels",))
    return _ensembleStats("modelPredQuantiles", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredEnergy(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, groups=((0, 1), (2,))):
    """modelPredStats plus the ensemble's energy score and the distances between the members as whole fields, still without forming
    modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleEnergy).  Every other score here is per pixel and does not change when
    the pixels of every member are shuffled independently; the energy score is the multivariate generalisation of the CRPS and scores
    each member as one vector over the pixels.  The target of kept step j is series step j * stride; a series that is too short
    raises.  Channel scales (u0, u0, u0^2).  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are
    identical.

    groups: tuples of channels that share a unit, each channel in at most one group; the default is velocity (0, 1) and pressure (2,).
    With xh_0..xh_{S-1} the un-normalised members, xh_S the un-normalised target and |.|_g the Euclidean norm over the pixels and the
    channels of group g, dist[m, n] = |xh_m - xh_n|_g.

    Returns modelPredStats' dict plus (CPU tensors; Gn groups, S = samples, kept steps t_start..Tk-1 are the timed ones):
      target_dist_mean [N, Tk, Gn]      (1/S) sum_m dist[m, S]: the mean distance of a member to the target
      pair_dist_mean [N, Tk, Gn]        (1/S^2) sum_m sum_n dist[m, n]: the mean distance of two members (m = n counted, as in crps)
      energy_score [N, Tk, Gn]          target_dist_mean - pair_dist_mean / 2; lower is better, a proper score of the whole field
      energy_score_fair [N, Tk, Gn]     the same with 1 / (S (S - 1)) on the pair sum (samples = 1: energy_score = dist[0, S])
      medoid [N, Tk, Gn] int64          argmin_m sum_n dist[m, n]: the representative member, the one to plot
      nearest [N, Tk, Gn] int64, nearest_dist [N, Tk, Gn]   the member closest to the target and its distance (ties: the lowest member)
      time_energy_score, time_energy_score_fair [N, Gn]     the means of the two scores over the timed steps
      traj_dist2 [N, Gn, S + 1, S + 1]  the sum of dist^2 over the timed steps: the squared distance between whole roll-outs, space and
                                        time as one vector; symmetric, zero diagonal, the target as the last row and column
      traj_energy_score, traj_energy_score_fair [N, Gn], traj_medoid, traj_nearest [N, Gn] int64
                                        the same formulas on sqrt(traj_dist2)
      energy_groups                     the groups as given.

    What to read from target_dist_mean against pair_dist_mean.  For a calibrated ensemble the target is exchangeable with the members,
    so the expected member-to-target distance equals the expected member-to-member distance: compare target_dist_mean with
    pair_dist_mean S / (S - 1) (the pair mean without its S zero terms m = n).  A target that is much further from the members than
    they are from each other means an over-confident (under-dispersive) or biased ensemble; members further apart than the target is
    from them mean an over-dispersive one."""
    import tmg_ops as ops
    groups = ops.energy_groups(groups, 3)
    acc = _Acc(lambda mb, S, T: ops.EnsembleEnergy(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_std, u=mb.u, groups=groups), target=True,
               extra={"energy_groups": tuple(groups)})
    return _ensembleStats("modelPredEnergy", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredFieldRanks(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, groups=((0, 1), (2,))):
    """modelPredStats plus the multivariate rank histograms of the target among the members as whole fields, still without forming
    modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleFieldRanks): the average-rank and band-depth histograms of
    Thorarinsdottir, Scheuerer & Heinz (2016), the depth being the modified band depth of Lopez-Pintado & Romo (2009).  rank_hist of
    modelPredScores is per pixel: it can be flat while every member is too smooth, or while the members never bracket the target as
    a field.  The energy score of modelPredEnergy is one number and cannot tell under-dispersion from bias.  These histograms do for
    fields what rank_hist does for pixels.  The target of kept step j is series step j * stride; a series that is too short raises.
    Ranks do not change under the un-normalisation (u0 out_std > 0), so no channel scale enters and the channels of a group combine
    without a norm.  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.

    groups: tuples of channels, each channel in at most one group; the default is velocity (0, 1) and pressure (2,).  With the rows
    x_0..x_{S-1} (members) and x_S (target), per pixel p and row i over the S other rows: lt, eq, gt the rows below, equal to and
    above x_i; A_i(p) = 2 lt + eq; D_i(p) = C(S,2) - C(lt,2) - C(gt,2), the pairs of other rows whose closed band holds x_i;
    O(p) = [the target is strictly outside the members' range].  The pre-rank of row i is the sum of A (or D) over the pixels and the
    group's channels; below / equal count the members whose pre-rank is under / equal to the target's.

    Returns modelPredStats' dict plus (CPU tensors; Gn groups, S = samples, kept steps t_start..Tk-1 are the Tn timed ones; int64
    unless stated):
      pre_raw [N, Tk, C, S + 1, 2]      sum_p A_i(p) and sum_p D_i(p) per channel, the target last
      avg_prerank, depth_prerank [N, Tk, Gn, S + 1]
      avg_rank_below, avg_rank_equal, depth_rank_below, depth_rank_equal [N, Tk, Gn]
                                        the field rank of the target.  Low average rank: the target lies under the members; low depth
                                        rank: the target is the most outlying row
      avg_rank_hist, depth_rank_hist [N, Gn, S + 1] float64
                                        over the timed steps, each step adding 1 / (equal + 1) to the bins below .. below + equal
                                        (the expectation of random tie-breaking); each sums to Tn.  Sum them over N to pool cases.
                                        U-shaped average ranks, or depth ranks piled at the low end, mean under-dispersion
      traj_avg_prerank, traj_depth_prerank [N, Gn, S + 1]
                                        the pre-ranks summed over the timed steps: the roll-out as one vector
      traj_avg_rank_below, traj_avg_rank_equal, traj_depth_rank_below, traj_depth_rank_equal [N, Gn]
      depth_median [N, Tk, Gn], traj_depth_median [N, Gn]
                                        the member with the largest depth pre-rank (the functional median; ties: the lowest member)
      outside_count [N, Tk, C], outside_frac float64
                                        the pixels whose target lies strictly outside the members' range, and their share of the
                                        field; a calibrated continuous ensemble gives 2 / (S + 1)
      time_outside_count [N, C, H, W], time_outside_frac float64
                                        the timed steps at which the pixel's target lay outside, and their share of Tn
      fieldrank_groups                  the groups as given.

    Not supported: the minimum-spanning-tree rank histogram, the functional boxplot and central-region envelopes, pixel boxes or
    thinning of the field, per-member field ranks beyond depth_median, pooling over cases, more than 1024 members, non-finite
    members (the outputs of a pixel that holds one are unspecified)."""
    import tmg_ops as ops
    groups = ops.energy_groups(groups, 3)
    acc = _Acc(lambda mb, S, T: ops.EnsembleFieldRanks(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, groups=groups), target=True,
               extra={"fieldrank_groups": tuple(groups)})
    return _ensembleStats("modelPredFieldRanks", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredStructure(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, lags=None, weights=None):
    """modelPredStats plus the structure functions of every member and of the target and the ensemble's variogram score, still without
    forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleStructure, grid = (args.dx, args.dy)).  This is the
    dependence between neighbouring pixels of ONE member: permute the members independently at every pixel and every per-pixel score
    (crps, rank_hist, quant) stays bit-identical, and the energy score barely moves; the increments D(p) = x(p + l) - x(p) at a pixel
    lag l = (dx, dy) (dx along W, dy along H) see it.  The target of kept step j is series step j * stride; a series that is too short
    raises.  Channel scales a = (u0, u0, u0^2) * out_std.  Same roll-outs as modelPredStats: under the same host RNG state the keys both
    return are identical.

    lags: up to 16 distinct (dx, dy) with dx >= 0, and dy > 0 when dx == 0, 0 <= dx <= 64, |dy| <= 64, dx < W, |dy| < H; None: (1, 0),
    (2, 0), .. in powers of two up to min(32, W // 2), then the same along H.  weights: one positive finite w_l per lag, default 1.

    Returns modelPredStats' dict plus (CPU tensors; L lags, S = samples, kept steps t_start..Tk-1 are the T timed ones, N_l the pairs
    of lag l):
      sf2, sf3, sf4 [N, Tk, C, L, S+1]  the structure functions <D^q> = a^q sum_p D^q / N_l of every member, the target's row last
      sf2_mean, sf2_std [N, Tk, C, L]   mean and population std of sf2 over the members, target excluded
      vario_lag [N, Tk, C, L]           w_l a sum_p (sqrt|D_target| - mean_m sqrt|D_m|)^2 / N_l: the variogram score of order 1/2
                                        (Scheuerer & Hamill 2015) per lag, in physical units; lower is better
      vario_score [N, Tk, C]            its sum over the lags
      time_sf2, time_sf3, time_sf4 [N, C, L, S+1]   the same averages over the timed steps as well
      time_skew, time_flat [N, C, L, S+1]           time_sf3 / time_sf2^1.5 and time_sf4 / time_sf2^2 (0 where time_sf2 == 0): the
                                        increment skewness and flatness, the standard measures of intermittency (3 for Gaussian increments)
      time_vario_lag [N, C, L], time_vario_score [N, C]   the means of vario_lag / vario_score over the timed steps
      lags [L, 2] int64, lag_dist [L] float64       the lags and their lengths hypot(dx args.dx, dy args.dy)."""
    import tmg_ops as ops
    if lags is not None:
        lags = ops.structure_lags(lags, 65, 65)                           # the rules that do not depend on the field; the field's come with it
    acc = _Acc(lambda mb, S, T: ops.EnsembleStructure(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_std, u=mb.u, lags=lags, weights=weights, grid=(args.dx, args.dy)),
               target=True, meta=("lags", "lag_dist"))
    return _ensembleStats("modelPredStructure", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredEvents(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, events=((0, 0.0, "<"),),
                    scales=(1, 3, 5, 9, 17, 33)):
    """modelPredStats plus the verification of the ensemble's event probabilities against the target, still without forming
    modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleEvents).  An event is (channel, value, ">" | "<"), strict, in
    physical units, as modelPredQuantiles' `exceed` entries (1 to 4 of them; (0, 0.0, "<") is reverse flow): the forecast probability
    of a pixel is the share n / S of the members in the event (modelPredQuantiles' exceed_prob), the observation o is whether the
    target is in it.  The target of kept step j is series step j * stride; a series that is too short raises.  scales: 1 to 8
    distinct odd neighbourhood widths in 1..33 pixels.  Same roll-outs as modelPredStats: under the same host RNG state the keys both
    return are identical.

    Returns modelPredStats' dict plus (CPU tensors; K events, NS widths, S = samples, kept steps t_start..Tk-1 are the Tn timed ones):
      rel_count, rel_hit [N, Tk, K, S+1]  int64: the pixels with j of S members in the event, and those of them where the target is
                                        in it: the reliability table.  rel_hit / rel_count against j / S is the reliability diagram: on
                                        the diagonal a forecast probability of 0.7 comes true 70 % of the time
      brier [N, Tk, K]                  the Brier score mean_p (n / S - o)^2; lower is better
      brier_rel, brier_res, brier_unc   its Murphy decomposition, brier = brier_rel - brier_res + brier_unc: reliability (0 is
                                        perfect), resolution (higher is better, at most brier_unc) and the target's own uncertainty
      base_rate, fcst_rate [N, Tk, K]   the share of pixels at which the target is in the event, and the mean forecast probability
      roc_area [N, Tk, K]               the area under the ROC curve of the rule "yes when n >= j": 0.5 = no discrimination between
                                        event and non-event pixels, 1 = perfect; NaN when the target has no event or no non-event
      fss_raw [N, Tk, K, NS, 3]         int64: (sum Nf^2, sum Nf No, sum No^2) of the w x w box sums of n and o (zeros outside the field)
      fss [N, Tk, K, NS]                the fractions skill score (Roberts & Lean 2008) per width: 1 = the forecast puts the same area
                                        fraction of the event into every neighbourhood, 0 = no overlap; NaN when neither has the event
      time_rel_count, time_rel_hit [N, K, S+1], time_rel_obs_freq [N, K, S+1]   the tables summed over the timed steps and the
                                        observed frequency per bin (NaN in empty bins): read it against the diagonal j / S
      time_roc_hit_rate, time_roc_false_rate [N, K, S+2]   the ROC curve of the summed tables, thresholds j = 0..S+1
      time_brier, time_brier_rel, time_brier_res, time_brier_unc, time_base_rate, time_roc_area [N, K]   the same formulas on the
                                        summed tables: pooled over steps and pixels
      time_fss [N, K, NS]               from the summed raw sums (the standard aggregation, not a mean of ratios).  Read it against
      time_fss_uniform [N, K]           = 0.5 + time_base_rate / 2: the smallest width at which time_fss exceeds it is the scale from
                                        which the forecast counts as skilful
      time_event_count, time_obs_count [N, K, H, W]   int64: sum_t n and sum_t o per pixel (the first is modelPredQuantiles'
                                        time_exceed_count); time_obs_count / Tn is the target's own event frequency
      time_brier_map [N, K, H, W]       the Brier score per pixel over the timed steps
      event_scales [NS] int64, events   the widths and the events as given."""
    import tmg_ops as ops
    events, scales = (tuple(v) for v in ops.event_args(events, scales, 3))
    acc = _Acc(lambda mb, S, T: ops.EnsembleEvents(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, events=events, scales=scales), target=True,
               meta=("event_scales",), extra={"events": events})
    return _ensembleStats("modelPredEvents", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredSpells(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, events=((0, 0.0, "<"),),
                    max_len=32):
    """modelPredStats plus the durations of the members' and the target's events over the kept steps t_start..Tk-1 (Tn = Tk - t_start
    >= 2 of them), still without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleSpells).  modelPredEvents says,
    step by step, whether a pixel is in an event; this says for how long: a member whose recirculation bubble flickers on and off
    and one whose bubble persists get the same tables there and different ones here.  An event is (channel, value, ">" | "<"), strict,
    in physical units, as modelPredEvents' (1 to 4 of them; (0, 0.0, "<") is reverse flow); a non-finite value is in no event.  Per
    row (the S = samples members, then the target as row S), case, event and pixel the indicator series splits into runs of equal
    value: polarity 1 is a spell (in the event), polarity 0 a gap.  A run that touches an end of the window is censored - its true
    length is unknown - and is counted apart as left (holds the first step), right (holds the last) or both (the whole window):
    censored runs are excluded from the histograms and the mean durations on purpose, so a short window biases neither towards short
    runs it merely cut; read spell_cens beside spell_hist to see how much of the record is censored.  Durations are in kept steps:
    `stride` scales them (a run of length l lasted between (l - 1) stride + 1 and (l + 1) stride - 1 model steps).  The target of
    kept step j is series step j * stride; a series that is too short raises.  max_len: the L length bins, 1..64.  Tn <= 32767.
    Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.

    Returns modelPredStats' dict plus (CPU tensors; K events, R = S + 1 rows with the target last, polarity 0 = gaps, 1 = spells):
      spell_hist [N, K, R, 2, L]          int64: the complete runs by length, pooled over the pixels; bin j - 1 holds length j, the
                                          last bin length >= L.  Compare a member's row with row S: mass at short lengths that the
                                          target does not have is flicker
      spell_len [N, K, R, 2]              int64: the sum of the complete runs' lengths
      spell_cens, spell_cens_len [N, K, R, 2, 3]   int64: the numbers and length sums of the left, right and both runs.  All lengths
                                          of a row over both polarities and all four classes sum to Tn H W
      spell_mean [N, K, R, 2]             the mean complete duration, NaN without a complete run
      spell_survival [N, K, R, 2, L]      entry j - 1: the share of complete runs that last at least j steps; a geometric decay
                                          is what a memoryless (Markov) state gives
      spell_p11, spell_p01 [N, K, R]      the probabilities to stay in the event and to enter it from one kept step to the next,
                                          exact from the tables; NaN when the row is never in (out of) the event before the last step
      spell_markov_mean [N, K, R]         1 / (1 - p11): the mean spell of a two-state chain with this persistence; spell_mean well
                                          above it means the state is held longer than its one-step statistics explain
      spell_w1 [N, K, S, 2], spell_w1_pooled [N, K, 2]   the Wasserstein-1 distance, in bins, between a member's (all members' pooled)
                                          distribution of complete durations and the target's; NaN when either is empty
      spell_mean_below, spell_mean_equal, spell_mean_valid [N, K, 2]   int64: of the members with a complete run (valid), those whose
                                          mean duration is strictly below / equal to the target's: the exact rank of the target's
                                          persistence within the ensemble (0 or valid: every member holds the state too long or too briefly)
      time_in_count [N, K, H, W]          int64: member-steps in the event per pixel (modelPredEvents' time_event_count)
      time_spell_count [N, K, H, W]       int64: the members' spells of any class per pixel
      time_longest_sum, time_longest_max [N, K, H, W]   int64: the sum and the maximum over the members of each member's longest spell
                                          of any class; time_longest_mean = time_longest_sum / S
      time_mean_duration [N, K, H, W]     time_in_count / time_spell_count, censored spells included: where the ensemble holds the
                                          event longest; NaN where no member is ever in it
      target_in_count, target_spell_count, target_longest, target_mean_duration [N, K, H, W]   the same of the target
      spell_bins [L] int64, events        the lengths 1..L of the bins and the events as given."""
    import tmg_ops as ops
    events, max_len = ops.spell_args(events, max_len, 3)
    events = tuple(events)
    acc = _Acc(lambda mb, S, T: ops.EnsembleSpells(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, events=events, max_len=max_len),
               target=True, window=True, meta=("spell_bins",), extra={"events": events})
    return _ensembleStats("modelPredSpells", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredIntensityScale(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, events=((0, 0.0, "<"),),
                            levels=None):
    """modelPredStats plus the intensity-scale verification of the members' events against the target's, still without forming
    modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleIntensityScale).  modelPredEvents says whether the event
    probabilities are right pixel by pixel and, through the fractions skill score, from which neighbourhood width on they count as
    skilful; this says at which spatial scale the error sits: a recirculation bubble drawn two pixels too long and one placed a
    quarter of the domain away both lower the FSS at small widths, and differ here.  An event is (channel, value, ">" | "<"), strict,
    in physical units, as modelPredEvents' (1 to 4 of them; (0, 0.0, "<") is reverse flow); a non-finite value is in no event.  The
    binary error field I_member - I_target of every event is split into the orthogonal 2-D Haar components of dyadic block size 2,
    4, .., 2^L (blocks aligned at pixel (0, 0), the field counting as zero outside H x W, so any H, W works) plus the coarse
    remainder, and the mean squared error of each component is read against that of a spatially random forecast with the same event
    rates (Casati, Ross & Stephenson 2004; the energy form of Casati 2010).  The same split of the probability error n / S - o
    decomposes modelPredEvents' Brier score by scale, exactly, and the difference to the members' mean error is the ensemble's spread
    at that scale.  levels: L in 1..6, None for max(1, min(6, floor(log2(min(H, W))))).  The target of kept step j is series step
    j * stride; a series that is too short raises.  Same roll-outs as modelPredStats: under the same host RNG state the keys both
    return are identical.

    Returns modelPredStats' dict plus (CPU tensors; K events, S members, L + 1 components, the last the remainder):
      iscale_member_raw [N, Tk, K, S, L+1, 2]   int64 (A, X): per level l = 0..L the sums over the blocks of s_l(I_m)^2 and s_l(I_m) s_l(o)
      iscale_target_raw [N, Tk, K, L+1]         int64 Cc: of s_l(o)^2
      iscale_ens_raw [N, Tk, K, L+1, 2]         int64 (AN, XN): of s_l(n)^2 and s_l(n) s_l(o), n the members in the event per pixel
      iscale_mse [N, Tk, K, S, L+1]             the component energies of a member's error over H W; they sum to its share of
                                                mismatched pixels
      iscale_skill [N, Tk, K, S, L+1]           1 - (L+1) mse_c / (f + o - 2 f o), f and o the member's and the target's event
                                                rates: 0 is no better than a random placement at that scale; NaN when that error is 0
      iscale_energy [N, Tk, K, S+1, L+1]        the component energies of the members' indicators and, as row S, of the target's
      iscale_energy_bias [N, Tk, K, S, L+1]     (Ef - Eo) / (Ef + Eo): too much (+) or too little (-) event structure at that
                                                scale; NaN when both are 0
      iscale_brier [N, Tk, K, L+1]              the component energies of n / S - o; they sum to modelPredEvents' brier
      iscale_brier_skill [N, Tk, K, L+1]        against mean p^2 + o - 2 mean p o shared equally among the components; NaN at 0
      iscale_spread [N, Tk, K, L+1]             the mean member mse minus iscale_brier, >= 0: the ensemble's spread at that scale
      iscale_spread_skill [N, Tk, K, L+1]       spread over brier; NaN at 0 / 0
      time_<key> [N, K, ...]                    every key above from the raw sums summed over the kept steps t_start..Tk-1, with the
                                                event rates pooled: the standard aggregation, not a mean of ratios
      iscale_blocks [L+1] int64, events         the block sizes 2 .. 2^L, then 0 for the remainder; the events as given."""
    import tmg_ops as ops
    events, _ = ops.event_args(events, (1,), 3)
    events = tuple(events)
    if levels is not None:
        levels = ops.iscale_args(events, levels, 3, 1, 1)[1]
    acc = _Acc(lambda mb, S, T: ops.EnsembleIntensityScale(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, events=events,
                                                           levels=levels),
               target=True, meta=("iscale_blocks",), extra={"events": events})
    return _ensembleStats("modelPredIntensityScale", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _morphology_factory(name, grid, stride, t_start, fields, thresholds, levels):
    """The make of modelPredMorphology's record.  thresholds None: per case and field `levels` values evenly spaced on the mean +- 2
    population std of the target's physical values over the kept steps from t_start on (plain torch in fp64; one level: the mean)."""
    def make(mb, members, steps):
        import tmg_ops as ops
        th = thresholds
        if th is None:
            tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride, list(fields)].double()       # [B, Tn, F, H, W]
            v = tk.permute(0, 2, 1, 3, 4).reshape(mb.B, len(fields), -1)
            mean = v.mean(-1, keepdim=True)
            sd = ((v - mean) ** 2).mean(-1, keepdim=True).sqrt()
            bad = ~(torch.isfinite(sd) & (sd > 0) & torch.isfinite(mean)).reshape(mb.B, -1).all(1)
            if bool(bad.any()):
                raise ValueError("%s: a field of the target of case %d is constant or not finite: give thresholds"
                                 % (name, mb.case0 + int(bad.nonzero()[0])))
            pos = torch.linspace(-2.0, 2.0, levels, dtype=torch.float64, device=v.device) if levels > 1 \
                else torch.zeros(1, dtype=torch.float64, device=v.device)
            th = (mean + sd * pos).cpu()
        return ops.EnsembleMorphology(members, mb.B, mb.C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, fields=fields,
                                      thresholds=th, grid=grid)
    return make


def modelPredMorphology(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, fields=(0,), thresholds=None,
                        levels=16):
    """modelPredStats plus the excursion-set morphology of every member and of the target, still without forming modelPred's
    [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleMorphology): the three Minkowski functionals of the sets {x > level} of a field
    as the level moves up a ladder: how much area lies above the level, how long its boundary is, and how many pieces and holes it
    has (the Euler characteristic or genus curve), the standard morphology diagnostic of random and turbulent fields.  The other
    diagnostics judge a roll-out pixel by pixel, scale by scale, along time, or by vortex objects at one criterion; a member can have
    the right pixel PDF and the right spectrum and still be speckled or over-smooth.  It then has the target's area curve, a wrong
    boundary length and an Euler characteristic wrong by a factor.  Reading the keys: equal mink_area but larger mink_edges and
    |mink_euler*| than the target's means speckle (many small pieces or holes); smaller means over-smooth; mink_euler4 and
    mink_euler8 far apart means one-pixel diagonal structure (pieces that touch only at corners); mink_below / mink_equal say where the
    target's curve ranks among the members', and mink_l1 is one number per member and curve for how far its curve is from the
    target's.  fields: 1 to 4 distinct channels of (ux, uy, p).  thresholds: per field J (1..32) strictly ascending physical values,
    the same for every case; None: per case and field `levels` (1..32) values evenly spaced on the mean +- 2 population std of the
    target over the kept steps t_start..Tk-1 (one level: the mean); a constant target raises.  Compares are strict; NaN is in no set,
    +Inf in every one.  The grid is (args.dx along W, args.dy along H); the target of kept step j is series step j * stride; a series
    that is too short raises.  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.

    Returns modelPredStats' dict plus (CPU tensors; F fields, R = S + 1 rows, the members then the target, J levels):
      mink_raw [N, Tk, F, R, J, 5]             int64 (N, Nh, Nv, Nq, Nd): pixels in the set, horizontal / vertical pairs with both in,
                                               2 x 2 quads with all four in, quads with exactly a diagonal pair in; in-field only
      mink_area [N, Tk, F, R, J]               the share of the field above the level
      mink_perimeter [N, Tk, F, R, J]          boundary length per unit area, the field's border included
      mink_edges [N, Tk, F, R, J] int64        exposed unit edges 4 N - 2 Nh - 2 Nv
      mink_euler4, mink_euler8 [.., R, J] int64   4-connected pieces minus 8-connected holes; 8-connected pieces minus 4-connected holes
      mink_euler4_density, mink_euler8_density    per unit area
      mink_mean, mink_std [N, Tk, F, 4, J]     mean and population std over the members of the curves (N, edges, euler4, euler8)
      mink_below, mink_equal [N, Tk, F, 4, J]  int64: the members strictly below / equal to the target on those curves
      mink_l1 [N, Tk, F, S, 4]                 the trapezoid integral over the physical ladder of |member - target| of (area,
                                               perimeter, euler4 density, euler8 density); 0 when J = 1
      time_<key> [N, F, ...]                   every key above from the raw counts summed over the kept steps t_start..Tk-1, with
                                               H W Tn pixels as the area: the standard aggregation, not a mean of ratios
      mink_levels [N, F, J] float64, fields    the physical ladder of every case; the fields as given.
    Not supported: derived fields such as vorticity, periodic domains (pairs and quads across the border are not counted), a
    Gaussian-random-field reference curve to read the genus curve against."""
    import tmg_ops as ops
    if thresholds is None:
        if isinstance(levels, bool) or not isinstance(levels, numbers.Integral) or not 1 <= levels <= ops.MINK_MAX_LEVELS:
            raise ValueError("levels is an integer in 1..%d, got %r" % (ops.MINK_MAX_LEVELS, levels))
        fields = ops.mink_args(fields, [[0.0]] * (len(fields) if hasattr(fields, "__len__") else 1), 3)[0]
    else:
        fields, thresholds = ops.mink_args(fields, thresholds, 3)
    acc = _Acc(_morphology_factory("modelPredMorphology", (float(args.dx), float(args.dy)), stride, t_start, fields, thresholds,
                                   None if thresholds is not None else int(levels)),
               target=True, extra={"fields": fields})
    return _ensembleStats("modelPredMorphology", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredDistance(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, events=((0, 0.0, "<"),),
                      cutoff=None, quantiles=(0.5, 0.75, 0.9)):
    """modelPredStats plus the distance-map verification of the members' events against the target's, still without forming
    modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleDistance).  modelPredEvents says whether the event probabilities
    are right pixel by pixel and from which neighbourhood width on they count as skilful, modelPredIntensityScale at which dyadic
    scale the error sits, modelPredMorphology how speckled the sets are; none says how FAR a member's event set lies from the
    target's: a recirculation bubble drawn six pixels downstream of the target's and one drawn a quarter of the domain away both
    give zero overlap, similar FSS at small widths and identical Minkowski curves, and differ here.  These are the distance-map
    measures of spatial forecast verification (Gilleland 2011; Baddeley 1992; Dubuisson & Jain 1994), all formed from the exact
    Euclidean distance transform of the event sets, in pixels.  An event is (channel, value, ">" | "<"), strict, in physical units,
    as modelPredEvents' (1 to 4 of them; (0, 0.0, "<") is reverse flow); a non-finite value is in no event.  cutoff: the distance c
    in whole pixels (1..255; None: max(1, min(255, max(H, W) // 4))) at which the distances behind the means and Baddeley's delta
    saturate, so that one stray pixel far away cannot dominate them; the Hausdorff distances are uncut.  quantiles: the
    probabilities of the partial Hausdorff distance.  Reading the keys: dist_med_miss large with dist_med_false small means the
    member's event covers only part of the target's (the rest is far from anything forecast); the reverse means spurious event area
    away from the target's; both of the size of a shift mean a displaced copy.  dist_hausdorff is the worst single pixel and reacts
    to one speck; dist_hausdorff_q at 0.9 forgives a tenth of the pixels; dist_baddeley also sees where neither set is and is a
    metric between the sets; dist_csi is the plain overlap, for contrast.  time_dist_bias_map > 0 marks where the ensemble keeps the
    event farther from the pixel than the target does.  The target of kept step j is series step j * stride; a series that is too
    short raises.  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.

    Returns modelPredStats' dict plus (CPU tensors; K events, S members, A a member's event set, O the target's):
      dist_pair_raw [N, Tk, K, S, 11]           int64 (nA, nO, nAO, sOA1, sOA2, sAO1, sAO2, sD1, sD2, hOA, hAO): set sizes and
                                                overlap; the sums over O of w_A and w_A^2 and over A of w_O and w_O^2, w = floor(256
                                                min(d, c)); the sums over all pixels of |w_A - w_O| and its square; the maxima over O
                                                of d2_A and over A of d2_O (squared pixels, uncut; -1 for an empty set, 2^30 against
                                                an empty set)
      dist_hist_raw [N, Tk, K, S, 2, c+1]       int64: over O the counts by min(floor(d_A), c), over A by min(floor(d_O), c)
      dist_med_miss, dist_med_false [N, Tk, K, S]   the mean error distances, target-to-member and member-to-target; NaN for an
                                                empty O / A
      dist_rms_miss, dist_rms_false             their root-mean-square forms
      dist_med [N, Tk, K, S]                    the larger of the two means: the modified Hausdorff distance
      dist_hausdorff_miss, dist_hausdorff_false, dist_hausdorff [N, Tk, K, S]   directed and symmetric Hausdorff distances; 0 when
                                                both sets are empty, inf when exactly one is
      dist_hausdorff_q [N, Tk, K, S, 2, NQ]     the partial Hausdorff distances in whole pixels (miss, false); c means "c or more";
                                                NaN for an empty set
      dist_baddeley, dist_baddeley1 [N, Tk, K, S]   Baddeley's delta with p = 2 and p = 1 on min(d, c)
      dist_csi [N, Tk, K, S]                    nAO / (nA + nO - nAO); NaN when both sets are empty
      dist_mean, dist_std [N, Tk, K, 6], dist_valid int64   mean and population std over the members of (dist_med_miss,
                                                dist_med_false, dist_med, dist_hausdorff, dist_baddeley, dist_csi), non-finite
                                                values dropped, and how many members were kept
      time_<key> [N, K, ...]                    every key above from the raw sums pooled over the kept steps t_start..Tk-1 (sums
                                                added, maxima maxed, H W Tn pixels as the area): not a mean of ratios
      time_dist_member_sum, time_dist_target_sum [N, K, H, W] int64   the sums over those steps (and the members) of w_A(p), of w_O(p)
      time_dist_mean_map [N, K, H, W]           member_sum / (256 S Tn): the ensemble's mean distance from the pixel to the event
      time_dist_bias_map [N, K, H, W]           that minus target_sum / (256 Tn)
      dist_cutoff, dist_quantiles, events       c (int64 scalar), the probabilities (float64), the events as given.
    Not supported: anisotropic metrics (pixels are the unit, as for modelPredEvents' widths), periodic domains, Pratt's figure of
    merit, distances finer than 1 / 256 pixel."""
    import tmg_ops as ops
    events, c0, quantiles = ops.dist_args(events, cutoff, quantiles, 3, 1, 1)
    events = tuple(events)
    cutoff = None if cutoff is None else c0
    acc = _Acc(lambda mb, S, T: ops.EnsembleDistance(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, events=events,
                                                     cutoff=cutoff, quantiles=quantiles),
               target=True, meta=("dist_cutoff", "dist_quantiles"), extra={"events": events})
    return _ensembleStats("modelPredDistance", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredPdfs(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, fields=("ux", "uy", "p", "vort"),
                  bins=64, ranges=None, joint=(("ux", "uy"),), joint_bins=32, regions=None, center=None):
    """modelPredStats plus the probability densities of the flow quantities themselves, pooled over regions of the flow, for the
    ensemble and for the target, still without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsemblePdfs, grid =
    (args.dx, args.dy)): the PDF of the streamwise velocity in the wake, of the vorticity (whose tails are the vortex cores a smeared
    surrogate loses first), of the divergence (nothing constrains a sampled field to be incompressible), and the joint PDF of
    (ux, uy), whose quadrants are the sweep and ejection events of quadrant analysis.  The target of kept step j is series step
    j * stride; a series that is too short raises.  Channel scales (u0, u0, u0^2).  Same roll-outs as modelPredStats: under the same
    host RNG state the keys both return are identical; no option draws from the host RNG, and the loader is iterated once.

    fields: up to 8 of a channel 0..2 ("ux", "uy", "p"), "speed", "vort", "div" (a field may be listed twice with two ranges).
    bins: 1..128 uniform bins per field, plus an underflow and an overflow bin; a value on an edge belongs to the bin above.
    ranges: one (lo, hi) per field in physical units, or [N, F, 2] per case; None: per case and field the min and max of that field of
    the case's target series over the kept steps from t_start on, both ends widened by a quarter of the span (a constant field raises).
    joint: up to 2 pairs of listed fields, joint_bins (1..32) bins per axis over the same ranges.  regions: up to 4 pixel boxes
    (x0, x1, y0, y1), half open, x along W, possibly overlapping; None: the whole field.  center: None, [N, C, H, W] in physical
    units, or "target" for the target's time mean over the same steps: channel fields are then binned as fluctuations about it, so
    that ("ux", "uy") is the quadrant plane about the reference mean flow.

    Returns modelPredStats' dict plus (CPU tensors; F fields, P pairs, R regions, nb = bins, nbj = joint_bins, S = samples, kept
    steps t_start..Tk-1 are the timed ones; bins 0 and nb + 1 are the under- and overflow):
      pdf_count, target_count [N, Tk, R, F, nb+2]   int64: the histograms per kept step, pooled over members and pixels / of the target
      joint_count, target_joint_count [N, Tk, R, P, nbj+2, nbj+2]   int64: the joint histograms, the first field of a pair on the rows
      time_member_count [N, S, R, F, nb+2]          int64: each member's histogram pooled over the timed steps
      time_count, time_target_count [N, R, F, nb+2], time_joint_count, time_target_joint_count [N, R, P, nbj+2, nbj+2]   int64
      pdf, target_pdf [N, Tk, R, F, nb]             inner count / (all counts * bin width): what is out of range is missing from
                                                    the integral
      time_pdf, time_target_pdf [N, R, F, nb]       the same of the pooled counts
      time_pdf_mean, time_pdf_std [N, R, F, nb]     mean / population std over the members of each member's own time-pooled density
      w1, js [N, Tk, R, F], time_w1, time_js [N, R, F]   the pooled ensemble against the target: the Wasserstein-1 distance (physical
                                                    units; each bin's mass at its centre, the out-of-range masses one width outside)
                                                    and the Jensen-Shannon divergence in bits over the nb + 2 bins, in [0, 1]
      time_member_w1 [N, S, R, F]                   each member's time-pooled distribution against the target's: one member is a
                                                    legitimate realisation, so it should match within sampling noise
      time_joint_js [N, R, P]                       the Jensen-Shannon divergence of the time-pooled joint tables
      pdf_edges [N, F, nb+1], joint_edges [N, P, 2, nbj+1], pdf_ranges [N, F, 2]   float64: the physical edges and the (lo, hi) used
      pdf_fields, pdf_joint, pdf_regions            as given (regions None: the whole field as one box)."""
    if isinstance(center, str) and center != "target":
        raise ValueError("center is None, an array [N, C, H, W] in physical units or \"target\", got %r" % (center,))
    pdfs = dict(fields=tuple(fields), bins=bins, ranges=ranges, joint=tuple(tuple(pr) for pr in joint), joint_bins=joint_bins,
                regions=regions, center=center)
    acc = _Acc(_pdf_factory("modelPredPdfs", args, stride, t_start, pdfs), target=True, meta=("pdf_fields", "pdf_joint", "pdf_regions"))
    return _ensembleStats("modelPredPdfs", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _modes_factory(name, stride, t_start, modes, channels):
    """The make of modelPredModes' record: the POD basis of the case's target over the kept steps from t_start on (tmg_ops.pod_basis,
    fp64: not the hot path), handed to tmg_ops.EnsembleModes as fp32 tables, and the basis itself as results."""
    def make(mb, members, steps):
        import tmg_ops as ops
        B, C = mb.B, mb.C
        # the target's series at the kept steps from t_start on, back in normalised units, in fp64
        tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride].double()
        u, sd, mu = mb.u.double(), mb.out_std.double()[:C], mb.out_mu.double()[:C]
        xn = (tk / u.view(B, 1, C, 1, 1) - mu.view(1, 1, C, 1, 1)) / sd.view(1, 1, C, 1, 1)
        m, psi, lam, lam_total, _ = ops.pod_basis(xn, u * sd.view(1, C), channels, modes, name=name, case0=mb.case0)
        acc = ops.EnsembleModes(members, B, C, mb.H, mb.W, steps, mb.dev, mb.out_std, u=mb.u, channels=channels, mean=m, basis=psi)
        acc.lam = lam
        acc.extra = {"pod_energy": lam, "pod_energy_frac": lam / lam_total.unsqueeze(1), "pod_modes": psi.float(),
                     "pod_mean": tk.mean(1)[:, list(channels)].float()}
        return acc
    return make


def modelPredModes(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, modes=8, channels=(0, 1)):
    """modelPredStats plus the proper orthogonal decomposition (POD) of the target and every member's projection on it, still without
    forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.pod_basis / tmg_ops.EnsembleModes): do the members hold the
    reference's coherent structures (the cylinder's shedding pair and its limit cycle in the (a1, a2) plane, the step's shear-layer
    flapping mode) with the right energy and the right dynamics?  Spectra see energy per scale or frequency, never which spatial
    pattern carries it; a member can match them all and still place its shedding mode half a diameter off.  The target of kept step
    j is series step j * stride; a series that is too short raises.  Channel scales a = (u0, u0, u0^2) * out_std.  Same roll-outs as
    modelPredStats: under the same host RNG state the keys both return are identical; the basis draws nothing from the host RNG.

    Per case the basis comes from the target's fluctuations d_j = a (x_j - mean_j x_j) at the Tn kept steps from t_start on, with
    <f, g> = (1 / HW) sum_{c in channels} sum_p f_c g_c, by the method of snapshots: modes psi_k with <psi_k, psi_l> = delta_kl (RMS
    1 over the pixels) and energies lam_0 >= lam_1 >= .., each mode's sign fixed so that its temporal coefficient of largest
    magnitude is positive.  modes: 1..16 and at most Tn - 1; channels: distinct channels of one unit, default the velocity.  A
    target with fewer energetic modes than asked for (a constant one has none) raises.

    Returns modelPredStats' dict plus (CPU tensors; K = modes, Cg channels, S = samples, kept steps t_start..Tk-1 are the timed ones):
      coef [N, S, Tk, K], target_coef [N, Tk, K]     <d, psi_k> of every member and of the target, d about the TARGET's mean: plot
                                                     (coef[.., 0], coef[.., 1]) for the limit cycle
      fluct_energy [N, S, Tk], target_fluct_energy [N, Tk]   <d, d>
      time_mode_energy [N, S, K]                     mean_t coef^2: each member's energy in target mode k; compare with pod_energy
      time_mode_mean [N, S, K]                       mean_t coef: the member's mean-flow error as mode k sees it (the target's is 0)
      time_coef_cov [N, S, K, K]                     the covariance of the coefficients over time: the target's is diag(pod_energy);
                                                     off-diagonals show a member whose structures are rotated inside the subspace
      time_captured_frac, time_resid_energy [N, S]   sum_k time_mode_energy / mean_t fluct_energy, and the energy outside the K modes
      target_time_mode_energy, target_time_mode_mean [N, K], target_time_coef_cov [N, K, K], target_time_captured_frac,
      target_time_resid_energy [N]                   the same of the target through the same kernel (pod_energy, 0, diag(pod_energy),
                                                     sum_k pod_energy_frac up to rounding)
      mode_energy_ratio_mean, mode_energy_ratio_std [N, K]   mean / std over the members of time_mode_energy / pod_energy
      pod_energy, pod_energy_frac [N, K] float64     lam_k and lam_k / trace: the share of the target's fluctuation energy in mode k
      pod_modes [N, K, Cg, H, W], pod_mean [N, Cg, H, W]   the modes and the target's time mean, physical units."""
    import tmg_ops as ops
    channels = ops.pod_channels(channels, 3)
    acc = _Acc(_modes_factory("modelPredModes", stride, t_start, int(modes), channels), target=True)
    return _ensembleStats("modelPredModes", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _phase_factory(name, stride, t_start, modes, channels, pair, bins, min_amp):
    """The make of modelPredPhase's record: the POD basis of the case's target as _modes_factory builds it, the target's all-channel
    time mean over the same steps in normalised units, a tmg_ops.EnsembleModes and the tmg_ops.EnsemblePhase that drives it."""
    make_modes = _modes_factory(name, stride, t_start, modes, channels)

    def make(mb, members, steps):
        import tmg_ops as ops
        B, C = mb.B, mb.C
        em = make_modes(mb, members, steps)
        tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride].double()
        u, sd, mu = mb.u.double(), mb.out_std.double()[:C], mb.out_mu.double()[:C]
        xn = (tk / u.view(B, 1, C, 1, 1) - mu.view(1, 1, C, 1, 1)) / sd.view(1, 1, C, 1, 1)
        acc = ops.EnsemblePhase(members, B, C, mb.H, mb.W, steps, mb.dev, mb.out_std, u=mb.u, modes=em, pair=pair, bins=bins,
                                min_amp=min_amp, mean=xn.mean(1), lam=em.lam[:, list(pair)])
        acc.mean_phys = tk.mean(1)
        return acc
    return make


def modelPredPhase(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, modes=8, channels=(0, 1),
                   pair=(0, 1), bins=8, min_amp=0.25):
    """modelPredModes plus the phase averages of the members and of the target on the shedding phase, and the triple decomposition
    u = U + u~ + u' of Reynolds & Hussain (applied to cylinder wakes by Cantwell & Coles), still without forming modelPred's
    [samples, N, T, C, H, W] tensor (tmg_ops.EnsemblePhase around tmg_ops.EnsembleModes; the projection runs once): at a given phase
    of the shedding cycle, do the members put the vortices where the reference simulation puts them, and how much of the Reynolds
    stress that modelPredTurbulence reports is organised motion, how much turbulence?  Same roll-outs as modelPredModes: under the
    same host RNG state the keys both return are identical.

    The phase of a row (a member or the target at a kept step) is the angle of (coef_i / sqrt(pod_energy_i), coef_j /
    sqrt(pod_energy_j)), (i, j) = pair, cut into `bins` (4, 8, 16 or 32) equal sectors from the positive first axis; a row whose
    squared radius is under 2 min_amp^2 (the limit cycle's is 2) is skipped.  Fluctuations are taken about the TARGET's time mean
    over the kept steps from t_start on, in physical units, for all three channels.  modes >= max(pair) + 1.  Every raw sum is bitwise
    reproducible and independent of max_rows.

    Returns modelPredModes' dict plus (CPU tensors; NB = bins, n_k the rows of sector k over the kept steps t_start..Tk-1; fields are
    NaN where a sector is empty and empty sectors are left out of every aggregate):
      phase_bin [N, S, Tk], target_phase_bin [N, Tk] int32           the sector of every row at every kept step, -1 for a skipped row
      phase_count [N, NB], member_phase_count [N, S, NB], target_phase_count [N, NB], phase_skipped, target_phase_skipped [N]
      phase_mean [N, NB, C, H, W], phase_var [N, NB, C, H, W], phase_uv [N, NB, H, W]
                                      the phase average <u>_k over all members, the incoherent <u'_c u'_c>_k and <u'_0 u'_1>_k
      coh_var, incoh_var [N, C, H, W], coh_uv, incoh_uv [N, H, W]    sum_k w_k (M_k - M)^2 with w_k = n_k / sum n, M = sum_k w_k M_k, and
                                      sum_k w_k phase_var_k; their sum is the variance of the labelled rows (law of total variance)
      coh_tke_frac [N]                the coherent share of the velocity variance summed over the pixels
      target_phase_mean, .. target_coh_tke_frac                      the same of the target's rows through the same kernels
      phase_mean_rmse [N, NB, C]      RMS over the pixels of phase_mean - target_phase_mean
      coh_corr [N, NB]                pattern correlation of the ensemble's and the target's coherent velocity fields of sector k
      phase_speed [N, S], target_phase_speed [N]                     mean phase increment per kept step in radians, wrapped to
                                      (-pi, pi]; over 2 pi stride dt it is the shedding frequency
      phase_edges [NB + 1] float64    the sector angles."""
    import tmg_ops as ops
    channels = ops.pod_channels(channels, 3)
    if isinstance(modes, bool) or not isinstance(modes, numbers.Integral):
        raise ValueError("modelPredPhase: modes must be an integer, got %r" % (modes,))
    pair, bins, min_amp = ops.phase_args(pair, bins, min_amp, int(modes))
    acc = _Acc(_phase_factory("modelPredPhase", stride, t_start, int(modes), channels, pair, bins, min_amp), target=True, meta=("phase_edges",))
    return _ensembleStats("modelPredPhase", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _budget_factory(stride, t_start, grid, nu, rho, per_member):
    """The make of modelPredBudget's record: the target's time mean over the kept steps from t_start on, back in normalised units
    (fp64, as _phase_factory forms it), and the tmg_ops.EnsembleBudget about it."""
    def make(mb, members, steps):
        import tmg_ops as ops
        B, C = mb.B, mb.C
        tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride].double()
        u, sd, mu = mb.u.double(), mb.out_std.double()[:C], mb.out_mu.double()[:C]
        xn = (tk / u.view(B, 1, C, 1, 1) - mu.view(1, 1, C, 1, 1)) / sd.view(1, 1, C, 1, 1)
        return ops.EnsembleBudget(members, B, C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=grid, nu=nu, rho=rho,
                                  mean=xn.mean(1), per_member=per_member)
    return make


def modelPredBudget(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, nu=None, rho=1.0,
                    per_member=False):
    """modelPredStats plus the budget of the turbulent kinetic energy k = 1/2 <u'_i u'_i> of every member and of the target, still
    without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleBudget): are the members' Reynolds stresses right for
    the right reason, is the energy of the fluctuations produced, transported and dissipated where the reference simulation does
    it?  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.  nu=None reads args.nu;
    the grid is (args.dx along W, args.dy along H).  The target of kept step j is series step j * stride.

    Rows are the S members and the target.  Every timed step (kept steps t_start..Tk-1) adds, per row and pixel, 14 fp32 sums of the
    row's fluctuation d = (u0, u0, u0^2) out_std (y - m) about the TARGET's time mean m: d, the second and third velocity moments,
    the pressure-velocity products and the squared outputs of the un-scaled 3x3 first-derivative stencils of pc/ (zero padding):
    Sx f = (f[h-1,w+1] - f[h-1,w-1]) + 2 (f[h,w+1] - f[h,w-1]) + (f[h+1,w+1] - f[h+1,w-1]), Sy with h and w exchanged, d/dx =
    Sx / (8 dx), d/dy = Sy / (8 dy).  The state takes 14 * 4 bytes per element of [S + 1, N, HW]; it is bitwise reproducible and
    independent of max_rows.  From it, in fp64 on the device, the central moments of each row about its OWN time mean (uu, uv, vv,
    uuu, uuv, uvv, vvv, pu, pv, the gradient variances gx, gy), k = (uu + vv) / 2, the row's mean velocity (U, V) and the terms, signed
    as they enter dk/dt:
      conv  = -(U dk/dx + V dk/dy)                       convection by the mean flow
      prod  = -(uu dU/dx + uv (dU/dy + dV/dx) + vv dV/dy)  production
      turb  = -1/2 (d(uuu + uvv)/dx + d(uuv + vvv)/dy)   turbulent transport
      pres  = -(1 / rho) (d pu/dx + d pv/dy)             pressure diffusion
      visc  = nu (second differences of k / dx^2, dy^2)  viscous diffusion
      diss  = -nu (gx / (64 dx^2) + gy / (64 dy^2))      dissipation, a sink
      resid = the sum of the six: what a resolved two-dimensional budget over a finite window cannot close (-dk/dt of the window,
              sub-grid dissipation, out-of-plane terms).  It is a term of the budget, not an error.
    Every term is NaN on the one-pixel frame of the field, where the stencils have no neighbours.

    Returns modelPredStats' dict plus (CPU tensors):
      budget_mean, budget_std [N, 7, H, W]               mean / population std (ddof 0) over the members of each member's terms
      target_budget [N, 7, H, W]                         the target's terms through the same kernels
      stress_mean, stress_std, target_stress [N, 3, H, W]   the same of (uu, uv, vv), defined on the whole field
      member_budget [N, S, 7, H, W]                      every member's terms (per_member=True only)
      budget_terms                                       ("conv", "prod", "turb", "pres", "visc", "diss", "resid").
    Not supported: pixel boxes and region integrals, the 5x5 stencils, a budget of the individual Reynolds stresses, the
    phase-conditioned budget, non-finite members."""
    import tmg_ops as ops
    fl = ops.budget_args(3, 3, 3, (args.dx, args.dy), args.nu if nu is None else nu, rho)
    acc = _Acc(_budget_factory(stride, t_start, fl[:2], fl[2], fl[3], bool(per_member)), target=True, meta=("budget_terms",))
    return _ensembleStats("modelPredBudget", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _flux_factory(grid, widths, per_member):
    """The make of modelPredFlux's record: the tmg_ops.EnsembleFlux of one mini-batch (its constructor checks the widths against the
    field before it touches the device)."""
    def make(mb, members, steps):
        import tmg_ops as ops
        return ops.EnsembleFlux(members, mb.B, mb.C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=grid, widths=widths,
                                per_member=per_member)
    return make


def modelPredFlux(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, widths=None, per_member=False):
    """modelPredStats plus the scale-to-scale energy flux and the sub-filter stresses of every member and of the target, still
    without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleFlux): per location, does energy go from the large
    scales to the small ones, at what rate, and how often does it go backwards?  The coarse-graining (filtering) analysis of Germano,
    Eyink and Aluie, which needs no homogeneity: for a box filter of width l, tau_ij(l) = bar(u_i u_j) - bar(u_i) bar(u_j) is the
    sub-filter stress and Pi_l(x, t) = -tau_ij d bar(u_i) / dx_j the local flux across l, positive for a forward cascade, negative for
    backscatter.  Same roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.  The grid is
    (args.dx along W, args.dy along H).

    widths: at most 8 odd box widths in pixels, strictly increasing, each in 3 .. 33 (None: (3, 5, 9, 17, 33) without those over
    min(H, W) - 2; an explicit width over that is a ValueError).  Rows are the S members and the target.  The filtered field is
    (u0, u0) out_std y (out_mu never enters: tau and the gradients of bar(u) are exactly invariant to a constant velocity).  Every
    timed step (kept steps t_start..Tk-1) adds, per row, width and valid pixel, 7 fp32 sums of un-normalised quantities: with the box
    sums Sg over the w x w box (N = w^2; separable, added from the centre outwards, no running window and no summed-area table),
    Q_ij = N Sg_ij - Sg_i Sg_j = N^2 tau_ij, A = Q_uu Sx Sg_u + Q_uv Sx Sg_v, B = Q_uv Sy Sg_u + Q_vv Sy Sg_v (the un-scaled 3x3 stencils of
    pc/ on the box sums of the eight neighbours) and Pi_s = -(A / (8 dx N^3) + B / (8 dy N^3)), the sums of A, B, Pi_s^2, [Pi_s < 0],
    Q_uu, Q_uv, Q_vv.  The state takes 28 L bytes per element of [S + 1, N, HW] for L widths; it is bitwise reproducible and
    independent of max_rows.  A pixel is valid for a width when the box and the ring of the stencils lie inside the field
    (r + 1 <= h <= H - 2 - r, r = w // 2, and the same in w); every output is NaN outside.

    Returns modelPredStats' dict plus (CPU tensors):
      flux_mean, flux_std, target_flux [N, L, H, W]         mean / population std (ddof 0) over the members of each member's
                                                            time-mean Pi, and the target's through the same kernels
      flux_tstd_mean, target_flux_tstd [N, L, H, W]         the same of the temporal std of Pi_s
      backscatter_mean, backscatter_std, target_backscatter [N, L, H, W]   ... of the fraction of timed steps with Pi_s < 0
      sgs_mean, sgs_std, target_sgs [N, L, 3, H, W]         ... of the time-mean tau (uu, uv, vv)
      member_flux [N, S, L, H, W]                           every member's Pi (per_member=True only)
      flux_curve, sgs_energy_curve [N, S + 1, L]            per row, the target last: the mean over the width's valid region of Pi
                                                            and of (tau_uu + tau_vv) / 2
      flux_widths [L], flux_lengths [L, 2]                  the widths in pixels and as lengths (w dx, w dy).
    Not supported: Gaussian or spectral filters, the boundary strip (one-sided filters), widths over 33, more than 8 widths, pixel
    boxes, the pressure and the three-dimensional terms, a per-step flux series, non-finite members."""
    import tmg_ops as ops
    ws, dx, dy = ops.flux_args(widths, 3, None, None, (args.dx, args.dy))
    acc = _Acc(_flux_factory((dx, dy), None if widths is None else ws, bool(per_member)), target=True, meta=("flux_widths", "flux_lengths"))
    return _ensembleStats("modelPredFlux", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _transport_factory(grid, step_dt, seed_stride, seed_origin, substeps, boxes, per_member, keep_paths):
    """The make of modelPredTransport's record: the tmg_ops.EnsembleTransport of one mini-batch (its constructor checks the seeds and
    the boxes against the field before it touches the device)."""
    def make(mb, members, steps):
        import tmg_ops as ops
        return ops.EnsembleTransport(members, mb.B, mb.C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=grid,
                                     step_dt=step_dt, seed_stride=seed_stride, seed_origin=seed_origin, substeps=substeps, boxes=boxes,
                                     per_member=per_member, keep_paths=keep_paths)
    return make


def modelPredTransport(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, dt=None, seed_stride=(2, 2),
                       seed_origin=None, substeps=1, boxes=(), per_member=False, keep_paths=False):
    """modelPredStats plus the Lagrangian transport of every member and of the target, still without forming modelPred's
    [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleTransport): what does the recirculation trap and for how long, where do the shear
    layer and the wake stretch and fold material, does a parcel released at a point end up where the reference simulation puts it?
    Every other diagnostic here looks at fixed pixels; a pathline integrates the velocity along a moving point, so a small phase or
    convection-speed error accumulates instead of averaging out.  Same roll-outs as modelPredStats: under the same host RNG state
    the keys both return are identical.  The grid is (args.dx along W, args.dy along H); dt, the time between two model steps, is
    required (a kept step lasts step_dt = stride * dt); the target of kept step j is series step j * stride.

    Rows are the S members and the target.  Positions are in pixels, px along W and py along H, pixel (h, w) at (w, h); a position is
    inside when 0 <= px <= W - 1 and 0 <= py <= H - 1.  The velocity (u0, u0) (out_std y + out_mu) step_dt / (dx, dy) in pixels per
    kept step is bilinear in space and linear in time between two kept steps.  seed_stride = (sy, sx) and seed_origin = (oy, ox)
    (None: (sy // 2, sx // 2)) place the seeds on the pixels (oy + i sy, ox + j sx) inside the field, a lattice [Gh, Gw].  The first
    timed step (kept step t_start) seeds; each of the Tn - 1 later ones advects every particle by `substeps` (1 .. 8) Heun steps, over
    T_int = (Tn - 1) step_dt in all; Tn = Tk - t_start >= 2.  A particle whose predictor or corrector leaves the field dies: it keeps
    its last inside position and the index of that advection.  boxes: at most 4 pixel boxes (h0, h1, w0, w1), inclusive; at every
    timed step an alive particle inside a box adds one step_dt to its residence time there.  The state takes 12 + 4 R bytes per
    particle and 8 bytes per pixel of every row and case; it is bitwise reproducible and independent of max_rows.

    Returns modelPredStats' dict plus (CPU tensors; mean / population std (ddof 0) over the members valid at the node, NaN where
    none is):
      ftle_mean, ftle_std, target_ftle [N, Gh, Gw]   the forward finite-time Lyapunov exponent ln(lam) / (2 T_int), lam the largest
                                                     eigenvalue of F^T F, F the central differences of the final physical positions
                                                     over the seeds' physical spacing; valid where the node and its four lattice
                                                     neighbours are alive in that row
      ftle_count [N, Gh, Gw] int32                   the members valid there
      disp_mean, disp_std, target_disp [N, 2, Gh, Gw]   final minus seed position in physical units, over the alive members
      alive_frac, target_alive [N, Gh, Gw]           the share of the members still alive; 1 / 0 for the target
      res_time_mean, res_time_std, target_res_time [N, R, Gh, Gw]   the residence times, all members (only with boxes)
      end_err_mean [N, Gh, Gw]                       the mean distance of the members' endpoints to the target's, over the members
                                                     alive together with the target
      end_spread [N, Gh, Gw]                         sqrt(var_x + var_y) of the alive members' endpoints; read beside end_err_mean
      member_ftle [N, S, Gh, Gw], member_end [N, S, 2, Gh, Gw] (pixels), member_exit [N, S, Gh, Gw] int32   (per_member=True only)
      paths [N, S + 1, Tn, 2, Gh, Gw]                the positions in pixels after every timed step (keep_paths=True only)
      transport_seeds [Gh, Gw, 2] (h, w), transport_boxes, transport_time = T_int.
    Not supported: backward-time (attracting) FTLE, sub-pixel or non-lattice seeds, re-seeding of dead particles, RK4, periodic
    domains, a per-step FTLE series, non-finite members (they only kill the particles that touch them)."""
    import tmg_ops as ops
    if dt is None:
        raise ValueError("modelPredTransport needs dt, the time between two model steps: a pathline is an integral over time")
    step_dt = float(stride) * float(dt)
    _, n, bx, dx, dy, step_dt = ops.transport_args(seed_stride, seed_origin, substeps, boxes, 3, None, None, (args.dx, args.dy), step_dt)
    nkeep = tmax // stride
    if nkeep >= 1 and 0 <= t_start < nkeep and nkeep - t_start < 2:            # (else _ensembleStats words the error)
        raise ValueError("modelPredTransport needs at least 2 kept steps from t_start on (one advection), got %d (tmax=%d, stride=%d, "
                         "t_start=%d)" % (nkeep - t_start, tmax, stride, t_start))
    acc = _Acc(_transport_factory((dx, dy), step_dt, tuple(seed_stride), seed_origin, n, bx, bool(per_member), bool(keep_paths)),
               target=True, meta=("transport_seeds", "transport_boxes", "transport_time"))
    return _ensembleStats("modelPredTransport", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _vortex_factory(name, grid, stride, t_start, kw):
    """The make of modelPredVortices' record.  kw: the keywords of tmg_ops.EnsembleVortices, with threshold / qscale None for the
    defaults of the case's target series over the kept steps from t_start on (tmg_ops.vortex_defaults, plain torch in fp64); arrays
    per case are cut to the mini-batch."""
    def make(mb, members, steps):
        import tmg_ops as ops
        kw2 = dict(kw)
        for key in ("threshold", "qscale", "circ_range"):
            v = kw2[key]
            if v is not None and torch.as_tensor(v).dim() == (2 if key == "circ_range" else 1):
                kw2[key] = torch.as_tensor(v)[mb.case0:mb.case0 + mb.B]
        if kw2["threshold"] is None or kw2["qscale"] is None:
            tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride]
            try:
                thr, qs = ops.vortex_defaults(tk, grid)
            except ValueError as e:
                raise ValueError("%s: cases from %d on: %s" % (name, mb.case0, e))
            kw2["threshold"] = thr if kw2["threshold"] is None else kw2["threshold"]
            kw2["qscale"] = qs if kw2["qscale"] is None else kw2["qscale"]
        return ops.EnsembleVortices(members, mb.B, mb.C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=grid, **kw2)
    return make


def modelPredVortices(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, threshold=None, qscale=None,
                      min_area=4, max_vortices=64, circ_bins=16, circ_range=None, per_member=False):
    """modelPredStats plus the vortex census of every member and of the target, still without forming modelPred's
    [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleVortices): how many vortices are in the field, how big and how strong are they,
    where do they live, and are the reference's vortices present in the members at the right place?  Every other diagnostic here is a
    statistic of fields at fixed pixels or of particles; a member can match them all and still shed vortices half as strong and
    twice as many, or break every vortex into speckle with the right vorticity PDF.  The Okubo-Weiss / Q-criterion census (McWilliams
    1990; the 0.2 sigma threshold of Isern-Fontanet et al.) and the object-based verification of meteorology (SAL, MODE).  Same
    roll-outs as modelPredStats: under the same host RNG state the keys both return are identical.  The grid is (args.dx along W,
    args.dy along H); the target of kept step j is series step j * stride.

    Rows are the S members and the target; the timed steps are the kept steps t_start..Tk-1 (Tn of them).  A pixel that is not on the
    field's one-pixel frame belongs to a vortex core of sign(w) when ow = w^2 - sn^2 - ss^2 > threshold (w the vorticity, sn, ss the
    normal and shear strain, all by the 3x3 stencils of pc/ in fp32); a vortex is a maximal 4-connected set of core pixels of one sign.
    threshold: physical 1/s^2, one number or [N]; None: per case 0.2 times the population std of the target's ow over the interior
    pixels and the timed steps (a constant target raises).  qscale: the power of two that turns w into the fixed-point integers q the
    measures sum, one or [N]; None: 2^(20 - ceil(log2(max |w| of the target))).  Pixels with |w qscale| > 2^31 or a NaN criterion are
    counted in vortex_rejected, never silently dropped; non-finite members become background.  min_area (>= 1): smaller vortices are
    neither listed nor counted.  max_vortices (<= 256): the slots K of a table, filled in increasing order of the vortex' first pixel;
    vortex_found counts past K and vortex_truncated reports it.  circ_bins (<= 32) bins of |circulation| over circ_range ((lo, hi),
    [N, 2], or None: [0, 1.25 max |G|] of the case's target table).  The state takes 64 K bytes per row, case and timed step and 16
    bytes per pixel and case; it holds integers only and is bitwise reproducible and independent of max_rows.

    Returns modelPredStats' dict plus the keys of tmg_ops.EnsembleVortices.finalize (CPU tensors, B = N), and vortex_args, the
    dict (min_area, max_vortices, circ_bins).
    Not supported: 8-connectivity, tracking identities across steps (the tables are returned for that), lambda-2 or swirling
    strength, pixel boxes, more than 256 vortices per field, periodic domains, fields over 512 per side."""
    import tmg_ops as ops
    ops.vortex_args(threshold, qscale, min_area, max_vortices, circ_bins, circ_range, 3, None, None, (args.dx, args.dy))
    kw = dict(threshold=threshold, qscale=qscale, min_area=min_area, max_vortices=max_vortices, circ_bins=circ_bins, circ_range=circ_range,
              per_member=bool(per_member))
    acc = _Acc(_vortex_factory("modelPredVortices", (float(args.dx), float(args.dy)), stride, t_start, kw), target=True,
               meta=("vortex_args",))
    return _ensembleStats("modelPredVortices", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def modelPredSpod(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, bins=None, modes=4, channels=(0, 1),
                  window="hann", loo=True, dt=None):
    """modelPredStats plus the spectral POD (SPOD; Towne, Schmidt & Colonius 2018) of the members over the kept steps t_start..Tk-1
    (Tn = Tk - t_start >= 2 of them), still without forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleSpod): per
    frequency bin the structures that are coherent in space AND time among the members, how much of the fluctuation energy at that
    frequency the leading ones hold, and whether the target's Fourier coefficient at that bin lies in the same subspace with the same
    energy.  A POD mode (modelPredModes) mixes every frequency that shares a spatial pattern and modelPredPhase conditions on one
    frequency; the cylinder array sheds at several, and the step's shear layer flaps and rolls up at different ones.  SPOD needs many
    independent realisations of one stationary process: the members stand where Welch's blocks stand.  The target of kept step j is
    series step j * stride; a series that is too short raises.  Channel scales (u0, u0, u0^2).  Same roll-outs as modelPredStats: under
    the same host RNG state the keys both return are identical; no option draws from the host RNG, and the loader is iterated once.

    X_m(c, p) at bin k is modelPredTimeSpectra's Fourier coefficient of member m (row S: the target), <f, g> = (1 / HW) sum_{c in
    channels} sum_p conj(f) g, kappa_k = c_k / Tn^2.  bins: None for 1..min(16, Tn // 2), else 1 to 16 strictly increasing bins in
    1..Tn // 2; modes: J in 1..8; channels: distinct channels of one unit, default the velocity; samples <= 255; loo: the leave-one-out
    yardstick, S eigendecompositions per case and bin on the host.

    Returns modelPredStats' dict plus (CPU tensors; NB bins, J modes, Cg channels, S = samples, R = S + 1):
      csd_raw [N, NB, 2, R, R]              the device's sums: raw0 + i raw1 = M[m, n] = sum conj(X_m) X_n, the target last
      csd [N, NB, R, R] complex128          M / HW: form coherences or other estimators from it
      spod_energy [N, NB, J], spod_total [N, NB], spod_energy_frac [N, NB, J], captured [N, NB]
                                            the eigenvalues lambda_j of A = kappa M[:S, :S] / (S HW), descending; trace A, which is the
                                            field mean over `channels` of psd_mean at the bin; their ratio and its sum over the J modes
      member_mode_energy [N, NB, S, J]      S lambda_j |Theta_mj|^2: each member's share of mode j
      spod_modes [N, NB, J, 2, Cg, H, W]    real and imaginary part of Phi_j, <Phi_i, Phi_j> = delta_ij, from the members alone
      target_coef [N, NB, J] complex128, target_mode_energy [N, NB, J], target_energy, target_captured [N, NB]
                                            b_j = <Phi_j, X_S>, kappa |b_j|^2 (for a realisation of the members' own process its
                                            expectation is lambda_j), kappa <X_S, X_S> and the share of it in the J modes
      loo_captured [N, NB, S], target_captured_rank [N, NB]   (loo) the share of member m's energy in the leading modes of the OTHER
                                            members - the fair yardstick for target_captured, captured being in-sample and
                                            optimistic - and the number of members strictly under the target; NaN for samples = 1
      spod_noise_floor [N, NB]              eigenvalues at or below it cannot be told from fp32 rounding: their modes, target_coef
                                            and target_mode_energy are NaN and they are left out of target_captured
      spod_bins [NB] int64, spod_freq [NB] float64   the bins and k / Tn, cycles per kept step, when dt is None; else k / (Tn stride dt)."""
    if window not in ("hann", None):
        raise ValueError("window must be 'hann' or None, got %r" % (window,))
    step_dt = 1.0 if dt is None else float(stride) * float(dt)
    if not (math.isfinite(step_dt) and step_dt > 0):
        raise ValueError("dt must be a positive finite time between two model steps, got %r" % (dt,))
    import tmg_ops as ops
    nkeep = tmax // stride
    if nkeep - t_start >= 2:                                                  # (else _ensembleStats words the error)
        bins, modes, channels = ops.spod_args(bins, modes, channels, nkeep - t_start, 3)
    acc = _Acc(lambda mb, S, T: ops.EnsembleSpod(S, mb.B, mb.C, mb.H, mb.W, T, mb.dev, mb.out_mu, mb.out_std, u=mb.u, bins=bins, modes=modes,
                                                 channels=channels, window=window, dt=step_dt, loo=loo),
               target=True, window=True, meta=("spod_bins", "spod_freq"))
    return _ensembleStats("modelPredSpod", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])


def _corr_factory(stride, t_start, grid, probes, pairs, lags, per_member, step_dt):
    """The make of modelPredCorrelation's record: the target's time mean over the kept steps from t_start on, back in normalised
    units (fp64, as _budget_factory forms it), and the tmg_ops.EnsembleCorrelation about it."""
    def make(mb, members, steps):
        import tmg_ops as ops
        B, C = mb.B, mb.C
        tk = mb.tgt[:, t_start * stride:(steps - 1) * stride + 1:stride].double()
        u, sd, mu = mb.u.double(), mb.out_std.double()[:C], mb.out_mu.double()[:C]
        xn = (tk / u.view(B, 1, C, 1, 1) - mu.view(1, 1, C, 1, 1)) / sd.view(1, 1, C, 1, 1)
        return ops.EnsembleCorrelation(members, B, C, mb.H, mb.W, steps, mb.dev, mb.out_mu, mb.out_std, u=mb.u, grid=grid, probes=probes,
                                       pairs=pairs, lags=lags, mean=xn.mean(1), per_member=per_member, step_dt=step_dt)
    return make


def modelPredCorrelation(args, model, testing_loader, log, samples=1, stride=1, tmax=1, t_start=0, max_rows=64, probes=None,
                         pairs=((0, 0), (1, 1)), lags=(0, 1, 2, 4), per_member=False, dt=None):
    """modelPredStats plus the two-point space-time correlations of every member and of the target about probe points, still without
    forming modelPred's [samples, N, T, C, H, W] tensor (tmg_ops.EnsembleCorrelation):

      R(x0; x, tau) = < u'_i(x0, t) u'_j(x, t + tau) >

    On an inhomogeneous domain it is the one statistic that shows the size and shape of the structure that passes a chosen point (the
    integral length scales), where that structure is tau later, and from that displacement the convection velocity: a surrogate that
    gets it wrong sheds vortices of the right energy at the wrong speed.  Same roll-outs as modelPredStats: under the same host RNG
    state the keys both return are identical.  The grid is (args.dx along W, args.dy along H).  The target of kept step j is series
    step j * stride.  dt=None counts time in kept steps, else a kept step lasts stride * dt.

    Rows are the S members and the target.  A row's fluctuation is d = (u0, u0, u0^2) out_std (y - m) about the TARGET's time mean m
    over the kept steps from t_start on.  probes: at most 8 pixels (h, w) inside the field, duplicates allowed (None: (H // 2, W // 4),
    (H // 2, W // 2), (H // 2, 3 W // 4)); pairs: at most 4 pairs (ci, cj) of channels in 0..2, ci taken at the probe and cj in the
    field; lags: at most 8 strictly increasing integers in kept steps, the first 0, the largest <= 64.  t = 0, 1, .. numbers the timed
    steps (kept steps t_start..Tk-1); after T of them lag l has n_l = T - tau_l pairs (probe at t - tau_l, field at t).  The state
    holds the rows' d at the probes at every timed step and, with J the distinct cj, NPL = P Q L + 2 |J| L fp32 planes per row: the
    sums of d_ci(x0, t - tau) d_cj(x, t), of d_j(x, t) and of d_j(x, t)^2 over t >= tau_l.  It takes NPL * 4 bytes per element of
    [S + 1, N, HW], 40 planes or 160 bytes at the defaults; it is bitwise reproducible and independent of max_rows.  From it, in fp64
    on the device, cov = X / n - pm mf and the Pearson coefficient rho = cov / sqrt(pv vf) of the n = n_l paired samples (pm, pv the
    mean and population variance of the probe's first n values, mf, vf those of the field's last n), NaN where pv or vf is not
    positive and for lags with n_l < 2.  |rho| <= 1 up to rounding, and it is 1 at the displaced point of a frozen pattern convected
    by whole pixels.

    Returns modelPredStats' dict plus (CPU tensors; P probes, Q pairs, L lags, S = samples):
      tp_cov_mean, tp_cov_std, tp_rho_mean, tp_rho_std [N, P, Q, L, H, W]   mean / population std (ddof 0) over the members
      target_tp_cov, target_tp_rho [N, P, Q, L, H, W]                      the target through the same kernels
      member_tp_rho [N, S, P, Q, L, H, W]                                  every member's rho (per_member=True only)
      tp_line_x [N, S + 1, P, Q, L, W], tp_line_y [N, S + 1, P, Q, L, H]    rho of every row (the target last) on the probe's field
                                                                           row and field column
      tp_len [N, S + 1, P, Q, 4]        integral lengths from the lag-0 lines in the directions (+x, -x, +y, -y): with rho_i the value
                                        i pixels from the probe and k the first i >= 1 that is outside the field or has rho_i <= 0 or
                                        NaN, len = step (rho_0 / 2 + sum_{i=1}^{k-1} rho_i), the trapezoid to a zero at k, step = dx
                                        or dy; tp_len_mean, tp_len_std [N, P, Q, 4] over the members, target_tp_len [N, P, Q, 4]
      tp_shift [N, S + 1, P, Q, L, 2]   the displacement (along x, along y) in pixels of the maximum of each line from the probe,
                                        refined by the parabola through the peak and its two neighbours when the peak is interior
                                        and all three are finite; NaN for an all-NaN line
      tp_speed [N, S + 1, P, Q, L, 2]   tp_shift * (dx, dy) / (tau_l step_dt), NaN at tau = 0; tp_speed_mean, tp_speed_std
                                        [N, P, Q, L, 2] over the members, target_tp_speed [N, P, Q, L, 2]
      tp_probes, tp_pairs, tp_lags      the arguments as used.
    Not supported: probes off the pixel grid, pixel-box averages of probes, negative lags (exchange ci and cj), more than 8 probes,
    4 pairs or 8 lags or a lag over 64, the full two-point tensor, non-finite members."""
    step_dt = 1.0 if dt is None else float(stride) * float(dt)
    if not (math.isfinite(step_dt) and step_dt > 0):
        raise ValueError("dt must be a positive finite time between two model steps, got %r" % (dt,))
    import tmg_ops as ops
    if probes is not None:                                                    # (the default probes need the field's size)
        ops.corr_args(probes, pairs, lags, 3, 1 << 30, 1 << 30)
    else:
        ops.corr_args(((0, 0),), pairs, lags, 3, 1, 1)
    acc = _Acc(_corr_factory(stride, t_start, (args.dx, args.dy), probes, pairs, lags, bool(per_member), step_dt), target=True,
               meta=("tp_probes", "tp_pairs", "tp_lags"))
    return _ensembleStats("modelPredCorrelation", args, model, testing_loader, log, samples, stride, tmax, t_start, max_rows, False, [acc])
