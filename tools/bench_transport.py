"""Cost of the Lagrangian transport: utils.modelPredTransport beside utils.modelPredStats (unchanged by it) at the cylinder test shape
of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 kept steps) for 4 / 8 / 32 members.

  the time step: one modelPredStats run first; dt is chosen so that the mean speed of the ensemble mean is half a pixel per kept step
  (the kernel's cost depends on how many particles are still alive; the share alive at the end is recorded)
  per member count S: one short warm-up run of each function, then --reps (at least 3) timed runs alternating the two, each window
  closed by torch.cuda.synchronize(); median and best seconds, the ratio transport / stats, and the spread (max / min) of the runs of
  each, which is the run-to-run noise the ratio has to be read against
  then, per S, one modelPredTransport run with a device event pair around every call of tmg_ens_lagr_advect, tmg_ens_lagr_store and
  tmg_ens_lagr_finalize at seed strides 2 and 1 and at substeps 1 and 4: calls, summed event time, microseconds per kept step.  An
  event pair also holds the launch gaps.
  then tmg_ens_lagr_advect alone on one random chunk of min(S, max_rows / B) members beside a torch.nn.functional.grid_sample
  composition of one Heun step (the same four bilinear samples of two planes, the time interpolation, the inside tests), and
  tmg_ens_lagr_finalize on the state of S members beside a torch fp64 composition of the same formulas, alternating call by call.

Writes profiles/transport_bench.json."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-turbulence_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_ensemble as BE        # noqa: E402  (the model, the loader and the yardstick are that tool's)
import bench_ensemble_turb as BT   # noqa: E402  (the grid)
import bench_quant as BQ           # noqa: E402  (the event wrapper)

FUNCS = ("stats", "transport")
KERNELS = ("ens_lagr_advect", "ens_lagr_store", "ens_lagr_finalize")
CFG = {"dt": 1.0, "seed_stride": (2, 2), "substeps": 1}


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=BT.GRID[0], dy=BT.GRID[1])
    kw = dict(samples=S, stride=1, tmax=steps, max_rows=max_rows)
    if which == "transport":
        return utils.modelPredTransport(args, model, loader, BE.LOG, dt=CFG["dt"], seed_stride=CFG["seed_stride"], substeps=CFG["substeps"],
                                        boxes=((64, 191, 64, 191),), **kw)
    return utils.modelPredStats(args, model, loader, BE.LOG, **kw)


def timed(which, model, loader, S, steps, max_rows):
    import time
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    alive = float(out["alive_frac"].mean()) if which == "transport" else None
    del out
    return dt, alive


def event_run(model, loader, S, steps, max_rows):
    saved = BQ.run
    BQ.run = run
    try:
        return BQ.event_run("transport", KERNELS, model, loader, S, steps, max_rows)
    finally:
        BQ.run = saved


def _events(fn, reps):
    import torch
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return ms


def torch_heun(prev, cur, pos, alive, Hh, Ww):
    """One Heun step (substeps = 1) as a torch.nn.functional.grid_sample composition.  prev, cur [N, 2, H, W] velocity planes in
    pixels per step, pos [N, 2, P] (px, py), alive [N, P] -> (pos, alive)."""
    import torch
    import torch.nn.functional as F
    scale = torch.tensor([2.0 / (Ww - 1), 2.0 / (Hh - 1)], device=pos.device).view(1, 2, 1)

    def vel(x, s):
        g = (x * scale - 1.0).permute(0, 2, 1).unsqueeze(1)                  # [N, 1, P, 2] in (x, y)
        v0 = F.grid_sample(prev, g, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]
        v1 = F.grid_sample(cur, g, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]
        return v0 + s * (v1 - v0)

    def inside(x):
        return (x[:, 0] >= 0) & (x[:, 0] <= Ww - 1) & (x[:, 1] >= 0) & (x[:, 1] <= Hh - 1)

    k1 = vel(pos, 0.0)
    xs = pos + k1
    ok = alive & inside(xs)
    k2 = vel(xs, 1.0)
    xn = pos + 0.5 * (k1 + k2)
    ok = ok & inside(xn)
    return torch.where(ok.unsqueeze(1), xn, pos), ok


def torch_finalize(pos, ex, res, fl, lattice):
    """The formulas of tmg_ens_lagr_finalize as a torch fp64 composition on the device -> the fields in LAGR_OUTS order (no member
    arrays), fp32."""
    import torch
    dx, dy, step_dt, T_int = fl
    Gh, Gw, oy, ox, sy, sx = lattice
    R, B = pos.shape[:2]
    S = R - 1
    nan = float("nan")
    p = pos.double().view(R, B, 2, Gh, Gw)
    alive = (ex < 0).view(R, B, Gh, Gw)
    X, Y = p[:, :, 0] * dx, p[:, :, 1] * dy
    c = lambda f, i, j: f[..., 1 + i:Gh - 1 + i, 1 + j:Gw - 1 + j]          # noqa: E731
    valid = torch.zeros_like(alive)
    valid[..., 1:-1, 1:-1] = c(alive, 0, 0) & c(alive, 0, 1) & c(alive, 0, -1) & c(alive, 1, 0) & c(alive, -1, 0)
    F11, F21 = (c(X, 0, 1) - c(X, 0, -1)) / (2 * sx * dx), (c(Y, 0, 1) - c(Y, 0, -1)) / (2 * sx * dx)
    F12, F22 = (c(X, 1, 0) - c(X, -1, 0)) / (2 * sy * dy), (c(Y, 1, 0) - c(Y, -1, 0)) / (2 * sy * dy)
    C11, C12, C22 = F11 * F11 + F21 * F21, F11 * F12 + F21 * F22, F12 * F12 + F22 * F22
    hd = 0.5 * (C11 - C22)
    ftle = torch.full_like(X, nan)
    ftle[..., 1:-1, 1:-1] = torch.log(0.5 * (C11 + C22) + torch.sqrt(hd * hd + C12 * C12)) / (2 * T_int)
    ftle = torch.where(valid, ftle, torch.full_like(ftle, nan))

    def stats(v, m):
        """Mean and population std over the members where m, NaN where none."""
        n = m.sum(0).double()
        mean = torch.where(m, v, torch.zeros_like(v)).sum(0) / n
        var = torch.where(m, (v - mean) ** 2, torch.zeros_like(v)).sum(0) / n
        return mean, var

    xs0 = (ox + sx * torch.arange(Gw, device=pos.device)).double().view(1, Gw)
    ys0 = (oy + sy * torch.arange(Gh, device=pos.device)).double().view(Gh, 1)
    dX, dY = (p[:, :, 0] - xs0) * dx, (p[:, :, 1] - ys0) * dy
    fm, fv = stats(ftle[:S], valid[:S])
    dxm, dxv = stats(dX[:S], alive[:S])
    dym, dyv = stats(dY[:S], alive[:S])
    _, exv = stats(X[:S], alive[:S])
    _, eyv = stats(Y[:S], alive[:S])
    both = alive[:S] & alive[S:]
    em, _ = stats(torch.sqrt((X[:S] - X[S:]) ** 2 + (Y[:S] - Y[S:]) ** 2), both)
    rt = res.double().view(R, B, -1, Gh, Gw) * step_dt
    f = lambda v: v.float()                                                  # noqa: E731
    nanw = lambda v, m: torch.where(m, v, torch.full_like(v, nan))          # noqa: E731
    return [f(fm), f(fv.sqrt()), f(ftle[S]), valid[:S].sum(0).int(), f(torch.stack([dxm, dym], 1)), f(torch.stack([dxv, dyv], 1).sqrt()),
            f(torch.stack([nanw(dX[S], alive[S]), nanw(dY[S], alive[S])], 1)), f(alive[:S].sum(0).double() / S), f(alive[S].double()),
            f(rt[:S].mean(0)), f(rt[:S].std(0, unbiased=False)), f(rt[S]), f(em), f((exv + eyv).sqrt())]


def direct(S, B, Hh, Ww, max_rows, reps, stride, dt_px):
    """The advect kernel on one chunk alone beside the grid_sample composition, and the finalize kernel beside the torch fp64
    composition -> dict.  dt_px: the size of the random velocities in pixels per step."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(S)
    k = max(1, min(S, max_rows // B))
    HW = Hh * Ww
    lattice, n, boxes, dx, dy, step_dt = ops.transport_args(stride, None, 1, ((64, 191, 64, 191),), 3, Hh, Ww, BT.GRID, 1.0)
    P = lattice[0] * lattice[1]
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)             # noqa: E731
    smooth = torch.nn.functional.interpolate(rnd((S + 1) * B, 3, Hh // 16, Ww // 16), size=(Hh, Ww), mode="bilinear")
    rows = (dt_px * smooth).permute(0, 2, 3, 1).contiguous()                 # NHWC as sampleEnsemble leaves it, rows member-major
    rows2 = (rows + 0.1 * dt_px * rnd((S + 1) * B, 1, 1, 3)).contiguous()
    a, o = torch.ones(B, 2, device="cuda"), torch.zeros(B, 2, device="cuda")
    pos = torch.empty(S + 1, B, 2, P, device="cuda")
    ex = torch.empty(S + 1, B, P, device="cuda", dtype=torch.int32)
    res = torch.empty(S + 1, B, 1, P, device="cuda", dtype=torch.int32)
    prev = torch.empty(S + 1, B, 2, HW, device="cuda")

    def step(src, t):
        for m0 in range(0, S + 1, k):
            kk = min(k, S + 1 - m0)
            chunk = src[m0 * B:(m0 + kk) * B]
            H.ens_lagr_advect(chunk, a, o, prev, pos, ex, res, lattice, boxes, 1, kk, m0, t)
            H.ens_lagr_store(chunk, a, o, prev, kk, m0)

    step(rows, 0)
    step(rows2, 1)
    chunk = rows[:k * B]
    keep = (pos.clone(), ex.clone(), res.clone())

    def advect():
        H.ens_lagr_advect(chunk, a, o, prev, pos, ex, res, lattice, boxes, 1, k, 0, 2)

    ms = []
    for i in range(reps + 2):                                                # every timed call starts from the same state
        pos.copy_(keep[0]), ex.copy_(keep[1]), res.copy_(keep[2])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        advect()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    pos.copy_(keep[0]), ex.copy_(keep[1]), res.copy_(keep[2])
    pv = prev[:k].reshape(k * B, 2, Hh, Ww)
    cur = chunk.permute(0, 3, 1, 2)[:, :2].contiguous()
    p0, al = pos[:k].reshape(k * B, 2, P), (ex[:k] < 0).reshape(k * B, P)
    tms = _events(lambda: torch_heun(pv, cur, p0, al, Hh, Ww), reps)
    med, tmed = statistics.median(ms), statistics.median(tms)
    out = {"samples": S, "seed_stride": list(stride), "chunk_members": k, "rows": k * B, "particles_per_row": P,
           "plan": H.ens_lagr_plan(S, B, Hh, Ww, P), "alive_share": float(al.float().mean()),
           "advect": {"event_ms": ms, "event_ms_median": med, "event_ms_min": min(ms), "event_ms_max": max(ms),
                      "particle_steps_per_s": k * B * P / (med * 1e-3),
                      "gather_bytes_per_s": k * B * P * float(al.float().mean()) * 32 * 4 / (med * 1e-3),
                      "grid_sample_ms": tms, "grid_sample_ms_median": tmed, "grid_sample_over_kernel": tmed / med}}
    fl = (dx, dy, 1.0, 2.0)
    shapes = {"ftle_count": (B, P), "disp_mean": (B, 2, P), "disp_std": (B, 2, P), "target_disp": (B, 2, P), "res_time_mean": (B, 1, P),
              "res_time_std": (B, 1, P), "target_res_time": (B, 1, P)}
    outs = [None if nm.startswith("member_") else
            torch.empty(shapes.get(nm, (B, P)), device="cuda", dtype=torch.int32 if nm in H.LAGR_INT_OUTS else torch.float32) for nm in H.LAGR_OUTS]
    tk, tt = [], []
    for _ in range(reps):
        tk += _events(lambda: H.ens_lagr_finalize(pos, ex, res, fl, outs, lattice, boxes, Hh, Ww), 1)[-1:]
        tt += _events(lambda: torch_finalize(pos, ex, res, fl, lattice), 1)[-1:]
    ref = torch_finalize(pos, ex, res, fl, lattice)
    err = max(float(torch.nan_to_num(o_.view(r.shape).double() - r.double()).abs().max() / torch.nan_to_num(r.double()).abs().max().clamp_min(1e-30))
              for o_, r in zip(outs[:14], ref))
    out["finalize"] = {"rows": S + 1, "kernel_ms": tk, "kernel_ms_median": statistics.median(tk), "torch_fp64_ms": tt,
                       "torch_fp64_ms_median": statistics.median(tt), "torch_over_kernel": statistics.median(tt) / statistics.median(tk),
                       "max_difference_over_largest_value": err}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transport_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C, B = loader[0][1].shape[2], a.batch
    first = run("stats", model, loader, 4, a.steps, a.max_rows)
    speed = float(torch.sqrt(first["mean"][:, :, 0] ** 2 + first["mean"][:, :, 1] ** 2).mean())
    CFG["dt"] = 0.5 * min(BT.GRID) / max(speed, 1e-12)
    rec = {"what": "modelPredStats vs modelPredTransport, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "grid": list(BT.GRID), "dt": CFG["dt"], "mean_speed": speed, "max_rows": a.max_rows, "reps": a.reps, "runs": [], "kernels_alone": []}
    for S in [int(s) for s in a.samples.split(",") if s]:
        CFG.update(seed_stride=(2, 2), substeps=1)
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 3, a.max_rows)
        times, alive = {w: [] for w in FUNCS}, None
        for r in range(max(3, a.reps)):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                dt, al = timed(which, model, loader, S, a.steps, a.max_rows)
                times[which].append(dt)
                alive = al if al is not None else alive
        row = {"samples": S, "member_steps": S * a.steps, "alive_frac_mean_at_the_end": alive}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts), "spread_max_over_min": max(ts) / min(ts)}
        row["transport_over_stats_seconds_median"] = row["transport"]["seconds_median"] / row["stats"]["seconds_median"]
        row["kernels"] = []
        for stride in ((2, 2), (1, 1)):
            for n in (1, 4):
                CFG.update(seed_stride=stride, substeps=n)
                ev = event_run(model, loader, S, a.steps, a.max_rows)
                row["kernels"].append({"seed_stride": list(stride), "substeps": n,
                                       **{nm: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c,
                                               "event_us_per_kept_step": 1e3 * ms / a.steps / len(loader)} for nm, (c, ms) in ev.items()}})
        base = row["kernels"][0]
        row["transport_kernels_share_of_transport_run"] = sum(base[nm]["event_ms"] for nm in KERNELS) / 1e3 / row["transport"]["seconds_median"]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.samples.split(",") if s]:
        for stride in ((2, 2), (1, 1)):
            row = direct(S, a.batch, 256, 256, a.max_rows, a.direct_reps, stride, 0.5)
            rec["kernels_alone"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
