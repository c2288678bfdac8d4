"""Cost of the structure functions and the variogram score: utils.modelPredStructure beside utils.modelPredStats (unchanged by it) at
the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps, the default 12
lags) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio structure / stats, and the spread (max / min) of the stats runs, which
  is the run-to-run noise the ratio has to be read against
  then one more modelPredStructure run per S with a device event pair around every call of tmg_ens_score_store and tmg_ens_sfun_step
  (moments kernel, variogram kernel and fold together), and in the same process one modelPredEnergy run with event pairs around
  tmg_ens_gram_step and one modelPredScores run with event pairs around tmg_ens_score_step at the same S: launches, summed event
  time, the structure step's share of the modelPredStructure run and the ratios of its time to the other two.  An event pair also
  holds the launch gaps, which all sides of the ratios carry.
  then the step alone on random members at the same [B, C, H, W], for --direct member counts (default 4, 8, 32): median event time of
  tmg_ens_sfun_step over --direct-reps calls, and the device time of each of its kernels from torch.profiler's kernel records of
  the same calls (median per call), against each kernel's algorithmic bytes: the moments kernel reads every row's plane once ((S + 1)
  B C HW floats; the L neighbour reads hit the same lines), the variogram kernel the same planes once more; partials and outputs are
  negligible beside them.

Writes profiles/structure_bench.json."""
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

import bench_ensemble as BE   # noqa: E402  (the model, the loader and the yardstick are that tool's)
import bench_quant as BQ      # noqa: E402  (the event wrapper)
import bench_energy as BG     # noqa: E402  (modelPredEnergy's run)

FUNCS = ("stats", "structure")
GRID = (0.05, 0.05)
KERNELS = ("ens_sfun_mom_kernel", "ens_sfun_var_kernel", "ens_sfun_fold_kernel")


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    if which == "structure":
        args = SimpleNamespace(device=None, dx=GRID[0], dy=GRID[1])
        return utils.modelPredStructure(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)
    return BG.run(which, model, loader, S, steps, max_rows)


def timed(which, model, loader, S, steps, max_rows):
    import time
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def event_run(which, names, model, loader, S, steps, max_rows):
    saved = BQ.run
    BQ.run = run
    try:
        return BQ.event_run(which, names, model, loader, S, steps, max_rows)
    finally:
        BQ.run = saved


def direct(S, B, C, Hh, Ww, reps):
    """The step alone on random members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    from torch.profiler import ProfilerActivity, profile
    g = torch.Generator(device="cuda").manual_seed(S)
    en = ops.EnsembleStructure(S, B, C, Hh, Ww, 1, "cuda", torch.ones(C), grid=GRID)
    en.xs.copy_(torch.randn(en.xs.shape, device="cuda", generator=g))
    tn = torch.randn((B, Hh, Ww, C), device="cuda", generator=g)

    def step():
        H.ens_sfun_step(en.xs, tn, en.lags, en.ws, en.mom[0], en.vsum[0], en.tmom, en.tvar, Hh, Ww, 0, 1)

    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    plane = (S + 1) * B * C * Hh * Ww * 4
    row = {"samples": S, "lags": [list(l) for l in en.lags], "plan": {k: en.plan[k] for k in ("P", "SL", "Lc", "ws")}, "event_ms": ms,
           "event_ms_median": med, "bytes": 2 * plane, "bytes_per_s": 2 * plane / (med * 1e-3), "kernels": {}}
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
    per = {k: [] for k in KERNELS}
    for ev in prof.events():
        for k in KERNELS:
            if k in ev.name:
                per[k].append(float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0)))
    for k, us in per.items():
        if len(us) != reps:
            raise RuntimeError("torch.profiler recorded %d launches of %s, expected %d" % (len(us), k, reps))
        m = statistics.median(us)
        nbytes = plane if k != "ens_sfun_fold_kernel" else en.plan["ws"] * 4
        row["kernels"][k] = {"device_us": us, "device_us_median": m, "bytes": nbytes, "bytes_per_s": nbytes / (m * 1e-6) if m > 0 else None}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredStructure, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "grid": list(GRID), "max_rows": a.max_rows, "reps": a.reps, "runs": [], "sfun_step_alone": []}
    for S in [int(s) for s in a.samples.split(",") if s]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 3, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
        row = {"samples": S, "member_steps": S * a.steps}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts)}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["structure_over_stats_seconds_median"] = statistics.median(times["structure"]) / statistics.median(times["stats"])
        ev = event_run("structure", ("ens_score_store", "ens_sfun_step"), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("energy", ("ens_gram_step",), model, loader, S, a.steps, a.max_rows))
        ev.update(event_run("scores", ("ens_score_step",), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"launches": c, "event_ms": ms} for n, (c, ms) in ev.items()}
        row["sfun_step_share_of_structure_run"] = ev["ens_sfun_step"][1] / 1e3 / statistics.median(times["structure"])
        row["sfun_step_over_gram_step_event_ms"] = ev["ens_sfun_step"][1] / ev["ens_gram_step"][1]
        row["sfun_step_over_score_step_event_ms"] = ev["ens_sfun_step"][1] / ev["ens_score_step"][1]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)                  # (kept if the profiler of the second part fails)
    for S in [int(s) for s in a.direct.split(",") if s]:
        row = direct(S, a.batch, C, 256, 256, a.direct_reps)
        rec["sfun_step_alone"].append(row)
        print(json.dumps(row), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
