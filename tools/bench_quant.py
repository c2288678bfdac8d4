"""Cost of the prediction intervals: utils.modelPredQuantiles (three levels, one reverse-flow threshold) beside utils.modelPredStats
(unchanged by the quantiles) at the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths,
batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio quantiles / stats, and the spread (max / min) of the stats runs, which
  is the run-to-run noise the ratio has to be read against
  then one more modelPredQuantiles run per S with a device event pair around every launch of tmg_ens_score_store and
  tmg_ens_quant_step, and in the same process one modelPredScores run with an event pair around every launch of tmg_ens_score_step at
  the same S: launches, summed event time, the quantile kernel's share of the modelPredQuantiles run and the ratio of its time to
  ens_score_step's.  An event pair around one launch also holds the launch gap, which both sides of the ratio carry.

Writes profiles/quant_bench.json."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-turbulence_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_ensemble as BE   # noqa: E402  (the model, the loader and the yardstick are that tool's)

FUNCS = ("stats", "quantiles")
LEVELS = (0.05, 0.5, 0.95)
EXCEED = ((0, 0.0, "<"),)


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    if which == "quantiles":
        return utils.modelPredQuantiles(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, levels=LEVELS,
                                        exceed=EXCEED)
    f = utils.modelPredStats if which == "stats" else utils.modelPredScores
    return f(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


def timed(which, model, loader, S, steps, max_rows):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def event_run(which, names, model, loader, S, steps, max_rows):
    """One run of `which` with an event pair around every launch of the binding functions `names` -> {name: (launches, ms)}."""
    import torch
    import tmg_hip as H
    pairs = {n: [] for n in names}
    orig = {n: getattr(H, n) for n in pairs}

    def wrap(name):
        def f(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig[name](*a, **k)
            e1.record()
            pairs[name].append((e0, e1))
        return f

    try:
        for n in pairs:
            setattr(H, n, wrap(n))
        run(which, model, loader, S, steps, max_rows)
        torch.cuda.synchronize()
    finally:
        for n in pairs:
            setattr(H, n, orig[n])
    return {n: (len(v), sum(a.elapsed_time(b) for a, b in v)) for n, v in pairs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredQuantiles, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "levels": list(LEVELS), "exceed": [list(e) for e in EXCEED], "max_rows": a.max_rows, "reps": a.reps, "runs": []}
    for S in [int(s) for s in a.samples.split(",")]:
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
        row["quantiles_over_stats_seconds_median"] = statistics.median(times["quantiles"]) / statistics.median(times["stats"])
        ev = event_run("quantiles", ("ens_score_store", "ens_quant_step"), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("scores", ("ens_score_step",), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"launches": c, "event_ms": ms} for n, (c, ms) in ev.items()}
        row["quant_step_share_of_quantiles_run"] = ev["ens_quant_step"][1] / 1e3 / statistics.median(times["quantiles"])
        row["quant_step_over_score_step_event_ms"] = ev["ens_quant_step"][1] / ev["ens_score_step"][1]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
