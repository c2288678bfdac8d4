"""Cost of the calibration scores: utils.modelPredScores beside utils.modelPredStats (unchanged by the scores) at the cylinder test
shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio scores / stats, and the spread (max / min) of the stats runs, which is
  the run-to-run noise the ratio has to be read against
  then one more modelPredScores run per S with a device event pair around every launch of the two new kernels
  (tmg_ens_score_store, tmg_ens_score_step): launches, summed event time, share of the run, and GB/s of the algorithmic bytes of
  score_traffic().  An event pair around one launch also holds the launch gap, so the GB/s is a lower bound of the kernel's own rate.

Writes profiles/scores_bench.json."""
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

FUNCS = ("stats", "scores")
SCORE_R = 8                   # csrc/tmg_scores.hip


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    f = utils.modelPredStats if which == "stats" else utils.modelPredScores
    return f(SimpleNamespace(device=None), model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


def timed(which, model, loader, S, steps, max_rows):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def score_traffic(S, B, C, HW, steps):
    """Algorithmic bytes the two kernels of one modelPredScores batch move (stride 1, t_start 0).  store: every member's C channels
    read and written once per step.  step, per (case, channel, pixel) and step: the target, the S members once for the first term
    and the register blocks, the members behind every full register block once more (sum over the blocks of S - m0 - R), two scores
    written, two time means read (from the second step on) and written; the histogram is negligible."""
    E = B * C * HW
    streamed = sum(max(0, S - m0 - SCORE_R) for m0 in range(0, S, SCORE_R))
    store = steps * S * E * 2 * 4
    step = sum(E * 4 * (1 + S + streamed + 2 + (2 if t > 0 else 0) + 2) for t in range(steps))
    return store, step


def event_run(model, loader, S, steps, max_rows):
    """One modelPredScores run with an event pair around every launch of the two new kernels -> {name: (launches, ms)}."""
    import torch
    import tmg_hip as H
    pairs = {"ens_score_store": [], "ens_score_step": []}
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
        run("scores", model, loader, S, steps, max_rows)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C, HW = loader[0][1].shape[2], loader[0][1].shape[-2] * loader[0][1].shape[-1]
    rec = {"what": "modelPredStats vs modelPredScores, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "max_rows": a.max_rows, "reps": a.reps, "runs": []}
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
        row["scores_over_stats_seconds_median"] = statistics.median(times["scores"]) / statistics.median(times["stats"])
        ev = event_run(model, loader, S, a.steps, a.max_rows)
        nbytes = dict(zip(("ens_score_store", "ens_score_step"), score_traffic(S, a.batch, C, HW, a.steps)))
        row["kernels"] = {n: {"launches": c, "event_ms": ms, "bytes": nbytes[n], "gb_per_s": nbytes[n] / ms / 1e6,
                              "share_of_scores_run": ms / 1e3 / statistics.median(times["scores"])} for n, (c, ms) in ev.items()}
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
