"""Cost of the turbulence statistics: utils.modelPredTurbulence beside utils.modelPredStats at the cylinder test shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); member-steps/s = S * steps / seconds (best and median), and the ratio turbulence / stats
  then one more modelPredTurbulence run per S with a device event pair around every launch of the two new kernels
  (tmg_ens_turb_accum, tmg_ens_turb_finalize): launches, summed event time, and GB/s of the algorithmic bytes of turb_traffic().
  An event pair around one launch also holds the launch gap, so the GB/s is a lower bound of the kernel's own rate.

Writes profiles/ensemble_turb_bench.json."""
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

import bench_ensemble as BE   # noqa: E402  (the model, the loader and the grid-free yardstick are that tool's)

GRID = (6.0 / 256, 6.0 / 256)
FUNCS = ("stats", "turbulence")


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=GRID[0], dy=GRID[1])
    f = utils.modelPredStats if which == "stats" else utils.modelPredTurbulence
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


def turb_traffic(S, B, HW, steps, max_rows):
    """Algorithmic bytes the two turbulence kernels of one modelPredTurbulence batch move (stride 1, t_start 0), the target's
    one-member pass included: per step and chunk two input channels, the members' time state (two time means, co-moment and
    time-mean vorticity read from the second step on; co-moment and vorticity written always), the step state (read by every chunk
    after the first, written by every chunk but the last) and the last chunk's two outputs; once at the end the members' two M2
    planes, co-moment and vorticity are read and six outputs written."""
    def one(S, per):
        chunks = [min(per, S - m0) for m0 in range(0, S, per)]
        acc = 0
        for t in range(steps):
            for i, k in enumerate(chunks):
                acc += k * B * HW * 2 * 4
                acc += k * B * HW * 4 * ((4 if t > 0 else 0) + 2)
                acc += B * HW * 2 * 4 * ((1 if i > 0 else 0) + 1)
        return acc, S * B * HW * 4 * 4 + 6 * B * HW * 4
    a1, f1 = one(S, max(1, max_rows // B))
    a2, f2 = one(1, 1)
    return a1 + a2, f1 + f2


def event_run(model, loader, S, steps, max_rows):
    """One modelPredTurbulence run with an event pair around every launch of the two new kernels -> {name: (launches, ms)}."""
    import torch
    import tmg_hip as H
    pairs = {"ens_turb_accum": [], "ens_turb_finalize": []}
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
        run("turbulence", model, loader, S, steps, max_rows)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_turb_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    HW = loader[0][1].shape[-2] * loader[0][1].shape[-1]
    rec = {"what": "modelPredStats vs modelPredTurbulence, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": 3, "steps": a.steps},
           "grid": list(GRID), "max_rows": a.max_rows, "reps": a.reps, "runs": []}
    for S in [int(s) for s in a.samples.split(",")]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 3, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
        row = {"samples": S, "member_steps": S * a.steps}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "member_steps_per_s_best": S * a.steps / min(ts),
                          "member_steps_per_s_median": S * a.steps / statistics.median(ts)}
        row["turbulence_over_stats_seconds_median"] = statistics.median(times["turbulence"]) / statistics.median(times["stats"])
        ev = event_run(model, loader, S, a.steps, a.max_rows)
        nbytes = dict(zip(("ens_turb_accum", "ens_turb_finalize"), turb_traffic(S, a.batch, HW, a.steps, a.max_rows)))
        row["kernels"] = {n: {"launches": c, "event_ms": ms, "bytes": nbytes[n], "gb_per_s": nbytes[n] / ms / 1e6}
                          for n, (c, ms) in ev.items()}
        row["kernel_event_share_of_turbulence_run"] = sum(ms for _, ms in ev.values()) / 1e3 / statistics.median(times["turbulence"])
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
