"""Cost of the vortex census: utils.modelPredVortices beside utils.modelPredStats (unchanged by it) at the cylinder test shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 kept steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps (at least 3) timed runs alternating the two, each window
  closed by torch.cuda.synchronize(); median and best seconds, the ratio vortices / stats, and the spread (max / min) of the runs of
  each, which is the run-to-run noise the ratio has to be read against
  then, per S, one modelPredVortices run with a device event pair around every call of tmg_ens_vortex_classify, tmg_ens_vortex_label
  and tmg_ens_vortex_census: calls, summed event time, microseconds per kept step.  An event pair also holds the launch gaps.
  then tmg_ens_vortex_label alone on one chunk of 16, 32 and 64 planes of 256 x 256 holding a blob mask (discs of both signs), a
  random mask of density 0.5 and the serpentine of tests/vortex_cases.py, beside the host's reference path for the same planes: the
  device-to-host copy, then scipy.ndimage.label per sign (the queue flood fill of tests/vortex_cases.py where scipy is missing).

Writes profiles/vortex_bench.json."""
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

import bench_ensemble as BE        # noqa: E402  (the model, the loader and the yardstick are that tool's)
import bench_ensemble_turb as BT   # noqa: E402  (the grid)
import bench_quant as BQ           # noqa: E402  (the event wrapper)

FUNCS = ("stats", "vortices")
KERNELS = ("ens_vortex_classify", "ens_vortex_label", "ens_vortex_census")


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=BT.GRID[0], dy=BT.GRID[1])
    kw = dict(samples=S, stride=1, tmax=steps, max_rows=max_rows)
    if which == "vortices":
        return utils.modelPredVortices(args, model, loader, BE.LOG, **kw)
    return utils.modelPredStats(args, model, loader, BE.LOG, **kw)


def timed(which, model, loader, S, steps, max_rows):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    info = None
    if which == "vortices":
        info = {"found_mean_per_field": float(out["vortex_found"].double().sum(-1).mean()), "truncated_tables": int(out["vortex_truncated"].sum()),
                "rejected_pixels": int(out["vortex_rejected"].sum())}
    del out
    return dt, info


def event_run(model, loader, S, steps, max_rows):
    saved = BQ.run
    BQ.run = run
    try:
        return BQ.event_run("vortices", KERNELS, model, loader, S, steps, max_rows)
    finally:
        BQ.run = saved


def bench_masks(hw):
    """name -> int8 [H, W]: discs of both signs, a random mask of density 0.5, the serpentine."""
    import numpy as np
    import vortex_cases as K
    Hh, Ww = hw
    m = K.masks(hw, 32, 32)
    y, x = np.mgrid[0:Hh, 0:Ww]
    blob = np.zeros(hw, np.int8)
    for i, (cy, cx) in enumerate((cy, cx) for cy in range(32, Hh, 64) for cx in range(32, Ww, 64)):
        blob[(y - cy) ** 2 + (x - cx) ** 2 <= 20 ** 2] = 1 if i % 2 == 0 else -1
    return {"blob": blob, "random_0.5": m["random_0.5"], "serpentine": m["serpentine"]}


def host_label(planes):
    """The reference path on the host: scipy.ndimage.label per sign, else the flood fill -> (seconds, method)."""
    import vortex_cases as K
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    t0 = time.perf_counter()
    for p in planes:
        if ndimage is None:
            K.label(p)
        else:
            ndimage.label(p == 1)
            ndimage.label(p == -1)
    return time.perf_counter() - t0, "flood fill" if ndimage is None else "scipy.ndimage.label"


def label_alone(rows, reps, hw=(256, 256)):
    import numpy as np
    import torch
    import tmg_hip as H
    import vortex_cases as K
    out = []
    for name, mask in bench_masks(hw).items():
        cls = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mask.reshape(1, -1), (rows, mask.size)))).to("cuda")
        lab = torch.empty((rows, mask.size), device="cuda", dtype=torch.int32)
        status = torch.zeros(1, device="cuda", dtype=torch.int32)
        ms = []
        for i in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            H.ens_vortex_label(cls, lab, status, hw[0], hw[1])
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        assert int(status.item()) == 0 and np.array_equal(lab[rows - 1].cpu().numpy().reshape(hw), K.label(mask))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = cls.cpu().numpy().reshape(rows, *hw)
        copy_s = time.perf_counter() - t0
        host_s, method = host_label(host)
        med = statistics.median(ms)
        out.append({"mask": name, "rows": rows, "hw": list(hw), "components": int(len(np.unique(K.label(mask))) - 1), "event_ms": ms,
                    "event_ms_median": med, "event_ms_min": min(ms), "event_ms_max": max(ms), "pixels_per_s": rows * mask.size / (med * 1e-3),
                    "host_method": method, "host_copy_ms": 1e3 * copy_s, "host_label_ms": 1e3 * host_s,
                    "host_over_kernel": (1e3 * (copy_s + host_s)) / med})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--label-rows", default="16,32,64")
    ap.add_argument("--label-reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vortex_bench.json"))
    a = ap.parse_args()
    import torch
    import tmg_hip as H
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredVortices, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "grid": list(BT.GRID), "max_rows": a.max_rows, "reps": a.reps, "plan": H.ens_vortex_plan(a.max_rows // a.batch, 32, a.batch, 256, 256, 64, a.steps),
           "runs": [], "label_alone": []}
    for S in [int(s) for s in a.samples.split(",") if s]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 3, a.max_rows)
        times, info = {w: [] for w in FUNCS}, None
        for r in range(max(3, a.reps)):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                dt, inf = timed(which, model, loader, S, a.steps, a.max_rows)
                times[which].append(dt)
                info = inf if inf is not None else info
        row = {"samples": S, "member_steps": S * a.steps, "census": info}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts), "spread_max_over_min": max(ts) / min(ts)}
        row["vortices_over_stats_seconds_median"] = row["vortices"]["seconds_median"] / row["stats"]["seconds_median"]
        ev = event_run(model, loader, S, a.steps, a.max_rows)
        row["kernels"] = {nm: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c,
                               "event_us_per_kept_step": 1e3 * ms / a.steps / len(loader)} for nm, (c, ms) in ev.items()}
        row["vortex_kernels_share_of_vortices_run"] = sum(row["kernels"][nm]["event_ms"] for nm in KERNELS) / 1e3 / row["vortices"]["seconds_median"]
        row["vortex_kernels_over_stats_spread"] = (sum(row["kernels"][nm]["event_ms"] for nm in KERNELS) / 1e3) / (
            max(row["stats"]["seconds"]) - min(row["stats"]["seconds"]) + 1e-30)
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for rows in [int(s) for s in a.label_rows.split(",") if s]:
        for row in label_alone(rows, a.label_reps):
            rec["label_alone"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
