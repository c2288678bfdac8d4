"""Cost of the temporal power spectra: utils.modelPredTimeSpectra beside utils.modelPredStats (unchanged by the spectra) at the cylinder
test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio tspec / stats, and the spread (max / min) of the stats runs, which is
  the run-to-run noise the ratio has to be read against
  then one more modelPredTimeSpectra run per S with a device event pair around every launch of the three new kernels
  (tmg_tspec_store, tmg_tspec_block, tmg_tspec_finalize; the ensemble's and the target's one-member pass together): launches, summed
  event time, share of the run, and GB/s of the algorithmic bytes of tspec_traffic().  An event pair around one launch also holds the
  launch gap, so the GB/s is a lower bound of the kernel's own rate.

Writes profiles/tspec_bench.json."""
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

FUNCS = ("stats", "tspec")
KERNELS = ("tspec_store", "tspec_block", "tspec_finalize")
BLOCK = 16                    # csrc/tmg_tspec.hip


def run(which, model, loader, S, steps, max_rows, nfreq):
    from utils import utils
    kw = dict(samples=S, stride=1, tmax=steps, max_rows=max_rows)
    if which == "stats":
        return utils.modelPredStats(SimpleNamespace(device=None), model, loader, BE.LOG, **kw)
    return utils.modelPredTimeSpectra(SimpleNamespace(device=None), model, loader, BE.LOG, nfreq=nfreq, **kw)


def timed(which, model, loader, S, steps, max_rows, nfreq):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows, nfreq)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def tspec_traffic(S, B, C, HW, steps, nfreq):
    """Algorithmic bytes the three kernels of one modelPredTimeSpectra batch move (stride 1, t_start 0), the S-member ensemble plus the
    target's one-member pass.  store: every element read and written once per step.  block, per pass over nb steps: nb ring slots
    read, the 2 NF + 1 accumulator rows written, and read first on every pass but the first.  finalize: per element the 2 NF + 1 rows
    read once (the sum row's re-reads by the other bins are cache hits), two outputs of NF values written per (case, channel, pixel)."""
    NF = min(nfreq, steps // 2 + 1)
    R = 2 * NF + 1
    tot = {k: 0 for k in KERNELS}
    for members in (S, 1):
        E = members * B * C * HW
        tot["tspec_store"] += steps * E * 2 * 4
        for n0 in range(0, steps, BLOCK):
            nb = min(BLOCK, steps - n0)
            tot["tspec_block"] += E * 4 * (nb + R * (1 if n0 == 0 else 2))
        tot["tspec_finalize"] += E * 4 * R + B * C * HW * NF * 2 * 4
    return tot


def event_run(model, loader, S, steps, max_rows, nfreq):
    """One modelPredTimeSpectra run with an event pair around every launch of the three new kernels -> {name: (launches, ms)}."""
    import torch
    import tmg_hip as H
    pairs = {n: [] for n in KERNELS}
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
        run("tspec", model, loader, S, steps, max_rows, nfreq)
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
    ap.add_argument("--nfreq", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tspec_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C, HW = loader[0][1].shape[2], loader[0][1].shape[-2] * loader[0][1].shape[-1]
    rec = {"what": "modelPredStats vs modelPredTimeSpectra, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "nfreq": a.nfreq, "bins": min(a.nfreq, a.steps // 2 + 1), "max_rows": a.max_rows, "reps": a.reps, "runs": []}
    for S in [int(s) for s in a.samples.split(",")]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 3, a.max_rows, a.nfreq)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, S, a.steps, a.max_rows, a.nfreq))
        row = {"samples": S, "member_steps": S * a.steps}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts)}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["tspec_over_stats_seconds_median"] = statistics.median(times["tspec"]) / statistics.median(times["stats"])
        ev = event_run(model, loader, S, a.steps, a.max_rows, a.nfreq)
        nbytes = tspec_traffic(S, a.batch, C, HW, a.steps, a.nfreq)
        row["kernels"] = {n: {"launches": c, "event_ms": ms, "bytes": nbytes[n], "gb_per_s": nbytes[n] / ms / 1e6,
                              "share_of_tspec_run": ms / 1e3 / statistics.median(times["tspec"])} for n, (c, ms) in ev.items()}
        row["kernels_share_of_tspec_run"] = sum(k["share_of_tspec_run"] for k in row["kernels"].values())
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
