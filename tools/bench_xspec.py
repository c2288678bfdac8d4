"""Cost of the ensemble spectral skill (tmg_xspec.hip, utils.modelPredSpectralSkill) at the cylinder test shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 kept steps) with 4 / 8 / 32 members.

  per member count:
  end to end one warm-up run of utils.modelPredStats, utils.modelPredSpectra and utils.modelPredSpectralSkill, then --reps timed runs
             of each, the order alternating from repeat to repeat (same process, same box), each closed by
             torch.cuda.synchronize(): seconds, each function's own run-to-run spread (max - min over median), and the ratios
  kernels    one more modelPredSpectralSkill run with an event pair around every launch of the four entries and of tmg_spec_rows:
             launches and event time per kept step.  An event pair around one launch also holds the launch gap
  once:
  columns    tmg_ens_xspec_cols (cross mode) beside tmg_spec_cols on the same row transform of one chunk of max_rows images,
             alternating call by call, an event pair around each: medians and their ratio.  Both do the same MFMA work; the cross
             mode stores two planes instead of one tile, re-stages the target's tile and walks the shell lists with three sums

Writes profiles/xspec_bench.json."""
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

import bench_ensemble as BE   # noqa: E402  (the model and the loader are that tool's)

FUNCS = ("stats", "spectra", "skill")
KERNELS = ("ens_xspec_prep", "spec_rows", "ens_xspec_cols", "ens_xspec_accum")


def run(which, model, loader, grid, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=grid[0], dy=grid[1])
    f = {"stats": utils.modelPredStats, "spectra": utils.modelPredSpectra, "skill": utils.modelPredSpectralSkill}[which]
    return f(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


def timed(*a):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(*a)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def columns(Hh, Ww, grid, n, reps):
    """tmg_ens_xspec_cols (cross mode) and tmg_spec_cols on the same rows of n images, alternating call by call -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn(n, Hh, Ww, 3, device="cuda", generator=g)
    mu, sd = torch.tensor([0.2, 0.2, 0.2]), torch.tensor([0.9, 0.9, 0.9])
    sk = ops.EnsembleSpectralSkill(n, 1, 3, Hh, Ww, 1, "cuda", mu, sd, grid=grid)
    sk.add(y.permute(0, 3, 1, 2), 0, y[:1].permute(0, 3, 1, 2))               # allocates the workspace, fills zt and the rows
    H.ens_xspec_prep(y, None, sk.mu, sk.sd, None, sk._f, sk.fsum, n, 1, n)
    H.spec_rows(sk._f, None, sk.zero, sk.one, sk.ft_w, sk._yw, n)
    part = torch.empty(n * (Ww // 16) * sk.NK, device="cuda")
    calls = {"xspec_cols": lambda: H.ens_xspec_cols(sk.ft_h, sk._yw, sk.perm, sk.offs, sk.zt, sk._part, n, 1, Hh, Ww, sk.NK, True),
             "spec_cols": lambda: H.spec_cols(sk.ft_h, sk._yw, sk.perm, sk.offs, part, n, Hh, Ww, sk.NK)}
    ms = {name: [] for name in calls}
    for i in range(reps + 3):
        for name in (("xspec_cols", "spec_cols") if i % 2 == 0 else ("spec_cols", "xspec_cols")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            calls[name]()
            e1.record()
            e1.synchronize()
            if i >= 3:
                ms[name].append(e0.elapsed_time(e1))
    med = {name: statistics.median(v) for name, v in ms.items()}
    return {"images": n, "shells": sk.NK, "xspec_cols_ms": med["xspec_cols"], "spec_cols_ms": med["spec_cols"],
            "xspec_cols_ms_min_max": [min(ms["xspec_cols"]), max(ms["xspec_cols"])],
            "spec_cols_ms_min_max": [min(ms["spec_cols"]), max(ms["spec_cols"])],
            "xspec_over_spec_cols": med["xspec_cols"] / med["spec_cols"], "cols_tf": 8.0 * Hh * Hh * Ww * n / med["xspec_cols"] / 1e9}


def event_run(model, loader, grid, S, steps, max_rows):
    """One modelPredSpectralSkill run with an event pair around every launch of its entries -> ({name: (launches, ms)}, seconds)."""
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
        dt = timed("skill", model, loader, grid, S, steps, max_rows)
    finally:
        for n in pairs:
            setattr(H, n, orig[n])
    return {n: (len(v), sum(a.elapsed_time(b) for a, b in v)) for n, v in pairs.items()}, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pass-reps", type=int, default=20)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xspec_bench.json"))
    a = ap.parse_args()
    import torch
    N, steps = a.size, a.steps
    grid = (6.0 / N, 6.0 / N)
    rec = {"what": "ensemble spectral skill: modelPredSpectralSkill beside modelPredSpectra and modelPredStats, event time of its "
                   "entries per kept step, tmg_ens_xspec_cols beside tmg_spec_cols",
           "device": torch.cuda.get_device_properties(0).name, "model": BE.KW, "out_hw": [N, N], "grid": list(grid), "batch": a.batch,
           "steps": steps, "max_rows": a.max_rows, "reps": a.reps, "runs": []}
    rec["columns"] = columns(N, N, grid, a.max_rows, a.pass_reps)
    print(json.dumps(rec["columns"]), flush=True)
    model, loader = BE.setup(a.batch, steps, hw_in=(N // 4, N // 4), up=4)
    for S in [int(s) for s in a.samples.split(",")]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, grid, S, 2, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, grid, S, steps, a.max_rows))
        med = {w: statistics.median(ts) for w, ts in times.items()}
        row = {"samples": S}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "median": med[which], "spread_over_median": (max(ts) - min(ts)) / med[which]}
        row["skill_over_stats"] = med["skill"] / med["stats"]
        row["skill_over_spectra"] = med["skill"] / med["spectra"]
        ev, dt = event_run(model, loader, grid, S, steps, a.max_rows)
        row["kernels"] = {n: {"launches": c, "event_ms": ms, "event_ms_per_kept_step": ms / steps} for n, (c, ms) in ev.items()}
        row["kernel_event_share_of_skill_run"] = sum(ms for _, ms in ev.values()) / 1e3 / dt
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
