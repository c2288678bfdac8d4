"""Cost of the energy score: utils.modelPredEnergy beside utils.modelPredStats (unchanged by it) at the cylinder test shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio energy / stats, and the spread (max / min) of the stats runs, which is
  the run-to-run noise the ratio has to be read against
  then one more modelPredEnergy run per S with a device event pair around every call of tmg_ens_score_store and tmg_ens_gram_step
  (mean pass, Gram kernel(s), slice reduction and finalize together), and in the same process one modelPredScores run with an event pair
  around every launch of tmg_ens_score_step at the same S: launches, summed event time, the Gram step's share of the modelPredEnergy
  run and the ratio of its time to ens_score_step's.  An event pair also holds the launch gaps, which both sides of the ratio carry.
  then the Gram step alone on random members at the same [B, C, HW], for --direct member counts (default 4, 8, 32, 256): median event
  time of tmg_ens_gram_step over --direct-reps calls, the bytes it has to move ((2 S + 3) planes of B C HW floats: the mean pass reads
  S and writes one, the Gram kernel reads S + 1 rows and the mean) per second, and the MFMA flops it issues (512 HW per live 16 x 16
  tile pair of the upper triangle, per case and channel) against the fp32 matrix peak of 157.3 TFLOP/s.

Writes profiles/energy_bench.json."""
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

_BQ_RUN = BQ.run
FUNCS = ("stats", "energy")
GROUPS = ((0, 1), (2,))
PEAK_F32_MATRIX = 157.3e12


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    if which == "energy":
        return utils.modelPredEnergy(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, groups=GROUPS)
    return _BQ_RUN(which, model, loader, S, steps, max_rows)


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


def live_tile_pairs(S):
    nt = (S + 1 + 15) // 16
    return nt * (nt + 1) // 2


def direct(S, B, C, Hh, Ww, reps):
    """The Gram step alone on random members -> dict."""
    import torch
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(S)
    en = ops.EnsembleEnergy(S, B, C, Hh, Ww, 1, "cuda", torch.ones(C), groups=GROUPS)
    en.xs.copy_(torch.randn(en.xs.shape, device="cuda", generator=g))
    tn = torch.randn((B, Hh, Ww, C), device="cuda", generator=g)
    import tmg_hip as H
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        H.ens_gram_step(en.xs, tn, en.a2, en.groups, en.r, en.ws, en.traj, en.outf, en.outi, 0, 0, 1)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    HW = Hh * Ww
    nbytes = (2 * S + 3) * B * C * HW * 4
    flops = live_tile_pairs(S) * 512 * HW * B * C
    plan = {k: v for k, v in en.plan.items() if k != "pairs"}
    plan["pairs"] = len(en.plan["pairs"])
    return {"samples": S, "plan": plan, "event_ms": ms, "event_ms_median": med, "bytes": nbytes, "bytes_per_s": nbytes / (med * 1e-3),
            "mfma_flops": flops, "flops_per_s": flops / (med * 1e-3), "share_of_fp32_matrix_peak": flops / (med * 1e-3) / PEAK_F32_MATRIX}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct", default="4,8,32,256")
    ap.add_argument("--direct-reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredEnergy, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "groups": [list(g) for g in GROUPS], "max_rows": a.max_rows, "reps": a.reps, "runs": [], "gram_step_alone": []}
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
        row["energy_over_stats_seconds_median"] = statistics.median(times["energy"]) / statistics.median(times["stats"])
        ev = event_run("energy", ("ens_score_store", "ens_gram_step"), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("scores", ("ens_score_step",), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"launches": c, "event_ms": ms} for n, (c, ms) in ev.items()}
        row["gram_step_share_of_energy_run"] = ev["ens_gram_step"][1] / 1e3 / statistics.median(times["energy"])
        row["gram_step_over_score_step_event_ms"] = ev["ens_gram_step"][1] / ev["ens_score_step"][1]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.direct.split(",") if s]:
        row = direct(S, a.batch, C, 256, 256, a.direct_reps)
        rec["gram_step_alone"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
