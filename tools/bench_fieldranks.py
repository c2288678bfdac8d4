"""Cost of the multivariate rank histograms: utils.modelPredFieldRanks beside utils.modelPredStats (unchanged by the field ranks) at
the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32
members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio fieldranks / stats, and the spread (max / min) of the stats runs, which
  is the run-to-run noise the ratio has to be read against
  then one more modelPredFieldRanks run per S with a device event pair around every call of tmg_ens_score_store and
  tmg_ens_frank_step (both of its launches), and in the same process one modelPredQuantiles run with an event pair around every
  launch of tmg_ens_quant_step at the same S: calls, summed event time, event time per kept step, the step's share of the
  modelPredFieldRanks run and the ratio of its time to ens_quant_step's.  An event pair around one call also holds the launch gap,
  which both sides of the ratio carry
  then both steps alone on the SAME member buffer (random members, batch 4), alternating call by call: median / min / max event time
  of tmg_ens_frank_step and of tmg_ens_quant_step (three levels, one threshold, no target).  Both load (rows)^2 / 8 values per pixel;
  the field ranks stream S + 1 rows, hold two counters per row instead of one and reduce 17 values per held block over the block
  and the step alone at 64 / 256 / 1024 members on one plane set (batch 1): median event time, and the compared pairs per second

Writes profiles/fieldranks_bench.json."""
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
import bench_quant as BQ      # noqa: E402  (the quantile side of the comparison)

FUNCS = ("stats", "fieldranks")


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    if which == "fieldranks":
        return utils.modelPredFieldRanks(SimpleNamespace(device=None), model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)
    return BQ.run(which, model, loader, S, steps, max_rows)


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
    """One run of `which` with an event pair around every call of the binding functions `names` -> {name: (calls, ms)}."""
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


def event_ms(fn, n):
    import torch
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        out.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in out]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def steps_alone(S, B, C, Hh, Ww, calls, with_quant=True):
    """tmg_ens_frank_step and tmg_ens_quant_step on one member buffer of random values, alternating call by call."""
    import torch
    import tmg_ops as ops
    dev = "cuda"
    fr = ops.EnsembleFieldRanks(S, B, C, Hh, Ww, 2, dev)
    fr.xs.copy_(torch.randn(fr.xs.shape, generator=torch.Generator().manual_seed(S)).to(dev))
    import tmg_hip as H

    def frank():
        H.ens_frank_step(fr.xs, fr.ws, fr.pre_raw, fr.outside, fr.tout, 0, 0, 1)

    row = {"members": S, "batch": B, "channels": C, "hw": [Hh, Ww], "pairs_per_pixel": (S + 1) * S}
    if with_quant:
        q = ops.EnsembleQuantiles(S, B, C, Hh, Ww, 2, dev, torch.zeros(C), torch.ones(C), levels=BQ.LEVELS, exceed=BQ.EXCEED)
        xs = fr.xs[:S]                                          # the same members; the target row is the field ranks' alone

        def quant():
            H.ens_quant_step(xs, None, q.u, q.mu, q.sd, q.lo, q.hi, q.w, q.thr, q.ex, q.out["quant"][:, 0], q.out["exceed_prob"][:, 0],
                             (q.tquant, q.tbelow, q.texceed), (2 * q.Q * C * Hh * Ww, 2 * q.K * Hh * Ww), 0, 1)
        for f in (frank, quant):
            f()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(calls):
            a += event_ms(frank, 1)
            b += event_ms(quant, 1)
        row["frank_step"], row["quant_step"] = summary(a), summary(b)
        row["frank_over_quant_median"] = row["frank_step"]["median_ms"] / row["quant_step"]["median_ms"]
    else:
        frank()
        torch.cuda.synchronize()
        row["frank_step"] = summary(event_ms(frank, calls))
    row["frank_pairs_per_second"] = (S + 1) * S * B * C * Hh * Ww / (row["frank_step"]["median_ms"] * 1e-3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--alone", default="64,256,1024")
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fieldranks_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    Hh, Ww = loader[0][1].shape[-2:]
    rec = {"what": "modelPredStats vs modelPredFieldRanks, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [int(Hh), int(Ww)], "channels": C, "steps": a.steps},
           "groups": [[0, 1], [2]], "max_rows": a.max_rows, "reps": a.reps, "reduction": "per-block int32 records, folded in block order "
           "(no atomics); the 64-bit-atomic form was not built", "runs": [], "steps_alone_same_buffer": [], "step_alone_one_plane_set": []}
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
        row["fieldranks_over_stats_seconds_median"] = statistics.median(times["fieldranks"]) / statistics.median(times["stats"])
        ev = event_run("fieldranks", ("ens_score_store", "ens_frank_step"), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("quantiles", ("ens_quant_step",), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_ms_per_kept_step": ms / a.steps} for n, (c, ms) in ev.items()}
        row["frank_step_share_of_fieldranks_run"] = ev["ens_frank_step"][1] / 1e3 / statistics.median(times["fieldranks"])
        row["frank_step_over_quant_step_event_ms"] = ev["ens_frank_step"][1] / ev["ens_quant_step"][1]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
        alone = steps_alone(S, a.batch, C, int(Hh), int(Ww), 20)
        rec["steps_alone_same_buffer"].append(alone)
        print(json.dumps(alone), flush=True)
    for S in [int(s) for s in a.alone.split(",") if s]:
        alone = steps_alone(S, 1, C, int(Hh), int(Ww), 5 if S > 256 else 20, with_quant=False)
        rec["step_alone_one_plane_set"].append(alone)
        print(json.dumps(alone), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
