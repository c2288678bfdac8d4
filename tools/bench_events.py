"""Cost of the event verification (Brier, reliability, ROC, fractions skill score): utils.modelPredEvents beside utils.modelPredStats
(unchanged by it) at the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41
steps, the reverse-flow event, the default six widths) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio events / stats, and the spread (max / min) of the stats runs, which
  is the run-to-run noise the ratio has to be read against
  then one more modelPredEvents run per S with a device event pair around every call of tmg_ens_event_count and tmg_ens_event_step
  (the zeroing launch and the tile kernel together), and in the same process one modelPredQuantiles run (three levels, the same
  event) with event pairs around tmg_ens_score_store and tmg_ens_quant_step at the same S: launches, summed event time, the event
  step's share of the modelPredEvents run and the ratio of its time to the quantile step's.  An event pair also holds the launch
  gaps, which both sides of the ratio carry.
  then the two steps alone on random members at the same [B, C, H, W], for --direct member counts (default 4, 8, 32): median event
  time of tmg_ens_event_step and of tmg_ens_quant_step over --direct-reps calls, and the device time of the event step's kernels from
  torch.profiler's kernel records of the same calls (median per call), against the tile kernel's algorithmic bytes: the count plane
  and the target's channel once (2 B K HW 4-byte words; the halo re-reads hit the same lines) plus the four per-pixel sums read and
  written.

Writes profiles/events_bench.json."""
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
import bench_quant as BQ      # noqa: E402  (the event wrapper, modelPredQuantiles' run)

FUNCS = ("stats", "events")
EVENTS = ((0, 0.0, "<"),)
SCALES = (1, 3, 5, 9, 17, 33)
KERNELS = ("ens_event_zero_kernel", "ens_event_step_kernel")
_BQ_RUN = BQ.run            # (event_run below swaps BQ.run for this module's run while it measures)


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    if which == "events":
        return utils.modelPredEvents(SimpleNamespace(device=None), model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows,
                                     events=EVENTS, scales=SCALES)
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


def _event_ms(step, reps):
    import torch
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return ms


def direct(S, B, C, Hh, Ww, reps):
    """The event step and the quantile step alone on random members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    from torch.profiler import ProfilerActivity, profile
    g = torch.Generator(device="cuda").manual_seed(S)
    en = ops.EnsembleEvents(S, B, C, Hh, Ww, 1, "cuda", torch.zeros(C), torch.ones(C), events=EVENTS, scales=SCALES)
    K = len(EVENTS)
    en.cnt.copy_(torch.randint(0, S + 1, en.cnt.shape, device="cuda", generator=g, dtype=torch.int32))
    tn = torch.randn((B, Hh, Ww, C), device="cuda", generator=g)

    def step():
        H.ens_event_step(en.cnt, tn, en.thr, en.ev, en.scales, en.rel[0, :, 0], en.rel[1, :, 0], en.fss_raw[:, 0], en.tsum,
                         (K * (S + 1), K * len(SCALES) * 3), S, 1, 1)

    en.tsum.zero_()
    ms = _event_ms(step, reps)
    en.tsum.zero_()
    med = statistics.median(ms)
    nbytes = (2 + 8) * B * K * Hh * Ww * 4
    row = {"samples": S, "events": [list(e) for e in EVENTS], "scales": list(SCALES),
           "plan": {k: en.plan[k] for k in ("TH", "TW", "halo", "NTY", "NTX", "lds", "blocks")}, "event_step_ms": ms,
           "event_step_ms_median": med, "kernels": {}}
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
        row["kernels"][k] = {"device_us": us, "device_us_median": m}
        if k == "ens_event_step_kernel":
            row["kernels"][k].update({"bytes": nbytes, "bytes_per_s": nbytes / (m * 1e-6) if m > 0 else None})
    # the quantile step on S random members of the same shape: three levels and the same event
    qt = ops.EnsembleQuantiles(S, B, C, Hh, Ww, 1, "cuda", torch.zeros(C), torch.ones(C), levels=BQ.LEVELS, exceed=EVENTS)
    qt.xs.copy_(torch.randn(qt.xs.shape, device="cuda", generator=g))
    HW = Hh * Ww

    def qstep():
        H.ens_quant_step(qt.xs, tn, qt.u, qt.mu, qt.sd, qt.lo, qt.hi, qt.w, qt.thr, qt.ex, qt.out["quant"][:, 0], qt.out["exceed_prob"][:, 0],
                         (qt.tquant, qt.tbelow, qt.texceed), (qt.Q * C * HW, qt.K * HW), 0, 3)

    qms = _event_ms(qstep, reps)
    row["quant_step_ms"] = qms
    row["quant_step_ms_median"] = statistics.median(qms)
    row["event_step_over_quant_step_ms"] = med / statistics.median(qms)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredEvents, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "events": [list(e) for e in EVENTS], "scales": list(SCALES), "max_rows": a.max_rows, "reps": a.reps, "runs": [],
           "steps_alone": []}
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
        row["events_over_stats_seconds_median"] = statistics.median(times["events"]) / statistics.median(times["stats"])
        ev = event_run("events", ("ens_event_count", "ens_event_step"), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("quantiles", ("ens_score_store", "ens_quant_step"), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"launches": c, "event_ms": ms} for n, (c, ms) in ev.items()}
        row["event_step_share_of_events_run"] = ev["ens_event_step"][1] / 1e3 / statistics.median(times["events"])
        row["event_step_over_quant_step_event_ms"] = ev["ens_event_step"][1] / ev["ens_quant_step"][1]
        row["event_count_over_score_store_event_ms"] = ev["ens_event_count"][1] / ev["ens_score_store"][1]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)                  # (kept if the profiler of the second part fails)
    for S in [int(s) for s in a.direct.split(",") if s]:
        row = direct(S, a.batch, C, 256, 256, a.direct_reps)
        rec["steps_alone"].append(row)
        print(json.dumps(row), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
