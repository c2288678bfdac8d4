"""Cost of the phase averages: utils.modelPredPhase beside utils.modelPredModes and utils.modelPredStats (both unchanged by it) at the
cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the three, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratios phase / modes and phase / stats, and the spread (max / min) of the
  stats runs, which is the run-to-run noise the ratios have to be read against
  then one more modelPredPhase run per S with a device event pair around every call of tmg_ens_phase_label and tmg_ens_phase_accum
  (the members' chunks and the target rows) and, for comparison, of tmg_ens_pod_project: calls, summed event time, microseconds per
  call and per kept step, and the two kernels' share of the modelPredPhase run.  An event pair also holds the launch gaps.
  then tmg_ens_phase_accum alone on one random chunk of min(S, max_rows / B) members at the same [B, C, HW] with the labels spread
  over the sectors in turn: median, min and max event time over --direct-reps calls, and the bytes it has to move per second: the
  chunk's rows read once (k B HW C floats), the mean planes once per sector that holds a row, and the touched accumulators, min(NB, k)
  sectors of Q = 2 C + 1 planes, read and written, beside the 6.3 TB/s a float4 copy reaches on this part (the kernel guide's HBM
  figure).  The accumulators of one chunk size stay in the last-level cache between calls, so the figure is a rate of the algorithmic
  bytes, not of HBM traffic.

Writes profiles/phase_bench.json."""
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
FUNCS = ("stats", "modes", "phase")
CHANNELS = (0, 1)
HBM_COPY = 6.3e12
MODES = [8]                   # --modes
BINS = [8]                    # --bins


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    kw = dict(samples=S, stride=1, tmax=steps, max_rows=max_rows, modes=MODES[0], channels=CHANNELS)
    if which == "phase":
        return utils.modelPredPhase(args, model, loader, BE.LOG, pair=(0, 1), bins=BINS[0], **kw)
    if which == "modes":
        return utils.modelPredModes(args, model, loader, BE.LOG, **kw)
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


def direct(S, B, C, Hh, Ww, NB, max_rows, reps):
    """The accumulate kernel on one chunk alone -> dict."""
    import torch
    import tmg_hip as H
    g = torch.Generator(device="cuda").manual_seed(S)
    k = max(1, min(S, max_rows // B))
    HW, Q = Hh * Ww, 2 * C + 1
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)             # noqa: E731
    yn = rnd(k * B, Hh, Ww, C)                                               # the chunk, NHWC as sampleEnsemble leaves it
    a, m = torch.ones(B, C, device="cuda"), rnd(B, C, HW)
    acc = torch.zeros(B, NB, Q, HW, device="cuda")
    lab = (torch.arange(k, device="cuda").view(1, k) + torch.arange(B, device="cuda").view(B, 1)).remainder(NB).to(torch.int32).contiguous()
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        H.ens_phase_accum(yn, lab, (k, 1), a, m, acc, k)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    touched = min(NB, k)
    nbytes = (k * B * HW * C + touched * B * C * HW + 2 * touched * B * Q * HW) * 4
    med = statistics.median(ms)
    return {"samples": S, "chunk_members": k, "rows": k * B, "bins": NB, "plan": H.ens_phase_plan(k, B, C, HW, NB),
            "sectors_touched_per_case": touched, "bytes": nbytes, "event_ms": ms, "event_ms_median": med, "event_ms_min": min(ms),
            "event_ms_max": max(ms), "bytes_per_s": nbytes / (med * 1e-3), "hbm_float4_copy_bytes_per_s": HBM_COPY,
            "share_of_hbm_copy_rate": nbytes / (med * 1e-3) / HBM_COPY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--bins", type=int, default=8)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_bench.json"))
    a = ap.parse_args()
    import torch
    if not 2 <= a.modes < a.steps:
        ap.error("--modes needs 2 <= modes <= steps - 1")
    MODES[0], BINS[0] = a.modes, a.bins
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredModes vs modelPredPhase, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "pod_channels": list(CHANNELS), "modes": a.modes, "pair": [0, 1], "bins": a.bins, "max_rows": a.max_rows, "reps": a.reps,
           "runs": [], "accum_alone": []}
    names = ("ens_phase_label", "ens_phase_accum", "ens_pod_project")
    for S in [int(s) for s in a.samples.split(",") if s]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects (K modes need K + 1 steps)
            timed(which, model, loader, S, a.modes + 1, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
        row = {"samples": S, "member_steps": S * a.steps}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts)}
        med = {w: statistics.median(ts) for w, ts in times.items()}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["phase_over_modes_seconds_median"] = med["phase"] / med["modes"]
        row["phase_over_stats_seconds_median"] = med["phase"] / med["stats"]
        ev = event_run("phase", names, model, loader, S, a.steps, a.max_rows)
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c, "event_us_per_kept_step": 1e3 * ms / a.steps / len(loader)}
                          for n, (c, ms) in ev.items()}
        row["label_and_accum_share_of_phase_run"] = (ev["ens_phase_label"][1] + ev["ens_phase_accum"][1]) / 1e3 / med["phase"]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.samples.split(",") if s]:
        row = direct(S, a.batch, C, 256, 256, a.bins, a.max_rows, a.direct_reps)
        rec["accum_alone"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
