"""Cost of the scale-to-scale energy flux: utils.modelPredFlux beside utils.modelPredStats (unchanged by it) at the cylinder test shape
of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, batch 4, 41 steps, the default widths 3, 5, 9, 17, 33) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio flux / stats, and the spread (max / min) of the stats runs, which is
  the run-to-run noise the ratio has to be read against
  then one more modelPredFlux run per S with a device event pair around every call of tmg_ens_flux_accum (the members' chunks and
  the target rows) and tmg_ens_flux_terms: calls, summed event time, microseconds per kept step, the accumulate kernel's bytes per
  second against the bytes it must move (per row and timed step 2 input floats per pixel and, per width, the 7 planes of its valid
  pixels written, and read from the second step on) as a fraction of the rate of a float4 copy of 1 GiB measured in the same run;
  and, in the same process, one modelPredBudget run with event pairs around tmg_ens_budget_accum with its bytes
  (bench_budget.accum_bytes).  An event pair also holds the launch gaps.
  then tmg_ens_flux_accum alone on one random chunk of min(S, max_rows / B) members (read-modify-write): median, min and max event
  time over --direct-reps calls and its bytes per second; and tmg_ens_flux_terms on the state of S members beside a torch fp64
  composition of the same formulas, alternating call by call.

  --accum-only runs nothing but four calls of tmg_ens_flux_accum on a random chunk of max_rows rows (the first stores): the program to
  put under `rocprofv3 --pmc ... --output-format csv -d DIR --`, counters only, in a run of its own; --counters DIR [DIR ...] then adds
  the counters of the last such dispatch found in the CSV files under each DIR to the JSON as "accum_counters" (SQ counters are in
  quad-cycles summed over the waves, GRBM_GUI_ACTIVE in cycles summed over the 8 XCDs) and runs nothing.

Writes profiles/flux_bench.json."""
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

import bench_budget as BB          # noqa: E402  (the budget's run and its bytes)
import bench_ensemble as BE        # noqa: E402  (the model, the loader and the yardstick are that tool's)
import bench_ensemble_turb as BT   # noqa: E402  (the grid)
import bench_quant as BQ           # noqa: E402  (the event wrapper)

FUNCS = ("stats", "flux")


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    if which == "budget":
        return BB.run(which, model, loader, S, steps, max_rows)
    args = SimpleNamespace(device=None, dx=BT.GRID[0], dy=BT.GRID[1])
    f = utils.modelPredFlux if which == "flux" else utils.modelPredStats
    return f(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


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


def step_bytes(rows, Hh, Ww, widths, first):
    """The bytes tmg_ens_flux_accum must move for `rows` rows of one timed step: 2 input floats per pixel and, per width, the 7 planes
    of its valid pixels written, and read unless the step is the first."""
    valid = sum((Hh - 2 - 2 * (w // 2)) * (Ww - 2 - 2 * (w // 2)) for w in widths)
    return rows * 4 * (2 * Hh * Ww + 7 * valid * (1 if first else 2))


def accum_bytes(rows, Hh, Ww, widths, steps):
    return sum(step_bytes(rows, Hh, Ww, widths, t == 0) for t in range(steps))


def copy_rate(reps=5):
    """Bytes per second (read + written) of a device copy of 1 GiB of fp32, the 16-byte-per-lane copy kernel of torch: the median of
    `reps` event-timed copies after two warm-up copies."""
    import torch
    src = torch.empty(1 << 28, device="cuda", dtype=torch.float32).normal_()
    dst = torch.empty_like(src)
    ms = BB._events(lambda: dst.copy_(src), reps)
    return 2 * src.numel() * 4 / (statistics.median(ms) * 1e-3)


def torch_terms(raw, k64, widths, T, Hh, Ww):
    """The formulas of tmg_ens_flux_terms as a torch fp64 composition on the device -> the 14 arrays of tmg_hip.FLUX_OUTS (member_flux
    left out: None), fp32."""
    import torch
    R, B, L = raw.shape[:3]
    r = raw.double().view(R, B, L, 7, Hh, Ww)
    nan = float("nan")
    valid = torch.zeros(L, Hh, Ww, dtype=torch.bool, device=raw.device)
    for l, w in enumerate(widths):
        valid[l, w // 2 + 1:Hh - 1 - w // 2, w // 2 + 1:Ww - 1 - w // 2] = True
    kx, ky = k64[:, 0].view(1, 1, L, 1, 1), k64[:, 1].view(1, 1, L, 1, 1)
    n2 = torch.tensor([float(w * w) ** 2 for w in widths], dtype=torch.float64, device=raw.device).view(1, 1, L, 1, 1, 1)
    pi = -((r[:, :, :, 0] * kx + r[:, :, :, 1] * ky) / T)
    tstd = torch.sqrt(torch.clamp(r[:, :, :, 2] / T - pi * pi, min=0.0))
    back = r[:, :, :, 3] / T
    tau = r[:, :, :, 4:7] / (n2 * T)
    mask = lambda v: torch.where(valid.view((1, 1, L) + (1,) * (v.dim() - 5) + (Hh, Ww)), v, torch.full_like(v, nan))   # noqa: E731
    pi, tstd, back, tau = mask(pi), mask(tstd), mask(back), mask(tau)
    f = lambda v: v.float()                                                  # noqa: E731
    ms = lambda v: (f(v[:-1].mean(0)), f(v[:-1].std(0, unbiased=False)), f(v[-1]))   # noqa: E731
    cnt = valid.view(L, -1).sum(1).double()
    curve = lambda v: f((torch.nan_to_num(v).view(R, B, L, -1).sum(-1) / cnt).permute(1, 0, 2))   # noqa: E731
    fm, fs, ft = ms(pi)
    tm, _, tt = ms(tstd)
    bm, bs, bt = ms(back)
    sm, ss, st = ms(tau)
    return [fm, fs, ft, tm, tt, bm, bs, bt, sm, ss, st, None, curve(pi), curve(0.5 * (tau[:, :, :, 0] + tau[:, :, :, 2]))]


def direct(S, B, Hh, Ww, widths, max_rows, reps, copy):
    """The accumulate kernel on one chunk alone (read-modify-write), and the terms kernel beside the torch composition -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(S)
    k = max(1, min(S, max_rows // B))
    HW, L = Hh * Ww, len(widths)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)             # noqa: E731
    yn = rnd(k * B, Hh, Ww, 3)                                               # the chunk, NHWC as sampleEnsemble leaves it
    a = torch.ones(B, 2, device="cuda")
    k64 = ops.flux_factors(widths, BT.GRID[0], BT.GRID[1]).cuda()
    kk = k64.float()
    raw = torch.empty(S + 1, B, L, 7, HW, device="cuda")
    for m0 in range(0, S + 1, k):                                            # a finite state for the terms kernel
        n = min(k, S + 1 - m0)
        H.ens_flux_accum(yn[:n * B], a, kk, raw, widths, n, m0, 0)
    ms = BB._events(lambda: H.ens_flux_accum(yn, a, kk, raw, widths, k, 0, 1), reps)
    nbytes = step_bytes(k * B, Hh, Ww, widths, False)
    med = statistics.median(ms)
    out = {"samples": S, "chunk_members": k, "rows": k * B, "plan": H.ens_flux_plan(S, B, Hh, Ww, widths), "bytes": nbytes, "event_ms": ms,
           "event_ms_median": med, "event_ms_min": min(ms), "event_ms_max": max(ms), "bytes_per_s": nbytes / (med * 1e-3),
           "float4_copy_bytes_per_s": copy, "share_of_copy_rate": nbytes / (med * 1e-3) / copy}
    new = lambda *s: torch.empty(s, device="cuda")                           # noqa: E731
    outs = [new(B, L, HW) for _ in range(8)] + [new(B, L, 3, HW) for _ in range(3)] + [None, new(B, S + 1, L), new(B, S + 1, L)]
    T = 1 + reps + 2
    tk, tt = [], []
    for i in range(reps):
        tk += BB._events(lambda: H.ens_flux_terms(raw, k64, outs, widths, Hh, Ww, T), 1)
        tt += BB._events(lambda: torch_terms(raw, k64, widths, T, Hh, Ww), 1)
    ref = torch_terms(raw, k64, widths, T, Hh, Ww)
    err = max(float(torch.nan_to_num(o.view(r.shape) - r).abs().max() / torch.nan_to_num(r).abs().max().clamp_min(1e-30))
              for o, r in zip(outs, ref) if r is not None)
    out["terms"] = {"rows": S + 1, "kernel_ms": tk, "kernel_ms_median": statistics.median(tk), "torch_fp64_ms": tt,
                    "torch_fp64_ms_median": statistics.median(tt), "torch_over_kernel": statistics.median(tt) / statistics.median(tk),
                    "max_difference_over_largest_value": err}
    return out


def accum_only(B, Hh, Ww, widths, max_rows):
    """Four calls of the accumulate kernel on one random chunk of max_rows rows: the first stores, three add."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    k = max(1, max_rows // B)
    yn = torch.randn(k * B, Hh, Ww, 3, device="cuda")
    a = torch.ones(B, 2, device="cuda")
    kk = ops.flux_factors(widths, BT.GRID[0], BT.GRID[1]).cuda().float()
    raw = torch.empty(k + 1, B, len(widths), 7, Hh * Ww, device="cuda")
    for t in range(4):
        H.ens_flux_accum(yn, a, kk, raw, widths, k, 0, t)
    torch.cuda.synchronize()


def read_counters(dirs):
    """{counter: value} of the last dispatch of ens_flux_accum_kernel in the rocprofv3 counter CSV files under `dirs`."""
    import csv
    out = {}
    for d in dirs:
        for root, _, files in os.walk(d):
            for f in sorted(files):
                if f.endswith("counter_collection.csv"):
                    for row in csv.DictReader(open(os.path.join(root, f))):
                        if "ens_flux_accum_kernel" in row["Kernel_Name"]:
                            out[row["Counter_Name"]] = float(row["Counter_Value"])   # (rows are in dispatch order: the last one stays)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accum-only", action="store_true")
    ap.add_argument("--counters", nargs="+", default=None)
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_bench.json"))
    a = ap.parse_args()
    if a.counters:
        rec = json.load(open(a.out))
        rec["accum_counters"] = dict(read_counters(a.counters), rows=a.max_rows, what="the last of four calls of tmg_ens_flux_accum alone "
                                     "on one chunk, rocprofv3 --pmc in runs of their own")
        json.dump(rec, open(a.out, "w"), indent=1)
        return
    import torch
    import tmg_ops as ops
    Hh, Ww = 256, 256
    if a.accum_only:
        return accum_only(a.batch, Hh, Ww, ops.flux_args(None, 3, Hh, Ww, BT.GRID)[0], a.max_rows)
    model, loader = BE.setup(a.batch, a.steps)
    C, B = loader[0][1].shape[2], a.batch
    HW = Hh * Ww
    widths = ops.flux_args(None, C, Hh, Ww, BT.GRID)[0]
    copy = copy_rate()
    rec = {"what": "modelPredStats vs modelPredFlux, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [Hh, Ww], "channels": C, "steps": a.steps},
           "grid": list(BT.GRID), "widths": list(widths), "state_bytes_per_row_pixel": 28 * len(widths), "max_rows": a.max_rows, "reps": a.reps,
           "float4_copy_bytes_per_s": copy, "runs": [], "kernels_alone": []}
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
        med = {w: statistics.median(ts) for w, ts in times.items()}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["flux_over_stats_seconds_median"] = med["flux"] / med["stats"]
        ev = event_run("flux", ("ens_flux_accum", "ens_flux_terms"), model, loader, S, a.steps, a.max_rows)
        nb = accum_bytes((S + 1) * B, Hh, Ww, widths, a.steps)
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c, "event_us_per_kept_step": 1e3 * ms / a.steps / len(loader)}
                          for n, (c, ms) in ev.items()}
        acc = row["kernels"]["ens_flux_accum"]
        acc.update(bytes=nb, bytes_per_s=nb / (acc["event_ms"] * 1e-3), share_of_copy_rate=nb / (acc["event_ms"] * 1e-3) / copy)
        row["flux_kernels_share_of_flux_run"] = (ev["ens_flux_accum"][1] + ev["ens_flux_terms"][1]) / 1e3 / med["flux"]
        old = event_run("budget", ("ens_budget_accum",), model, loader, S, a.steps, a.max_rows)
        ob, (oc, oms) = BB.accum_bytes((S + 1) * B, HW, a.steps), old["ens_budget_accum"]
        row["budget_accum"] = {"calls": oc, "event_ms": oms, "event_us_per_kept_step": 1e3 * oms / a.steps / len(loader), "bytes": ob,
                               "bytes_per_s": ob / (oms * 1e-3), "share_of_copy_rate": ob / (oms * 1e-3) / copy}
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.samples.split(",") if s]:
        row = direct(S, a.batch, Hh, Ww, widths, a.max_rows, a.direct_reps, copy)
        rec["kernels_alone"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
