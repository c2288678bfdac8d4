"""Cost of the pooled ensemble PDFs (marginal and joint histograms of the members and of the target): utils.modelPredPdfs beside
utils.modelPredStats (unchanged by it) at the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, batch 4, 41
steps; the default fields ux, uy, p, vort at 64 bins, the joint (ux, uy) table at 32 x 32, the whole field, default ranges) for
4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio pdfs / stats, and the spread (max / min) of the stats runs, which is
  the run-to-run noise the ratio has to be read against
  then one more modelPredPdfs run per S with a device event pair around every call of tmg_ens_pdf_count (members and target), and in
  the same process one modelPredEvents run (the reverse-flow event, the default widths) with event pairs around tmg_ens_event_count,
  the nearest existing kernel (one pass over a chunk with integer adds): launches, summed event time, the PDF step's share of the
  modelPredPdfs run and the ratio of its time per call to the event count's.  An event pair also holds the launch gaps, which both
  sides of the ratio carry.
  then tmg_ens_pdf_count alone on one chunk of --direct members at the same [B, C, H, W] (default 4, 8, 16 members: 16, 32, 64 rows)
  on the two contention extremes: "one_bin" (a constant field: every lane of every wave on one LDS address per histogram) and
  "spread" (members uniform over the range: the lanes of a wave on different addresses), median event time over --direct-reps calls,
  against tmg_ens_event_count on the same chunk and against the chunk's bytes (k B HW C 4-byte words read once).

Writes profiles/pdf_bench.json."""
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
import bench_events as BV     # noqa: E402  (modelPredEvents' run, the event timer)
import bench_quant as BQ      # noqa: E402  (the event wrapper)

FUNCS = ("stats", "pdfs")
FIELDS = ("ux", "uy", "p", "vort")
JOINT = (("ux", "uy"),)
GRID = (0.05, 0.05)
_BV_RUN = BV.run


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    if which == "pdfs":
        return utils.modelPredPdfs(SimpleNamespace(device=None, dx=GRID[0], dy=GRID[1]), model, loader, BE.LOG, samples=S, stride=1, tmax=steps,
                                   max_rows=max_rows, fields=FIELDS, joint=JOINT)
    return _BV_RUN(which, model, loader, S, steps, max_rows)


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


def direct(k, B, C, Hh, Ww, reps):
    """tmg_ens_pdf_count alone on one chunk of k members, on the two contention extremes, beside tmg_ens_event_count -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(k)
    en = ops.EnsemblePdfs(k, B, C, Hh, Ww, 1, "cuda", torch.zeros(C), torch.ones(C), fields=FIELDS, bins=64,
                          ranges=[(-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0), (-20.0, 20.0)], joint=JOINT, joint_bins=32, grid=GRID)
    ev = ops.EnsembleEvents(k, B, C, Hh, Ww, 1, "cuda", torch.zeros(C), torch.ones(C), events=BV.EVENTS, scales=(1,))
    row = {"members": k, "rows": k * B, "plan": H.ens_pdf_plan(k, B, Hh, Ww, en.F, en.nb, en.P, en.nbj, en.R, en.derived),
           "chunk_bytes": k * B * Hh * Ww * C * 4}
    for name in ("one_bin", "spread"):
        y = torch.zeros((k * B, Hh, Ww, C), device="cuda") if name == "one_bin" else \
            torch.rand((k * B, Hh, Ww, C), device="cuda", generator=g) * 2 - 1
        yn = y.permute(0, 3, 1, 2)
        for v in (en.cnt, en.jnt, en.mt[0], en.tj):
            v.zero_()
        ms = BV._event_ms(lambda: en._count(0, yn.permute(0, 2, 3, 1), k, k, 0, 0, True), reps)
        ems = BV._event_ms(lambda: H.ens_event_count(yn.permute(0, 2, 3, 1), ev.thr, ev.ev, ev.cnt, k, k, 0), reps)
        med = statistics.median(ms)
        inner = int(en.cnt[0, :, 0, :, :, 1:-1].sum()) / max(1, int(en.cnt[0, :, 0].sum()))
        row[name] = {"pdf_count_ms": ms, "pdf_count_ms_median": med, "bytes_per_s": row["chunk_bytes"] / (med * 1e-3),
                     "event_count_ms_median": statistics.median(ems), "pdf_count_over_event_count": med / statistics.median(ems),
                     "share_of_samples_in_range": inner}
    row["one_bin_over_spread"] = row["one_bin"]["pdf_count_ms_median"] / row["spread"]["pdf_count_ms_median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct", default="4,8,16")
    ap.add_argument("--direct-reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdf_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredPdfs, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "fields": list(FIELDS), "bins": 64, "joint": [list(p) for p in JOINT], "joint_bins": 32, "max_rows": a.max_rows, "reps": a.reps,
           "runs": [], "count_alone": []}
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
        row["pdfs_over_stats_seconds_median"] = statistics.median(times["pdfs"]) / statistics.median(times["stats"])
        ev = event_run("pdfs", ("ens_pdf_count",), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("events", ("ens_event_count",), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"launches": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c} for n, (c, ms) in ev.items()}
        row["pdf_count_share_of_pdfs_run"] = ev["ens_pdf_count"][1] / 1e3 / statistics.median(times["pdfs"])
        row["pdf_count_over_event_count_per_call"] = (ev["ens_pdf_count"][1] / ev["ens_pdf_count"][0]) / (ev["ens_event_count"][1] / ev["ens_event_count"][0])
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    for k in [int(s) for s in a.direct.split(",") if s]:
        row = direct(k, a.batch, C, 256, 256, a.direct_reps)
        rec["count_alone"].append(row)
        print(json.dumps(row), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
