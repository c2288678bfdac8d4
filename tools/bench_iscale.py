"""Cost of the intensity-scale verification (Haar skill by scale): tmg_ens_iscale_chunk beside tmg_ens_event_count on the same chunks,
tmg_ens_iscale_step alone, and utils.modelPredIntensityScale beside utils.modelPredStats (unchanged by it), at the shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, the field of the metric configuration, default widths, batch 4, 41 steps, the
reverse-flow event, 6 levels) with 32 members.

  chunk alone    a chunk is --max-rows rows: k = max_rows / batch whole members of [B, 256, 256, 3].  --buffers distinct chunks
                 (together beyond the 256 MiB of the last-level cache, so a pass re-reads nothing from it) are taken in turn; one pass
                 over all of them sits between two device events, after two warm-up passes, --direct-reps passes per operation, the
                 operations alternating: tmg_ens_event_count (reads the same NHWC rows and folds the same count plane),
                 tmg_ens_iscale_chunk as a later chunk of its step (m0 > 0: no zeroing launch, the count read and written), the
                 same as the step's first chunk (m0 = 0: the zeroing launch and Cc), tmg_ens_iscale_step, and a device-to-device copy
                 of the chunk.  An event window also holds the launch gaps, which all of them carry.  Bytes from the shapes: the
                 NHWC lines of the chunk, plus the count plane read and written, plus for the intensity-scale chunk the target's
                 lines; the step reads the count plane and the target's lines; the copy moves the chunk twice.  Both chunk kernels
                 read the same member bytes, so the ratio the bytes give stands beside the measured one.
  whole function one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
                 torch.cuda.synchronize(); median and best seconds, the ratio iscale / stats, and the spread (max / min) of the stats
                 runs, which is the run-to-run noise the ratio has to be read against.

Writes profiles/iscale_bench.json."""
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

FUNCS = ("stats", "iscale")
EVENTS = ((0, 0.0, "<"),)
LEVELS = 6


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    if which == "iscale":
        return utils.modelPredIntensityScale(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, events=EVENTS,
                                             levels=LEVELS)
    return utils.modelPredStats(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


def timed(which, model, loader, S, steps, max_rows):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def chunk_alone(B, C, Hh, Ww, k, nbuf, reps):
    """The operations on nbuf distinct chunks of k members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    HW, K, S, L = Hh * Ww, len(EVENTS), k * nbuf, LEVELS
    g = torch.Generator(device="cuda").manual_seed(5)
    ys = [torch.randn((k * B, Hh, Ww, C), device="cuda", generator=g) for _ in range(nbuf)]
    tg = torch.randn((B, Hh, Ww, C), device="cuda", generator=g)
    dst = [torch.empty_like(y) for y in ys]
    thr = torch.zeros((B, K), device="cuda")
    ev = ops._ens_directions(EVENTS)
    plan = H.ens_iscale_plan(S, B, Hh, Ww, K, L)
    i64 = dict(device="cuda", dtype=torch.int64)
    member, tt, ens = torch.empty((B, K, S, L + 1, 2), **i64), torch.empty((B, K, L + 1), **i64), torch.empty((B, K, L + 1, 2), **i64)
    first = torch.empty((B, K, k, L + 1, 2), **i64)                            # the table of a step whose only chunk this is
    cnt = torch.empty((B, K, HW), device="cuda", dtype=torch.int32)
    cnt2 = torch.empty_like(cnt)
    H.ens_iscale_chunk(ys[0], tg, thr, ev, cnt, member, tt, ens, S, k, 0)      # the count and the tables are written once
    passes = {
        "event_count": lambda: [H.ens_event_count(y, thr, ev, cnt2, S, k, i * k) for i, y in enumerate(ys)],
        "iscale_chunk": lambda: [H.ens_iscale_chunk(y, tg, thr, ev, cnt, member, tt, ens, S, k, max(1, i * k) if k < S else 0) for i, y in enumerate(ys)],
        "iscale_chunk_first": lambda: [H.ens_iscale_chunk(y, tg, thr, ev, cnt, first, tt, ens, k, k, 0) for y in ys],
        "iscale_step": lambda: [H.ens_iscale_step(cnt, tg, thr, ev, ens, S) for _ in ys],
        "copy": lambda: [d.copy_(y) for d, y in zip(dst, ys)],
    }
    chunk, plane, tline = k * B * HW * C * 4, B * K * HW * 4, B * HW * C * 4
    nbytes = {"event_count": chunk + 2 * plane, "iscale_chunk": chunk + 2 * plane + tline, "iscale_chunk_first": chunk + plane + tline,
              "iscale_step": plane + tline, "copy": 2 * chunk}
    ms = {name: [] for name in passes}
    for r in range(reps + 2):
        for name in (list(passes) if r % 2 == 0 else list(passes)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            passes[name]()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ms[name].append(e0.elapsed_time(e1) / nbuf)
    row = {"members_per_chunk": k, "chunks": nbuf, "rows_per_chunk": k * B, "events": [list(e) for e in EVENTS], "levels": L,
           "plan": {key: plan[key] for key in ("blocks", "threads", "group", "lds_bytes", "step_lds_bytes")},
           "members_per_block": H.ens_iscale_plan(k, B, Hh, Ww, K, L)["group"],   # group(k): the plan's group is group(S)
           "footprint_bytes": nbuf * chunk}
    for name in passes:
        med = statistics.median(ms[name])
        row[name] = {"ms_per_call": ms[name], "ms_per_call_median": med, "bytes_per_call": nbytes[name],
                     "bytes_per_s": nbytes[name] / (med * 1e-3)}
    row["iscale_chunk_over_event_count_ms"] = row["iscale_chunk"]["ms_per_call_median"] / row["event_count"]["ms_per_call_median"]
    row["iscale_chunk_over_event_count_bytes"] = nbytes["iscale_chunk"] / nbytes["event_count"]
    row["iscale_chunk_first_over_iscale_chunk_ms"] = row["iscale_chunk_first"]["ms_per_call_median"] / row["iscale_chunk"]["ms_per_call_median"]
    row["iscale_chunk_share_of_copy_bytes_per_s"] = row["iscale_chunk"]["bytes_per_s"] / row["copy"]["bytes_per_s"]
    row["event_count_share_of_copy_bytes_per_s"] = row["event_count"]["bytes_per_s"] / row["copy"]["bytes_per_s"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--direct-reps", type=int, default=9)
    ap.add_argument("--kernels-only", action="store_true",
                    help="run the chunk-alone part and stop, writing nothing: the run to put under a kernel trace for device times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iscale_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_iscale measures on the GPU: no device found (there is no CPU path)")
    if a.kernels_only:
        print(json.dumps(chunk_alone(a.batch, 3, 256, 256, max(1, a.max_rows // a.batch), a.buffers, a.direct_reps)), flush=True)
        return
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    S = a.samples
    rec = {"what": "tmg_ens_iscale_chunk vs tmg_ens_event_count vs a device copy, tmg_ens_iscale_step; modelPredIntensityScale vs "
                   "modelPredStats; cylinder test shape",
           "device": torch.cuda.get_device_properties(0).name, "model": BE.KW,
           "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps, "samples": S},
           "events": [list(e) for e in EVENTS], "levels": LEVELS, "max_rows": a.max_rows, "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    rec["chunk_alone"] = chunk_alone(a.batch, C, 256, 256, max(1, a.max_rows // a.batch), a.buffers, a.direct_reps)
    print(json.dumps(rec["chunk_alone"]), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)                                 # (kept if the second part fails)
    for which in FUNCS:                                                        # warm-up: plans, allocator, code objects
        timed(which, model, loader, S, 3, a.max_rows)
    times = {w: [] for w in FUNCS}
    for r in range(a.reps):
        for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
            times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
    row = {"samples": S, "member_steps": S * a.steps}
    for which, ts in times.items():
        row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts)}
    row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
    row["iscale_over_stats_seconds_median"] = statistics.median(times["iscale"]) / statistics.median(times["stats"])
    row["difference_inside_stats_spread"] = bool(abs(row["iscale_over_stats_seconds_median"] - 1.0) <= row["stats_spread_max_over_min"] - 1.0)
    rec["whole_function"] = row
    print(json.dumps(row), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
