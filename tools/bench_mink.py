"""Cost of the excursion-set morphology (Minkowski functionals): tmg_ens_mink_chunk beside tmg_ens_event_count on the same chunks, and
utils.modelPredMorphology beside utils.modelPredStats (unchanged by it), at the shape of tools/bench_ensemble.py (3 channels, 64x64 ->
256x256, the field of the metric configuration, default widths, batch 4, 41 steps) with 32 members, F = 3 fields and J = 16 levels.

  chunk alone    a chunk is --max-rows rows: k = max_rows / batch whole members of [B, 256, 256, 3].  --buffers distinct chunks
                 (together beyond the 256 MiB of the last-level cache, so a pass re-reads nothing from it) are taken in turn; one pass
                 over all of them sits between two device events, after two warm-up passes, --direct-reps passes per operation, the
                 operations alternating: tmg_ens_event_count (reads the same NHWC rows, one event), tmg_ens_mink_chunk as a later
                 chunk of its step (m0 > 0: no zeroing launch, no target row), the same as the step's first chunk (m0 = 0: the zeroing
                 launch and the target's blocks), and a device-to-device copy of the chunk.  An event window also holds the launch
                 gaps, which all of them carry.  Bytes from the shapes: the NHWC lines of the chunk (both kernels read each line
                 once, whatever the number of fields), plus for the event count its count plane read and written, plus for the first
                 chunk the target's lines and the table; the copy moves the chunk twice.  Two kinds of data, the extremes of the
                 histogram traffic: `noise` (independent normal pixels: the rank changes at every pixel, every pixel is an LDS
                 atomic, spread over the bins) and `smooth` (a few long waves plus 2 % noise: long runs of one rank down a column, an
                 atomic only where a contour crosses).
  whole function one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
                 torch.cuda.synchronize(); median and best seconds, the ratio morphology / stats, and the spread (max / min) of the
                 stats runs, which is the run-to-run noise the ratio has to be read against.

Writes profiles/mink_bench.json."""
import argparse
import json
import math
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

FUNCS = ("stats", "morphology")
FIELDS = (0, 1, 2)
LEVELS = 16
EVENTS = ((0, 0.0, "<"),)


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=1.0, dy=1.0)
    if which == "morphology":
        return utils.modelPredMorphology(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, fields=FIELDS,
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


def fields_of(kind, n, Hh, Ww, C, g):
    """n rows [n, H, W, C] of unit variance: independent pixels, or three long waves of random phase and direction plus 2 % noise."""
    import torch
    noise = torch.randn((n, Hh, Ww, C), device="cuda", generator=g)
    if kind == "noise":
        return noise
    yy = torch.arange(Hh, device="cuda", dtype=torch.float32).view(1, Hh, 1, 1)
    xx = torch.arange(Ww, device="cuda", dtype=torch.float32).view(1, 1, Ww, 1)
    v = torch.zeros((n, Hh, Ww, C), device="cuda")
    for _ in range(3):
        kx, ky, ph = (torch.rand((n, 1, 1, C), device="cuda", generator=g) for _ in range(3))
        v += torch.sin(2 * math.pi * ((4 * kx - 2) * xx / Ww + (4 * ky - 2) * yy / Hh + ph))
    return v * (2.0 / 3.0) ** 0.5 + 0.02 * noise


def chunk_alone(kind, B, C, Hh, Ww, k, nbuf, reps):
    """The operations on nbuf distinct chunks of k members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    HW, F, J, S = Hh * Ww, len(FIELDS), LEVELS, k * nbuf
    g = torch.Generator(device="cuda").manual_seed(5)
    ys = [fields_of(kind, k * B, Hh, Ww, C, g) for _ in range(nbuf)]
    tg = fields_of(kind, B, Hh, Ww, C, g)
    dst = [torch.empty_like(y) for y in ys]
    thr = torch.linspace(-2.0, 2.0, J, device="cuda").view(1, 1, J).repeat(B, F, 1).contiguous()
    thr1 = torch.zeros((B, 1), device="cuda")
    ev = ops._ens_directions(EVENTS)
    plan = H.ens_mink_plan(S, B, Hh, Ww, F, J)
    table = torch.empty((B, F, S + 1, J, 5), device="cuda", dtype=torch.int64)
    first = torch.empty((B, F, k + 1, J, 5), device="cuda", dtype=torch.int64)  # the table of a step whose only chunk this is
    cnt = torch.empty((B, 1, HW), device="cuda", dtype=torch.int32)
    H.ens_mink_chunk(ys[0], tg, thr, FIELDS, table, S, k, 0)                  # the table is zeroed once
    passes = {
        "event_count": lambda: [H.ens_event_count(y, thr1, ev, cnt, S, k, i * k) for i, y in enumerate(ys)],
        "mink_chunk": lambda: [H.ens_mink_chunk(y, tg, thr, FIELDS, table, S, k, max(1, i * k) if k < S else 0) for i, y in enumerate(ys)],
        "mink_chunk_first": lambda: [H.ens_mink_chunk(y, tg, thr, FIELDS, first, k, k, 0) for y in ys],
        "copy": lambda: [d.copy_(y) for d, y in zip(dst, ys)],
    }
    chunk, plane, tline = k * B * HW * C * 4, B * HW * 4, B * HW * C * 4
    nbytes = {"event_count": chunk + 2 * plane, "mink_chunk": chunk, "mink_chunk_first": chunk + tline + first.numel() * 8, "copy": 2 * chunk}
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
    row = {"data": kind, "members_per_chunk": k, "chunks": nbuf, "rows_per_chunk": k * B, "fields": list(FIELDS), "levels": J,
           "plan": {key: plan[key] for key in ("tile_h", "tile_w", "tiles_x", "tiles_y", "threads", "group", "lds_bytes")},
           "members_per_block": H.ens_mink_plan(k, B, Hh, Ww, F, J)["group"],   # group(k): the plan's group is group(S)
           "footprint_bytes": nbuf * chunk, "table_nonzero_share": float((table != 0).double().mean())}
    for name in passes:
        med = statistics.median(ms[name])
        row[name] = {"ms_per_call": ms[name], "ms_per_call_median": med, "bytes_per_call": nbytes[name],
                     "bytes_per_s": nbytes[name] / (med * 1e-3)}
    row["mink_chunk_over_event_count_ms"] = row["mink_chunk"]["ms_per_call_median"] / row["event_count"]["ms_per_call_median"]
    row["mink_chunk_over_event_count_bytes"] = nbytes["mink_chunk"] / nbytes["event_count"]
    row["mink_chunk_first_over_mink_chunk_ms"] = row["mink_chunk_first"]["ms_per_call_median"] / row["mink_chunk"]["ms_per_call_median"]
    row["mink_chunk_share_of_copy_bytes_per_s"] = row["mink_chunk"]["bytes_per_s"] / row["copy"]["bytes_per_s"]
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
    ap.add_argument("--kernels-only", choices=("noise", "smooth"), default=None,
                    help="run the chunk-alone part on that data and stop, writing nothing: the run to put under a kernel trace or a "
                         "counter collection")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mink_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_mink measures on the GPU: no device found (there is no CPU path)")
    k = max(1, a.max_rows // a.batch)
    if a.kernels_only:
        print(json.dumps(chunk_alone(a.kernels_only, a.batch, 3, 256, 256, k, a.buffers, a.direct_reps)), flush=True)
        return
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    S = a.samples
    rec = {"what": "tmg_ens_mink_chunk vs tmg_ens_event_count vs a device copy; modelPredMorphology vs modelPredStats; cylinder test shape",
           "device": torch.cuda.get_device_properties(0).name, "model": BE.KW,
           "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps, "samples": S},
           "fields": list(FIELDS), "levels": LEVELS, "max_rows": a.max_rows, "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    rec["chunk_alone"] = [chunk_alone(kind, a.batch, C, 256, 256, k, a.buffers, a.direct_reps) for kind in ("noise", "smooth")]
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
    row["morphology_over_stats_seconds_median"] = statistics.median(times["morphology"]) / statistics.median(times["stats"])
    row["difference_inside_stats_spread"] = bool(abs(row["morphology_over_stats_seconds_median"] - 1.0) <= row["stats_spread_max_over_min"] - 1.0)
    rec["whole_function"] = row
    print(json.dumps(row), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
