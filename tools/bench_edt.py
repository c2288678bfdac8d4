"""Cost of the distance-map verification: tmg_ens_edt_chunk beside tmg_ens_event_count and a device copy on the same chunks, and
utils.modelPredDistance beside utils.modelPredStats (unchanged by it), at the shape of tools/bench_ensemble.py (3 channels, 64x64 ->
256x256, the field of the metric configuration, default widths, batch 4, 41 steps) with 32 members and one event.

  chunk alone    a chunk is --max-rows rows: k = max_rows / batch whole members of [B, 256, 256, 3].  --buffers distinct chunks
                 (together beyond the 256 MiB of the last-level cache, so a pass re-reads nothing from it) are taken in turn; one pass
                 over all of them sits between two device events, after two warm-up passes, --direct-reps passes per operation, the
                 operations alternating: tmg_ens_event_count (reads the same NHWC rows, one event), tmg_ens_edt_chunk as a later
                 chunk of its step (m0 > 0: the mask and the members' distance launch), the same as the step's first chunk (m0 = 0:
                 the preset launch, the target's words and the target's distance launch as well), and a device-to-device copy of the
                 chunk.  An event window also holds the launch gaps, which all of them carry.  Bytes from the shapes: the event's
                 channel is read through whole NHWC lines, so the chunk counts in full; the distance kernel adds the indicator
                 words (written, then read), the target's map (read) and the member sum (an atomic add: read and written) per
                 member.  Four kinds of data, which differ in the length of the search, not in the bytes:
                   noise   independent normal pixels against 0: half of them set, every distance near 0, the walk ends at once
                   smooth  a few long waves: one or two large connected sets, distances up to tens of pixels
                   sparse  one set pixel per field: the worst case, every pixel walks every row of every tile
                   empty   no set pixel: the count is 0 and the search is skipped
  whole function one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
                 torch.cuda.synchronize(); median and best seconds, the ratio distance / stats, and the spread (max / min) of the
                 stats runs, which is the run-to-run noise the ratio has to be read against.

Every part runs in a child process of its own under a time limit, and the first part that fails or runs out of time ends the
benchmark; what was measured until then is kept.  Writes profiles/edt_bench.json."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-turbulence_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

FUNCS = ("stats", "distance")
EVENTS = ((0, 0.0, "<"),)
KINDS = ("noise", "smooth", "sparse", "empty")
PART_LIMIT = {"chunk": 120, "whole": 420}                                     # seconds per child


def run(which, model, loader, S, steps, max_rows):
    import bench_ensemble as BE
    from utils import utils
    args = SimpleNamespace(device=None, dx=1.0, dy=1.0)
    if which == "distance":
        return utils.modelPredDistance(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, events=EVENTS)
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
    """n rows [n, H, W, C]; the event is channel 0 below 0."""
    import torch
    if kind == "noise":
        return torch.randn((n, Hh, Ww, C), device="cuda", generator=g)
    if kind == "empty":
        return torch.ones((n, Hh, Ww, C), device="cuda")
    if kind == "sparse":
        v = torch.ones((n, Hh, Ww, C), device="cuda")
        at = torch.randint(0, Hh * Ww, (n,), device="cuda", generator=g)
        v.view(n, Hh * Ww, C)[torch.arange(n, device="cuda"), at, 0] = -1.0
        return v
    yy = torch.arange(Hh, device="cuda", dtype=torch.float32).view(1, Hh, 1, 1)
    xx = torch.arange(Ww, device="cuda", dtype=torch.float32).view(1, 1, Ww, 1)
    v = torch.zeros((n, Hh, Ww, C), device="cuda")
    for _ in range(2):
        kx, ky, ph = (torch.rand((n, 1, 1, C), device="cuda", generator=g) for _ in range(3))
        v += torch.sin(2 * math.pi * ((2 * kx - 1) * xx / Ww + (2 * ky - 1) * yy / Hh + ph))
    return v


def chunk_alone(kind, B, C, Hh, Ww, k, nbuf, reps):
    """The operations on nbuf distinct chunks of k members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    HW, K, S = Hh * Ww, len(EVENTS), k * nbuf
    c = ops.dist_args(EVENTS, None, (0.5,), C, Hh, Ww)[1]
    g = torch.Generator(device="cuda").manual_seed(5)
    ys = [fields_of(kind, k * B, Hh, Ww, C, g) for _ in range(nbuf)]
    tg = fields_of(kind, B, Hh, Ww, C, g)
    dst = [torch.empty_like(y) for y in ys]
    thr = torch.zeros((B, K), device="cuda")
    ev = ops._ens_directions(EVENTS)
    plan = H.ens_edt_plan(S, B, Hh, Ww, K, c)
    i32, i64 = dict(device="cuda", dtype=torch.int32), dict(device="cuda", dtype=torch.int64)

    def buffers(s):
        return dict(scratch=torch.empty((s + 1, B, K, Hh, plan["strips"]), **i64), count=torch.empty((B, K, s + 1), **i32),
                    dmap=torch.empty((B, K, HW), **i32), msum=torch.empty((B, K, HW), **i32), pair=torch.empty((B, K, s, 11), **i64),
                    hist=torch.empty((B, K, s, 2, c + 1), **i64))
    full, first = buffers(S), buffers(k)                                      # a step of all the chunks; a step whose only chunk this is
    cnt = torch.empty((B, 1, HW), **i32)
    H.ens_edt_chunk(ys[0], tg, thr, ev, S=S, k=k, m0=0, **full)               # the step is preset once
    passes = {
        "event_count": lambda: [H.ens_event_count(y, thr, ev, cnt, S, k, i * k) for i, y in enumerate(ys)],
        "edt_chunk": lambda: [H.ens_edt_chunk(y, tg, thr, ev, S=S, k=k, m0=max(1, i * k) if k < S else 0, **full) for i, y in enumerate(ys)],
        "edt_chunk_first": lambda: [H.ens_edt_chunk(y, tg, thr, ev, S=k, k=k, m0=0, **first) for y in ys],
        "copy": lambda: [d.copy_(y) for d, y in zip(dst, ys)],
    }
    chunk, plane, tline, words = k * B * HW * C * 4, B * HW * 4, B * HW * C * 4, B * K * Hh * plan["strips"] * 8
    per_member = 2 * words + 3 * K * plane                                    # words written and read, the target's map, the member sum
    nbytes = {"event_count": chunk + 2 * plane, "edt_chunk": chunk + k * per_member,
              "edt_chunk_first": chunk + tline + (k + 1) * per_member + 2 * K * plane + first["pair"].numel() * 8 + first["hist"].numel() * 8,
              "copy": 2 * chunk}
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
    row = {"data": kind, "members_per_chunk": k, "chunks": nbuf, "rows_per_chunk": k * B, "events": [list(e) for e in EVENTS], "cutoff": c,
           "plan": {key: plan[key] for key in ("tile_w", "band", "strips", "bands", "threads", "lds_bytes")},
           "distance_blocks_per_call": plan["strips"] * plan["bands"] * K * k * B, "footprint_bytes": nbuf * chunk,
           "set_share": float(first["pair"][..., 0].double().mean() / HW)}   # (of the last first-chunk call: its step is preset)
    hmax = first["pair"][..., 9:]
    finite = hmax[(hmax >= 0) & (hmax < ops.DIST_INF)]
    row["largest_finite_hausdorff_pixels"] = float(finite.max().double().sqrt()) if finite.numel() else None
    for name in passes:
        med = statistics.median(ms[name])
        row[name] = {"ms_per_call": ms[name], "ms_per_call_median": med, "bytes_per_call": nbytes[name],
                     "bytes_per_s": nbytes[name] / (med * 1e-3)}
    row["edt_chunk_over_event_count_ms"] = row["edt_chunk"]["ms_per_call_median"] / row["event_count"]["ms_per_call_median"]
    row["edt_chunk_over_event_count_bytes"] = nbytes["edt_chunk"] / nbytes["event_count"]
    row["edt_chunk_over_copy_ms"] = row["edt_chunk"]["ms_per_call_median"] / row["copy"]["ms_per_call_median"]
    row["edt_chunk_first_over_edt_chunk_ms"] = row["edt_chunk_first"]["ms_per_call_median"] / row["edt_chunk"]["ms_per_call_median"]
    return row


def whole_function(a):
    import bench_ensemble as BE
    model, loader = BE.setup(a.batch, a.steps)
    S = a.samples
    for which in FUNCS:                                                        # warm-up: plans, allocator, code objects
        timed(which, model, loader, S, 3, a.max_rows)
    times = {w: [] for w in FUNCS}
    for r in range(a.reps):
        for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
            times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
    row = {"samples": S, "member_steps": S * a.steps, "model": BE.KW,
           "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": int(loader[0][1].shape[2]), "steps": a.steps}}
    for which, ts in times.items():
        row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts)}
    row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
    row["distance_over_stats_seconds_median"] = statistics.median(times["distance"]) / statistics.median(times["stats"])
    row["difference_inside_stats_spread"] = bool(abs(row["distance_over_stats_seconds_median"] - 1.0) <= row["stats_spread_max_over_min"] - 1.0)
    return row


def child(a):
    """One part, in this process: its JSON row is the last line printed."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_edt measures on the GPU: no device found (there is no CPU path)")
    k = max(1, a.max_rows // a.batch)
    if a.part == "whole":
        row = whole_function(a)
    else:
        row = chunk_alone(a.part, a.batch, 3, 256, 256, k, a.buffers, a.direct_reps)
        row["device"] = torch.cuda.get_device_properties(0).name
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--buffers", type=int, default=8)
    ap.add_argument("--direct-reps", type=int, default=9)
    ap.add_argument("--part", choices=KINDS + ("whole",), default=None,
                    help="run that part alone in this process and print its row, writing nothing: a chunk-alone kind is the run to put "
                         "under a kernel trace or a counter collection")
    ap.add_argument("--skip-whole", action="store_true", help="the chunk-alone parts only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_bench.json"))
    a = ap.parse_args()
    if a.part:
        child(a)
        return
    rec = {"what": "tmg_ens_edt_chunk vs tmg_ens_event_count vs a device copy; modelPredDistance vs modelPredStats; cylinder test shape",
           "events": [list(e) for e in EVENTS], "max_rows": a.max_rows, "reps": a.reps, "chunk_alone": []}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    passed = [sys.executable, os.path.abspath(__file__)] + [w for key in ("samples", "steps", "batch", "reps", "max_rows", "buffers", "direct_reps")
                                                             for w in ("--" + key.replace("_", "-"), str(getattr(a, key)))]
    for part in KINDS + (() if a.skip_whole else ("whole",)):
        limit = PART_LIMIT["whole" if part == "whole" else "chunk"]
        try:
            r = subprocess.run(passed + ["--part", part], stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            rec["stopped"] = "%s ran past its %d s" % (part, limit)
        else:
            if r.returncode != 0:
                rec["stopped"] = "%s ended with status %d" % (part, r.returncode)
        if "stopped" in rec:
            print(rec["stopped"], flush=True)
            json.dump(rec, open(a.out, "w"), indent=1)
            sys.exit(1)
        row = json.loads(r.stdout.strip().splitlines()[-1])
        if part == "whole":
            rec["whole_function"] = row
        else:
            rec["device"] = row.pop("device")
            rec["chunk_alone"].append(row)
        print(json.dumps(row), flush=True)
        json.dump(rec, open(a.out, "w"), indent=1)                             # (kept if a later part fails)


if __name__ == "__main__":
    main()
