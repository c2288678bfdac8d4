"""Cost of the event durations (spells, gaps, persistence): tmg_ens_spell_step beside tmg_ens_event_count on the same chunks, and
utils.modelPredSpells beside utils.modelPredStats (unchanged by it), at the shape of tools/bench_ensemble.py (3 channels, 64x64 ->
256x256, the field of the metric configuration, default widths, batch 4, 41 steps, the reverse-flow event) with 32 members.

  step alone     a chunk is --max-rows rows: k = max_rows / batch whole members of [B, 256, 256, 3].  --buffers distinct chunks with
                 their own state rows (together beyond the 256 MiB of the last-level cache, so a pass re-reads nothing from it) are
                 taken in turn; one pass over all of them sits between two device events, after two warm-up passes, --direct-reps
                 passes per operation, the operations alternating: tmg_ens_event_count (reads the same NHWC rows), the
                 tmg_ens_spell_step of a later window step (the state is read and written) on the chunks of the step before, so
                 that no run ends, the same on independent chunks in turn, so that every other pixel ends a run (the most LDS
                 atomics a step can meet), and a device-to-device copy of the chunk.  An event window also holds the launch gaps,
                 which all of them carry.  Bytes from the shapes: the NHWC lines of
                 the chunk, plus for the count its plane read and written, plus for the spell step 8 bytes of state per (member,
                 event, pixel) and its two map planes read and written; the copy moves the chunk twice.
  whole function one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
                 torch.cuda.synchronize(); median and best seconds, the ratio spells / stats, and the spread (max / min) of the stats
                 runs, which is the run-to-run noise the ratio has to be read against.

Writes profiles/spells_bench.json."""
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

FUNCS = ("stats", "spells")
EVENTS = ((0, 0.0, "<"),)
MAX_LEN = 32


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    if which == "spells":
        return utils.modelPredSpells(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, events=EVENTS,
                                     max_len=MAX_LEN)
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


def step_alone(B, C, Hh, Ww, k, nbuf, reps):
    """The three operations on nbuf distinct chunks of k members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    HW, K, S, Tn = Hh * Ww, len(EVENTS), k * nbuf, 32767
    g = torch.Generator(device="cuda").manual_seed(5)
    ys = [torch.randn((k * B, Hh, Ww, C), device="cuda", generator=g) for _ in range(nbuf)]
    dst = [torch.empty_like(y) for y in ys]
    thr = torch.zeros((B, K), device="cuda")
    ev = ops._ens_directions(EVENTS)
    plan = H.ens_spell_plan(S, B, HW, K, MAX_LEN, Tn)
    state = torch.empty((S + 1, B, K, HW), device="cuda", dtype=torch.int32)
    table = torch.empty((B, K, S + 1, 2, MAX_LEN + 7), device="cuda", dtype=torch.int64)
    maps = torch.empty((H.SPELL_MAPS, B, K, HW), device="cuda", dtype=torch.int32)
    cnt = torch.empty((B, K, HW), device="cuda", dtype=torch.int32)
    # two states: one is fed the same chunks every step (no run ever ends: the persistent flow the feature is for), the other is fed
    # independent chunks in turn (every other pixel ends a run at every step: the most LDS atomics a step can meet)
    ys2 = [torch.randn((k * B, Hh, Ww, C), device="cuda", generator=g) for _ in range(nbuf)]
    state2 = torch.empty_like(state)
    table2, maps2 = torch.empty_like(table), torch.empty_like(maps)
    for i, y in enumerate(ys):                                                 # step 0 writes the state
        H.ens_spell_step(y, thr, ev, state, table, maps, S, k, i * k, Tn, 0)
        H.ens_spell_step(y, thr, ev, state2, table2, maps2, S, k, i * k, Tn, 0)
    turn = [0]

    def flipping():
        turn[0] += 1
        for i, y in enumerate(ys2 if turn[0] % 2 else ys):
            H.ens_spell_step(y, thr, ev, state2, table2, maps2, S, k, i * k, Tn, 1)

    passes = {
        "event_count": lambda: [H.ens_event_count(y, thr, ev, cnt, S, k, i * k) for i, y in enumerate(ys)],
        "spell_step": lambda: [H.ens_spell_step(y, thr, ev, state, table, maps, S, k, i * k, Tn, 1) for i, y in enumerate(ys)],
        "spell_step_flipping": flipping,
        "copy": lambda: [d.copy_(y) for d, y in zip(dst, ys)],
    }
    chunk = k * B * HW * C * 4
    nbytes = {"event_count": chunk + 2 * B * K * HW * 4, "spell_step": chunk + 8 * k * B * K * HW + 4 * B * K * HW * 4, "copy": 2 * chunk}
    nbytes["spell_step_flipping"] = nbytes["spell_step"]
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
    row = {"members_per_chunk": k, "chunks": nbuf, "rows_per_chunk": k * B, "events": [list(e) for e in EVENTS], "max_len": MAX_LEN,
           "plan": {key: plan[key] for key in ("blocks", "threads", "group", "lds_bytes")},
           "footprint_bytes": nbuf * chunk + state.numel() * 4}
    for name in passes:
        med = statistics.median(ms[name])
        row[name] = {"ms_per_call": ms[name], "ms_per_call_median": med, "bytes_per_call": nbytes[name],
                     "bytes_per_s": nbytes[name] / (med * 1e-3)}
    row["spell_step_over_event_count_ms"] = row["spell_step"]["ms_per_call_median"] / row["event_count"]["ms_per_call_median"]
    row["spell_step_over_event_count_bytes"] = nbytes["spell_step"] / nbytes["event_count"]
    row["spell_step_flipping_over_spell_step_ms"] = row["spell_step_flipping"]["ms_per_call_median"] / row["spell_step"]["ms_per_call_median"]
    row["spell_step_share_of_copy_bytes_per_s"] = row["spell_step"]["bytes_per_s"] / row["copy"]["bytes_per_s"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spells_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_spells measures on the GPU: no device found (there is no CPU path)")
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    S = a.samples
    rec = {"what": "tmg_ens_spell_step vs tmg_ens_event_count vs a device copy; modelPredSpells vs modelPredStats; cylinder test shape",
           "device": torch.cuda.get_device_properties(0).name, "model": BE.KW,
           "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps, "samples": S},
           "events": [list(e) for e in EVENTS], "max_len": MAX_LEN, "max_rows": a.max_rows, "reps": a.reps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    rec["step_alone"] = step_alone(a.batch, C, 256, 256, max(1, a.max_rows // a.batch), a.buffers, a.direct_reps)
    print(json.dumps(rec["step_alone"]), flush=True)
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
    row["spells_over_stats_seconds_median"] = statistics.median(times["spells"]) / statistics.median(times["stats"])
    row["difference_inside_stats_spread"] = bool(abs(row["spells_over_stats_seconds_median"] - 1.0) <= row["stats_spread_max_over_min"] - 1.0)
    rec["whole_function"] = row
    print(json.dumps(row), flush=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
