"""Cost of the line spectra: tmg_ens_lspec_chunk beside tmg_spec_rows + tmg_spec_cols and a device copy on the same chunks, and
utils.modelPredLineSpectra beside utils.modelPredStats (unchanged by it), at the shape of tools/bench_ensemble.py (3 channels, 64x64 ->
256x256, the field of the metric configuration, default widths, batch 4, 41 steps) with 32 members.

  chunk alone    a chunk is --max-rows rows: k = max_rows / batch whole members of [B, 256, 256, 3]; the ensemble is --samples members,
                 so samples / k distinct chunks are taken in turn, each with its own members' state (field and state together are
                 beyond the 256 MiB of the last-level cache, so a pass re-reads nothing from it).  One pass over all of them sits
                 between two device events, after two warm-up passes, --direct-reps passes per operation, the operations alternating:
                 tmg_spec_rows + tmg_spec_cols (the 2-D transform of EnsembleSpectrum on the same rows), tmg_ens_lspec_chunk as a
                 timed step after the first (it reads and writes the members' state) along x and along y, the same without the time
                 flag (the transform and the partials alone), and a device-to-device copy of the chunk.  An event window also holds
                 the launch gaps, which all of them carry.  Bytes and flops from the shapes: the chunk in full (NHWC lines are read
                 whole), 2 x 4 (3 C + 2) bytes of state per member, line and mode, the partials; 4 C L N NQP flops per image on the
                 fp32 matrix pipe.  The share of each roof: the least time at 6.29 TB/s (measured copy rate) and at 157.3 TFLOP/s.
  whole function one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
                 torch.cuda.synchronize(); median and best seconds, the ratio line spectra / stats, and the spread (max / min) of the
                 stats runs, which is the run-to-run noise the ratio has to be read against.
  resources      VGPRs and scratch of the chunk kernel from the compiler's resource usage (a cross-compile of the source with the
                 flags of tmg_hip.build; no device).

Every GPU part runs in a child process of its own under a time limit, and the first part that fails or runs out of time ends the
benchmark; what was measured until then is kept.  Writes profiles/lspec_bench.json."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-turbulence_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

FUNCS = ("stats", "lspec")
PART_LIMIT = {"chunk": 150, "whole": 420}                                     # seconds per child
HBM_BYTES_PER_S = 6.29e12
MATRIX_F32_FLOPS = 157.3e12


def run(which, model, loader, S, steps, max_rows):
    import bench_ensemble as BE
    from utils import utils
    args = SimpleNamespace(device=None, dx=1.0, dy=1.0)
    if which == "lspec":
        return utils.modelPredLineSpectra(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)
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


def chunk_alone(B, C, Hh, Ww, k, S, reps):
    """The operations on the S / k distinct chunks of k members -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    nbuf = max(1, S // k)
    S = k * nbuf
    g = torch.Generator(device="cuda").manual_seed(5)
    ys = [torch.randn((k * B, Hh, Ww, C), device="cuda", generator=g) for _ in range(nbuf)]
    dst = [torch.empty_like(y) for y in ys]
    f32 = dict(device="cuda", dtype=torch.float32)
    mu, sd = torch.zeros(C, **f32), torch.ones(C, **f32)
    NQ = Ww // 2 + 1
    F = C + 2
    plan = H.ens_lspec_plan(k, S, B, C, Hh, Ww)
    op = ops._lspec_operand(Ww, "hann").to("cuda")
    mean = torch.zeros((S, B, C, Hh, NQ, 2), **f32)
    comom = torch.zeros((S, B, F, Hh, NQ), **f32)
    part = torch.empty(plan["part_floats"], **f32)
    ft = ops._spectrum_operand(Ww, "hann").to("cuda")
    bins, kk = ops.spectrum_bins(Hh, Ww, 1.0, 1.0)
    NK = kk.numel()
    perm, offs = (t.to("cuda") for t in ops._spectrum_lists(bins, NK))
    yw = torch.empty(2 * k * B * Hh * Ww, **f32)
    spart = torch.empty(k * B * (Ww // 16) * NK, **f32)

    def spectrum(y):
        H.spec_rows(y, None, mu, sd, ft, yw, k)
        H.spec_cols(ft, yw, perm, offs, spart, k * B, Hh, Ww, NK)

    def lspec(timed_, columns):
        return lambda: [H.ens_lspec_chunk(y, None, mu, sd, op, mean, comom, part, S, k, i * k, 1, timed_, columns=columns)
                        for i, y in enumerate(ys)]
    passes = {"spec_rows_cols": lambda: [spectrum(y) for y in ys], "lspec_chunk_x": lspec(True, False), "lspec_chunk_y": lspec(True, True),
              "lspec_chunk_untimed": lspec(False, False), "copy": lambda: [d.copy_(y) for d, y in zip(dst, ys)]}
    chunk = k * B * Hh * Ww * C * 4
    state = 2 * 4 * (3 * C + 2) * k * B * Hh * NQ                               # read and written
    pbytes = plan["part_floats"] * 4
    lflops = 4 * C * Hh * Ww * plan["nqp"] * k * B
    nbytes = {"spec_rows_cols": chunk + 2 * yw.numel() * 4 + spart.numel() * 4, "lspec_chunk_x": chunk + state + pbytes,
              "lspec_chunk_y": chunk + state + pbytes, "lspec_chunk_untimed": chunk + pbytes, "copy": 2 * chunk}
    flops = {"spec_rows_cols": 16 * Hh * Ww * (Hh + Ww) * k * B, "lspec_chunk_x": lflops, "lspec_chunk_y": lflops,
             "lspec_chunk_untimed": lflops, "copy": 0}
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
    row = {"members": S, "members_per_chunk": k, "chunks": nbuf, "rows_per_chunk": k * B, "field": [Hh, Ww, C],
           "plan": {key: plan[key] for key in ("tiles", "mode_tiles", "threads", "lds_bytes", "nq", "nqp")},
           "blocks_per_call": plan["grid_x"] * plan["grid_y"], "footprint_bytes": nbuf * chunk + 4 * (mean.numel() + comom.numel())}
    for name in passes:
        med = statistics.median(ms[name])
        least = max(nbytes[name] / HBM_BYTES_PER_S, flops[name] / MATRIX_F32_FLOPS)
        row[name] = {"ms_per_call": ms[name], "ms_per_call_median": med, "bytes_per_call": nbytes[name], "flops_per_call": flops[name],
                     "bytes_per_s": nbytes[name] / (med * 1e-3), "flops_per_s": flops[name] / (med * 1e-3),
                     "share_of_memory_roof": nbytes[name] / HBM_BYTES_PER_S / (med * 1e-3),
                     "share_of_matrix_roof": flops[name] / MATRIX_F32_FLOPS / (med * 1e-3),
                     "bound_by": "bytes" if nbytes[name] / HBM_BYTES_PER_S >= flops[name] / MATRIX_F32_FLOPS else "flops",
                     "share_of_roof": least / (med * 1e-3)}
    row["lspec_chunk_over_spec_rows_cols_ms"] = row["lspec_chunk_x"]["ms_per_call_median"] / row["spec_rows_cols"]["ms_per_call_median"]
    row["lspec_chunk_over_copy_ms"] = row["lspec_chunk_x"]["ms_per_call_median"] / row["copy"]["ms_per_call_median"]
    row["lspec_chunk_y_over_x_ms"] = row["lspec_chunk_y"]["ms_per_call_median"] / row["lspec_chunk_x"]["ms_per_call_median"]
    row["state_share_of_chunk_ms"] = 1.0 - row["lspec_chunk_untimed"]["ms_per_call_median"] / row["lspec_chunk_x"]["ms_per_call_median"]
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
    row["lspec_over_stats_seconds_median"] = statistics.median(times["lspec"]) / statistics.median(times["stats"])
    row["difference_inside_stats_spread"] = bool(abs(row["lspec_over_stats_seconds_median"] - 1.0) <= row["stats_spread_max_over_min"] - 1.0)
    return row


def resources():
    """{kernel: {vgprs, scratch_bytes_per_lane, occupancy_waves_per_simd}} of tmg_lspec.hip from the compiler's resource usage."""
    import tmg_hip as H
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result", "-I", os.path.join(ROOT, "include")]
    if "tmg_lspec.hip" in H.NO_PACKED_F32:
        cmd += ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
    cmd += ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(H.CSRC, "tmg_lspec.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=300)
    out, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, ln)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def child(a):
    """One part, in this process: its JSON row is the last line printed."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_lspec measures on the GPU: no device found (there is no CPU path)")
    if a.part == "whole":
        row = whole_function(a)
    else:
        row = chunk_alone(a.batch, 3, 256, 256, max(1, a.max_rows // a.batch), a.samples, a.direct_reps)
        row["device"] = torch.cuda.get_device_properties(0).name
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--direct-reps", type=int, default=9)
    ap.add_argument("--part", choices=("chunk", "whole"), default=None,
                    help="run that part alone in this process and print its row, writing nothing: the chunk part is the run to put "
                         "under a kernel trace or a counter collection")
    ap.add_argument("--skip-whole", action="store_true", help="the chunk-alone part only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lspec_bench.json"))
    a = ap.parse_args()
    if a.part:
        child(a)
        return
    rec = {"what": "tmg_ens_lspec_chunk vs tmg_spec_rows + tmg_spec_cols vs a device copy; modelPredLineSpectra vs modelPredStats; "
                   "cylinder test shape", "max_rows": a.max_rows, "reps": a.reps,
           "roofs": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "matrix_f32_flops_per_s": MATRIX_F32_FLOPS}, "resources": resources()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    passed = [sys.executable, os.path.abspath(__file__)] + [w for key in ("samples", "steps", "batch", "reps", "max_rows", "direct_reps")
                                                             for w in ("--" + key.replace("_", "-"), str(getattr(a, key)))]
    for part in ("chunk",) + (() if a.skip_whole else ("whole",)):
        limit = PART_LIMIT[part]
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
            rec["chunk_alone"] = row
        print(json.dumps(row), flush=True)
        json.dump(rec, open(a.out, "w"), indent=1)                             # (kept if a later part fails)


if __name__ == "__main__":
    main()
