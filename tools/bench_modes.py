"""Cost of the POD projection: utils.modelPredModes beside utils.modelPredStats (unchanged by it) at the cylinder test shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the two, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratio modes / stats, and the spread (max / min) of the stats runs, which is
  the run-to-run noise the ratio has to be read against
  then one more modelPredModes run per S with a device event pair around every call of tmg_ens_pod_project (projection and fold
  together; the members' chunks and the target rows), and in the same process one modelPredEnergy run with an event pair around every
  call of tmg_ens_gram_step at the same S: calls, summed event time, microseconds per call, the projection's share of the
  modelPredModes run and the ratio of its time per kept step to the Gram step's.  An event pair also holds the launch gaps, which
  both sides of the ratio carry.
  then the projection alone on one random chunk of min(S, max_rows / B) members at the same [B, C, HW] with K modes, ALTERNATING call
  by call with a torch-native composition of the same arithmetic on the same chunk (sub, mul, matmul, and mul + sum for the energy):
  median, min and max event time of each over --direct-reps calls, the bytes the projection has to move (the rows' NHWC lines, m and
  psi once) per second, and the MFMA flops it issues (512 per 16-member tile and 64-pixel chunk of a channel) against the fp32
  matrix peak of 157.3 TFLOP/s.

Writes profiles/modes_bench.json."""
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
import bench_energy as BG     # noqa: E402  (modelPredEnergy's run)

_BQ_RUN = BQ.run
FUNCS = ("stats", "modes")
CHANNELS = (0, 1)
PEAK_F32_MATRIX = 157.3e12
MODES = [8]                   # --modes


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    if which == "modes":
        return utils.modelPredModes(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows, modes=MODES[0],
                                    channels=CHANNELS)
    if which == "energy":
        return BG.run(which, model, loader, S, steps, max_rows)
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


def direct(S, B, C, Hh, Ww, K, max_rows, reps):
    """The projection of one chunk alone, alternating with the torch composition of the same arithmetic -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(S)
    k = max(1, min(S, max_rows // B))
    HW, Cg = Hh * Ww, len(CHANNELS)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)             # noqa: E731
    en = ops.EnsembleModes(S, B, C, Hh, Ww, 1, "cuda", torch.ones(C), channels=CHANNELS, mean=rnd(B, Cg, Hh, Ww).cpu(),
                           basis=rnd(B, K, Cg, Hh, Ww).cpu())
    yn = rnd(k * B, Hh, Ww, C)                                               # the chunk, NHWC as sampleEnsemble leaves it
    ostr = (S * K, K, S, 1)
    a4, m4, psiT = en.a.view(1, B, 1, Cg), en.m.view(1, B, Cg, HW).permute(0, 1, 3, 2), en.psi.view(B, K, Cg * HW).transpose(1, 2)

    def kernel():
        H.ens_pod_project(yn, CHANNELS, en.a, en.m, en.psi, en.ws, en.coef_raw, en.en_raw, ostr, k)

    def composed():
        d = (yn.view(k, B, HW, C)[..., list(CHANNELS)] - m4) * a4              # [k, B, HW, Cg]
        dm = d.permute(1, 0, 3, 2).reshape(B, k, Cg * HW)
        return torch.bmm(dm, psiT), (dm * dm).sum(2)

    ms = {"kernel": [], "torch": []}
    for i in range(reps + 2):
        for name, f in (("kernel", kernel), ("torch", composed)) if i % 2 == 0 else (("torch", composed), ("kernel", kernel)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms[name].append(e0.elapsed_time(e1))
    c_ref, _ = composed()
    kernel()
    torch.cuda.synchronize()
    got = en.coef_raw[:, :k, 0].double()
    err = float((got - c_ref.double()).abs().max() / c_ref.double().abs().max())
    med = statistics.median(ms["kernel"])
    nbytes = (k * B * HW * C + B * Cg * HW + B * K * Cg * HW) * 4
    flops = ((k + 15) // 16) * 512 * HW * Cg * B
    row = {"samples": S, "chunk_members": k, "rows": k * B, "modes": K, "plan": en.plan, "bytes": nbytes, "mfma_flops": flops,
           "coef_max_rel_difference_to_torch": err}
    for name, v in ms.items():
        row[name] = {"event_ms": v, "event_ms_median": statistics.median(v), "event_ms_min": min(v), "event_ms_max": max(v)}
    row["bytes_per_s"] = nbytes / (med * 1e-3)
    row["flops_per_s"] = flops / (med * 1e-3)
    row["share_of_fp32_matrix_peak"] = row["flops_per_s"] / PEAK_F32_MATRIX
    row["kernel_over_torch_event_ms_median"] = med / statistics.median(ms["torch"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modes_bench.json"))
    a = ap.parse_args()
    import torch
    if not 1 <= a.modes < a.steps:
        ap.error("--modes needs 1 <= modes <= steps - 1")
    MODES[0] = a.modes
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredModes, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "pod_channels": list(CHANNELS), "modes": a.modes, "max_rows": a.max_rows, "reps": a.reps, "runs": [], "project_alone": []}
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
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["modes_over_stats_seconds_median"] = statistics.median(times["modes"]) / statistics.median(times["stats"])
        ev = event_run("modes", ("ens_pod_project",), model, loader, S, a.steps, a.max_rows)
        ev.update(event_run("energy", ("ens_gram_step",), model, loader, S, a.steps, a.max_rows))
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c} for n, (c, ms) in ev.items()}
        row["project_share_of_modes_run"] = ev["ens_pod_project"][1] / 1e3 / statistics.median(times["modes"])
        row["project_over_gram_step_event_ms_per_kept_step"] = ev["ens_pod_project"][1] / ev["ens_gram_step"][1]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.samples.split(",") if s]:
        row = direct(S, a.batch, C, 256, 256, a.modes, a.max_rows, a.direct_reps)
        rec["project_alone"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
