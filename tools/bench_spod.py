"""Cost of the spectral POD: utils.modelPredSpod beside utils.modelPredTimeSpectra and utils.modelPredStats (both unchanged by it) at
the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32
members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the three, each window closed by
  torch.cuda.synchronize(); median and best seconds, seconds per kept step (the feeding cost: the SPOD feeds one more row per step than
  the temporal spectra, the target's), the ratios to stats and the spread (max / min) of the stats runs, which is the run-to-run noise
  the ratios have to be read against
  then one more modelPredSpod run per S with a device event pair around every call of tmg_ens_spod_csd and tmg_ens_spod_modes and a
  host timer around tmg_ops.spod_decompose (fp64 eigh on the CPU, with the leave-one-out): the finalize cost, once per mini-batch
  then the two kernels alone on a random accumulator [2 NF + 1, S + 1, B, C, HW] at the same shape with the default bins and modes,
  ALTERNATING call by call with a torch composition of the same arithmetic on the read-back accumulator (the correction, then a complex
  einsum): median, min and max event time of each, and the algorithmic flops (CSD: the upper triangle of the 2 R x 2 R Gram, 2 flops
  per product; modes: 2 J x 2 S) against the fp32 matrix peak of 157.3 TFLOP/s.

Writes profiles/spod_bench.json."""
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
import bench_quant as BQ      # noqa: E402  (the event wrapper)

FUNCS = ("stats", "tspec", "spod")
CHANNELS = (0, 1)
PEAK_F32_MATRIX = 157.3e12
MODES = [4]                   # --modes


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    kw = dict(samples=S, stride=1, tmax=steps, max_rows=max_rows)
    if which == "spod":
        return utils.modelPredSpod(args, model, loader, BE.LOG, modes=MODES[0], channels=CHANNELS, **kw)
    if which == "tspec":
        return utils.modelPredTimeSpectra(args, model, loader, BE.LOG, nfreq=17, **kw)
    return utils.modelPredStats(args, model, loader, BE.LOG, **kw)


def timed(which, model, loader, S, steps, max_rows):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(which, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def event_run(names, model, loader, S, steps, max_rows):
    """One modelPredSpod run with event pairs around the binding functions `names` and a host timer around spod_decompose."""
    import tmg_ops as ops
    saved, orig, host = BQ.run, ops.spod_decompose, []

    def decompose(*a, **k):
        t0 = time.perf_counter()
        o = orig(*a, **k)
        host.append(time.perf_counter() - t0)
        return o

    BQ.run, ops.spod_decompose = run, decompose
    try:
        ev = BQ.event_run("spod", names, model, loader, S, steps, max_rows)
    finally:
        BQ.run, ops.spod_decompose = saved, orig
    return ev, host


def direct(S, B, C, Hh, Ww, Tn, J, reps):
    """The two kernels alone, alternating with the torch composition of the same arithmetic -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(S)
    sp = ops.EnsembleSpod(S, B, C, Hh, Ww, Tn, "cuda", torch.zeros(C), torch.ones(C), modes=J, channels=CHANNELS)
    R, HW, NF, NB, Cg = S + 1, Hh * Ww, sp.NF, len(sp.bins), len(CHANNELS)
    sp.acc.copy_(torch.randn(sp.acc.shape, device="cuda", generator=g))
    raw = torch.empty((B, NB, 2, R, R), device="cuda")
    SP = (S + 3) // 4 * 4
    wc = torch.complex(torch.randn((B, NB, S, J), device="cuda", generator=g), torch.randn((B, NB, S, J), device="cuda", generator=g))
    wr = torch.zeros((B, NB, 16, 2 * SP), device="cuda")
    wt = wc.transpose(2, 3)
    wr[:, :, 0:2 * J:2, :S], wr[:, :, 0:2 * J:2, SP:SP + S] = wt.real, -wt.imag
    wr[:, :, 1:2 * J:2, :S], wr[:, :, 1:2 * J:2, SP:SP + S] = wt.imag, wt.real
    modes = torch.empty((B, NB, 2 * J, Cg, HW), device="cuda")
    bins, inv_t = list(sp.bins), torch.tensor(1.0 / Tn, device="cuda")

    def coef():
        xbar = sp.acc[2 * NF] * inv_t                                       # [R, B, C, HW]
        re = sp.acc[bins] - xbar * sp.cst[0, bins].view(-1, 1, 1, 1, 1)
        im = sp.acc[[NF + k for k in bins]] - xbar * sp.cst[1, bins].view(-1, 1, 1, 1, 1)
        return torch.complex(re, im)[:, :, :, list(CHANNELS)].reshape(NB, R, B, Cg * HW)

    fns = {"csd": (lambda: H.ens_spod_csd(sp.acc, sp.cst, sp.bins, sp.channels, sp.ws, raw, Tn),
                   lambda: torch.einsum("kmbe,knbe->bkmn", coef().conj(), coef())),
           "modes": (lambda: H.ens_spod_modes(sp.acc, sp.cst, sp.bins, sp.channels, wr, modes, Tn),
                     lambda: torch.einsum("bkmj,kmbe->bkje", wc, coef()[:, :S]))}
    flops = {"csd": 2 * (2 * R) * (2 * R + 1) // 2 * Cg * HW * B * NB, "modes": 2 * (2 * J) * (2 * S) * Cg * HW * B * NB}
    row = {"samples": S, "rows": R, "bins": NB, "n_modes": J, "plan": sp.plan, "acc_bytes": sp.acc.numel() * 4}
    for name, (kernel, composed) in fns.items():
        ms = {"kernel": [], "torch": []}
        for i in range(reps + 2):
            for who, f in (("kernel", kernel), ("torch", composed)) if i % 2 == 0 else (("torch", composed), ("kernel", kernel)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ms[who].append(e0.elapsed_time(e1))
        ref = composed()
        kernel()
        torch.cuda.synchronize()
        if name == "csd":
            got = torch.complex(raw[:, :, 0], raw[:, :, 1])
        else:
            m = modes.view(B, NB, J, 2, Cg * HW)
            got = torch.complex(m[:, :, :, 0], m[:, :, :, 1])
        med = statistics.median(ms["kernel"])
        r = {"flops": flops[name], "max_rel_difference_to_torch": float((got - ref).abs().max() / ref.abs().max())}
        for who, v in ms.items():
            r[who] = {"event_ms": v, "event_ms_median": statistics.median(v), "event_ms_min": min(v), "event_ms_max": max(v)}
        r["flops_per_s"] = flops[name] / (med * 1e-3)
        r["share_of_fp32_matrix_peak"] = r["flops_per_s"] / PEAK_F32_MATRIX
        r["kernel_over_torch_event_ms_median"] = med / statistics.median(ms["torch"])
        row[name] = r
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--modes", type=int, default=4)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spod_bench.json"))
    a = ap.parse_args()
    import torch
    MODES[0] = a.modes
    model, loader = BE.setup(a.batch, a.steps)
    C = loader[0][1].shape[2]
    rec = {"what": "modelPredStats vs modelPredTimeSpectra vs modelPredSpod, cylinder test shape",
           "device": torch.cuda.get_device_properties(0).name, "model": BE.KW,
           "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "spod_channels": list(CHANNELS), "modes": a.modes, "bins": "1..16", "max_rows": a.max_rows, "reps": a.reps, "runs": [],
           "kernels_alone": []}
    for S in [int(s) for s in a.samples.split(",") if s]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 4, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
        row = {"samples": S, "member_steps": S * a.steps}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts),
                          "seconds_per_kept_step_median": statistics.median(ts) / a.steps}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        for which in ("tspec", "spod"):
            row[which + "_over_stats_seconds_median"] = statistics.median(times[which]) / statistics.median(times["stats"])
        ev, host = event_run(("ens_spod_csd", "ens_spod_modes", "tspec_store", "tspec_block"), model, loader, S, a.steps, a.max_rows)
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c} for n, (c, ms) in ev.items()}
        row["spod_decompose_host_seconds"] = host
        row["finalize_ms"] = ev["ens_spod_csd"][1] + ev["ens_spod_modes"][1] + 1e3 * sum(host)
        row["feeding_event_ms_per_kept_step"] = (ev["tspec_store"][1] + ev["tspec_block"][1]) / a.steps
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.samples.split(",") if s]:
        row = direct(S, a.batch, C, 256, 256, a.steps, a.modes, a.direct_reps)
        rec["kernels_alone"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
