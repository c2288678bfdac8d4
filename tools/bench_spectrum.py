"""Cost of the ensemble kinetic-energy spectra (tmg_spectrum.hip, utils.modelPredSpectra) at the cylinder test shape of
tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4) and at 512x512 (128x128 inputs), 32 members.

  per shape:
  passes     one chunk of max_rows images of random data through tmg_spec_rows and tmg_spec_cols, a device event pair around each
             launch, --pass-reps launches after a warm-up: median event time, executed TF (8 H W^2 and 8 H^2 W flop per image) and
             the fraction of the 157.3 TF fp32 matrix peak.  An event pair around one launch also holds the launch gap, so the rate
             is a lower bound of the kernel's own.
  torch      for comparison only: the same chunk's spectra by torch.fft.fft2 + index_add_ on the device from a materialised
             (un-normalised, planar) chunk, event pair around the whole pipeline, median
  end to end one warm-up run of utils.modelPredTurbulence and utils.modelPredSpectra, then --reps timed runs alternating the two
             (same process, same box), each closed by torch.cuda.synchronize(): seconds, member-steps/s, and the ratio
  share      one more modelPredSpectra run with an event pair around every launch of the four spectral kernels: launches, summed event
             time and its share of the run

Writes profiles/spectrum_bench.json."""
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

import bench_ensemble as BE   # noqa: E402  (the model and the loader are that tool's)

PEAK_TF = 157.3
FUNCS = ("turbulence", "spectra")
KERNELS = ("spec_rows", "spec_cols", "spec_accum", "spec_finalize")


def run(which, model, loader, grid, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=grid[0], dy=grid[1])
    f = utils.modelPredTurbulence if which == "turbulence" else utils.modelPredSpectra
    return f(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


def timed(*a):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(*a)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def _event_ms(fn, reps):
    import torch
    ms = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def passes(Hh, Ww, grid, n, reps):
    """The two transform passes and the torch pipeline on one chunk of n images -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(5)
    y = torch.randn(n, Hh, Ww, 3, device="cuda", generator=g)
    mu, sd = torch.tensor([0.2, 0.2, 0.2]), torch.tensor([0.9, 0.9, 0.9])
    sp = ops.EnsembleSpectrum(n, 1, Hh, Ww, 1, "cuda", mu, sd, grid=grid)
    sp.add(y.permute(0, 3, 1, 2), 0)                       # allocates the workspace
    rows = _event_ms(lambda: H.spec_rows(y, sp.u, sp.mu, sp.sd, sp.ft_w, sp._yw, n), reps)
    cols = _event_ms(lambda: H.spec_cols(sp.ft_h, sp._yw, sp.perm, sp.offs, sp._part, n, Hh, Ww, sp.NK), reps)
    bins = sp.bins.to("cuda").long().reshape(-1)
    yh = (sd.cuda() * y[..., :2] + mu.cuda()).permute(0, 3, 1, 2).contiguous()      # the materialised chunk
    w = sp.ft_w[0, :, 0].contiguous(), sp.ft_h[0, :, 0].contiguous()                # mode 0 of the operand: the window itself
    win = (w[1][:, None] * w[0][None, :]).contiguous()

    def torch_pipeline():
        Z = torch.fft.fft2(torch.complex(win * yh[:, 0], win * yh[:, 1]))
        E2 = (Z.real ** 2 + Z.imag ** 2).reshape(n, -1) * (0.5 / float(Hh * Ww) ** 2)
        return torch.zeros(n, sp.NK, device="cuda").index_add_(1, bins, E2)

    tp = _event_ms(torch_pipeline, reps)
    fr, fc = 8.0 * Hh * Ww * Ww * n, 8.0 * Hh * Hh * Ww * n
    return {"images": n, "rows_ms": rows, "cols_ms": cols, "rows_tf": fr / rows / 1e9, "cols_tf": fc / cols / 1e9,
            "rows_fraction_of_peak": fr / rows / 1e9 / PEAK_TF, "cols_fraction_of_peak": fc / cols / 1e9 / PEAK_TF,
            "torch_fft2_index_add_ms": tp, "hip_over_torch": (rows + cols) / tp}


def event_run(model, loader, grid, S, steps, max_rows):
    """One modelPredSpectra run with an event pair around every launch of the spectral kernels -> {name: (launches, ms)}."""
    import torch
    import tmg_hip as H
    pairs = {n: [] for n in KERNELS}
    orig = {n: getattr(H, n) for n in pairs}

    def wrap(name):
        def f(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            orig[name](*a, **k)
            e1.record()
            pairs[name].append((e0, e1))
        return f

    try:
        for n in pairs:
            setattr(H, n, wrap(n))
        dt = timed("spectra", model, loader, grid, S, steps, max_rows)
    finally:
        for n in pairs:
            setattr(H, n, orig[n])
    return {n: (len(v), sum(a.elapsed_time(b) for a, b in v)) for n, v in pairs.items()}, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256:21,512:6", help="out size : roll-out steps, comma separated")
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pass-reps", type=int, default=20)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_bench.json"))
    a = ap.parse_args()
    import torch
    S = a.samples
    rec = {"what": "ensemble kinetic-energy spectra: transform passes, share of the folded roll-out, modelPredSpectra vs "
                   "modelPredTurbulence, torch.fft pipeline for comparison", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "samples": S, "batch": a.batch, "max_rows": a.max_rows, "reps": a.reps, "peak_tf": PEAK_TF, "runs": []}
    for spec in a.shapes.split(","):
        N, steps = (int(v) for v in spec.split(":"))
        grid = (6.0 / N, 6.0 / N)
        row = {"out_hw": [N, N], "steps": steps, "grid": list(grid), "passes": passes(N, N, grid, a.max_rows, a.pass_reps)}
        print(json.dumps(row), flush=True)
        model, loader = BE.setup(a.batch, steps, hw_in=(N // 4, N // 4), up=4)
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, grid, S, 2, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, grid, S, steps, a.max_rows))
        for which, ts in times.items():
            row[which] = {"seconds": ts, "member_steps_per_s_median": S * steps / statistics.median(ts)}
        row["spectra_over_turbulence_seconds_median"] = statistics.median(times["spectra"]) / statistics.median(times["turbulence"])
        ev, dt = event_run(model, loader, grid, S, steps, a.max_rows)
        row["kernels"] = {n: {"launches": c, "event_ms": ms} for n, (c, ms) in ev.items()}
        row["kernel_event_share_of_spectra_run"] = sum(ms for _, ms in ev.values()) / 1e3 / dt
        row["transform_event_ms_per_member_step"] = (ev["spec_rows"][1] + ev["spec_cols"][1]) / (S * steps)
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
        del model, loader
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
