"""Cost of the two-point correlations: utils.modelPredCorrelation (default probes, pairs and lags: 40 planes) beside utils.modelPredStats
and utils.modelPredBudget (both unchanged by it) at the cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256,
default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the three, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratios correlation / stats and correlation / budget, and the spread
  (max / min) of the stats runs, which is the run-to-run noise the ratios have to be read against
  then one more modelPredCorrelation run per S with a device event pair around every call of tmg_ens_corr_probe, tmg_ens_corr_accum
  (the members' chunks and the target rows) and tmg_ens_corr_finalize: calls, summed event time, microseconds per kept step, the
  accumulate kernel's bytes per second against the bytes it must move (per row and timed step the 3 input floats and every live
  plane written, and read after its first step) beside the 6.3 TB/s a float4 copy reaches on this part, and the kernels' share of
  the run; and, in the same process, one modelPredBudget run with event pairs around tmg_ens_budget_accum with its bytes
  (bench_budget.accum_bytes): the share of the copy rate that kernel reaches on the same run.  An event pair also holds the launch
  gaps.
  then tmg_ens_corr_accum alone on one random chunk of min(S, max_rows / B) members with every plane live (read-modify-write):
  median, min and max event time over --direct-reps calls and its bytes per second; and tmg_ens_corr_finalize on the state of S
  members beside a torch fp64 composition of the same formulas, alternating call by call.

Writes profiles/corr_bench.json."""
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

import bench_budget as BB          # noqa: E402  (the budget's run and bytes, the event loop)
import bench_ensemble as BE        # noqa: E402  (the model, the loader and the yardstick are that tool's)
import bench_ensemble_turb as BT   # noqa: E402  (the grid)
import bench_quant as BQ           # noqa: E402  (the event wrapper)

FUNCS = ("stats", "budget", "correlation")
HBM_COPY = 6.3e12
PAIRS, LAGS = ((0, 0), (1, 1)), (0, 1, 2, 4)


def probes_of(Hh, Ww):
    return ((Hh // 2, Ww // 4), (Hh // 2, Ww // 2), (Hh // 2, 3 * Ww // 4))


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    if which != "correlation":
        return BB.run(which, model, loader, S, steps, max_rows)
    args = SimpleNamespace(device=None, dx=BT.GRID[0], dy=BT.GRID[1])
    return utils.modelPredCorrelation(args, model, loader, BE.LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


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


def accum_bytes(rows, HW, steps, P=3, pairs=PAIRS, lags=LAGS):
    """The bytes tmg_ens_corr_accum must move over `steps` timed steps for `rows` rows of HW pixels: the 3 inputs, every live plane
    written and, after its first step, read."""
    per_lag = P * len(pairs) + 2 * len({cj for _ci, cj in pairs})
    total = 0
    for t in range(steps):
        written = per_lag * sum(1 for tau in lags if tau <= t)
        read = per_lag * sum(1 for tau in lags if tau < t)
        total += rows * HW * 4 * (3 + written + read)
    return total


def torch_finalize(raw, pm, pv, Hh, Ww, T, P=3, pairs=PAIRS, lags=LAGS):
    """The formulas of tmg_ens_corr_finalize as a torch fp64 composition on the device -> (cov_mean, cov_std, rho_mean, rho_std,
    target_cov, target_rho) [B, P, Q, L, HW] fp32."""
    import torch
    R, B, NPL, HW = raw.shape
    Q, L = len(pairs), len(lags)
    J = sorted({cj for _ci, cj in pairs})
    n = torch.tensor([float(T - tau) for tau in lags], device=raw.device, dtype=torch.float64).view(1, 1, 1, 1, L, 1)
    r = raw.double()
    X = r[:, :, :P * Q * L].view(R, B, P, Q, L, HW)
    F = r[:, :, P * Q * L:P * Q * L + len(J) * L].view(R, B, len(J), L, HW)
    G = r[:, :, P * Q * L + len(J) * L:].view(R, B, len(J), L, HW)
    jx = [J.index(cj) for _ci, cj in pairs]
    mf = (F[:, :, jx] / n[:, :, 0]).unsqueeze(2)                             # [R, B, 1, Q, L, HW]
    vf = (G[:, :, jx] / n[:, :, 0]).unsqueeze(2) - mf * mf
    cov = X / n - pm.unsqueeze(-1) * mf
    rho = torch.where((pv.unsqueeze(-1) > 0) & (vf > 0), cov / torch.sqrt(pv.unsqueeze(-1) * vf), torch.full_like(cov, float("nan")))
    dead = (n < 2).expand_as(cov)
    cov, rho = cov.masked_fill(dead, float("nan")), rho.masked_fill(dead, float("nan"))
    f = lambda v: v.float()                                                  # noqa: E731
    return (f(cov[:-1].mean(0)), f(cov[:-1].std(0, unbiased=False)), f(rho[:-1].mean(0)), f(rho[:-1].std(0, unbiased=False)), f(cov[-1]),
            f(rho[-1]))


def direct(S, B, Hh, Ww, max_rows, reps):
    """The accumulate kernel on one chunk alone (every plane live, read-modify-write), and the finalize kernel beside the torch
    composition -> dict."""
    import torch
    import tmg_hip as H
    import tmg_ops as ops
    g = torch.Generator(device="cuda").manual_seed(S)
    k = max(1, min(S, max_rows // B))
    HW = Hh * Ww
    probes = probes_of(Hh, Ww)
    P, Q, L = len(probes), len(PAIRS), len(LAGS)
    steps = LAGS[-1] + 2
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)             # noqa: E731
    yn = rnd(k * B, Hh, Ww, 3)                                               # the chunk, NHWC as sampleEnsemble leaves it
    a, m = torch.ones(B, 3, device="cuda"), rnd(B, 3, HW)
    plan = H.ens_corr_plan(S, B, Hh, Ww, P, Q, L, 2)
    raw = torch.empty(S + 1, B, plan["planes"], HW, device="cuda")
    series = torch.empty(S + 1, B, steps, P, 3, device="cuda")
    cfg = (probes, PAIRS, LAGS)
    for t in range(steps):                                                   # a finite state: every plane written, T = steps
        for m0 in range(0, S + 1, k):
            kk = min(k, S + 1 - m0)
            y = yn[:kk * B] * (1.0 + 0.1 * t)
            H.ens_corr_probe(y, a, m, series, *cfg, kk, m0, t)
            H.ens_corr_accum(y, a, m, series, raw, *cfg, kk, m0, t)
    ms = BB._events(lambda: H.ens_corr_accum(yn, a, m, series, raw, *cfg, k, 0, steps - 1), reps)
    nbytes = k * B * HW * 4 * (3 + 2 * plan["planes"])
    med = statistics.median(ms)
    out = {"samples": S, "chunk_members": k, "rows": k * B, "plan": plan, "bytes": nbytes, "event_ms": ms, "event_ms_median": med,
           "event_ms_min": min(ms), "event_ms_max": max(ms), "bytes_per_s": nbytes / (med * 1e-3), "hbm_float4_copy_bytes_per_s": HBM_COPY,
           "share_of_hbm_copy_rate": nbytes / (med * 1e-3) / HBM_COPY}
    T = steps
    pm, pv = [v.cuda() for v in ops.corr_probe_stats(series, PAIRS, LAGS, T)]
    outs = [torch.empty(B, P, Q, L, HW, device="cuda") for _ in range(6)]
    lines = [torch.empty(B, S + 1, P, Q, L, n, device="cuda") for n in (Ww, Hh)]
    tk, tt = [], []
    for i in range(reps):
        tk += BB._events(lambda: H.ens_corr_finalize(raw, pm, pv, outs, None, lines, *cfg, Hh, Ww, T), 1)
        tt += BB._events(lambda: torch_finalize(raw, pm, pv, Hh, Ww, T), 1)
    ref = torch_finalize(raw, pm, pv, Hh, Ww, T)
    err = max(float(torch.nan_to_num(o - r).abs().max() / torch.nan_to_num(r).abs().max().clamp_min(1e-30)) for o, r in zip(outs, ref))
    out["finalize"] = {"rows": S + 1, "kernel_ms": tk, "kernel_ms_median": statistics.median(tk), "torch_fp64_ms": tt,
                       "torch_fp64_ms_median": statistics.median(tt), "torch_over_kernel": statistics.median(tt) / statistics.median(tk),
                       "max_difference_over_largest_value": err}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="4,8,32")
    ap.add_argument("--direct-reps", type=int, default=11)
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C, B, HW = loader[0][1].shape[2], a.batch, 256 * 256
    rec = {"what": "modelPredStats vs modelPredBudget vs modelPredCorrelation, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "grid": list(BT.GRID), "probes": [list(p) for p in probes_of(256, 256)], "pairs": [list(p) for p in PAIRS], "lags": list(LAGS),
           "planes": 40, "max_rows": a.max_rows, "reps": a.reps, "runs": [], "kernels_alone": []}
    for S in [int(s) for s in a.samples.split(",") if s]:
        for which in FUNCS:                                   # warm-up: plans, allocator, code objects
            timed(which, model, loader, S, 6, a.max_rows)
        times = {w: [] for w in FUNCS}
        for r in range(a.reps):
            for which in (FUNCS if r % 2 == 0 else FUNCS[::-1]):
                times[which].append(timed(which, model, loader, S, a.steps, a.max_rows))
        row = {"samples": S, "member_steps": S * a.steps}
        for which, ts in times.items():
            row[which] = {"seconds": ts, "seconds_median": statistics.median(ts), "seconds_best": min(ts)}
        med = {w: statistics.median(ts) for w, ts in times.items()}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["correlation_over_stats_seconds_median"] = med["correlation"] / med["stats"]
        row["correlation_over_budget_seconds_median"] = med["correlation"] / med["budget"]
        names = ("ens_corr_probe", "ens_corr_accum", "ens_corr_finalize")
        ev = event_run("correlation", names, model, loader, S, a.steps, a.max_rows)
        nb = accum_bytes((S + 1) * B, HW, a.steps)
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c, "event_us_per_kept_step": 1e3 * ms / a.steps / len(loader)}
                          for n, (c, ms) in ev.items()}
        acc = row["kernels"]["ens_corr_accum"]
        acc.update(bytes=nb, bytes_per_s=nb / (acc["event_ms"] * 1e-3), share_of_hbm_copy_rate=nb / (acc["event_ms"] * 1e-3) / HBM_COPY)
        row["corr_kernels_share_of_correlation_run"] = sum(ev[n][1] for n in names) / 1e3 / med["correlation"]
        old = event_run("budget", ("ens_budget_accum",), model, loader, S, a.steps, a.max_rows)
        ob = BB.accum_bytes((S + 1) * B, HW, a.steps)
        oms = old["ens_budget_accum"][1]
        row["budget_accum_same_run"] = {"calls": old["ens_budget_accum"][0], "event_ms": oms, "event_us_per_kept_step": 1e3 * oms / a.steps / len(loader),
                                        "bytes": ob, "bytes_per_s": ob / (oms * 1e-3), "share_of_hbm_copy_rate": ob / (oms * 1e-3) / HBM_COPY}
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    for S in [int(s) for s in a.samples.split(",") if s]:
        row = direct(S, a.batch, 256, 256, a.max_rows, a.direct_reps)
        rec["kernels_alone"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
