"""Cost of the TKE budget: utils.modelPredBudget beside utils.modelPredStats and utils.modelPredTurbulence (both unchanged by it) at the
cylinder test shape of tools/bench_ensemble.py (3 channels, 64x64 -> 256x256, default widths, batch 4, 41 steps) for 4 / 8 / 32 members.

  per member count S: one short warm-up run of each function, then --reps timed runs alternating the three, each window closed by
  torch.cuda.synchronize(); median and best seconds, the ratios budget / stats and budget / turbulence, and the spread (max / min) of
  the stats runs, which is the run-to-run noise the ratios have to be read against
  then one more modelPredBudget run per S with a device event pair around every call of tmg_ens_budget_accum (the members' chunks
  and the target rows) and tmg_ens_budget_terms: calls, summed event time, microseconds per kept step, the accumulate kernel's bytes
  per second against the bytes it must move (per row and timed step 3 input floats and the 14 planes written, and read from the
  second step on) beside the 6.3 TB/s a float4 copy reaches on this part, and the kernels' share of the run; and, in the same
  process, one modelPredTurbulence run with event pairs around tmg_ens_accum and tmg_ens_turb_accum with their bytes
  (bench_ensemble.ens_traffic, bench_ensemble_turb.turb_traffic): the share of the copy rate the older state-bound kernels reach on
  the same run.  An event pair also holds the launch gaps.
  then tmg_ens_budget_accum alone on one random chunk of min(S, max_rows / B) members (read-modify-write): median, min and max event
  time over --direct-reps calls and its bytes per second; and tmg_ens_budget_terms on the state of S members beside a torch fp64
  composition of the same formulas, alternating call by call.

Writes profiles/budget_bench.json."""
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

import bench_ensemble as BE        # noqa: E402  (the model, the loader and the yardstick are that tool's)
import bench_ensemble_turb as BT   # noqa: E402  (the grid and the traffic of the turbulence kernels)
import bench_quant as BQ           # noqa: E402  (the event wrapper)

FUNCS = ("stats", "turbulence", "budget")
HBM_COPY = 6.3e12
NU, RHO = 1.0e-3, 1.0


def run(which, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None, dx=BT.GRID[0], dy=BT.GRID[1], nu=NU)
    kw = dict(samples=S, stride=1, tmax=steps, max_rows=max_rows)
    if which == "budget":
        return utils.modelPredBudget(args, model, loader, BE.LOG, rho=RHO, **kw)
    f = utils.modelPredStats if which == "stats" else utils.modelPredTurbulence
    return f(args, model, loader, BE.LOG, **kw)


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


def accum_bytes(rows, HW, steps):
    """The bytes tmg_ens_budget_accum must move over `steps` timed steps for `rows` rows of HW pixels."""
    return sum(rows * HW * 4 * (3 + 14 * (2 if t > 0 else 1)) for t in range(steps))


def torch_terms(raw, M, fl, T, Hh, Ww):
    """The formulas of tmg_ens_budget_terms as a torch fp64 composition on the device -> (budget_mean, budget_std, target_budget,
    stress_mean, stress_std, target_stress), fp32."""
    import torch
    dx, dy, nu, rho = fl
    r = raw.double().view(raw.shape[0], raw.shape[1], 14, Hh, Ww) / T
    Du, Dv, Dp = r[:, :, 0], r[:, :, 1], r[:, :, 2]
    uu, uv, vv = r[:, :, 3] - Du * Du, r[:, :, 4] - Du * Dv, r[:, :, 5] - Dv * Dv
    uuu = r[:, :, 6] - 3 * Du * r[:, :, 3] + 2 * Du ** 3
    uuv = r[:, :, 7] - 2 * Du * r[:, :, 4] - Dv * r[:, :, 3] + 2 * Du * Du * Dv
    uvv = r[:, :, 8] - 2 * Dv * r[:, :, 4] - Du * r[:, :, 5] + 2 * Du * Dv * Dv
    vvv = r[:, :, 9] - 3 * Dv * r[:, :, 5] + 2 * Dv ** 3
    pu, pv = r[:, :, 10] - Dp * Du, r[:, :, 11] - Dp * Dv
    c = lambda f, i, j: f[..., 1 + i:Hh - 1 + i, 1 + j:Ww - 1 + j]          # noqa: E731
    sx = lambda f: (c(f, -1, 1) - c(f, -1, -1)) + 2 * (c(f, 0, 1) - c(f, 0, -1)) + (c(f, 1, 1) - c(f, 1, -1))   # noqa: E731
    sy = lambda f: (c(f, 1, -1) - c(f, -1, -1)) + 2 * (c(f, 1, 0) - c(f, -1, 0)) + (c(f, 1, 1) - c(f, -1, 1))   # noqa: E731
    ddx, ddy = (lambda f: sx(f) / (8 * dx)), (lambda f: sy(f) / (8 * dy))
    Mv = M.view(1, M.shape[0], 2, Hh, Ww)
    U, V, k = Mv[:, :, 0] + Du, Mv[:, :, 1] + Dv, 0.5 * (uu + vv)
    gx = c(r[:, :, 12], 0, 0) - sx(Du) ** 2 - sx(Dv) ** 2
    gy = c(r[:, :, 13], 0, 0) - sy(Du) ** 2 - sy(Dv) ** 2
    t = [-(c(U, 0, 0) * ddx(k) + c(V, 0, 0) * ddy(k)),
         -(c(uu, 0, 0) * ddx(U) + c(uv, 0, 0) * (ddy(U) + ddx(V)) + c(vv, 0, 0) * ddy(V)),
         -0.5 * (ddx(uuu + uvv) + ddy(uuv + vvv)), -(ddx(pu) + ddy(pv)) / rho,
         nu * ((c(k, 0, 1) - 2 * c(k, 0, 0) + c(k, 0, -1)) / (dx * dx) + (c(k, 1, 0) - 2 * c(k, 0, 0) + c(k, -1, 0)) / (dy * dy)),
         -nu * (gx / (64 * dx * dx) + gy / (64 * dy * dy))]
    t.append(sum(t))
    terms = torch.full(r.shape[:2] + (7, Hh, Ww), float("nan"), dtype=torch.float64, device=raw.device)
    terms[..., 1:-1, 1:-1] = torch.stack(t, 2)
    st = torch.stack([uu, uv, vv], 2)
    f = lambda v: v.float()                                                  # noqa: E731
    return (f(terms[:-1].mean(0)), f(terms[:-1].std(0, unbiased=False)), f(terms[-1]), f(st[:-1].mean(0)), f(st[:-1].std(0, unbiased=False)),
            f(st[-1]))


def _events(fn, reps):
    import torch
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    return ms


def direct(S, B, Hh, Ww, max_rows, reps):
    """The accumulate kernel on one chunk alone (read-modify-write), and the terms kernel beside the torch composition -> dict."""
    import torch
    import tmg_hip as H
    g = torch.Generator(device="cuda").manual_seed(S)
    k = max(1, min(S, max_rows // B))
    HW = Hh * Ww
    rnd = lambda *s: torch.randn(s, device="cuda", generator=g)             # noqa: E731
    yn = rnd(k * B, Hh, Ww, 3)                                               # the chunk, NHWC as sampleEnsemble leaves it
    a, m = torch.ones(B, 3, device="cuda"), rnd(B, 3, HW)
    raw = torch.empty(S + 1, B, 14, HW, device="cuda")
    for m0 in range(0, S + 1, k):                                            # a finite state for the terms kernel
        kk = min(k, S + 1 - m0)
        H.ens_budget_accum(yn[:kk * B], a, m, raw, kk, m0, 0)
    ms = _events(lambda: H.ens_budget_accum(yn, a, m, raw, k, 0, 1), reps)
    nbytes = k * B * HW * 4 * (3 + 28)
    med = statistics.median(ms)
    out = {"samples": S, "chunk_members": k, "rows": k * B, "plan": H.ens_budget_plan(S, B, Hh, Ww), "bytes": nbytes, "event_ms": ms,
           "event_ms_median": med, "event_ms_min": min(ms), "event_ms_max": max(ms), "bytes_per_s": nbytes / (med * 1e-3),
           "hbm_float4_copy_bytes_per_s": HBM_COPY, "share_of_hbm_copy_rate": nbytes / (med * 1e-3) / HBM_COPY}
    M = rnd(B, 2, HW).double()
    fl = (BT.GRID[0], BT.GRID[1], NU, RHO)
    outs = [torch.empty(B, n, HW, device="cuda") for n in (7, 7, 7, 3, 3, 3)]
    T = 1 + reps + 2
    tk, tt = [], []
    for i in range(reps):
        tk += _events(lambda: H.ens_budget_terms(raw, M, fl, outs, None, Hh, Ww, T), 1)
        tt += _events(lambda: torch_terms(raw, M, fl, T, Hh, Ww), 1)
    ref = torch_terms(raw, M, fl, T, Hh, Ww)
    err = max(float(torch.nan_to_num(o.view(r.shape) - r).abs().max() / torch.nan_to_num(r).abs().max().clamp_min(1e-30)) for o, r in zip(outs, ref))
    out["terms"] = {"rows": S + 1, "kernel_ms": tk, "kernel_ms_median": statistics.median(tk), "torch_fp64_ms": tt,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_bench.json"))
    a = ap.parse_args()
    import torch
    model, loader = BE.setup(a.batch, a.steps)
    C, B, HW = loader[0][1].shape[2], a.batch, 256 * 256
    rec = {"what": "modelPredStats vs modelPredTurbulence vs modelPredBudget, cylinder test shape", "device": torch.cuda.get_device_properties(0).name,
           "model": BE.KW, "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": C, "steps": a.steps},
           "grid": list(BT.GRID), "nu": NU, "rho": RHO, "max_rows": a.max_rows, "reps": a.reps, "runs": [], "kernels_alone": []}
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
        med = {w: statistics.median(ts) for w, ts in times.items()}
        row["stats_spread_max_over_min"] = max(times["stats"]) / min(times["stats"])
        row["budget_over_stats_seconds_median"] = med["budget"] / med["stats"]
        row["budget_over_turbulence_seconds_median"] = med["budget"] / med["turbulence"]
        ev = event_run("budget", ("ens_budget_accum", "ens_budget_terms"), model, loader, S, a.steps, a.max_rows)
        nb = accum_bytes((S + 1) * B, HW, a.steps)
        row["kernels"] = {n: {"calls": c, "event_ms": ms, "event_us_per_call": 1e3 * ms / c, "event_us_per_kept_step": 1e3 * ms / a.steps / len(loader)}
                          for n, (c, ms) in ev.items()}
        acc = row["kernels"]["ens_budget_accum"]
        acc.update(bytes=nb, bytes_per_s=nb / (acc["event_ms"] * 1e-3), share_of_hbm_copy_rate=nb / (acc["event_ms"] * 1e-3) / HBM_COPY)
        row["budget_kernels_share_of_budget_run"] = (ev["ens_budget_accum"][1] + ev["ens_budget_terms"][1]) / 1e3 / med["budget"]
        old = event_run("turbulence", ("ens_accum", "ens_turb_accum"), model, loader, S, a.steps, a.max_rows)
        ob = BE.ens_traffic(S, B, HW, C, a.steps, a.max_rows)[0] + BE.ens_traffic(1, B, HW, C, a.steps, a.max_rows)[0] + \
            BT.turb_traffic(S, B, HW, a.steps, a.max_rows)[0]
        oms = old["ens_accum"][1] + old["ens_turb_accum"][1]
        row["older_state_kernels"] = {"calls": old["ens_accum"][0] + old["ens_turb_accum"][0], "event_ms": oms, "bytes": ob,
                                      "bytes_per_s": ob / (oms * 1e-3), "share_of_hbm_copy_rate": ob / (oms * 1e-3) / HBM_COPY}
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
