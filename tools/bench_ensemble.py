"""Serial ensemble prediction (utils.modelPred: one TMGlow.sample call of B rows per member and step) against the folded path
(utils.modelPredStats: TMGlow.sampleEnsemble calls of up to --max-rows rows, statistics on the device) at the cylinder test shape:
3 channels, 64x64 -> 256x256, the reference's default widths (enc [4,4,4], glow [16,16,16], 32 conditioning / 64 recurrent
features, growth 4, 16 initial features), cglow_upscale 4, batch 4, 41 steps.

  time mode (default)   per member count S: one short warm-up run of each path, then --reps timed runs alternating the two paths,
                        each window closed by torch.cuda.synchronize(); member-steps/s = S * steps / seconds (best and median)
  --profile PATH        one run of one path (serial | folded) for a kernel-trace run of its own:
                          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_ensemble.py --profile folded
                        writes DIR/meta.json (member-steps, bytes the statistics kernels move) beside the trace
  --summarize SERIAL_DIR FOLDED_DIR   launches per member-step of both paths and the statistics kernels' HBM fraction, merged into --out
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-turbulence_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_TBS = 8.0
LOG = SimpleNamespace(log=lambda *a, **k: None, warning=lambda *a, **k: None)
KW = dict(in_features=3, out_features=3, enc_blocks=[4, 4, 4], glow_blocks=[16, 16, 16], cond_features=32, cglow_upscale=4, growth_rate=4,
          init_features=16, rec_features=64, bn_size=8)


def setup(batch, steps, hw_in=(64, 64), up=4):
    import contextlib
    import io
    import torch
    import common as C
    from nn.tmGlow import TMGlow
    torch.manual_seed(12345)
    with contextlib.redirect_stdout(io.StringIO()):
        model = TMGlow(**KW)
    C.perturb_(model, 7, 0.004, 0.02, 0.004)
    model = model.cuda().eval()
    with torch.no_grad():
        model.in_mu.fill_(0.1); model.in_std.fill_(1.2); model.out_mu.fill_(0.2); model.out_std.fill_(0.9)
    g = torch.Generator(device="cuda").manual_seed(3)
    inp = torch.randn(batch, steps, 3, *hw_in, device="cuda", generator=g)
    tgt = torch.randn(batch, steps, 3, hw_in[0] * up, hw_in[1] * up, device="cuda", generator=g)
    u0 = torch.linspace(0.8, 1.6, batch)
    return model, [(inp, tgt, u0)]


def run(path, model, loader, S, steps, max_rows):
    from utils import utils
    args = SimpleNamespace(device=None)
    if path == "serial":
        return utils.modelPred(args, model, loader, LOG, samples=S, stride=1, tmax=steps)
    return utils.modelPredStats(args, model, loader, LOG, samples=S, stride=1, tmax=steps, max_rows=max_rows)


def timed(path, model, loader, S, steps, max_rows):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run(path, model, loader, S, steps, max_rows)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def ens_traffic(S, B, HW, C, steps, max_rows):
    """HBM bytes the statistics kernels of one modelPredStats batch move (stride 1, t_start 0): per step and chunk the chunk's
    input (C floats per pixel), the members' time state (read from the second step on, written always), the step
    state (read by every chunk after the first, written by every chunk but the last) and the last chunk's planar outputs; once at
    the end the time state is read and the four time outputs are written."""
    per = max(1, max_rows // B)
    chunks = [min(per, S - m0) for m0 in range(0, S, per)]
    acc = 0
    for t in range(steps):
        for i, k in enumerate(chunks):
            acc += k * B * HW * C * 4                         # input (useful bytes)
            acc += k * B * HW * C * 2 * 4 * (2 if t > 0 else 1)
            acc += B * HW * (C + 1) * 2 * 4 * ((1 if i > 0 else 0) + (1 if i < len(chunks) - 1 else 0))
            if i == len(chunks) - 1:
                acc += B * HW * (C + 1) * 2 * 4
    fin = S * B * HW * C * 2 * 4 + 4 * B * HW * C * 4
    return acc, fin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1,4,16,32")
    ap.add_argument("--steps", type=int, default=41)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--max-rows", type=int, default=64)
    ap.add_argument("--profile", choices=["serial", "folded"])
    ap.add_argument("--profile-dir")
    ap.add_argument("--summarize", nargs=2, metavar=("SERIAL_DIR", "FOLDED_DIR"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    a = ap.parse_args()
    Ss = [int(s) for s in a.samples.split(",")]
    if a.summarize:
        return summarize(a)
    import torch
    model, loader = setup(a.batch, a.steps)
    if a.profile:
        S = Ss[0]
        run(a.profile, model, loader, S, a.steps, a.max_rows)
        torch.cuda.synchronize()
        meta = {"path": a.profile, "samples": S, "steps": a.steps, "batch": a.batch, "max_rows": a.max_rows, "member_steps": S * a.steps}
        if a.profile == "folded":
            with torch.no_grad():
                y, _, _ = model.sampleEnsemble(loader[0][0][:, 0], None, 1)
            ps = int(y.permute(0, 2, 3, 1).stride(2))
            acc, fin = ens_traffic(S, a.batch, y.shape[2] * y.shape[3], y.shape[1], a.steps, a.max_rows)
            meta.update(y_pixel_stride=ps, ens_accum_bytes=acc, ens_time_finalize_bytes=fin)
        if a.profile_dir:
            os.makedirs(a.profile_dir, exist_ok=True)
            json.dump(meta, open(os.path.join(a.profile_dir, "meta.json"), "w"), indent=1)
        print(json.dumps(meta))
        return
    dev = torch.cuda.get_device_properties(0)
    rec = {"what": "serial modelPred vs folded modelPredStats, cylinder test shape", "device": dev.name, "model": KW,
           "shape": {"batch": a.batch, "in_hw": [64, 64], "out_hw": [256, 256], "channels": 3, "steps": a.steps},
           "max_rows": a.max_rows, "reps": a.reps, "runs": []}
    for S in Ss:
        for path in ("serial", "folded"):                     # warm-up: plans, allocator, code objects
            timed(path, model, loader, S, 3, a.max_rows)
        times = {"serial": [], "folded": []}
        for r in range(a.reps):
            order = ("serial", "folded") if r % 2 == 0 else ("folded", "serial")
            for path in order:
                times[path].append(timed(path, model, loader, S, a.steps, a.max_rows))
        row = {"samples": S, "member_steps": S * a.steps}
        for path, ts in times.items():
            row[path] = {"seconds": ts, "member_steps_per_s_best": S * a.steps / min(ts),
                         "member_steps_per_s_median": S * a.steps / statistics.median(ts)}
        row["speedup_best"] = row["folded"]["member_steps_per_s_best"] / row["serial"]["member_steps_per_s_best"]
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    old.update(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(old, open(a.out, "w"), indent=1)


def _stats_rows(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not f:
        raise SystemExit("no kernel_stats.csv under %s" % d)
    return list(csv.DictReader(open(f[0])))


def summarize(a):
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    prof = {}
    for d in a.summarize:
        meta = json.load(open(os.path.join(d, "meta.json")))
        rows = _stats_rows(d)
        launches = sum(int(r["Calls"]) for r in rows)
        ent = {"samples": meta["samples"], "steps": meta["steps"], "launches": launches,
               "launches_per_member_step": launches / meta["member_steps"]}
        if meta["path"] == "folded":
            for name, key in (("ens_accum_kernel", "ens_accum_bytes"), ("ens_time_finalize_kernel", "ens_time_finalize_bytes")):
                r = [x for x in rows if x["Name"].startswith(name)]
                if not r:
                    continue
                ns = float(r[0]["TotalDurationNs"])
                tbs = meta[key] / ns / 1e3
                ent[name] = {"calls": int(r[0]["Calls"]), "avg_us": float(r[0]["AverageNs"]) / 1e3, "bytes": meta[key],
                             "tb_per_s": tbs, "hbm_fraction": tbs / HBM_TBS}
            ent["y_pixel_stride"] = meta["y_pixel_stride"]
        prof[meta["path"]] = ent
    prof["note"] = ("launch counts include the per-batch set-up (seed states, conditioning) of the profiled run; bytes are the useful "
                    "bytes of tools/bench_ensemble.py:ens_traffic against %g TB/s" % HBM_TBS)
    rec["profile"] = prof
    json.dump(rec, open(a.out, "w"), indent=1)
    print(json.dumps(prof, indent=1))


if __name__ == "__main__":
    main()
