"""Pooled ensemble PDFs on the device (`-m gpu`): tmg_ens_pdf_count through tmg_ops.EnsemblePdfs against the reference of
tests/pdf_cases.py (searchsorted, bincount, histogram2d on explicit region slices; a float32 mirror and an fp64 reference of the derived
fields; other formulas for the floats), and utils.modelPredPdfs against the same reference over modelPred's samples.

Every integer output must EQUAL the reference: on integer data (edges ON data values, so the side rule shows), on real data for the
channel fields (comparisons of raw values have no rounding, the centre is one rounded subtraction) and for the derived fields against
the float32 mirror; against the fp64 reference the cumulative counts at every edge differ by no more than that edge's near-edge
samples.  The time planes are checked after every step.  Every float32 output lies within 2^-24 |ref| + 2^-40 of the reference, with
NaNs where the reference has them.  Every case runs with every plane the kernel adds into pre-filled with garbage before the class's
own zeroing.

Worst share of the float tolerance reached on an MI355X (the tests print it; LAB_NOTES.md): 0.997 on integer data, 0.985 on real
data, 0.988 end to end.  The tolerance is one float32 rounding to nearest, which reaches 2^-24 |ref| just above a power of two, so
shares close to 1 are what a correctly rounded output gives."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import pdf_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
F32 = np.float32
GARBAGE = -1077952577                                                         # 0xBFBFBFBF as int32


def run_pdfs(c, sizes=None, padded=None, ref=None):
    """Feed EnsemblePdfs as utils.modelPredPdfs does, in chunks of `sizes` members per step; padded: y and target are channel slices
    of wider NaN-filled NHWC buffers.  Every plane the kernel adds into is pre-filled with garbage.  With ref (the reference's
    integers) the four time planes are compared after every step.  -> (dict of numpy arrays, the launch plan)."""
    import tmg_ops as ops
    xs, tgt, t_start = c["xs"], c["tgt"], c["t_start"]
    Tn, S, B, Cc, Hh, Ww = xs.shape
    sizes = K.SC.chunk_sizes(S, c["chunk"]) if sizes is None else sizes
    padded = c["padded"] if padded is None else padded
    xd, td = torch.from_numpy(xs).to(DEV), torch.from_numpy(tgt).to(DEV)

    def nhwc(v):
        v = v.permute(0, 2, 3, 1)
        if not padded:
            return v.contiguous().permute(0, 3, 1, 2)
        wide = torch.full(tuple(v.shape[:3]) + (Cc + 3,), float("nan"), device=v.device)
        wide[..., 1:1 + Cc] = v
        return wide[..., 1:1 + Cc].permute(0, 3, 1, 2)

    en = ops.EnsemblePdfs(S, B, Cc, Hh, Ww, Tn, DEV, torch.from_numpy(c["mu"]), torch.from_numpy(c["sd"]),
                          u=None if c["u"] is None else torch.from_numpy(c["u"]), fields=c["fields"], bins=c["nb"], ranges=c["ranges"],
                          joint=c["joint"], joint_bins=c["nbj"], regions=c["regions"], grid=c["grid"],
                          center=None if c["center"] is None else torch.from_numpy(c["center"]))
    planes = (en.cnt, en.jnt, en.mt[0], en.mt[1], en.tj)
    for v in planes:
        v.fill_(GARBAGE)
    nj = c["nbj"] + 2
    for t in range(Tn):
        target = nhwc(td[t])
        m0 = 0
        for k in sizes:
            en.add(nhwc(xd[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww)), m0, target, time=t >= t_start)
            m0 += k
        assert bool((en.cnt[:, :, t + 1:] == GARBAGE).all()) and bool((en.jnt[:, :, t + 1:] == GARBAGE).all())   # a step adds into its own planes
        if t < t_start:
            assert all(bool((v == GARBAGE).all()) for v in planes[2:])         # an untimed step leaves the time planes alone
        elif ref is not None:
            w = slice(t_start, t + 1)
            assert np.array_equal(en.mt[0].cpu().numpy(), ref["member_steps"][w].sum(0).transpose(1, 0, 2, 3, 4)), "member time planes after step %d" % t
            assert np.array_equal(en.mt[1].cpu().numpy()[:, 0], ref["target_count"][:, w].sum(1)), "target time plane after step %d" % t
            tj = en.tj.cpu().numpy().reshape(2, B, en.R, en.P, nj, nj)
            assert np.array_equal(tj[0], ref["joint_count"][:, w].sum(1)) and np.array_equal(tj[1], ref["target_joint_count"][:, w].sum(1)), t
    before = [v.cpu().numpy().copy() for v in planes]
    got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in en.finalize().items()}
    assert all(np.array_equal(v.cpu().numpy(), b) for v, b in zip(planes, before))
    return got, en.plan


def check_all(got, c, ints, floats, what):
    S, B, Tn = c["S"], c["B"], c["xs"].shape[0]
    F, P, R = len(c["fields"]), len(c["joint"]), len(K.boxes_of(c["regions"], c["hw"]))
    nb, nj = c["nb"], c["nbj"] + 2
    assert set(got) == set(K.ALL_KEYS)
    assert got["pdf_count"].shape == (B, Tn, R, F, nb + 2) and got["joint_count"].shape == (B, Tn, R, P, nj, nj)
    assert got["time_member_count"].shape == (B, S, R, F, nb + 2) and got["time_joint_count"].shape == (B, R, P, nj, nj)
    assert got["pdf"].shape == (B, Tn, R, F, nb) and got["time_member_w1"].shape == (B, S, R, F) and got["time_joint_js"].shape == (B, R, P)
    K.check_integers(got, ints, what)
    K.check_identities(got, c, what)
    ks = K.kinds_of(c["fields"])
    E, _ = K.edge_tables(ks, c["ranges"], nb, c["mu"], c["sd"], c["u"], c["center"] is not None)
    assert got["pdf_edges"].dtype == np.float64 and np.array_equal(got["pdf_edges"], E) and np.array_equal(got["pdf_ranges"], c["ranges"])
    assert got["joint_edges"].shape == (B, P, 2, c["nbj"] + 1)
    assert got["pdf_fields"] == tuple(c["fields"]) and got["pdf_joint"] == tuple(c["joint"])
    assert got["pdf_regions"] == tuple(K.boxes_of(c["regions"], c["hw"]))
    return K.check_floats(got, floats, what)


# ---- integer data: equality on every branch of the launch plan ---------------------------------------------------------------------------
def _integer_case(idx):
    c, ints, floats = K.int_reference(idx)
    got, plan = run_pdfs(c, ref=ints)
    worst = check_all(got, c, ints, floats, "integer %d %s" % (idx, c["hw"]))
    print("integer %d S=%d %s: %d slices per row, instance %d, lds %d B; worst share of the float tolerance %.3f"
          % (idx, c["S"], c["hw"], plan["NSL"], plan["instance"], plan["lds"], worst))
    return plan


@pytest.mark.parametrize("idx", range(len(K.INT_TABLE)))
def test_integer_data_gives_the_integer_reference_bit_for_bit(idx):
    _integer_case(idx)


def test_integer_data_on_33_slices_per_row():
    plan = _integer_case(len(K.INT_TABLE))
    assert plan["NSL"] == 33 and plan["instance"] == 1


# ---- Gaussian, smooth and biased members with a real normalisation ---------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.REAL_TABLE)))
def test_real_data_gives_the_reference_and_the_float32_mirror(idx):
    """Channel fields: raw comparisons, no rounding.  Derived fields: the float32 mirror bit for bit; against the fp64 reference the
    cumulative counts at every edge (ensemble and target pooled) differ by no more than that edge's near-edge samples."""
    c, ints, floats = K.real_reference(idx)
    got, plan = run_pdfs(c, ref=ints)
    worst = check_all(got, c, ints, floats, "real %d %s" % (idx, K.REAL_TABLE[idx][:5]))
    i64, near, _ = K.near_counts(idx)
    cum = lambda d: (d["pdf_count"] + d["target_count"]).cumsum(-1)[..., :-1]   # noqa: E731
    diff = np.abs(cum(got) - cum(i64))
    assert bool((diff <= near.swapaxes(0, 1)).all())
    print("real %d %s: cumulative counts that differ from fp64: %d (near-edge samples %d); worst share of the float tolerance %.3f"
          % (idx, K.REAL_TABLE[idx][:5], int((diff > 0).sum()), int(near.sum()), worst))


# ---- exact properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 4, 7])
def test_outputs_are_bitwise_the_same_for_every_feed_and_run(idx):
    c = K.real_case(idx)
    outs = [run_pdfs(c, K.SC.chunk_sizes(c["S"], kd), padded)[0] for kd, padded in ((0, False), (1, True), (2, False), (2, False))]
    for o in outs[1:]:
        assert set(o) == set(outs[0])
        for name, v in outs[0].items():
            assert np.array_equal(v, o[name], equal_nan=True) if isinstance(v, np.ndarray) else v == o[name], name


def test_a_perfect_ensemble_has_zero_distance_and_a_smeared_one_has_not():
    """Members equal to the target: every distance is 0.  Members that are the target smoothed by a 3 x 3 mean: every field's
    distribution narrows, so every distance is positive (and still the reference's)."""
    S, B, Cc, hw = 3, 1, 2, (48, 64)
    _, tgt = K.SC.real_inputs(S, B, Cc, hw, "gauss", 71)
    c = dict(K.real_case(0))
    c.update(S=S, B=B, C=Cc, hw=hw, xs=np.ascontiguousarray(np.broadcast_to(tgt[:, None], (K.T, S) + tgt.shape[1:])), tgt=tgt,
             mu=np.zeros(Cc, F32), sd=np.ones(Cc, F32), u=None, fields=("ux", "uy", "vort"), joint=(("ux", "uy"),), regions=None, center=None,
             nb=32, nbj=8, ranges=np.array([[(-3.0, 3.6), (-3.0, 3.6), (-8.0, 8.0)]]), t_start=0, chunk=1, padded=True)
    got, _ = run_pdfs(c)
    for key in ("w1", "js", "time_w1", "time_js", "time_member_w1", "time_joint_js"):
        assert not got[key].any(), key
    assert float(got["time_pdf_std"].max()) <= 2.0 ** -40
    assert np.array_equal(got["pdf_count"], S * got["target_count"])
    t = torch.from_numpy(tgt)
    sm = torch.nn.functional.avg_pool2d(t.reshape(-1, 1, *hw), 3, 1, 1, count_include_pad=False).reshape(t.shape).numpy()
    c["xs"] = np.ascontiguousarray(np.broadcast_to(sm[:, None], (K.T, S) + tgt.shape[1:]))
    got, _ = run_pdfs(c)
    ints = K.integers(c)
    check_all(got, c, ints, K.floats(ints, c["ranges"], c["nb"]), "smeared")
    w1, js = got["time_w1"][0, 0], got["time_js"][0, 0]
    assert bool((js > 0).all()) and bool((w1 > 0).all())
    print("smeared by a 3 x 3 mean: time_w1 %s, time_js %s" % (np.round(w1, 4).tolist(), np.round(js, 4).tolist()))


def test_feeding_errors_are_the_event_class_errors():
    import tmg_ops as ops
    en = ops.EnsemblePdfs(3, 2, 3, 4, 5, 2, DEV, torch.zeros(3), torch.ones(3), fields=("ux",), ranges=[(-1.0, 1.0)])
    y = torch.zeros(2, 3, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match="target shape None"):
        en.add(y, 0, None)
    with pytest.raises(ValueError, match="whole members"):
        en.add(y[:1], 0, y)
    with pytest.raises(ValueError, match="fed in order"):
        en.add(y, 1, y)
    with pytest.raises(RuntimeError, match="0 of 2 steps"):
        en.finalize()
    for _ in range(2):
        for m in range(3):
            en.add(y, m, y, time=False)
    with pytest.raises(RuntimeError, match="no time statistics"):
        en.finalize()


# ---- end to end: modelPredPdfs against the reference over modelPred's samples ----------------------------------------------------------
@pytest.mark.parametrize("case", ["cylinder", "step"])
def test_model_pred_pdfs_matches_the_reference_over_model_pred_and_shares_model_pred_stats_keys(monkeypatch, tmp_path, case):
    """modelPred's samples through the reference.  modelPred un-normalises every member in fp32 as xh = fl(u fl(fl(sd x) + mu)), the
    kernel's own formula, so the float32 mirror applies to every field: the raw members x are recorded from modelPred's own
    model.sample calls, fl(u fl(fl(sd x) + mu)) of them must be modelPred's returned samples bit for bit, and every integer output must
    equal the reference, every float lie inside the tolerance.  The default ranges (the target's min and max widened by a quarter
    of the span) and center="target" (the target's time mean) are formed here independently in numpy.  The keys shared with
    modelPredStats are bit-identical to a modelPredStats run from the same host RNG state."""
    import tmg_ops as ops
    import test_ensemble_gpu as E
    from utils import utils
    model, te = (E._cylinder_case if case == "cylinder" else E._step_case)(tmp_path)
    S, tmax, stride, t_start, max_rows = 5, 6, 2, 1, 4
    fields, joint, bins, jbins = ("ux", "uy", "p", "vort", "speed", "div"), (("ux", "uy"), ("vort", "p")), 32, 8
    batches = [int(b[0].shape[0]) for b in te]
    kp = E._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None, dx=K.GRID[0], dy=K.GRID[1])
    for _ in range(2):                                                        # two folded runs: modelPredPdfs, modelPredStats
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    for bi, B in enumerate(batches):
        for m in range(S):
            for t in range(tmax):
                kp.queue_serial(bi, t, m)
    Hh, Ww = [int(v) for v in next(iter(te))[1].shape[-2:]]
    regions = ((0, Ww, 0, Hh), (Ww // 4, Ww, Hh // 4, 3 * Hh // 4))
    torch.manual_seed(77)
    got = utils.modelPredPdfs(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows, fields=fields,
                              bins=bins, joint=joint, joint_bins=jbins, regions=regions, center="target")
    torch.manual_seed(77)
    stats = utils.modelPredStats(args, model, te, E.LOG, samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    assert not kp.fold
    raw = []
    sample = model.sample

    def recording(x, h):
        y, logp, h = sample(x, h)
        raw.append(y.detach().cpu())
        return y, logp, h

    class Recorded:
        """The loader, keeping what it hands out: its batches are drawn inside modelPred, under the same host RNG state as in the
        two runs above."""
        seen = []

        def __iter__(self):
            for b in te:
                self.seen.append(b)
                yield b

        def __len__(self):
            return len(te)

    monkeypatch.setattr(model, "sample", recording)
    torch.manual_seed(77)
    pred, tgt, _ = utils.modelPred(args, model, Recorded(), E.LOG, samples=S, stride=stride, tmax=tmax)
    te = Recorded.seen
    assert not kp.serial and len(raw) == len(batches) * S * tmax
    assert set(got) == set(stats) | set(K.ALL_KEYS)
    for name, v in stats.items():
        assert torch.equal(got[name], v), name
    Tk = pred.shape[2]
    # the raw members in modelPred's call order (batch, member, step) -> [Tk, S, N, C, H, W]
    it = iter(raw)
    per_batch = [torch.stack([torch.stack([next(it) for _ in range(tmax)]) for _ in range(S)]) for _ in batches]   # [S, tmax, B, C, H, W]
    xs = torch.cat(per_batch, 2)[:, ::stride][:, :Tk].permute(1, 0, 2, 3, 4, 5).contiguous().numpy()
    mu = model.out_mu.detach().float().cpu().numpy().reshape(-1)
    sd = model.out_std.detach().float().cpu().numpy().reshape(-1)
    u0 = torch.cat([b[2].reshape(-1).cpu() for b in te]).float()
    u = torch.stack([u0, u0, u0 ** 2], 1).numpy()
    tall = torch.cat([b[1].cpu() for b in te]).float().numpy()                # the normalised target series [N, T, C, H, W]
    ys = np.ascontiguousarray(tall[:, ::stride][:, :Tk].transpose(1, 0, 2, 3, 4))
    N, Cc = ys.shape[1], ys.shape[2]
    assert np.array_equal(K.physical(xs, mu, sd, u, F32), pred.numpy().transpose(2, 0, 1, 3, 4, 5)), "the recorded members are modelPred's samples"
    tp = tgt.double().numpy()[:, ::stride][:, t_start:Tk]                     # the physical target at the timed steps [N, 2, C, H, W]
    center = tp.mean(1).astype(F32)
    ks = K.kinds_of(fields)
    vals = K.field_values(tp, ks, np.zeros(Cc, F32), np.ones(Cc, F32), None, K.GRID, None, np.float64)
    ranges = np.zeros((N, len(ks), 2))
    for f, k in enumerate(ks):
        v = vals[f] - center[:, None, k].astype(np.float64) if k < 4 else vals[f]
        lo, hi = v.reshape(N, -1).min(1), v.reshape(N, -1).max(1)
        ranges[:, f, 0], ranges[:, f, 1] = lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo)
    g = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
    assert float(np.abs(g["pdf_ranges"] - ranges).max()) <= 1e-11 * float(np.abs(ranges).max()), "the default ranges"
    c = dict(S=S, B=N, C=Cc, hw=(Hh, Ww), t_start=t_start, nb=bins, nbj=jbins, fields=fields, joint=joint, regions=regions, center=center,
             xs=xs, tgt=ys, mu=mu[:Cc], sd=sd[:Cc], u=u[:, :Cc], ranges=g["pdf_ranges"], grid=K.GRID)
    ints = K.integers(c)
    K.check_integers(g, ints, case)
    K.check_identities(g, c, case)
    worst = K.check_floats(g, K.floats(ints, c["ranges"], bins), case)
    assert g["pdf_fields"] == fields and g["pdf_joint"] == joint and g["pdf_regions"] == regions
    inner = ints["time_count"][..., 1:-1].sum() / ints["time_count"].sum()
    print("%s: every output held to the reference; %.3f of the ensemble's samples inside the default ranges; worst share of the float "
          "tolerance %.3f" % (case, inner, worst))
