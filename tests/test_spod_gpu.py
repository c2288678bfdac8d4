"""Spectral POD on the device (`-m gpu`): tmg_ens_spod_csd / tmg_ens_spod_modes called directly on hand-made accumulators (integers bit
for bit, Gaussian data inside the counted bound of tests/spod_cases.py), tmg_ops.EnsembleSpod end to end against an fp64 statement
from scratch (numpy rfft of the fp64 un-normalised rows), a planted structure, and utils.modelPredSpod on the tiny model.

Measured on an MI355X (the tests print each figure before they assert; run with -s).  CSD kernel on Gaussian data: the largest error
is 0.0021 .. 0.0116 of the counted bound (cnt 521 .. 1035), with and without the common offset.  Modes kernel: 0.06 .. 0.29 of its bound.
End to end: csd errors of 1.0e-8 .. 4.0e-8 scale against the restatement's 8.0e-9 .. 3.0e-8, 0.7 % .. 1.8 % of the yardstick bound;
spod_total against psd_mean 6.5e-8 .. 1.7e-7 relative against bounds of 2.5e-5 .. 5.0e-5.  Planted structure: s = 2.3e-7, alignment
with the reference's leading mode 1 - O(1e-9), target_captured 0.999979 for a target of the same process and 0.000000 (reference
0.000000) for psi_2's pattern in bin k1.
Durations (pytest --durations): 32 tests in 3.7 s; modelPredSpod end to end 0.86 s, the first kernel call 0.27 s, every end-to-end
case under 0.25 s, everything else 0.01 s or less."""
import hashlib
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import spod_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
NAN = float("nan")
GUARD = 64                        # floats of NaN before and after a hand-made accumulator


def guarded(acc, shift=0):
    """The accumulator on the device inside a NaN-filled buffer (what lies beside it is never read: 0 * NaN would show); shift: floats
    by which the view is moved off the 16-byte grid (1: the scalar load path whatever HW is)."""
    buf = torch.full((acc.numel() + 2 * GUARD + 4,), NAN, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + acc.numel()].view(acc.shape)
    view.copy_(acc)
    return view


def run_csd(acc, cst, case, shift=0):
    import tmg_hip as H
    a = guarded(acc, shift)
    HW, R = acc.shape[4], acc.shape[1]
    plan = H.ens_spod_plan(R - 1, case["B"], len(case["channels"]), HW, len(case["bins"]), a)
    assert plan["vec"] == (HW % 4 == 0 and shift == 0)
    ws = torch.full((plan["ws"] + GUARD,), NAN, device=DEV)
    raw = torch.full((case["B"], len(case["bins"]), 2, R, R), NAN, device=DEV)
    H.ens_spod_csd(a, cst.to(DEV), case["bins"], case["channels"], ws, raw, case["Tn"])
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[plan["ws"]:]).all())                            # nothing is written behind the planned workspace
    return raw.cpu(), plan


def check_symmetry(raw):
    assert torch.equal(raw[:, :, 0], raw[:, :, 0].transpose(-1, -2))           # raw0 bitwise symmetric
    assert torch.equal(raw[:, :, 1], -raw[:, :, 1].transpose(-1, -2))          # raw1 bitwise antisymmetric
    d = torch.diagonal(raw[:, :, 1], dim1=-2, dim2=-1)
    assert bool((d == 0).all())                                                # with an exactly zero diagonal


# ---- 1. the CSD kernel: integers, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in K.CSD_CASES])
def test_csd_integers_bit_for_bit(name):
    case = K.CSD_BY_NAME[name]
    acc, cst = K.int_acc(case, 40 + K.CSD_CASES.index(case))
    ref = K.int_csd(acc, cst, case)
    raw, plan = run_csd(acc, cst, case)
    assert K.csd_branches(plan, case["R"]) == K.CSD_BRANCHES[name]
    assert bool(torch.isfinite(raw).all())
    assert torch.equal(raw.double() * case["Tn"] ** 2, ref.double()), name
    check_symmetry(raw)


@pytest.mark.parametrize("name", ["r9_hw64", "r33_hw272_16bins"])
def test_csd_scalar_loads_for_a_base_off_the_16_byte_grid(name):
    case = K.CSD_BY_NAME[name]
    acc, cst = K.int_acc(case, 70)
    raw, _ = run_csd(acc, cst, case, shift=1)
    assert torch.equal(raw.double() * case["Tn"] ** 2, K.int_csd(acc, cst, case).double())
    other, _ = run_csd(acc, cst, case)
    assert torch.equal(raw, other)                                             # both load paths: the same bits


# ---- 2. the CSD kernel: real data inside the counted bound -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,offset", K.REAL_CASES)
def test_csd_real_data_inside_the_counted_bound(name, offset):
    case = K.CSD_BY_NAME[name]
    acc, cst = K.gauss_acc(case, 90 + K.CSD_CASES.index(case), offset)
    raw, plan = run_csd(acc, cst, case)
    ref, mag = K.csd_ref64(acc, cst, case["bins"], case["channels"], case["Tn"])
    cnt = plan["L"] + plan["P"] + K.C_ROUNDINGS
    bound = K.csd_bound(mag, cnt)
    err = (raw.double() - ref).abs()
    share = float((err / bound.clamp_min(1e-300)).max())
    print("%s offset %g: cnt %d (L %d, P %d), max err %.3e, %.4f of the bound" % (name, offset, cnt, plan["L"], plan["P"], float(err.max()), share))
    assert bool((err <= bound).all()), (name, share)
    check_symmetry(raw)


# ---- 2b. the CSD kernel: the bits of the commit before the Gram engine moved to csrc/tmg_symgram.h --------------------------------------
# The same inputs give the same bits and there are no float atomics, so csd_raw of the real-data cases above, and of the two-macro-tile
# case on the scalar load path, is pinned by its SHA-256 (tests/golden/symgram_bits.json, written by
# tests/golden/make_symgram_golden.py on an MI355X from the commit before).
BITS = os.path.join(C.GOLDEN, "symgram_bits.json")
BITS_CASES = [(n, o, 0) for n, o in K.REAL_CASES] + [("r33_hw272_16bins", 0.0, 1)]


def bits_name(c):
    return "%s_offset%g_shift%d" % c


def csd_bits(name, offset, shift):
    """-> (SHA-256 of csd_raw, what the plan says of the engine's branches)"""
    case = K.CSD_BY_NAME[name]
    acc, cst = K.gauss_acc(case, 90 + K.CSD_CASES.index(case), offset)
    raw, plan = run_csd(acc, cst, case, shift)
    return (hashlib.sha256(raw.contiguous().numpy().tobytes()).hexdigest(),
            {"part": plan["part"], "NT": plan["NT"], "P": plan["P"], "vec": plan["vec"], "HW": acc.shape[4], "Cg": len(case["channels"])})


@pytest.mark.parametrize("c", BITS_CASES, ids=bits_name)
def test_csd_real_data_gives_the_bits_of_the_commit_before_the_shared_engine(c):
    gold = json.load(open(BITS))["spod"][bits_name(c)]
    sha, plan = csd_bits(*c)
    assert plan == gold["plan"]
    assert sha == gold["sha256"]


# ---- 3. the modes kernel -----------------------------------------------------------------------------------------------------------------
SENTINEL = -777.0


def run_modes(acc, cst, case, wr32):
    import tmg_hip as H
    a = guarded(acc)
    HW = acc.shape[4]
    B, NB, J, Cg = case["B"], len(case["bins"]), case["J"], len(case["channels"])
    n = B * NB * 2 * J * Cg * HW
    buf = torch.full((n + 4096,), SENTINEL, device=DEV)
    out = buf[:n].view(B, NB, 2 * J, Cg, HW)
    H.ens_spod_modes(a, cst.to(DEV), case["bins"], case["channels"], wr32.to(DEV).contiguous(), out, case["Tn"])
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all())                                   # rows >= 2 J of the last tile and pixels >= HW: untouched
    return out.cpu()


def modes_acc(case, seed, integer):
    full = dict(case, R=case["S"] + 1, gint=True)
    return K.int_acc(full, seed) if integer else K.gauss_acc(full, seed, 0.0)


@pytest.mark.parametrize("name", [c["name"] for c in K.MODES_CASES])
def test_modes_integers_are_exact(name):
    case = next(c for c in K.MODES_CASES if c["name"] == name)
    acc, cst = modes_acc(case, 11, True)
    g = torch.Generator().manual_seed(5)
    S, J = case["S"], case["J"]
    w = torch.complex(torch.randint(-2, 3, (case["B"], len(case["bins"]), S, J), generator=g).double(),
                      torch.randint(-2, 3, (case["B"], len(case["bins"]), S, J), generator=g).double())
    wr = K.modes_operand(w, S)
    wr[:, :, 2 * J:] = 3.0                                                     # rows >= 2 J: read, finite, never stored
    wr32 = wr.float()
    got = run_modes(acc, cst, case, wr32)
    ref, _ = K.modes_ref64(acc, cst, case, wr32)
    assert torch.equal(got.double(), ref), name                               # dyadic values with sums far under 2^24: exact


@pytest.mark.parametrize("name", [c["name"] for c in K.MODES_CASES])
def test_modes_real_data_inside_the_counted_bound(name):
    case = next(c for c in K.MODES_CASES if c["name"] == name)
    acc, cst = modes_acc(case, 12, False)
    g = torch.Generator().manual_seed(6)
    S, J = case["S"], case["J"]
    w = torch.complex(torch.randn((case["B"], len(case["bins"]), S, J), generator=g, dtype=torch.float64),
                      torch.randn((case["B"], len(case["bins"]), S, J), generator=g, dtype=torch.float64))
    wr32 = K.modes_operand(w, S).float()
    got = run_modes(acc, cst, case, wr32)
    ref, mag = K.modes_ref64(acc, cst, case, wr32)
    bound = (2 * S + 1) * K.U24 * mag
    err = (got.double() - ref).abs()
    print("%s: max err %.3e, %.4f of the bound" % (name, float(err.max()), float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), name


# ---- 4. EnsembleSpod end to end ----------------------------------------------------------------------------------------------------------
def run_spod(ys, u, window, bins, channels, J, sizes, loo=True, dt=1.0):
    """ys [Tn, R, B, C, H, W] fp32 on the device (row S the target), fed in chunks of `sizes` members."""
    import tmg_ops as ops
    Tn, R, B, Cc, Hh, Ww = ys.shape
    S = R - 1
    sp = ops.EnsembleSpod(S, B, Cc, Hh, Ww, Tn, DEV, K.MU[:Cc], K.SD[:Cc], u=None if u is None else u.to(DEV), bins=bins, modes=J,
                          channels=channels, window=window, dt=dt, loo=loo)
    assert sum(sizes) == S
    for t in range(Tn):
        tgt = ys[t, S].contiguous(memory_format=torch.channels_last)
        m0 = 0
        for k in sizes:
            y = ys[t, m0:m0 + k].reshape(k * B, Cc, Hh, Ww).contiguous(memory_format=torch.channels_last)
            sp.add(y, m0, tgt)
            m0 += k
    out = sp.finalize()
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()}, sp


def chunkings(S):
    out = [[S], [1] * S]
    if S >= 3:
        out.append([1, S - 2, 1])
    return out


HOST_KEYS = ("spod_energy", "spod_total", "spod_energy_frac", "captured", "member_mode_energy", "spod_noise_floor", "target_coef",
             "target_mode_energy", "target_energy", "target_captured", "csd", "loo_captured", "target_captured_rank", "spod_bins", "spod_freq")


def same_bits(a, b):
    return torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b) or \
        bool(((a == b) | ((a != a) & (b != b))).all())                         # NaN where NaN


@pytest.mark.parametrize("idx", range(len(K.E2E_CASES)))
def test_ensemble_spod_end_to_end(idx):
    import tmg_ops as ops
    Tn, (Hh, Ww), Cc, B, S, u_given, window, _, channels, J = K.E2E_CASES[idx]
    bins = K.e2e_bins(idx)
    ys, u = K.e2e_inputs(idx)
    x64, x32 = K.fields(ys, u)
    ysd = ys.to(DEV)
    HW, NB, Cg = Hh * Ww, len(bins), len(channels)
    runs = [run_spod(ysd, u, window, K.E2E_CASES[idx][7], channels, J, sizes, dt=0.25) for sizes in chunkings(S) + [[S]]]
    got, sp = runs[0]
    # shapes and keys
    assert set(got) == set(HOST_KEYS) | {"csd_raw", "spod_modes"}
    assert tuple(got["csd_raw"].shape) == (B, NB, 2, S + 1, S + 1) and got["csd_raw"].is_cuda and got["csd_raw"].dtype == torch.float32
    assert tuple(got["spod_modes"].shape) == (B, NB, J, 2, Cg, Hh, Ww) and got["spod_modes"].is_cuda
    assert tuple(got["spod_energy"].shape) == (B, NB, J) and tuple(got["loo_captured"].shape) == (B, NB, S)
    assert tuple(got["csd"].shape) == (B, NB, S + 1, S + 1) and got["csd"].dtype == torch.complex128 and not got["csd"].is_cuda
    assert got["spod_bins"].tolist() == list(bins)
    np.testing.assert_allclose(got["spod_freq"].numpy(), np.array(bins) / (Tn * 0.25), rtol=1e-15)
    # every chunking and a second run: the same bits
    for other, _ in runs[1:]:
        for key in got:
            assert same_bits(got[key].cpu(), other[key].cpu()), key
    raw = got["csd_raw"].cpu()
    check_symmetry(raw)
    # csd against the fp64 statement from scratch, under the yardstick rule
    ref = K.ref_spod(x64, bins, channels, window, J, cnt=sp.cnt)
    bound, e32, rel = K.csd_tolerance(ref["csd"], x64, x32, bins, channels, window)
    err = np.abs(got["csd"].numpy() - ref["csd"])
    scale = K.csd_scale(x64, channels, window)[:, None]
    print("case %d: csd max err %.3e = %.3e scale (restatement %.3e scale), %.3f of the bound"
          % (idx, float(err.max()), float((err / scale).max()), rel, float((err / bound).max())))
    assert bool((err <= bound).all()), (idx, float((err / bound).max()))
    # eigenvalues inside Weyl's bound ||dA||_F of the reference's
    kap = K.kappa_of(bins, Tn).reshape(1, NB, 1, 1)
    dA = kap * (got["csd"].numpy() - ref["csd"])[:, :, :S, :S] / S             # csd = M / HW: A = kappa csd / S
    weyl = np.sqrt((np.abs(dA) ** 2).sum((-2, -1)))
    lam_err = np.abs(got["spod_energy"].numpy() - ref["spod_energy"])
    assert bool((lam_err <= weyl[..., None] + 1e-12 * ref["spod_total"][..., None]).all()), (idx, lam_err.max(), weyl.max())
    np.testing.assert_allclose(got["spod_total"].numpy(), ref["spod_total"], rtol=0, atol=float(weyl.max()) * math.sqrt(S) + 1e-300)
    # spod_total against EnsembleTimeSpectrum's psd_mean on the same member rows: both are non-negative fp32 sums.  Relative bound
    # (cnt + 6 + 4 S^2) u: cnt for the diagonal of csd_raw; 6 for P = c_k (re^2 + im^2) with the fp32 c_k / Tn^2 and the host's fp64
    # sums; Welford's mean takes 4 roundings per member, each relative to the largest P_m <= S mean_m P_m of the pixel: 4 S^2
    ts = ops.EnsembleTimeSpectrum(S, B, Cc, Hh, Ww, Tn, DEV, K.MU[:Cc], K.SD[:Cc], u=None if u is None else u.to(DEV), nfreq=max(bins) + 1,
                                  window=window)
    for t in range(Tn):
        ts.add(ysd[t, :S].reshape(S * B, Cc, Hh, Ww).contiguous(memory_format=torch.channels_last), 0)
    psd = ts.finalize()["psd_mean"].double().cpu()[:, list(bins)][:, :, list(channels)]   # [B, NB, Cg, H, W]
    field = psd.reshape(B, NB, Cg, -1).mean(-1).sum(-1)
    relb = (sp.cnt + 6 + 4 * S * S) * K.U24
    dev = ((got["spod_total"] - field).abs() / field)
    print("case %d: spod_total vs psd_mean: %.3e relative, bound %.3e" % (idx, float(dev.max()), relb))
    assert bool((dev <= relb).all())
    # modes: NaN exactly where the mode is under the floor or j >= S; elsewhere orthonormal in <., .> within the kernels' roundings
    modes = got["spod_modes"].cpu().double()
    valid = got["spod_energy"] > got["spod_noise_floor"].unsqueeze(-1)
    valid[..., S:] = False
    assert torch.equal(torch.isnan(modes).reshape(B, NB, J, -1).all(-1), ~valid)
    assert torch.equal(torch.isnan(modes).reshape(B, NB, J, -1).any(-1), ~valid)
    assert torch.equal(torch.isnan(got["target_mode_energy"]), ~valid)
    phi = torch.complex(modes[:, :, :, 0], modes[:, :, :, 1]).reshape(B, NB, J, -1)
    gram = torch.einsum("bkie,bkje->bkij", phi.conj(), phi) / HW
    for b in range(B):
        for k in range(NB):
            v = valid[b, k]
            # <Phi_i, Phi_j> - delta_ij = w_i^H dM w_j / HW + the synthesis' own error.  |w_j|^2 = kappa / (S lambda_j) and
            # kappa |dM| / (S HW) = |dA| <= cnt u spod_total (the noise floor), so the first term is at most cnt u spod_total /
            # lambda_min.  The synthesis: |dPhi_j| <= (2 S + 2) u sum_m |w_mj| (|Re X_m| + |Im X_m|) (one chain of 2 S terms, the
            # weights' rounding), whose norm is at most sqrt(2) (2 S + 2) u sqrt(spod_total / lambda_j) by Cauchy-Schwarz with
            # trace M / HW = S spod_total / kappa; it enters twice.  Both are under 4 (cnt + 2 S + 2) u spod_total / lambda_min.
            lam_min = float(got["spod_energy"][b, k][v].min())
            tol = 4 * (sp.cnt + 2 * S + 2) * K.U24 * float(got["spod_total"][b, k]) / lam_min
            g = gram[b, k][v][:, v]
            assert float((g - torch.eye(int(v.sum()), dtype=g.dtype)).abs().max()) <= tol, (idx, b, k, tol)


# ---- 5. planted structure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["same", "psi2_at_k1"])
def test_planted_structure(target):
    p = K.PLANTED
    S, Tn, J = p["S"], p["Tn"], p["J"]
    HW = p["hw"][0] * p["hw"][1]
    x, psi1, psi2 = K.planted(target)
    ys = K.normalised(x, None)
    x64, x32 = K.fields(ys, None)
    got, sp = run_spod(ys.to(DEV), None, None, (p["k1"],), p["channels"], J, [5, 4, 3])
    ref = K.ref_spod(x64, (p["k1"],), p["channels"], None, J, cnt=sp.cnt)
    kap = K.kappa_of((p["k1"],), Tn)[0]
    dcsd = got["csd"].numpy()[0, 0] - ref["csd"][0, 0]
    dA = kap / S * math.sqrt((np.abs(dcsd[:S, :S]) ** 2).sum())
    lam = ref["lam_all"][0, 0]
    s = 2 * dA / (lam[0] - lam[1])                                             # Davis-Kahan: sin of the angle between the leading eigenvectors
    assert s < 0.1
    # the modes kernel's counted bound: |w_m0| <= sqrt(kappa / (S lambda_0)), one chain of 2 S terms and the rounding of the weights
    X = K.ref_coef(x64, (p["k1"],), None)[0, 0, :S][:, list(p["channels"])].reshape(S, -1)
    lam0 = min(float(got["spod_energy"][0, 0, 0]), lam[0])
    mag = math.sqrt(kap / (S * lam0)) * (np.abs(X.real) + np.abs(X.imag)).sum(0)
    eps = (2 * S + 2) * K.U24 * math.sqrt((mag ** 2).sum() / HW)
    m = got["spod_modes"].cpu().double()[0, 0, 0]
    phi = torch.complex(m[0], m[1]).reshape(-1).numpy()
    align = abs((phi.conj() * ref["modes"][0, 0, 0]).sum() / HW)
    print("planted %s: s %.3e, eps %.3e, |<Phi_0, Phi_0 ref>| %.9f, with psi_1 %.6f" % (target, s, eps, align, abs((phi.conj() * psi1).sum() / HW)))
    assert align >= math.sqrt(1 - s * s) - eps
    assert abs((phi.conj() * psi1).sum() / HW) > 0.999                         # the leading mode at k1 is psi_1
    # target_captured is a function of M alone: the eigenvector turns by at most s, the target's column, its energy and lambda_0 move
    # by their own relative errors
    col, rcol = got["csd"].numpy()[0, 0, :S, S], ref["csd"][0, 0, :S, S]
    relc = np.linalg.norm(col - rcol) / np.linalg.norm(rcol) + abs(dcsd[S, S]) / abs(ref["csd"][0, 0, S, S]) + dA / lam[0]
    tol = 2 * s + s * s + 3 * relc
    tc, rc = float(got["target_captured"][0, 0]), float(ref["target_captured"][0, 0])
    print("planted %s: target_captured %.6f, reference %.6f, tolerance %.3e" % (target, tc, rc, tol))
    if target == "same":
        assert abs(tc - rc) <= tol and tc > 0.99
    else:
        assert tc <= rc + tol and tc < 0.05


# ---- 6. modelPredSpod on the tiny model ----------------------------------------------------------------------------------------------
def test_model_pred_spod_end_to_end(monkeypatch, tmp_path):
    import tmg_hip
    import tmg_ops as ops
    from utils import utils
    import test_tspec_gpu as TS
    model, te = TS._cylinder_case(tmp_path)
    steps = min(int(b[0].shape[1]) for b in te)
    S, stride, t_start, max_rows, J, channels, window = 5, 2, 1, 4, 3, (0, 1), "hann"
    tmax = steps - steps % stride
    nkeep = tmax // stride
    Tn = nkeep - t_start
    assert Tn >= 3
    bins = tuple(range(1, Tn // 2 + 1))
    batches = [int(b[0].shape[0]) for b in te]
    kp = TS._KeyPatch(monkeypatch, ops)
    args = SimpleNamespace(device=None)
    for rep in range(3):                                                       # modelPredSpod, modelPredStats, modelPredTimeSpectra
        for bi, B in enumerate(batches):
            per = max(1, max_rows // B)
            for t in range(tmax):
                for m0 in range(0, S, per):
                    kp.queue_fold(bi, t, m0, min(per, S - m0))
    kw = dict(samples=S, stride=stride, tmax=tmax, t_start=t_start, max_rows=max_rows)
    torch.manual_seed(77)
    got = utils.modelPredSpod(args, model, te, TS.LOG, modes=J, channels=channels, window=window, **kw)
    torch.manual_seed(77)
    plain = utils.modelPredStats(args, model, te, TS.LOG, **kw)
    torch.manual_seed(77)
    tsp = utils.modelPredTimeSpectra(args, model, te, TS.LOG, nfreq=max(bins) + 1, window=window, **kw)
    assert not kp.fold
    assert set(got) == set(plain) | set(HOST_KEYS) | {"csd_raw", "spod_modes"}
    for name in plain:
        assert torch.equal(got[name], plain[name]), name
    N = got["target"].shape[0]
    NB, R = len(bins), S + 1
    Hh, Ww = got["target"].shape[-2:]
    HW = Hh * Ww
    assert tuple(got["csd_raw"].shape) == (N, NB, 2, R, R) and tuple(got["spod_modes"].shape) == (N, NB, J, 2, 2, Hh, Ww)
    assert tuple(got["csd"].shape) == (N, NB, R, R) and tuple(got["spod_energy"].shape) == (N, NB, J)
    assert tuple(got["loo_captured"].shape) == (N, NB, S) and tuple(got["target_captured_rank"].shape) == (N, NB)
    assert got["spod_bins"].tolist() == list(bins) and got["spod_freq"].dtype == torch.float64
    np.testing.assert_allclose(got["spod_freq"].numpy(), np.array(bins) / float(Tn), rtol=1e-15)
    # spod_total against modelPredTimeSpectra's psd_mean under the same RNG state (the bound of the end-to-end test)
    plans = [tmg_hip.ens_spod_plan(S, B, 2, HW, NB) for B in batches]
    relb = (max(q["L"] + q["P"] for q in plans) + K.C_ROUNDINGS + 6 + 4 * S * S) * K.U24
    field = tsp["psd_mean"].double()[:, list(bins)][:, :, list(channels)].reshape(N, NB, 2, -1).mean(-1).sum(-1)
    dev = (got["spod_total"] - field).abs() / field
    print("modelPredSpod: spod_total vs psd_mean %.3e relative, bound %.3e" % (float(dev.max()), relb))
    assert bool((dev <= relb).all())
    # the target row is the loader's target at steps j * stride: its own energy against the fp64 statement, under the yardstick rule
    t32 = got["target"][:, [j * stride for j in range(t_start, nkeep)]].permute(1, 0, 2, 3, 4).unsqueeze(1).contiguous()   # [Tn, 1, N, C, H, W]
    t64 = t32.double().numpy()
    X = K.ref_coef(t64, bins, window)[:, :, 0][:, :, list(channels)].reshape(N, NB, -1)
    ref_ss = ((np.abs(X) ** 2).sum(-1) / HW).reshape(N, NB, 1, 1)
    bound, _, _ = K.csd_tolerance(ref_ss.astype(np.complex128), t64, t32, bins, channels, window)
    err = np.abs(got["csd"].numpy()[:, :, S, S].reshape(N, NB, 1, 1) - ref_ss)
    print("modelPredSpod: target row max err %.3e, %.3f of the bound" % (float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    np.testing.assert_allclose(got["target_energy"].numpy(), K.kappa_of(bins, Tn).reshape(1, NB) * got["csd"].numpy()[:, :, S, S].real,
                               rtol=1e-12)
