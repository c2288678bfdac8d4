"""Shared tables, fp64 references and rounding counts of the spectral POD tests (test_spod_cpu.py, test_spod_gpu.py).

Rounding count of one csd_raw entry (csrc/tmg_spod.hip).  raw0[m][n] and raw1[m][n] are each one fp32 addition of two Gram sums over the
Cg HW elements.  One Gram sum is built from partials: a partial is four waves' fmaf chains of L / 4 terms each (L = Cg SL, the plan's)
added in wave order, which is at most L roundings on a dependent path; the P partials are added in slice order (at most P).  Beside
L + P the code holds, per entry:
  3 per operand, 6 in all: xbar = sum * fl(1 / Tn), the product xbar G, the subtraction re_k - xbar G.  The contract DEFINES X_m as the
    result of exactly these fp32 operations (tspec_finalize_kernel's), and the reference below forms X the same way, so they are slack
    here; they are counted because they are roundings of the entry against the exact coefficient
  1 for the final combine (RR + II, RI - RI^T)
  1 for the second-order terms of the (1 + u)^n product
so c = C_ROUNDINGS = 8 and cnt = L + P + 8, with u = 2^-24.  |got - ref| <= cnt u sum_e |X_m(e)| |X_n(e)| then follows from the standard
bound of a recursive fp32 sum of products, because |Re_m Re_n| + |Im_m Im_n| <= |X_m| |X_n| and |Re_m Im_n| + |Im_m Re_n| <= |X_m| |X_n|
(Cauchy-Schwarz on the pairs (|Re_m|, |Im_m|) and (|Re_n|, |Im_n|), in either order), element by element.

Modes kernel: one output element is ONE fmaf chain of 2 SP terms, of which 2 S are not exact zeros: 2 S roundings, + 1 second order:
|got - ref| <= (2 S + 1) u sum_q |w_q| |Z_q| against the fp64 product of the same fp32 operands.

The end-to-end yardstick (as tests/test_tspec_gpu.py applies it): bound = max(1e-5 |ref| + C_SCALE scale, 3 e32) with
scale[m][n] = Cg Tn^2 sqrt(Praw_m Praw_n), Praw_m the mean over the selected channels and the pixels of mean_n (g_n xh_n)^2 of row m (the
power INCLUDING the mean: the blocked DFT and the subtraction of xbar G make the fp32 error absolute in it), and e32 the largest error
against fp64 of the plain fp32 torch restatement f32_csd below.  C_SCALE = 10 x the largest e32 / scale that test_spod_cpu.py measures
over E2E_CASES on the CPU: measured 7.7e-8 (case 3: one channel without a mean; the others stay under 3.5e-8), so C_SCALE = 7.7e-7."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
C_ROUNDINGS = 8
C_SCALE = 7.7e-7
E32_MEASURED = 7.7e-8
BLOCK = 16                       # steps per ring pass (csrc/tmg_tspec.hip)

MU = torch.tensor([0.3, -0.2, 0.5, 0.1])
SD = torch.tensor([1.7, 0.6, 2.5, 1.1])
U = torch.tensor([[1.3, 0.7, 1.69, 0.9], [0.8, 1.2, 0.64, 1.1], [1.1, 0.9, 1.21, 1.0]])


# ---- kernel-level case tables ---------------------------------------------------------------------------------------------------------
# name, R, (H, W), B, C, channels, bins, NF, Tn, integer G
#   R: 2 (the smallest), 8 (2 R = 16: the one-tile instance, full), 9 (18 rows: the last tile holds two rows), 32 (one full macro-tile),
#   33 (a second macro-tile of two rows: the off-diagonal launch), 129 (five macro-tiles), 256 (the limit: eight)
#   HW: 1, 63 (scalar loads), 64, 65 (scalar, one pixel in the second chunk), 272 (two slices), 528 (three slices)
CSD_CASES = [
    dict(name="r2_hw1", R=2, hw=(1, 1), B=1, C=2, channels=(0, 1), bins=(1,), NF=2, Tn=4, gint=False),
    dict(name="r8_hw63_b3", R=8, hw=(7, 9), B=3, C=3, channels=(2, 0), bins=(1, 3), NF=5, Tn=8, gint=True),
    dict(name="r9_hw64", R=9, hw=(8, 8), B=1, C=4, channels=(3, 1, 0), bins=(2,), NF=3, Tn=8, gint=False),
    dict(name="r32_hw65_b3", R=32, hw=(5, 13), B=3, C=2, channels=(1,), bins=(1, 2), NF=3, Tn=4, gint=True),
    dict(name="r33_hw272_16bins", R=33, hw=(16, 17), B=1, C=3, channels=(0, 1, 2), bins=tuple(range(1, 17)), NF=17, Tn=32, gint=True),
    dict(name="r129_hw528", R=129, hw=(16, 33), B=1, C=2, channels=(1, 0), bins=(1,), NF=2, Tn=4, gint=False),
    dict(name="r256_hw65", R=256, hw=(5, 13), B=1, C=2, channels=(0,), bins=(2, 5), NF=6, Tn=16, gint=True),
    dict(name="r2_hw528_b3", R=2, hw=(16, 33), B=3, C=4, channels=(1, 2, 3, 0), bins=(1, 4), NF=5, Tn=8, gint=True),
]
CSD_BY_NAME = {c["name"]: c for c in CSD_CASES}
# What the plan reports for each case: (one-tile instance, macro-tiles NT, the last 16-row tile is full, P > 1, vector loads).  Pinned:
# a table entry that is removed, or a plan that changes, fails test_spod_cpu.py.
CSD_BRANCHES = {
    "r2_hw1": (True, 1, False, False, False),
    "r8_hw63_b3": (True, 1, True, False, False),
    "r9_hw64": (False, 1, False, False, True),
    "r32_hw65_b3": (False, 1, True, False, False),
    "r33_hw272_16bins": (False, 2, False, True, True),
    "r129_hw528": (False, 5, False, True, True),
    "r256_hw65": (False, 8, True, False, False),
    "r2_hw528_b3": (True, 1, False, True, True),
}


def csd_branches(plan, R):
    return (plan["part"] == 256, plan["NT"], (2 * R) % 16 == 0, plan["P"] > 1, plan["vec"])


def int_acc(case, seed):
    """A hand-made accumulator of small integers and its constants: acc [2 NF + 1, R, B, C, HW] in -3..3 (fp32), cst [3, NF] with
    G = 0 or integer G in -2..2 (Tn a power of two: xbar, xbar G and the subtraction are exact dyadic numbers)."""
    g = torch.Generator().manual_seed(seed)
    H_, W_ = case["hw"]
    NF = case["NF"]
    acc = torch.randint(-3, 4, (2 * NF + 1, case["R"], case["B"], case["C"], H_ * W_), generator=g).float()
    cst = torch.zeros(3, NF)
    if case["gint"]:
        cst[:2] = torch.randint(-2, 3, (2, NF), generator=g).float()
    cst[2] = 2.0 / case["Tn"] ** 2
    return acc, cst


def int_csd(acc, cst, case):
    """Tn^2 csd_raw of an integer accumulator as exact int64: Tn X = Tn re_k - sum G."""
    Tn, NF = case["Tn"], case["NF"]
    a = acc.to(torch.int64)
    G = cst.to(torch.int64)
    ch = list(case["channels"])
    out = []
    for k in case["bins"]:
        re = (Tn * a[k] - a[2 * NF] * G[0, k])[:, :, ch].permute(1, 0, 2, 3).reshape(case["B"], case["R"], -1)
        im = (Tn * a[NF + k] - a[2 * NF] * G[1, k])[:, :, ch].permute(1, 0, 2, 3).reshape(case["B"], case["R"], -1)
        rr = torch.einsum("bme,bne->bmn", re, re) + torch.einsum("bme,bne->bmn", im, im)
        ri = torch.einsum("bme,bne->bmn", re, im)
        out.append(torch.stack((rr, ri - ri.transpose(1, 2)), 1))
    return torch.stack(out, 1)                                                # [B, NB, 2, R, R]


def form_x32(acc, cst, k, Tn):
    """(Re X, Im X) of bin k as the contract defines them, with tspec_finalize_kernel's fp32 roundings: [R, B, C, HW] fp32 (CPU)."""
    NF = cst.shape[1]
    xbar = acc[2 * NF] * torch.tensor(1.0 / Tn, dtype=torch.float32)
    return acc[k] - xbar * cst[0, k], acc[NF + k] - xbar * cst[1, k]


def rows_of(x, channels):
    """[R, B, C, HW] -> [B, R, Cg HW] over the selected channels in their order."""
    return x[:, :, list(channels)].permute(1, 0, 2, 3).reshape(x.shape[1], x.shape[0], -1)


def csd_ref64(acc, cst, bins, channels, Tn):
    """-> (ref [B, NB, 2, R, R] fp64, mag [B, NB, R, R] fp64 = sum_e |X_m| |X_n|): the fp64 Gram of the contract's X."""
    ref, mag = [], []
    for k in bins:
        re, im = (rows_of(v.double(), channels) for v in form_x32(acc, cst, k, Tn))
        rr = re @ re.transpose(1, 2) + im @ im.transpose(1, 2)
        ri = re @ im.transpose(1, 2)
        ref.append(torch.stack((rr, ri - ri.transpose(1, 2)), 1))
        ab = torch.sqrt(re * re + im * im)
        mag.append(ab @ ab.transpose(1, 2))
    return torch.stack(ref, 1), torch.stack(mag, 1)


def csd_bound(mag, cnt):
    """[B, NB, 2, R, R]: cnt u sum |X_m| |X_n|, for raw0 and for raw1."""
    b = cnt * U24 * mag
    return torch.stack((b, b), 2)


def gauss_acc(case, seed, offset):
    """A Gaussian accumulator; offset: a large common value on every plane (the mean of a series ends up in all of them)."""
    g = torch.Generator().manual_seed(seed)
    H_, W_ = case["hw"]
    NF, Tn = case["NF"], case["Tn"]
    acc = torch.randn((2 * NF + 1, case["R"], case["B"], case["C"], H_ * W_), generator=g) + offset
    cst = torch.zeros(3, NF)
    if case["gint"]:
        cst[:2] = torch.randn((2, NF), generator=g)
    cst[2] = 2.0 / Tn ** 2
    return acc.float(), cst.float()


REAL_CASES = [("r9_hw64", 0.0), ("r8_hw63_b3", 40.0), ("r33_hw272_16bins", 0.0), ("r129_hw528", 25.0), ("r2_hw528_b3", 0.0)]

# modes kernel: name, S, (H, W), B, C, channels, bins, NF, Tn, J.  S 1 (one padded step), 4 (exact steps), 5, 37; HW 1, 63, 65 (a tail
# inside a column tile), 272 (two pixel blocks)
MODES_CASES = [
    dict(name="s1_hw1", S=1, hw=(1, 1), B=1, C=2, channels=(1,), bins=(1,), NF=2, Tn=4, J=1),
    dict(name="s4_hw63", S=4, hw=(7, 9), B=3, C=3, channels=(2, 0), bins=(1, 3), NF=5, Tn=8, J=4),
    dict(name="s5_hw65", S=5, hw=(5, 13), B=1, C=4, channels=(3, 1, 0), bins=(2,), NF=3, Tn=8, J=8),
    dict(name="s37_hw272", S=37, hw=(16, 17), B=2, C=2, channels=(0, 1), bins=(1, 2, 4), NF=5, Tn=16, J=3),
]


def modes_operand(w, S):
    """complex weights w [B, NB, S, J] -> the kernel's operand [B, NB, 16, 2 SP] fp64 (row 2 j = [Re w_j | -Im w_j], row 2 j + 1 =
    [Im w_j | Re w_j], SP = S rounded up to 4)."""
    B, NB, _, J = w.shape
    SP = (S + 3) // 4 * 4
    wt = w.transpose(2, 3)
    wr = torch.zeros((B, NB, 16, 2 * SP), dtype=torch.float64)
    wr[:, :, 0:2 * J:2, :S], wr[:, :, 0:2 * J:2, SP:SP + S] = wt.real, -wt.imag
    wr[:, :, 1:2 * J:2, :S], wr[:, :, 1:2 * J:2, SP:SP + S] = wt.imag, wt.real
    return wr


def modes_ref64(acc, cst, case, wr32):
    """-> (ref, mag) [B, NB, 2 J, Cg, HW] fp64: wr32 (the fp32 operand) times the contract's X of the members' rows, and sum |w| |Z|."""
    S, J = case["S"], case["J"]
    SP = (S + 3) // 4 * 4
    ref, mag = [], []
    for i, k in enumerate(case["bins"]):
        re, im = (v[:S, :, list(case["channels"])].double() for v in form_x32(acc, cst, k, case["Tn"]))   # [S, B, Cg, HW]
        w = wr32[:, i, :2 * J].double()                                       # [B, 2 J, 2 SP]
        r = torch.einsum("brq,qbce->brce", w[:, :, :S], re) + torch.einsum("brq,qbce->brce", w[:, :, SP:SP + S], im)
        m = torch.einsum("brq,qbce->brce", w[:, :, :S].abs(), re.abs()) + torch.einsum("brq,qbce->brce", w[:, :, SP:SP + S].abs(), im.abs())
        ref.append(r)
        mag.append(m)
    return torch.stack(ref, 1), torch.stack(mag, 1)


# ---- the fp64 statement from scratch ----------------------------------------------------------------------------------------------------
def hann(n):
    w = 0.5 - 0.5 * np.cos(2 * math.pi * np.arange(n, dtype=np.float64) / n)
    return w / np.sqrt(np.mean(w * w))


def kappa_of(bins, Tn):
    return np.array([(1.0 if (Tn % 2 == 0 and k == Tn // 2) else 2.0) / float(Tn) ** 2 for k in bins])


def ref_coef(x, bins, window):
    """x [Tn, R, B, C, H, W] fp64 -> X [B, NB, R, C, HW] complex128: numpy rfft of g (x - mean)."""
    Tn = x.shape[0]
    g = hann(Tn) if window == "hann" else np.ones(Tn)
    d = g.reshape(-1, 1, 1, 1, 1, 1) * (x - x.mean(0, keepdims=True))
    X = np.fft.rfft(d, axis=0)[list(bins)]                                     # [NB, R, B, C, H, W]
    return np.moveaxis(X.reshape(X.shape[:4] + (-1,)), 2, 0)


def ref_spod(x, bins, channels, window, J, cnt=0.0, conj_swapped=False, unbiased=False, no_kappa=False, with_target=False):
    """The issue's definitions in fp64 numpy from the series x [Tn, R, B, C, H, W] (rows: the S members, then the target).  The keyword
    arguments state WRONG definitions (test_spod_cpu.py: the reference must tell them apart).  -> dict of numpy arrays; modes
    [B, NB, J, Cg HW] complex."""
    Tn, R = x.shape[:2]
    S = R - 1
    HW = x.shape[4] * x.shape[5]
    X = ref_coef(x, bins, window)[:, :, :, list(channels)]
    B, NB = X.shape[:2]
    X = X.reshape(B, NB, R, -1)
    M = np.einsum("bkme,bkne->bkmn", X if conj_swapped else X.conj(), X.conj() if conj_swapped else X)
    kap = (np.ones(len(bins)) if no_kappa else kappa_of(bins, Tn)).reshape(1, NB, 1, 1)
    n = R if with_target else S
    A = kap * M[:, :, :n, :n] / ((n - 1 if unbiased else n) * HW)
    lam, th = np.linalg.eigh(A)
    lam, th = lam[..., ::-1], th[..., ::-1]
    Jn = min(J, n)
    total = np.trace(A, axis1=-2, axis2=-1).real
    floor = cnt * U24 * total
    energy = np.zeros((B, NB, J))
    energy[..., :Jn] = lam[..., :Jn]
    valid = np.zeros((B, NB, J), dtype=bool)
    valid[..., :Jn] = lam[..., :Jn] > floor[..., None]
    modes = np.full((B, NB, J, X.shape[-1]), np.nan + 1j * np.nan)
    tme = np.full((B, NB, J), np.nan)
    for b in range(B):
        for k in range(NB):
            for j in range(Jn):
                if valid[b, k, j]:
                    phi = (th[b, k, :, j][:, None] * X[b, k, :n]).sum(0) * math.sqrt(kap[0, k, 0, 0] / (n * lam[b, k, j]))
                    modes[b, k, j] = phi
                    tme[b, k, j] = kap[0, k, 0, 0] * abs((phi.conj() * X[b, k, S]).sum() / HW) ** 2
    ten = kap[0, :, 0, 0] * M[:, :, S, S].real / HW
    return {"csd": M / HW, "A": A, "spod_energy": energy, "spod_total": total, "valid": valid, "modes": modes, "target_mode_energy": tme,
            "target_energy": ten, "target_captured": np.nansum(tme, -1) / ten, "lam_all": lam}


# ---- the fp32 yardstick ---------------------------------------------------------------------------------------------------------------
def operand32(Tn, NF, window):
    """The constants of the blocked DFT, fp64 rounded once to fp32: tm [Tn, 2 NF + 1] (g cos, -g sin, ones), cst [3, NF]."""
    g = hann(Tn) if window == "hann" else np.ones(Tn)
    n, k = np.arange(Tn, dtype=np.int64), np.arange(NF, dtype=np.int64)
    ang = ((n[:, None] * k[None, :]) % Tn).astype(np.float64) * (2 * math.pi / Tn)
    tm = np.concatenate([g[:, None] * np.cos(ang), -g[:, None] * np.sin(ang), np.ones((Tn, 1))], axis=1)
    G = np.stack([tm[:, :NF].sum(0), tm[:, NF:2 * NF].sum(0)])
    G[np.abs(G) < 1e-9 * Tn] = 0.0
    ck = np.full(NF, 2.0)
    ck[0] = 1.0
    if Tn % 2 == 0 and NF > Tn // 2:
        ck[Tn // 2] = 1.0
    f = lambda a: torch.from_numpy(a.astype(np.float32))                       # noqa: E731
    return f(tm), f(np.concatenate([G, (ck / float(Tn) ** 2)[None]]))


def f32_acc(x32, NF, window):
    """The accumulator as a plain fp32 torch restatement: x32 [Tn, R, B, C, H, W] fp32 (CPU) -> (acc [2 NF + 1, R, B, C, HW], cst)."""
    Tn = x32.shape[0]
    tm, cst = operand32(Tn, NF, window)
    flat = x32.reshape(Tn, -1)
    acc = None
    for n0 in range(0, Tn, BLOCK):
        blk = tm[n0:n0 + BLOCK].t() @ flat[n0:n0 + BLOCK]
        acc = blk if acc is None else acc + blk
    return acc.reshape((2 * NF + 1,) + tuple(x32.shape[1:4]) + (-1,)), cst


def f32_csd(x32, bins, channels, window):
    """csd [B, NB, R, R] complex (fp32 parts, as fp64 numpy) of the restatement: blocked DFT, the contract's X, fp32 matmuls, / HW."""
    Tn = x32.shape[0]
    HW = x32.shape[4] * x32.shape[5]
    acc, cst = f32_acc(x32, max(bins) + 1, window)
    out = []
    for k in bins:
        re, im = (rows_of(v, channels) for v in form_x32(acc, cst, k, Tn))
        rr = re @ re.transpose(1, 2) + im @ im.transpose(1, 2)
        ri = re @ im.transpose(1, 2)
        out.append(torch.complex(rr.double(), (ri - ri.transpose(1, 2)).double()))
    return (torch.stack(out, 1) / HW).numpy()


def csd_scale(x64, channels, window):
    """[B, R, R]: Cg Tn^2 sqrt(Praw_m Praw_n)."""
    Tn = x64.shape[0]
    g = (hann(Tn) if window == "hann" else np.ones(Tn)).reshape(-1, 1, 1, 1, 1, 1)
    praw = ((g * x64[:, :, :, list(channels)]) ** 2).mean(0).mean((2, 3, 4))    # [R, B]
    s = np.sqrt(praw.T[:, :, None] * praw.T[:, None, :])
    return len(channels) * float(Tn) ** 2 * s


def csd_tolerance(ref_csd, x64, x32, bins, channels, window):
    """-> (bound [B, NB, R, R], e32, the largest e32 / scale): max(1e-5 |ref| + C_SCALE scale, 3 e32)."""
    scale = csd_scale(x64, channels, window)[:, None]
    err32 = np.abs(f32_csd(x32, bins, channels, window) - ref_csd)
    e32 = float(err32.max())
    return np.maximum(1e-5 * np.abs(ref_csd) + C_SCALE * scale, 3 * e32), e32, float((err32 / scale).max())


# ---- series -------------------------------------------------------------------------------------------------------------------------------
def synthetic(Tn, R, B, Cc, Hh, Ww, seed, amp=0.3, noise=0.05):
    """[Tn, R, B, C, H, W] fp64: per case a few spatial patterns oscillating at integer and non-integer frequencies with a random
    complex amplitude per row (so that the rows are coherent), plus white noise, on a mean of 1 in channel 0."""
    rng = np.random.default_rng(seed)
    n = np.arange(Tn, dtype=np.float64).reshape(-1, 1, 1, 1, 1, 1)
    x = noise * rng.standard_normal((Tn, R, B, Cc, Hh, Ww))
    for f in (1.0, 2.0, 2.6, min(5.0, Tn / 2.0)):
        pat = rng.standard_normal((2, 1, 1, B, Cc, Hh, Ww))
        a = rng.standard_normal((2, 1, R, B, 1, 1, 1))
        ph = 2 * math.pi * f * n / Tn
        x = x + amp * ((a[0] * pat[0] - a[1] * pat[1]) * np.cos(ph) - (a[0] * pat[1] + a[1] * pat[0]) * np.sin(ph))
    x[:, :, :, 0] += 1.0
    return x


def normalised(f, u):
    """The model-side tensor whose un-normalisation u[b, c] (sd y + mu) gives f: [Tn, R, B, C, H, W] fp32 (CPU)."""
    Cc = f.shape[3]
    y = torch.from_numpy(f)
    if u is not None:
        y = y / u.double().view(1, 1, u.shape[0], Cc, 1, 1)
    y = (y - MU[:Cc].double().view(1, 1, 1, Cc, 1, 1)) / SD[:Cc].double().view(1, 1, 1, Cc, 1, 1)
    return y.float()


def fields(ys, u):
    """(fp64, fp32) un-normalised series of the fp32 tensor ys: the fp64 statement's input and the kernel's own fp32 form."""
    yc = ys.cpu()
    Cc = yc.shape[3]
    mu, sd = MU[:Cc].view(1, 1, 1, Cc, 1, 1), SD[:Cc].view(1, 1, 1, Cc, 1, 1)
    f64 = sd.double() * yc.double() + mu.double()
    f32 = sd * yc + mu
    if u is not None:
        f64 = f64 * u.double().view(1, 1, u.shape[0], Cc, 1, 1)
        f32 = f32 * u.view(1, 1, u.shape[0], Cc, 1, 1)
    return f64.numpy(), f32


# (Tn, (H, W), C, B, S, u given, window, bins, channels, J): Tn 5: a remainder fold alone; 16: one exact ring; 19: a ring and a remainder
E2E_CASES = [
    (5, (5, 7), 3, 2, 3, True, "hann", None, (0, 1), 4),
    (16, (12, 20), 2, 1, 5, False, None, (1, 3, 8), (1, 0), 3),
    (19, (8, 8), 4, 2, 4, True, "hann", (2, 5, 9), (0, 1, 3), 4),
    (19, (5, 7), 3, 2, 6, False, None, None, (2,), 2),
    (16, (5, 13), 3, 3, 3, True, "hann", (1, 2), (0, 1), 8),
    (5, (16, 17), 2, 1, 1, False, "hann", (1, 2), (0, 1), 2),
]


def e2e_inputs(idx):
    """-> (ys fp32 [Tn, R, B, C, H, W] on the CPU, u or None) of case idx; row S is the target."""
    Tn, (Hh, Ww), Cc, B, S, u_given, window, bins, channels, J = E2E_CASES[idx]
    u = U[:B, :Cc].contiguous() if u_given else None
    return normalised(synthetic(Tn, S + 1, B, Cc, Hh, Ww, 500 + idx), u), u


def e2e_bins(idx):
    Tn, bins = E2E_CASES[idx][0], E2E_CASES[idx][7]
    return tuple(range(1, min(16, Tn // 2) + 1)) if bins is None else bins


# ---- planted structure ----------------------------------------------------------------------------------------------------------------
PLANTED = dict(Tn=16, S=12, B=1, C=2, hw=(8, 9), k1=3, k2=5, channels=(0, 1), J=1, noise=0.01, seed=77)


def planted(target="same"):
    """Rows Re[a_m psi_1 e^{2 pi i k1 n / Tn}] + Re[b_m psi_2 e^{2 pi i k2 n / Tn}] + a mean field + small noise, psi_1 and psi_2
    orthonormal complex fields in <., .>, a_m and b_m random complex, no window.  target: "same" (one more realisation of the process) or
    "psi2_at_k1" (psi_2's pattern oscillating in bin k1).  -> (x [Tn, R, 1, C, H, W] fp64, psi_1, psi_2 [C HW] complex)."""
    p = PLANTED
    rng = np.random.default_rng(p["seed"])
    Tn, S, Cc = p["Tn"], p["S"], p["C"]
    Hh, Ww = p["hw"]
    N = Cc * Hh * Ww
    q, _ = np.linalg.qr(rng.standard_normal((N, 2)) + 1j * rng.standard_normal((N, 2)))
    psi = q.T * math.sqrt(Hh * Ww)                                             # <psi_i, psi_j> = delta_ij with the 1 / HW
    a = rng.standard_normal(S + 1) + 1j * rng.standard_normal(S + 1)
    b = 0.5 * (rng.standard_normal(S + 1) + 1j * rng.standard_normal(S + 1))
    n = np.arange(Tn).reshape(-1, 1, 1)
    e1, e2 = np.exp(2j * math.pi * p["k1"] * n / Tn), np.exp(2j * math.pi * p["k2"] * n / Tn)
    x = (a.reshape(1, -1, 1) * psi[0].reshape(1, 1, -1) * e1).real + (b.reshape(1, -1, 1) * psi[1].reshape(1, 1, -1) * e2).real
    if target == "psi2_at_k1":
        x[:, S] = (a[S] * psi[1].reshape(1, -1) * e1[:, 0]).real
    x = x + rng.standard_normal(N).reshape(1, 1, -1) + p["noise"] * rng.standard_normal((Tn, S + 1, N))
    return x.reshape(Tn, S + 1, 1, Cc, Hh, Ww), psi[0], psi[1]
