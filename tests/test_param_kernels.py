"""The kernels of the parameter and sampling side - tmg_mat_inverse, tmg_lu_fold_fwd / _bwd_split (tmg_pointwise.hip), the in-kernel
latent draw of tmg_gauss_sample / _keyed, tmg_reverse_loss_fwd / _bwd, tmg_sum_terms (tmg_glue.hip) and tmg_adam_step
(tmg_physics.hip) - each against a plain fp64 statement of the SAME operation, on every branch of its launcher.  The tmg_hip wrappers
are called directly; share / check / gauss_ref and the Gaussian tolerances are those of tests/test_pointwise_kernels.py (imported).

Case map (the plan of every case is computed in the test from the launcher's formula and asserted):
  tmg_mat_inverse (one block per matrix, dynamic LDS (2 C^2 + C) 8 + 16 + 4 C bytes): INV_CASES C in {1, 2, 3, 12, 48, 63, 64}: c63 =
      64 276 B, the last size below 64 KiB; c64 / c64n = 66 320 B, the opt-in branch.  K in {1, 5, 16}; b given / None; W a
      non-contiguous slice (c3 c12 c64); kappa 1 (c1 c12 c64n) and 1e3.  test_inverse_zero_diagonal: a cyclic row shift of a
      diagonally dominant matrix with the shifted-in entries zeroed: W_ii = 0 exactly, the pivot search swaps rows in every column
      but the last (C in {12, 64}).  test_inverse_dead_channels: zero row and column at 0, at C - 1 and at two interior indices
      (C in {8, 64}; one launch, K = 3).  C = 65: the wrapper raises.
  tmg_lu_fold_fwd / _bwd_split (grid (min(64, ceil(C^2 / 256)), K)): FOLD_CASES x reverse {0, 1}: c1k1 c3k2 c12k16 (K C = 192: every
      thread of the log-det loop takes at most one term) c48k16 (K C = 768 > 256: the loop) c127k1 (ceil(16129 / 256) = 64 blocks and
      16129 <= 64 * 256: the cap reached without looping) c130k2 (16900 > 16384: threads loop under the cap; K C = 260) c256k2 (the
      256-entry LDS arrays full).  (a, b) given / given (gg), null / null (c3k2), given / null (c48k16); dbm None (c127k1); dld None
      (c12k16); tail split - dWm / dbm over K - 1 layers plus tail tensors - c12k16 c130k2, and K = 1 with dWm None and only the
      tail: c1k1; sgn +1 / -1; layer k's row permutation is random / identity / reversal in turn.  C = 257: refused by the
      forward wrapper's assert and by the backward launcher (-1, _chk raises).
  tmg_gauss_sample, latents drawn in the kernel (grid (gx, B), gx = min(ceil((per / 4) / 256), clamp(ceil(2048 / B), 4, 256))):
      float4 path: v8 v8s5 (Ch = 8, 16 x 16, B = 3).  Scalar path by shape: s5 (Ch = 5, 7 x 9: 315 elements, the last quad holds 3)
      s6 (Ch = 6: quads straddle pixels); forced on Ch = 8 by a view: hodd8 (hz at channel offset 1) ostr8 (out with pixel stride
      17) - test_draw_scalar_equals_float4: their eps_out is torch.equal to v8's.  Cap 256 with every thread looping: cap256
      (B = 1, 512 x 512, Ch = 8: 524 288 quads on 256 x 256 threads).  Cap 4: cap4loop (B = 600, 24 x 24, Ch = 8: 1152 quads on 1024
      threads) and cap4 (B = 512, 20 x 20, Ch = 10, scalar: 1000 quads, four blocks, no loop).  site in {0, 5}; "hi" keys have bits
      63 and 31 of both words set; z1 given / None; eps_out None: test_draw_without_eps_out.  tmg_gauss_sample_keyed:
      rows_per_key in {1, 2, B} at B = 6 on both paths, every member against the host reference with its own key row and a counter
      that restarts.  Refused: B % rows_per_key != 0 (-4), eps and nonce both null (-3).  Out of reach: the high counter word
      (gq >= 2^32) needs B nquad >= 2^32 quads in one call - 64 GiB of latents; no case is built for it.
  tmg_adam_step (grid min(nchunks, 4096), chunks of <= 4096 elements): tensors of 1, 255, 4095, 4096, 4097, 3 * 4096 + 1 elements
      (10 chunks; the last chunk of the last tensor holds one element), and 4200 one-element tensors (nchunks > 4096: blocks loop).
      wd 0 (branch skipped) / 0.05, amsgrad 0 / 1 with vmax above and below the new v, bias corrections of steps 1 and 1000.  All
      tensors of a kind sit in one flat buffer with NaN gaps (3 and 1 elements): the gaps must stay NaN.
  tmg_reverse_loss_fwd (grid min(1024, ceil((n / 4) / 256))) / _bwd (cap 4096): n in {1, 3, 4, 5, 7, 1027}, n = 4 * 1024 * 256 + 7 (the
      forward loops), n = 4 * 4096 * 256 + 5 (both loop); B in {1, 256, 257, 1000} (the ld / dld loops above 256); misaligned y / dy
      refused (-2).  tmg_sum_terms: 1 and 8 terms, one-element terms mixed with vectors, B in {1, 256, 257, 70 000}; 9 terms (-2)
      and a term of the wrong length (-3) refused.
  Sensitivity (test_*_detects_*): the reference with one unit of work altered moves the measure to >= 10x its bound: one dead row
      left alive; one entry of l in the last row of the last layer; one Philox quad's counter off by one in the last image; the last
      element of the last Adam chunk; the tail element of the loss.

Bounds (measure and u = 2^-24 as in tests/test_pointwise_kernels.py: share = max_e |a_e - ref_e| / (tol (|ref_e| + s_e) + 2^-126)):
  inverse: fp64 Gauss-Jordan rounded once: tol = 1 u of |ref_e|, plus the elimination error kappa C 2^-52 max|Winv| as
      s_e = kappa C 2^-52 max|Winv| / u (printed: INVERSE lines; at most 1.5e-8 here, the rounding is what the share measures).
      binv_r = - sum_c Winv_rc b_c inherits sum_c |dWinv_rc| |b_c| <= (that error) sum|b|: s_e = kappa C 2^-52 max|Winv| sum|b| / u.
      kappa is asserted from the construction Q1 diag(sigma) Q2 (sigma log-spaced 1 .. 1 / kappa; fp32 rounding of W moves it by
      less than 1 %), and computed in fp64 for the shifted and the dead-channel matrices.  Independent: |Winv W - I| <= u (|Winv| |W|)
      elementwise on the live block (0.5 u of |Winv| |W| from the one rounding of Winv).
  fold: fp64 throughout, rounded once: 1 u of |ref_e| plus (C + 4) 2^-53 of S_e, the sum of the |terms| of the element's inner
      product: W: |lower| |upper| with diagonal e^{log_s} + 0.01 (row-permuted), Wm: S_W |a| or S_W / |a|, bm: S_W |b| or |b / a|,
      ld: hw (sum |log_s| + sum |log|a||); with A = |dWm| / |a_i| (reverse) or |dWm| |a_j| + |dbm_i| |b_j| the |terms| of dW and
      A_M its rows scattered by perm: dl: A_M |upper|^T, du: |lower|^T A_M, dlogs: S_du,ii e^{log_s} + |hw g|, da: sum |dWm| S_W
      (/ a^2) + |dbm b| / a^2 + |g hw / a|, db: S_W^T |dbm| or |dbm / a|.  The fp64 scratch W: (C + 4) 2^-53 S_e without the 1 u.
      dl is exactly 0 on and above the diagonal, du on and below it.  The masked halves of l and u hold junk: the kernel must not
      read them.
  draw: the reference uniform is (x + 0.5) 2^-32 exactly; the kernel's is the fp32 result of a conversion, a multiply and an add: up
      to 1.5 ulp away.  s_e = the spread (max - min over the 3 x 3 grid) of the fp64 Box-Muller value over u1 +- 1.5 ulp (clipped
      at 1, where the kernel returns +-0) and u2 +- 1.5 ulp, divided by the tolerance so that it counts once.  Function errors by
      the rule of the existing file - the same fp32 formula on the CPU against fp64 on 2e6 points, FOUR times the observed error
      allowed: sqrtf(-2 logf(u)) 1.50 u -> 6.0 u; cos / sin(2 pi u) 2.45 u -> 9.8 u (torch has no sincospif: the fp32 formula
      measured reduces 2 u exactly to |t| <= 1 / 4 and takes sin / cos(pi t)); + 1 u for the product: TOL_EPS = 16.8 u.
      out and logp: gauss_ref (mode 1) on the kernel's own eps with TOL_GAUSS / TOL_LP of the existing file.
  adam (G = |g| + wd |p|, gi = g + wd p by one fmaf): m: u (omb1 G + 2 omb1 |gi - m| + |m'|) (gi, the difference, the product, the
      sum); v: u (omb2 (2 |gi| G + 2 gi^2) + b2 v + v') (gi twice in the square, the square, two products, the sum); vmax: as v;
      p: u |p'| + (step / den) E_m + |upd| (E_v / (2 vx) + 6 u) (sqrt halves v's relative error; sqrtf, / bc2s, + eps, lr / bc1, m / den,
      step *: 6 roundings).  The fp32 values of lr, beta2, eps, wd, bc1, sqrt(bc2), 1 - beta1, 1 - beta2 enter the reference.
  loss: (1 + sqrt K) u of s1 sum y^2 + s2 sum |ld|, K = n + B; dy 2 u (s1 g, a y); dld = fl(s2 g) exactly.  sum_terms: n u of the
      sum of the |terms| (n - 1 additions in sequence).

Observed on an MI355X (largest share of each bound; LAB_NOTES.md, "The fold, inverse, draw, loss and Adam kernels against fp64 on
every dispatch path"; from the SHARE lines of a run of the whole GPU suite, every test of this file passing): inverse Winv 0.9941,
binv 0.9621, Winv W - I 0.9378; fold W (fp64) 0.1644, Wm 0.9979, bm 0.9677, ld 0.4247, dl 0.9981, du 0.9967, dlogs 0.9538, da 0.9805,
db 0.9693; draw eps 0.1946, out 0.1434, logp 0.0179; adam m 0.8487, v 0.9377, vmax 0.9377, p 0.9953; loss value 0.3143, dy 0.7847;
sum_terms 0.6502.  Shares near 1 are what a 1 u bound means: one correct rounding to fp32 is an error of up to 1 u of the value, so
over some thousand elements a correctly rounded result reaches 0.99 of it; the fp64 reference rounded once to fp32 on the CPU gives
the same figures for the inverse and the fold (0.9941 / 0.9979 / 0.9981 ...), i.e. those kernels are right to the last bit."""
import math

import numpy as np
import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import philox_ref as PH
import test_pointwise_kernels as PW

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
U = PW.U
E53 = 2.0 ** -53
TOL_EPS = 4 * 1.50 * U + 4 * 2.45 * U + U
F64 = torch.float64
GUARD = 64              # elements on either side of an output (256 bytes of fp32: keeps a 16-byte aligned view aligned)
MINE = set()
share = PW.share


def _H():
    import tmg_hip as H
    return H


def check(a, ref, s, tol, what, case=""):
    MINE.add(what)
    PW.check(a, ref, s, tol, what, case)


@pytest.fixture(scope="module", autouse=True)
def _report_shares():
    yield
    for k in sorted(MINE):
        print("SHARE %-28s %.4f" % (k, PW.SHARES.pop(k, NAN)))


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def guarded(shape, dtype=torch.float32, fill=NAN):
    """(buffer, view): `shape` elements of `fill` between two NaN guards."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    v = buf[GUARD:GUARD + n].view(shape)
    v.fill_(fill)
    return buf, v


def intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def raises_code(code, fn, *a, **k):
    with pytest.raises(RuntimeError, match="code %d" % code):
        fn(*a, **k)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. tmg_mat_inverse
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, C, K, kappa, b given, W a non-contiguous slice)
INV_CASES = [
    ("c1", 1, 1, 1.0, True, False),
    ("c2", 2, 5, 1e3, False, False),
    ("c3", 3, 16, 1e3, True, True),
    ("c12", 12, 5, 1.0, True, True),
    ("c48", 48, 1, 1e3, True, False),
    ("c63", 63, 5, 1e3, True, False),
    ("c64", 64, 16, 1e3, True, True),
    ("c64n", 64, 1, 1.0, False, False),
]


def inv_lds(Cn):
    """tmg_mat_inverse: bytes of dynamic LDS."""
    return (2 * Cn * Cn + Cn) * 8 + 16 + Cn * 4


def _orth(n, g):
    return torch.linalg.qr(torch.randn(n, n, generator=g, dtype=F64))[0]


def conditioned(n, kappa, g):
    """Q1 diag(sigma) Q2, sigma log-spaced from 1 to 1 / kappa (fp64)."""
    sig = torch.logspace(0, -math.log10(kappa), n, dtype=F64) if n > 1 else torch.ones(1, dtype=F64)
    return _orth(n, g) @ torch.diag(sig) @ _orth(n, g)


def _inv_run(W0, b0, sliced=False):
    K, Cn = W0.shape[:2]
    if sliced:
        big = torch.full((K, Cn + 1, Cn + 3), NAN, device=DEV)
        W = big[:, :Cn, :Cn]
        W.copy_(W0)
        assert not W.is_contiguous()
    else:
        W = W0.to(DEV)
    Winv, binv = _H().mat_inverse(W, b0.to(DEV) if b0 is not None else None)
    torch.cuda.synchronize()
    assert (binv is None) == (b0 is None)
    return Winv.cpu(), binv.cpu() if binv is not None else None


def inv_ref(Wk, bk, dead=()):
    """fp64: the inverse of the live block embedded in zeros, binv (zero on dead rows), the live indices."""
    Cn = Wk.shape[0]
    live = torch.tensor([i for i in range(Cn) if i not in dead])
    ref = torch.zeros(Cn, Cn, dtype=F64)
    ref[live[:, None], live[None, :]] = torch.linalg.inv(Wk.double()[live[:, None], live[None, :]])
    return ref, (-(ref @ bk.double()) if bk is not None else None), live


def _inv_check(name, W0, b0, Winv, binv, kappas, deads=None, must_fail=False):
    K, Cn = W0.shape[:2]
    out = {}
    for k in range(K):
        ref, bref, live = inv_ref(W0[k], b0[k] if b0 is not None else None, deads[k] if deads else ())
        elim = kappas[k] * Cn * 2.0 ** -52 * float(ref.abs().max())
        if k == 0 and not must_fail:
            print("INVERSE %-8s kappa C 2^-52 max|Winv| = %.3e (u max|Winv| = %.3e)" % (name, elim, U * float(ref.abs().max())))
        Wl = W0[k].double()[live[:, None], live[None, :]]
        Il = Winv[k].double()[live[:, None], live[None, :]]
        res = [("inverse Winv", Winv[k], ref, elim / U),
               ("inverse Winv W - I", Il @ Wl, torch.eye(len(live), dtype=F64), Il.abs() @ Wl.abs() - torch.eye(len(live), dtype=F64))]
        if b0 is not None:
            res.append(("inverse binv", binv[k], bref, elim * float(b0[k].abs().sum()) / U))
        for what, a, r, s in res:
            if must_fail:
                out[what] = max(out.get(what, 0.0), share(a, r, s, U))
            else:
                check(a, r, s, U, what, "%s k=%d" % (name, k))
    return out


@pytest.mark.parametrize("case", INV_CASES, ids=[c[0] for c in INV_CASES])
def test_inverse(case):
    name, Cn, K, kappa, has_b, sliced = case
    assert (inv_lds(Cn) > 64 * 1024) == (Cn == 64), name
    if Cn == 63:
        assert inv_lds(63) == 64276 and inv_lds(64) == 66320
    g = _gen(700 + Cn + K)
    W0 = torch.stack([conditioned(Cn, kappa, g) for _ in range(K)]).float()
    for k in range(K):
        if Cn > 1:
            assert abs(float(torch.linalg.cond(W0[k].double())) / kappa - 1) < 0.01, name
    b0 = torch.randn(K, Cn, generator=g) if has_b else None
    Winv, binv = _inv_run(W0, b0, sliced)
    _inv_check(name, W0, b0, Winv, binv, [kappa] * K)


@pytest.mark.parametrize("Cn", [12, 64])
def test_inverse_zero_diagonal(Cn):
    """W = the rows of a diagonally dominant A shifted down by one, A[i - 1, i] = 0: every diagonal entry of W is exactly zero and the
    largest entry of column i sits in row i + 1: a row swap in every column but the last."""
    g = _gen(720 + Cn)
    K = 2
    A = torch.eye(Cn, dtype=F64) + 0.3 * torch.randn(K, Cn, Cn, generator=g, dtype=F64) / math.sqrt(Cn)
    idx = torch.arange(Cn)
    A[:, (idx - 1) % Cn, idx] = 0
    W0 = torch.roll(A, 1, 1).float()
    assert bool((torch.diagonal(W0, dim1=1, dim2=2) == 0).all())
    assert bool((W0.abs().argmax(1)[:, :-1] == (idx[:-1] + 1)).all())
    b0 = torch.randn(K, Cn, generator=g)
    kap = [float(torch.linalg.cond(W0[k].double())) for k in range(K)]
    assert max(kap) < 20
    Winv, binv = _inv_run(W0, b0)
    _inv_check("zdiag%d" % Cn, W0, b0, Winv, binv, kap)


def _dead_data(Cn):
    g = _gen(740 + Cn)
    deads = [(0,), (Cn - 1,), (2, 5) if Cn == 8 else (17, 40)]
    W0 = torch.zeros(3, Cn, Cn)
    kap = []
    for k, d in enumerate(deads):
        live = torch.tensor([i for i in range(Cn) if i not in d])
        blk = conditioned(len(live), 1e3, g).float()
        W0[k][live[:, None], live[None, :]] = blk
        kap.append(float(torch.linalg.cond(blk.double())))
        assert bool((W0[k][list(d)] == 0).all()) and bool((W0[k][:, list(d)] == 0).all())
    return W0, torch.randn(3, Cn, generator=g), deads, kap


@pytest.mark.parametrize("Cn", [8, 64])
def test_inverse_dead_channels(Cn):
    W0, b0, deads, kap = _dead_data(Cn)
    Winv, binv = _inv_run(W0, b0)
    _inv_check("dead%d" % Cn, W0, b0, Winv, binv, kap, deads)
    for k, d in enumerate(deads):
        assert bool((Winv[k][list(d)] == 0).all()) and bool((Winv[k][:, list(d)] == 0).all()) and bool((binv[k][list(d)] == 0).all())


def test_inverse_detects_a_dead_row_left_alive():
    """The reference of a kernel that kept one dead channel alive (a unit pivot on its diagonal)."""
    W0, b0, deads, kap = _dead_data(8)
    Winv, binv = _inv_run(W0, b0)
    alive = W0.clone()
    alive[2, 5, 5] = 1.0
    sh = _inv_check("alive", alive, b0, Winv, binv, kap, [deads[0], deads[1], (2,)], must_fail=True)
    assert sh["inverse Winv"] >= 10 and sh["inverse binv"] >= 10 and sh["inverse Winv W - I"] >= 10, sh


def test_inverse_refuses_65():
    raises_code(-1, _H().mat_inverse, torch.eye(65, device=DEV).unsqueeze(0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. tmg_lu_fold_fwd / tmg_lu_fold_bwd_split
# ---------------------------------------------------------------------------------------------------------------------------------
# (id, C, K, (a, b): g given / n null, dbm given, dld given, tail split, sgn)
FOLD_CASES = [
    ("c1k1", 1, 1, "gg", True, True, True, 1.0),
    ("c3k2", 3, 2, "nn", True, True, False, -1.0),
    ("c12k16", 12, 16, "gg", True, False, True, -1.0),
    ("c48k16", 48, 16, "gn", True, True, False, 1.0),
    ("c127k1", 127, 1, "gg", False, True, False, -1.0),
    ("c130k2", 130, 2, "gg", True, True, True, 1.0),
    ("c256k2", 256, 2, "gg", True, True, False, -1.0),
]
FOLD_IDS = ["%s-r%d" % (c[0], r) for c in FOLD_CASES for r in (0, 1)]
FOLD_PARAMS = [(c, r) for c in FOLD_CASES for r in (0, 1)]
HW = 35.0 * 33.0


def fold_plan(Cn, K):
    """tmg_lu_fold_fwd / _bwd_split: (gx, element loop runs more than once, log-det loop runs more than once)."""
    gx = min(64, (Cn * Cn + 255) // 256)
    return gx, Cn * Cn > gx * 256, K * Cn > 256


def _fold_data(Cn, K, ab, seed):
    """fp32 CPU parameters as the module initialises them (LU factors of a random orthogonal matrix, perturbed), junk in the masked
    halves of l and u, sign_s of mixed signs, a of both signs and magnitudes 1e-3 .. 2, layer k's permutation random / identity /
    reversal in turn."""
    g = _gen(seed)
    d = dict(l=[], u=[], ls=[], sg=[], perm=[], a=[], b=[])
    for k in range(K):
        A = _orth(Cn, g) + 0.05 * torch.randn(Cn, Cn, generator=g, dtype=F64)
        _, L, Uu = torch.linalg.lu(A)
        dg = torch.diagonal(Uu)
        d["l"].append((torch.tril(L, -1) + torch.triu(0.3 * torch.randn(Cn, Cn, generator=g, dtype=F64))).float())
        d["u"].append((torch.triu(Uu, 1) + torch.tril(0.3 * torch.randn(Cn, Cn, generator=g, dtype=F64))).float())
        d["ls"].append((dg.abs().log() + 0.05 * torch.randn(Cn, generator=g, dtype=F64)).float())
        sg = torch.sign(dg).float()
        if k % 2 == 1:
            sg[0] = -sg[0]
        d["sg"].append(sg)
        kind = (k + seed) % 3
        d["perm"].append(torch.randperm(Cn, generator=g) if kind == 0 else torch.arange(Cn) if kind == 1 else torch.arange(Cn - 1, -1, -1))
        sa = torch.where(torch.rand(Cn, generator=g) < 0.5, -1.0, 1.0)
        d["a"].append((sa * 10.0 ** (torch.rand(Cn, generator=g) * 3.3 - 3.0)).float() if ab[0] == "g" else None)
        d["b"].append(torch.randn(Cn, generator=g) if ab[1] == "g" else None)
    if Cn * K >= 6:
        assert bool((torch.stack(d["sg"]) > 0).any()) and bool((torch.stack(d["sg"]) < 0).any())
        if ab[0] == "g":
            a = torch.stack(d["a"])
            assert bool((a > 0).any()) and bool((a < 0).any())
    gr = dict(gW=torch.randn(K, Cn, Cn, generator=g), gb=torch.randn(K, Cn, generator=g), g=torch.randn(1, generator=g))
    return d, gr


def fold_ref(d, reverse, sgn, hw):
    """fp64 torch statement of the fold (differentiable leaves in `P`) and the |terms| of every element's inner product."""
    st = lambda k: torch.stack([t.double() for t in d[k]])  # noqa: E731
    P = {k: st(k).requires_grad_(True) for k in ("l", "u", "ls")}
    has_a, has_b = d["a"][0] is not None, d["b"][0] is not None
    if has_a:
        P["a"] = st("a").requires_grad_(True)
    if has_b:
        P["b"] = st("b").requires_grad_(True)
    sg, perm = st("sg"), torch.stack(d["perm"])
    K, Cn = sg.shape
    eye = torch.eye(Cn, dtype=F64)
    idx = perm[:, :, None].expand(K, Cn, Cn)
    e = torch.exp(P["ls"])
    lower = torch.tril(P["l"], -1) + eye
    upper = torch.triu(P["u"], 1) + torch.diag_embed(e * sg + 0.01)
    W = torch.gather(lower @ upper, 1, idx)                    # row i of W = row perm[i] of lower upper
    a = P["a"] if has_a else torch.ones(K, Cn, dtype=F64)
    b = P["b"] if has_b else torch.zeros(K, Cn, dtype=F64)
    if reverse:
        Wm, bm = W / a[:, :, None], -b / a
    else:
        Wm, bm = W * a[:, None, :], (W @ b[:, :, None])[:, :, 0]
    ld = hw * (sgn * P["ls"].sum() + a.abs().log().sum())
    with torch.no_grad():
        AL = torch.tril(P["l"].abs(), -1) + eye
        AU = torch.triu(P["u"].abs(), 1) + torch.diag_embed(e + 0.01)
        SW = torch.gather(AL @ AU, 1, idx)
        S = dict(W=SW, Wm=SW / a.abs()[:, :, None] if reverse else SW * a.abs()[:, None, :],
                 bm=(b / a).abs() if reverse else (SW @ b.abs()[:, :, None])[:, :, 0],
                 ld=hw * (P["ls"].abs().sum() + a.abs().log().abs().sum()))
        aux = dict(AL=AL, AU=AU, e=e, idx=idx, a=a.detach(), b=b.detach())
    return P, dict(W=W, Wm=Wm, bm=bm, ld=ld.view(1)), S, aux


def fold_grad_ref(P, out, S, aux, gW, gb, g, reverse, sgn, hw):
    """Autograd gradients of sum gW Wm + sum gb bm + g ld and the |terms| of each of their elements."""
    gW, gb, g = gW.double(), gb.double(), g.double()
    loss = (gW * out["Wm"]).sum() + (gb * out["bm"]).sum() + (g * out["ld"]).sum()
    names = list(P)
    grads = dict(zip(names, torch.autograd.grad(loss, [P[k] for k in names], allow_unused=True)))
    a, b, AL, AU, e, SW = aux["a"].abs(), aux["b"].abs(), aux["AL"], aux["AU"], aux["e"], S["W"]
    with torch.no_grad():
        AdW = gW.abs() / a[:, :, None] if reverse else gW.abs() * a[:, None, :] + gb.abs()[:, :, None] * b[:, None, :]
        AM = torch.zeros_like(AdW).scatter_(1, aux["idx"], AdW)                  # M[perm[i]] = dW[i]
        Sdu = AL.transpose(1, 2) @ AM
        ghw = float((g * hw).abs())
        Sg = dict(l=torch.tril(AM @ AU.transpose(1, 2), -1), u=torch.triu(Sdu, 1), ls=torch.diagonal(Sdu, dim1=1, dim2=2) * e + ghw)
        if reverse:
            Sg["a"] = (gW.abs() * SW).sum(2) / a ** 2 + (gb * aux["b"]).abs() / a ** 2 + ghw / a
            Sg["b"] = gb.abs() / a
        else:
            Sg["a"] = (gW.abs() * SW).sum(1) + ghw / a
            Sg["b"] = (SW.transpose(1, 2) @ gb.abs()[:, :, None])[:, :, 0]
    return grads, Sg


def _fold_run(case, reverse):
    name, Cn, K, ab, has_dbm, has_dld, split, sgn = case
    H = _H()
    gx, eloop, ldloop = fold_plan(Cn, K)
    want = {"c1k1": (1, False, False), "c3k2": (1, False, False), "c12k16": (1, False, False), "c48k16": (9, False, True),
            "c127k1": (64, False, False), "c130k2": (64, True, True), "c256k2": (64, True, True)}[name]
    assert (gx, eloop, ldloop) == want, (name, gx, eloop, ldloop)
    d, gr = _fold_data(Cn, K, ab, 800 + Cn + K)
    dev = {k: [t.to(DEV).contiguous() if t is not None else None for t in d[k]] for k in ("l", "u", "ls", "a", "b")}
    tab = torch.tensor([[dev[n][k].data_ptr() if dev[n][k] is not None else 0 for n in ("l", "u", "ls", "a", "b")] for k in range(K)],
                       dtype=torch.int64).to(DEV)
    sign_s = torch.stack(d["sg"]).to(DEV).contiguous()
    perm = torch.stack(d["perm"])
    iperm = torch.argsort(perm, 1)
    assert bool((torch.gather(perm, 1, iperm) == torch.arange(Cn)).all())
    perm_d, iperm_d = perm.to(torch.int32).to(DEV).contiguous(), iperm.to(torch.int32).to(DEV).contiguous()
    o = {}
    for key, shape, dt in (("W", (K, Cn, Cn), F64), ("Wm", (K, Cn, Cn), torch.float32), ("bm", (K, Cn), torch.float32), ("ld", (1,), torch.float32),
                           ("dl", (K, Cn, Cn), torch.float32), ("du", (K, Cn, Cn), torch.float32), ("dlogs", (K, Cn), torch.float32),
                           ("da", (K, Cn), torch.float32), ("db", (K, Cn), torch.float32)):
        o[key + "_buf"], o[key] = guarded(shape, dt)
    H.lu_fold_fwd(tab, sign_s, perm_d, iperm_d, o["W"], o["Wm"], o["bm"], o["ld"], reverse, sgn, HW)
    gW, gb, g = gr["gW"].to(DEV), gr["gb"].to(DEV) if has_dbm else None, gr["g"].to(DEV) if has_dld else None
    if split:
        head = lambda t: None if (t is None or K == 1) else t[:K - 1].contiguous()  # noqa: E731
        tail = lambda t: None if t is None else t[K - 1].clone()  # noqa: E731
        H.lu_fold_bwd(tab, sign_s, perm_d, iperm_d, o["W"], head(gW), head(gb), g, o["dl"], o["du"], o["dlogs"], o["da"], o["db"], reverse,
                      sgn, HW, dWm_tail=tail(gW), dbm_tail=tail(gb))
    else:
        H.lu_fold_bwd(tab, sign_s, perm_d, iperm_d, o["W"], gW, gb, g, o["dl"], o["du"], o["dlogs"], o["da"], o["db"], reverse, sgn, HW)
    torch.cuda.synchronize()
    for key in ("W", "Wm", "bm", "ld", "dl", "du", "dlogs", "da", "db"):
        assert intact(o[key + "_buf"]), (name, key)
    o = {k: v.cpu() for k, v in o.items() if not k.endswith("_buf")}
    gr = dict(gW=gr["gW"], gb=gr["gb"] if has_dbm else torch.zeros(K, Cn), g=gr["g"] if has_dld else torch.zeros(1))
    return d, gr, o, dev


def _fold_check(case, reverse, d, gr, o, must_fail=False):
    name, Cn, K, ab, has_dbm, has_dld, split, sgn = case
    P, out, S, aux = fold_ref(d, reverse, sgn, HW)
    grads, Sg = fold_grad_ref(P, out, S, aux, gr["gW"], gr["gb"], gr["g"], reverse, sgn, HW)
    c53 = (Cn + 4) * E53
    z = torch.zeros(K, Cn, dtype=F64)
    res = [("fold W (fp64)", o["W"], out["W"], (S["W"] - out["W"].detach().abs()).clamp(min=0), c53)]
    for what, key in (("fold Wm", "Wm"), ("fold bm", "bm"), ("fold ld", "ld")):
        res.append((what, o[key], out[key], c53 * S[key] / U, U))
    for what, key, pk in (("fold dl", "dl", "l"), ("fold du", "du", "u"), ("fold dlogs", "dlogs", "ls"), ("fold da", "da", "a"),
                          ("fold db", "db", "b")):
        gref = grads.get(pk)
        if gref is None:                 # a / b null, or no path to b (dbm None): the kernel writes zeros
            res.append((what, o[key], z, 0.0, U))
        else:
            res.append((what, o[key], gref, c53 * Sg[pk] / U, U))
    if must_fail:
        return {w: share(a, r.detach(), s, tol) for w, a, r, s, tol in res}
    for w, a, r, s, tol in res:
        check(a, r.detach(), s, tol, w, "%s r%d" % (name, reverse))
    assert bool((torch.triu(o["dl"]) == 0).all()) and bool((torch.tril(o["du"]) == 0).all()), name


@pytest.mark.parametrize("case,reverse", FOLD_PARAMS, ids=FOLD_IDS)
def test_fold(case, reverse):
    d, gr, o, _ = _fold_run(case, reverse)
    _fold_check(case, reverse, d, gr, o)


def test_fold_detects_a_wrong_entry_of_l():
    """One entry of l in the last row of the last layer: it reaches one row of W / Wm (and bm) and one row of du."""
    case = FOLD_CASES[3]
    for reverse in (0, 1):
        d, gr, o, _ = _fold_run(case, reverse)
        alt = {k: [t.clone() if t is not None else None for t in v] for k, v in d.items()}
        alt["l"][-1][-1, 0] += 0.5
        sh = _fold_check(case, reverse, alt, gr, o, must_fail=True)
        for w in ("fold W (fp64)", "fold Wm", "fold du", "fold da"):
            assert sh[w] >= 10, (reverse, w, sh[w])
        assert sh["fold dl"] <= 1.0            # (dlower = M upper^T does not see l)


def test_fold_refuses_257():
    H = _H()
    K, Cn = 1, 257
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    tab = torch.zeros(K, 5, dtype=torch.int64, device=DEV)
    perm = torch.arange(Cn, dtype=torch.int32, device=DEV).view(1, Cn)
    W = torch.zeros(K, Cn, Cn, dtype=F64, device=DEV)
    with pytest.raises(AssertionError):
        H.lu_fold_fwd(tab, z(K, Cn), perm, perm, W, z(K, Cn, Cn), z(K, Cn), z(1), 0, 1.0, HW)
    raises_code(-1, H.lu_fold_bwd, tab, z(K, Cn), perm, perm, W, z(K, Cn, Cn), z(K, Cn), z(1), z(K, Cn, Cn), z(K, Cn, Cn), z(K, Cn), z(K, Cn),
                z(K, Cn), 0, 1.0, HW)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. tmg_gauss_sample / _keyed: latents drawn in the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
KEY_HI = (0x80000000_80000001 | 0x1234_0000_0000_5678, 0xD1B54A32_D192ED03)      # bits 63 and 31 of both words set
KEY_LO = (12345, 678)
# (id, B, H, W, Ch, hz channel offset, extra channels after out, site, key, z1 given, float4 path, (cap, gx, threads loop))
DRAW_CASES = [
    ("v8", 3, 16, 16, 8, 0, 0, 0, KEY_HI, True, True, (256, 2, False)),
    ("v8s5", 3, 16, 16, 8, 0, 0, 5, KEY_LO, False, True, (256, 2, False)),
    ("s5", 3, 7, 9, 5, 0, 0, 5, KEY_HI, True, False, (256, 1, False)),
    ("s6", 3, 7, 9, 6, 0, 0, 0, KEY_LO, False, False, (256, 1, False)),
    ("hodd8", 3, 16, 16, 8, 1, 0, 0, KEY_HI, True, False, (256, 2, False)),
    ("ostr8", 3, 16, 16, 8, 0, 1, 0, KEY_HI, True, False, (256, 2, False)),
    ("cap256", 1, 512, 512, 8, 0, 0, 5, KEY_HI, True, True, (256, 256, True)),
    ("cap4loop", 600, 24, 24, 8, 0, 0, 0, KEY_LO, False, True, (4, 4, True)),
    ("cap4", 512, 20, 20, 10, 0, 0, 5, KEY_HI, False, False, (4, 4, False)),
]
DRAW = {c[0]: c for c in DRAW_CASES}


def _signed(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def key_table(keys):
    return torch.tensor([[_signed(k0), _signed(k1)] for k0, k1 in keys], dtype=torch.int64).to(DEV)


def draw_plan(B, ppi, Ch, hz, out, eps_out, z1):
    """gauss_sample_launch: (float4 path, cap, gx, threads loop)."""
    per = ppi * Ch
    cap = min(256, max(4, -(-2048 // B)))
    gx = max(1, min(cap, (per // 4 + 255) // 256))
    st = lambda t: _H().seg(t)[1]  # noqa: E731
    al = lambda t: t is None or t.data_ptr() % 16 == 0  # noqa: E731
    vec = Ch % 4 == 0 and st(hz) % 4 == 0 and st(out) % 4 == 0 and (out.shape[3] - Ch) % 4 == 0 and al(hz) and al(out) and al(eps_out)
    if z1 is not None:
        vec = vec and st(z1) % 4 == 0 and al(z1)
    return vec, cap, gx, (per + 3) // 4 > gx * 256


def _draw_run(case, with_eps=True, keyed=None):
    """keyed: (key rows, rows_per_key) -> tmg_gauss_sample_keyed; else one key, tmg_gauss_sample."""
    name, B, Hh, Ww, Ch, hoff, oextra, site, key, has_z1, vec, plan = case
    H = _H()
    clip = Ch % 2
    hz0, z10, _, _, lp0, lim = PW._gauss_data(B, Hh, Ww, Ch, clip, 900 + Ch + B)
    _, hz = PW.view(B, Hh, Ww, 2 * Ch, hoff, (4 - hoff) % 4, hz0)
    ob = torch.full((B, Hh, Ww, 2 * Ch + oextra), NAN, device=DEV)
    out = ob[..., :2 * Ch]
    z1 = z10.to(DEV) if has_z1 else None
    eb, eps = guarded((B, Hh, Ww, Ch)) if with_eps else (None, None)
    lp = lp0.to(DEV)
    assert draw_plan(B, Hh * Ww, Ch, hz, out, eps, z1) == (vec,) + plan, (name, draw_plan(B, Hh * Ww, Ch, hz, out, eps, z1))
    if keyed is not None:
        H.gauss_sample_keyed(hz, None, z1, out, lp, clip, lim, key_table(keyed[0]), keyed[1], site=site, eps_out=eps)
    else:
        H.gauss_sample(hz, None, z1, out, lp, clip, lim, eps_out=eps, nonce=key_table([key]).view(-1), site=site)
    torch.cuda.synchronize()
    if with_eps:
        assert intact(eb), name
    if oextra:
        assert bool(torch.isnan(ob[..., 2 * Ch:]).all()), name
    return dict(hz0=hz0, z10=z10 if has_z1 else None, lp0=lp0, lim=lim, clip=clip, out=out.cpu(), lp=lp.cpu(), eps=eps.cpu() if with_eps else None)


def ulp32(u):
    """The spacing of fp32 numbers at the fp64 value u."""
    return 2.0 ** (np.frexp(u)[1] - 24)


def draw_ref(B, ppi, Ch, keys, rpk, site, gq_shift=None):
    """fp64 latents [B, ppi Ch] and their spread over u1, u2 +- 1.5 ulp."""
    u1, u2, sn = PH.draw_uniforms(B, ppi, Ch, keys, rpk, site, gq_shift)
    ref = PH.box_muller(u1, u2, sn)
    d1, d2 = 1.5 * ulp32(u1), 1.5 * ulp32(u2)
    hi, lo = ref.copy(), ref.copy()
    for i in (-1, 0, 1):
        v1 = np.minimum(u1 + i * d1, 1.0)
        assert (v1 > 0).all()
        for j in (-1, 0, 1):
            v = PH.box_muller(v1, u2 + j * d2, sn)
            hi, lo = np.maximum(hi, v), np.minimum(lo, v)
    assert np.isfinite(hi - lo).all()
    return torch.from_numpy(ref), torch.from_numpy(hi - lo)


def _draw_check(case, t, keys, rpk, gq_shift=None, must_fail=False, eps=None):
    name, B, Hh, Ww, Ch = case[:5]
    site = case[7]
    eps = t["eps"] if eps is None else eps
    ref, spread = draw_ref(B, Hh * Ww, Ch, keys, rpk, site, gq_shift)
    if must_fail:
        return share(eps.view(B, -1), ref, spread / TOL_EPS, TOL_EPS)
    check(eps.view(B, -1), ref, spread / TOL_EPS, TOL_EPS, "draw eps", name)
    out, so, lpt, slp = PW.gauss_ref(t["hz0"], eps, None, None, 1, t["clip"], t["lim"])[:4]
    check(t["out"][..., Ch:], out, so, PW.TOL_GAUSS, "draw out", name)
    lp0 = t["lp0"].double()
    check(t["lp"], lp0 + lpt, lp0.abs() + slp, 2 * PW.TOL_GAUSS + 4 * U + math.sqrt(Hh * Ww * Ch) * U, "draw logp", name)
    if t["z10"] is not None:
        assert torch.equal(t["out"][..., :Ch], t["z10"]), name
    else:
        assert bool(torch.isnan(t["out"][..., :Ch]).all()), name


@pytest.mark.parametrize("case", DRAW_CASES, ids=[c[0] for c in DRAW_CASES])
def test_draw(case):
    name, B = case[:2]
    if name == "s5":
        assert (case[2] * case[3] * case[4]) % 4 == 3
    t = _draw_run(case)
    _draw_check(case, t, [case[8]], B)


def test_draw_scalar_equals_float4():
    """The scalar kernel forced on a float4 shape by a view draws the same numbers, bit for bit."""
    base = _draw_run(DRAW["v8"])["eps"]
    assert not bool(torch.isnan(base).any())
    for name in ("hodd8", "ostr8"):
        assert DRAW[name][1:5] == DRAW["v8"][1:5] and DRAW[name][7:9] == DRAW["v8"][7:9] and not DRAW[name][10]
        assert torch.equal(_draw_run(DRAW[name])["eps"], base), name


@pytest.mark.parametrize("name", ["v8", "s5"])
def test_draw_without_eps_out(name):
    """eps_out None: the same sample (bit for bit) and the same log-probability (to its bound: the blocks' atomics come in any order)."""
    case = DRAW[name]
    full = _draw_run(case)
    t = _draw_run(case, with_eps=False)
    assert torch.equal(t["out"][..., case[4]:], full["out"][..., case[4]:]), name
    _draw_check(case, t, [case[8]], case[1], eps=full["eps"])


@pytest.mark.parametrize("rpk", [1, 2, 6])
@pytest.mark.parametrize("vec", [True, False])
def test_draw_keyed(vec, rpk):
    B = 6
    case = ("k8", B, 4, 6, 8, 0, 0, 5, None, True, True, (256, 1, False)) if vec else ("k5", B, 7, 9, 5, 0, 0, 0, None, False, False, (256, 1, False))
    keys = [(KEY_HI[0] ^ (m * 0x9E3779B97F4A7C15 % 2 ** 64), KEY_HI[1] + m) for m in range(B // rpk)]
    t = _draw_run(case, keyed=(keys, rpk))
    _draw_check(case, t, keys, rpk)
    if rpk < B:     # the counter restarts at every key: with one key for all members, member 1 repeats member 0
        t2 = _draw_run(case, keyed=([keys[0]] * (B // rpk), rpk))
        assert torch.equal(t2["eps"][:rpk], t2["eps"][rpk:2 * rpk]) and torch.equal(t2["eps"][:rpk], t["eps"][:rpk])


def test_draw_refusals():
    H = _H()
    B, Hh, Ww, Ch = 3, 4, 4, 4
    hz = torch.zeros(B, Hh, Ww, 2 * Ch, device=DEV)
    out = torch.zeros(B, Hh, Ww, 2 * Ch, device=DEV)
    lp = torch.zeros(B, device=DEV)
    raises_code(-4, H.gauss_sample_keyed, hz, None, None, out, lp, 0, PW.TOP_LIMITS, key_table([KEY_LO]), 2)
    raises_code(-3, H.gauss_sample, hz, None, None, out, lp, 0, PW.TOP_LIMITS)


def test_draw_detects_a_counter_off_by_one():
    """The reference with the counter of ONE quad (the last of the last image) off by one."""
    for name in ("v8", "s5"):
        case = DRAW[name]
        B, Hh, Ww, Ch = case[1:5]
        t = _draw_run(case)
        nquad = (Hh * Ww * Ch + 3) // 4
        shift = np.zeros((B, nquad), dtype=np.int64)
        shift[B - 1, nquad - 1] = 1
        assert _draw_check(case, t, [case[8]], B, gq_shift=shift, must_fail=True) >= 10, name
        shift[B - 1, nquad - 1] = 0
        assert _draw_check(case, t, [case[8]], B, gq_shift=shift, must_fail=True) <= 1, name


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. tmg_adam_step
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = [1, 255, 4095, 4096, 4097, 3 * 4096 + 1]
# (id, sizes, gap, weight decay, amsgrad, step)
ADAM_CASES = [
    ("sizes-wd0-ams1-s1", ADAM_SIZES, 3, 0.0, 1, 1),
    ("sizes-wd-ams0-s1000", ADAM_SIZES, 3, 0.05, 0, 1000),
    ("sizes-wd-ams1-s1000", ADAM_SIZES, 3, 0.05, 1, 1000),
    ("sizes-wd0-ams0-s1", ADAM_SIZES, 3, 0.0, 0, 1),
    ("many-wd-ams1-s1", [1] * 4200, 1, 0.05, 1, 1),
    ("many-wd0-ams0-s1000", [1] * 4200, 1, 0.0, 0, 1000),
]
LR, B1, B2, AEPS = 1e-3, 0.9, 0.999, 1e-8
KINDS = ("p", "g", "m", "v", "vm")


def adam_chunks(sizes):
    """The chunk table of tmg_optim: every tensor in pieces of at most 4096 elements."""
    return [(t, e0, min(4096, n - e0)) for t, n in enumerate(sizes) for e0 in range(0, n, 4096)]


def _adam_run(case):
    name, sizes, gap, wd, ams, step = case
    H = _H()
    g = _gen(1000 + len(sizes) + step)
    offs, tot = [], gap
    for n in sizes:
        offs.append(tot)
        tot += n + gap
    live = torch.zeros(tot, dtype=torch.bool)
    for o, n in zip(offs, sizes):
        live[o:o + n] = True
    nl = int(live.sum())
    vals = dict(p=torch.randn(nl, generator=g), g=torch.randn(nl, generator=g), m=0.1 * torch.randn(nl, generator=g),
                v=0.01 * torch.rand(nl, generator=g) + 1e-6)
    vals["vm"] = vals["v"] * torch.where(torch.rand(nl, generator=g) < 0.5, 0.5, 2.0)
    host = {}
    for k in KINDS:
        host[k] = torch.full((tot,), NAN)
        host[k][live] = vals[k]
    dev = {k: host[k].to(DEV) for k in KINDS}
    tab = torch.tensor([[dev[k].data_ptr() + 4 * o for k in KINDS] for o in offs], dtype=torch.int64).to(DEV)
    chunks = adam_chunks(sizes)
    nchunks = len(chunks)
    assert sum(c[2] for c in chunks) == nl and max(c[2] for c in chunks) <= 4096
    if len(sizes) == 6:
        assert nchunks == 10 and chunks[-1] == (5, 3 * 4096, 1) and min(nchunks, 4096) == nchunks
    else:
        assert nchunks == 4200 and min(nchunks, 4096) == 4096          # blocks 0..103 take a second chunk
    bc1, bc2s = 1.0 - B1 ** step, (1.0 - B2 ** step) ** 0.5
    H.adam_step(tab, torch.tensor(chunks, dtype=torch.int32).to(DEV), nchunks, LR, B1, B2, AEPS, wd, bc1, bc2s, ams)
    torch.cuda.synchronize()
    got = {k: dev[k].cpu() for k in KINDS}
    for k in KINDS:
        assert bool(torch.isnan(got[k][~live]).all()), (name, k, "a gap was written")
    bits = lambda t: t.view(torch.int32)  # noqa: E731
    assert torch.equal(bits(got["g"]), bits(host["g"])), name
    if not ams:
        assert torch.equal(bits(got["vm"]), bits(host["vm"])), name
    return vals, {k: got[k][live] for k in KINDS}, (wd, ams, bc1, bc2s)


def adam_ref(vals, wd, ams, bc1, bc2s):
    """fp64 statement of the header's formula on the fp32 values of the hyper-parameters; {name: (ref, s)} with tol = u."""
    p, g, m, v, vm = (vals[k].double() for k in KINDS)
    lr, b2, eps, wd, bc1, bc2s, omb1, omb2 = (f32(x) for x in (LR, B2, AEPS, wd, bc1, bc2s, 1.0 - B1, 1.0 - B2))
    G = g.abs() + wd * p.abs()
    gi = g + wd * p
    m1 = m + (gi - m) * omb1
    s_m = omb1 * G + 2 * omb1 * (gi - m).abs()
    v1 = b2 * v + omb2 * gi * gi
    s_v = omb2 * (2 * gi.abs() * G + 2 * gi * gi) + b2 * v
    vx = torch.maximum(vm, v1) if ams else v1
    den = vx.sqrt() / bc2s + eps
    step = lr / bc1
    upd = step * m1 / den
    s_p = (step / den) * (m1.abs() + s_m) + upd.abs() * ((v1 + s_v) / (2 * vx) + 6)
    ref = {"adam m": (m1, s_m), "adam v": (v1, s_v), "adam p": (p - upd, s_p)}
    if ams:
        ref["adam vmax"] = (vx, s_v)
        assert bool((vm > v1).any()) and bool((vm < v1).any())
    return ref


@pytest.mark.parametrize("case", ADAM_CASES, ids=[c[0] for c in ADAM_CASES])
def test_adam(case):
    vals, got, hp = _adam_run(case)
    for what, (r, s) in adam_ref(vals, *hp).items():
        check(got[{"adam m": "m", "adam v": "v", "adam p": "p", "adam vmax": "vm"}[what]], r, s, U, what, case[0])


def test_adam_detects_a_wrong_last_element():
    """The last element of the last chunk (one element past three full chunks of the last tensor) with another gradient."""
    case = ADAM_CASES[2]
    vals, got, hp = _adam_run(case)
    alt = dict(vals)
    alt["g"] = vals["g"].clone()
    alt["g"][-1] += 1.0
    ref = adam_ref(alt, *hp)
    for what, key in (("adam m", "m"), ("adam v", "v"), ("adam p", "p")):
        assert share(got[key], ref[what][0], ref[what][1], U) >= 10, what
        assert share(got[key][:-1], ref[what][0][:-1], ref[what][1][:-1], U) <= 1, what


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. tmg_reverse_loss_fwd / _bwd, tmg_sum_terms
# ---------------------------------------------------------------------------------------------------------------------------------
N_FWD_LOOP = 4 * 1024 * 256 + 7
N_BWD_LOOP = 4 * 4096 * 256 + 5
# (n, B)
LOSS_CASES = [(1, 1), (3, 256), (4, 257), (5, 1000), (7, 1), (1027, 257), (N_FWD_LOOP, 256), (N_BWD_LOOP, 1000)]


def loss_plan(n):
    """(forward grid, forward loops, backward grid, backward loops, tail elements)."""
    n4 = n // 4
    gf, gb = PW.grid_for(n4, 1024), PW.grid_for(n4)
    return gf, n4 > gf * 256, gb, n4 > gb * 256, n - 4 * n4


def _loss_run(n, B):
    H = _H()
    g = _gen(1100 + n % 1000 + B)
    y0 = torch.randn(n, generator=g)
    y0[-1] = 2.0
    ld0 = 50 * torch.randn(B, generator=g)
    gv = torch.tensor([0.7])
    s1, s2 = 1.0 / n, 1.0 / (3 * n)
    y, ld = y0.to(DEV), ld0.to(DEV)
    lb, loss = guarded((1,), fill=0.0)
    H.reverse_loss_fwd(y, ld, loss, s1, s2)
    db, dy = guarded((n,))
    lb2, dld = guarded((B,))
    assert dy.data_ptr() % 16 == 0
    H.reverse_loss_bwd(y, gv.to(DEV), dy, dld, s1, s2)
    torch.cuda.synchronize()
    assert intact(lb) and intact(db) and intact(lb2), (n, B)
    return y0, ld0, gv, f32(s1), f32(s2), loss.cpu(), dy.cpu(), dld.cpu()


def _loss_check(n, B, y0, ld0, gv, s1, s2, loss, dy, dld, must_fail=False):
    yd, ldd = y0.double(), ld0.double()
    ref = s1 * (yd * yd).sum() + s2 * ldd.sum()
    sab = s1 * (yd * yd).sum() + s2 * ldd.abs().sum()
    res = [("loss value", loss, ref.view(1), (sab - ref.abs()).view(1), (1 + math.sqrt(n + B)) * U),
           ("loss dy", dy, 2 * s1 * float(gv) * yd, 0.0, 2 * U)]
    if must_fail:
        return {w: share(a, r, s, tol) for w, a, r, s, tol in res}
    for w, a, r, s, tol in res:
        check(a, r, s, tol, w, "n=%d B=%d" % (n, B))
    assert torch.equal(dld, torch.full((B,), s2 * float(gv), dtype=F64).float()), (n, B)      # one product of two fp32 numbers


@pytest.mark.parametrize("n,B", LOSS_CASES)
def test_reverse_loss(n, B):
    gf, floop, gb, bloop, tail = loss_plan(n)
    assert floop == (n >= N_FWD_LOOP) and bloop == (n >= N_BWD_LOOP), (n, gf, gb)
    assert tail == {1: 1, 3: 3, 4: 0, 5: 1, 7: 3, 1027: 3, N_FWD_LOOP: 3, N_BWD_LOOP: 1}[n]
    if n >= N_FWD_LOOP:
        assert gf == 1024 and gb == (4096 if n >= N_BWD_LOOP else 1025)
    _loss_check(n, B, *_loss_run(n, B))


def test_reverse_loss_refuses_a_misaligned_view():
    H = _H()
    y = torch.randn(64, device=DEV)
    ym = PW.misaligned(y)
    one = torch.zeros(1, device=DEV)
    raises_code(-2, H.reverse_loss_fwd, ym, one, one.clone(), 1.0, 1.0)
    raises_code(-2, H.reverse_loss_bwd, ym, one, torch.empty_like(y), one.clone(), 1.0, 1.0)
    raises_code(-2, H.reverse_loss_bwd, y, one, PW.misaligned(torch.empty_like(y)), one.clone(), 1.0, 1.0)


def test_reverse_loss_detects_a_wrong_tail_element():
    n, B = 1027, 257
    t = _loss_run(n, B)
    alt = t[0].clone()
    alt[-1] = 0.0                # element 1026: the last of the three that block 0 takes after the quads
    sh = _loss_check(n, B, alt, *t[1:], must_fail=True)
    assert sh["loss value"] >= 10 and sh["loss dy"] >= 10, sh


# (B, pattern: v = a vector of B elements, s = a one-element term)
SUM_CASES = [(1, "v"), (256, "vsvvsvvv"), (257, "ssssssss"), (70000, "vsv"), (70000, "vvvvvvvv"), (257, "s")]


@pytest.mark.parametrize("B,pattern", SUM_CASES)
def test_sum_terms(B, pattern):
    H = _H()
    assert len(pattern) in (1, 3, 8) and H.SUM_TERMS_MAX == 8
    g = _gen(1200 + B + len(pattern))
    terms = [10 * torch.randn(B if c == "v" else 1, generator=g) for c in pattern]
    ob, out = guarded((B,))
    H.sum_terms([t.to(DEV) for t in terms], out)
    torch.cuda.synchronize()
    assert intact(ob)
    ref = sum(t.double().expand(B) for t in terms)
    sab = sum(t.double().abs().expand(B) for t in terms)
    check(out.cpu(), ref, sab - ref.abs(), len(terms) * U, "sum_terms", "B=%d %s" % (B, pattern))


def test_sum_terms_refusals():
    H = _H()
    out = torch.zeros(16, device=DEV)
    v = torch.ones(16, device=DEV)
    raises_code(-2, H.sum_terms, [v] * 9, out)
    raises_code(-3, H.sum_terms, [v, torch.ones(15, device=DEV)], out)
