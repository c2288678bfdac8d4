"""Case tables, fp64 references and error measures of the Winograd kernels (tmg_wino.hip), shared by test_wino_plans_cpu.py (plan
coverage, budgets and the sensitivity of the measures; no device) and test_wino_kernels.py (the kernels).  Segment specs, descriptors,
data generators, bit_equal / gauss_share / int_terms_ok are conv_cases.py's.

References.  The VALUE an output must have is plain fp64: F.conv2d of the activated, padded input (forward, narrow; the input-gradient
operand through the transposed, flipped weight) and the tap-by-tap einsum conv_cases.wg_dense (weight gradient).  Beside it stands an
fp64 restatement of the Winograd algorithm itself (wino_fwd / wino_wg below), evaluated on absolute values for the bound
  forward / narrow   S^W = |A^T| ( sum_c (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ) |A| + |bias|
  weight gradient    S^W = |A'^T| ( sum_tiles (|B^T| |x| |B|) (.) (|G'| |dy| |G'^T|) ) |A'| + |previous contents|
per output element: the sum of the absolute values of the terms the KERNEL adds up, which is what its rounding errors scale with (it is
larger than the direct sum's: Winograd's cancellation).  The restatement with signed matrices equals the plain reference up to fp64
rounding (test_wino_plans_cpu) and carries the injected defects of the sensitivity tests.

Two measures (u = 2^-24):
  integer mode  activations, weights and dy are small integers, so every Winograd-domain value is a multiple of 1/4 (G and G' only
    halve, B^T, A^T, A'^T are signed sums) and, with 4 S^W < 2^24 everywhere (int_terms_ok at granule 0.25), every partial sum in every
    order is an exact fp32 number: the kernel - the bf16x3 one included, whose three-way split is exact and whose part products are
    products of 8-bit integers - must equal fp64 BIT FOR BIT.  Small integers leave the second and third bf16 parts zero; the cases
    bf3_parts_v / bf3_parts_u (16 / 32 input channels, activations up to 200 / weights up to 300) make V / U need more than 8 bits.
  Gaussian mode  |a_i - ref_i| <= (K + c) u S^W_i, K the contraction length (Cin_pad forward; the number of 2x2 dy tiles
    B ceil(H/2) ceil(W/2) for a weight gradient), c the other roundings on an element's path, counted from the code:
      wino_fwd_kernel / wino_fwdp_kernel (TMG_WN_POSITION)   c = 4 + 2 + 1 + (66 + 4 nchunks) + 1
          4 additions of G g G^T (two per pass), 2 of B^T d B (one per pass), 1 for the product; per 32-channel chunk a Y tile receives
          4 tile additions beside its own MFMA chain (Cin_pad in all: K); a product that enters through a column sum first passes its
          chain (32), T1 -= acc (1), the chain of nu = 3 onto T1 (32) and Y += T1 (1): 66; 1 for the bias (Y starts at it).
      wino_fwd3_kernel   c = 4 + 2 + 1 + 9 nchunks + 1 + 3: every Y tile receives 9 position sums per chunk; 3 for the dropped part
          products a1 b2, a2 b1, a2 b2 <= (2 + 2^-8) 2^-24 |a| |b|.
      wino_nn_kernel     c = 4 + 2 + 1 + 4 + 1: the accumulators run over all channels; A^T M A is two passes of two additions; bias.
      wino_wgrad_kernel + reduce   c = 2 + 2 + 1 + ceil(gx / NG) + (NG - 1) + 4 + 1: B^T x B (one addition per pass), G' dy G'^T (one
          per pass), the product, a thread's walk over its slabs, the fold of the NG groups, A'^T . A' (two per pass), dW += .
      dbias   K_b + 1 with K_b = UD max_tiles + 512 / KD + gx: a thread's pixels (UD = 128 KD / 512 per tile, KD = 8 float4 slots per
          pixel for NCO <= 2, else 16), the 512 / KD thread partials of a channel, the gx block partials; dbias += .
    Used only where K <= 2048 (conv_cases: a dropped product must stand out of K u S).  Measured shares: LAB_NOTES.md.
"""
import math

import torch
import torch.nn.functional as F

import conv_cases as CC
from conv_cases import seg

GRAN = 0.25
CU_DEFAULT = 256
KERNELS = ("wino_fwd_kernel", "wino_fwdp_kernel", "wino_fwd3_kernel", "wino_nn_kernel")

_T = lambda rows: torch.tensor(rows, dtype=torch.float64)   # noqa: E731
BT = _T([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
G = _T([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
AT = _T([[1, 1, 1, 0], [0, 1, -1, -1]])
GP = _T([[1, 0], [.5, .5], [.5, -.5], [0, 1]])                      # G'
APT = _T([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]])              # A'^T


def _two_sided(Mx, t):
    """Mx t Mx^T over the last two dimensions."""
    return torch.einsum("ai,...ij,bj->...ab", Mx, t, Mx)


def patches(xp):
    """Padded NCHW (B, C, H + 2, W + 2) -> the 4x4 input patches of the 2x2 output tiles, (B th tw, C, 4, 4), zero beyond the padding."""
    B, C, Hp, Wp = xp.shape
    th, tw = (Hp - 2 + 1) // 2, (Wp - 2 + 1) // 2
    xe = F.pad(xp, (0, 2 * tw + 2 - Wp, 0, 2 * th + 2 - Hp))
    p = xe.unfold(2, 4, 2).unfold(3, 4, 2)                      # (B, C, th, tw, 4, 4)
    return p.permute(0, 2, 3, 1, 4, 5).reshape(B * th * tw, C, 4, 4), th, tw


def activate(x, relu_in, pad_rep):
    """NHWC fp64 -> activated, padded NCHW."""
    xp = x.permute(0, 3, 1, 2)
    if relu_in:
        xp = xp.clamp(min=0)
    return F.pad(xp, (1, 1, 1, 1), mode="replicate" if pad_rep else "constant")


def wino_fwd(xp, w, bias, absolute=False, fault=None, hw=None):
    """The forward algorithm in fp64: Y = A^T [sum_c (G g G^T) (.) (B^T d B)] A + bias, NHWC (B, H, W, Cout).  absolute: every matrix
    and operand by its absolute value (S^W).  fault: ("chan", c0, c1) input channels [c0, c1) dropped from the contraction;
    ("nu3",) the column nu = 3 of V with the wrong sign (the kernels store -V there and chain it with a plus); ("tile", t) the 8x16-pixel
    tile t (index b tiles_y tiles_x + ty tiles_x + tx) keeps the bias only."""
    B, C, Hp, Wp = xp.shape
    Hh, Ww = Hp - 2, Wp - 2
    m = (lambda t: t.abs()) if absolute else (lambda t: t)
    d, th, tw = patches(m(xp))
    V = _two_sided(m(BT), d).reshape(-1, C, 16)
    U = _two_sided(m(G), m(w)).reshape(w.shape[0], C, 16)
    if fault and fault[0] == "chan":
        V = V.clone()
        V[:, fault[1]:fault[2]] = 0
    if fault and fault[0] == "nu3":
        V = V.clone().reshape(-1, C, 4, 4)
        V[..., 3] = -V[..., 3]
        V = V.reshape(-1, C, 16)
    A2 = torch.kron(m(AT), m(AT))                               # (4, 16): output (a, b) from position (i, j)
    O = w.shape[0]
    Y = torch.empty(V.shape[0], O, 4, dtype=torch.float64)
    Vp = V.permute(2, 0, 1).contiguous()                        # (16, T, C)
    for o0 in range(0, O, 256):
        Up = U[o0:o0 + 256].permute(2, 1, 0).contiguous()       # (16, C, o)
        M = torch.bmm(Vp, Up)                                   # (16, T, o)
        Y[:, o0:o0 + 256] = torch.einsum("ap,pto->toa", A2, M)
    Y = Y.reshape(B, th, tw, O, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * th, 2 * tw, O)[:, :Hh, :Ww]
    if fault and fault[0] == "tile":
        tx_n, ty_n = (Ww + 15) // 16, (Hh + 7) // 8
        t = fault[1]
        b, ty, tx = t // (tx_n * ty_n), (t // tx_n) % ty_n, t % tx_n
        Y = Y.clone()
        Y[b, 8 * ty:8 * ty + 8, 16 * tx:16 * tx + 16] = 0
    if bias is not None:
        Y = Y + m(bias)
    return Y.contiguous()


def wino_wg(xp, dy, absolute=False):
    """The weight-gradient algorithm in fp64: dW[co][ci] = A'^T [sum_tiles (B^T x B)[ci] (.) (G' dy G'^T)[co]] A', (Cout, Cin, 3, 3);
    xp activated padded NCHW, dy NHWC."""
    m = (lambda t: t.abs()) if absolute else (lambda t: t)
    d, th, tw = patches(m(xp))
    B, Hh, Ww, Co = dy.shape
    dyn = F.pad(m(dy).permute(0, 3, 1, 2), (0, 2 * tw - Ww, 0, 2 * th - Hh))
    dt = dyn.unfold(2, 2, 2).unfold(3, 2, 2).permute(0, 2, 3, 1, 4, 5).reshape(B * th * tw, Co, 2, 2)
    X = _two_sided(m(BT), d).reshape(-1, d.shape[1], 16).permute(2, 0, 1).contiguous()      # (16, T, Ci)
    D = _two_sided(m(GP), dt).reshape(-1, Co, 16).permute(2, 1, 0).contiguous()             # (16, Co, T)
    M = torch.bmm(D, X)                                                                     # (16, Co, Ci)
    A2 = torch.kron(m(APT), m(APT))                                                         # (9, 16)
    return torch.einsum("kp,poc->ock", A2, M).reshape(Co, d.shape[1], 3, 3).contiguous()


def split_bf16(t):
    """(part 0, part 1, part 2) of the kernels' three-way truncating bf16 split (tmg_split3), as fp64 of fp32 values."""
    v = t.float()
    out = []
    for _ in range(2):
        hi = (v.view(torch.int32) & -65536).view(torch.float32)
        out.append(hi.double())
        v = v - hi
    out.append((v.view(torch.int32) & -65536).view(torch.float32).double())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# forward (tmg_conv_wino_fwd / _fwd3) and narrow (tmg_conv_wino_narrow) cases
# ---------------------------------------------------------------------------------------------------------------------------------
SWITCHES = ("bias", "relu_in", "rep", "relu_out")


def fcase(name, npw, hw, ins, outs, sw="", B=1, cap=None, plan=None, gauss=True, amp=(3, 2), narrow=False, dgrad=None):
    """npw: NPW of the wide kernels (1: wino_fwdp_kernel<1> / wino_fwd3_kernel<1>, 2: wino_fwd_kernel<2> / wino_fwd3_kernel<2>), NTN of
    wino_nn_kernel for a narrow case.  B: first batch tried, cap: last (resolve_fwd).  plan: further plan fields the case is about
    ("unequal": blocks with different tile counts).  amp: integer amplitudes of (activations, weights).  dgrad = (Cw, nvalid): the
    operand is the mode-1 pack of a [Cin][Cw][3][3] weight, the output its first nvalid input channels' gradient."""
    sw = set(sw.split())
    assert sw <= set(SWITCHES) and ("relu_out" not in sw or narrow), sw
    cin, cout = sum(i[0] for i in ins), sum(o[0] for o in outs)
    assert dgrad is None or dgrad[1] == cout
    return dict(name=name, npw=npw, hw=hw, ins=ins, outs=outs, sw=sw, B=B, cap=cap or B, plan=plan or {}, amp=amp, narrow=narrow,
                dgrad=dgrad, cin=cin, cout=cout, gauss=gauss)


def cin_pad(case, arith):
    g = 32 if arith == "bf16x3" else 16
    return (case["cin"] + g - 1) // g * g


def want_kernel(case, arith):
    if case["narrow"]:
        return 3
    return 2 if arith == "bf16x3" else (1 if case["npw"] == 1 else 0)


def fwd_c(kernel, nchunks):
    """The count c of the Gaussian bound (module docstring)."""
    if kernel == 3:
        return 4 + 2 + 1 + 4 + 1
    if kernel == 2:
        return 4 + 2 + 1 + 9 * nchunks + 1 + 3
    return 4 + 2 + 1 + (66 + 4 * nchunks) + 1


SMALL_HW = ((1, 1), (1, 17), (2, 3), (3, 2), (7, 9), (9, 7), (17, 1), (9, 17))

FWD_CASES = [
    # input channel counts: Cin_pad above Cin (4, 8, 20, 104), a single 16-channel chunk (4, 8), a half-full last chunk (48: 32 + 16;
    # 104: 3 x 32 + 16 with 8 valid); bf16x3: Cin % 32 = 4, 8, 20, 16, 8
    fcase("f_cin4_cout64", 1, (9, 17), [seg(4)], [seg(64)], B=2, sw="bias", plan={"nchunks": 1}),
    fcase("f_cin8_cout128", 1, (9, 17), [seg(8)], [seg(128)], B=2, sw="rep", plan={"ntt": 8}),
    fcase("f_cin20_cout68", 1, (9, 17), [seg(20)], [seg(68)], B=2, sw="bias relu_in", plan={"ntt": 5}),
    fcase("f_cin48_cout72", 1, (9, 17), [seg(48)], [seg(72)], B=2, sw="bias rep", plan={"nchunks": 2}),
    fcase("f_cin104_cout76", 1, (9, 17), [seg(104)], [seg(76)], B=2, sw="relu_in rep", plan={"nchunks": 4}),
    # two n-tiles per wave: Npad / 16 odd (the repeated last tile is dropped), gy = 1 and 2 (a part-filled last block row)
    fcase("f2_cin4_cout132", 2, (9, 17), [seg(4)], [seg(132)], B=2, sw="bias", plan={"ntt": 9, "grid_y": 1}),
    fcase("f2_cin48_cout248", 2, (9, 17), [seg(48)], [seg(248)], B=2, sw="relu_in", plan={"ntt": 16, "grid_y": 1}),
    fcase("f2_cin104_cout256", 2, (9, 17), [seg(104)], [seg(256)], B=1, sw="bias rep", plan={"ntt": 16}),
    fcase("f2_cin20_cout264", 2, (9, 17), [seg(20)], [seg(264)], B=2, sw="bias rep relu_in", plan={"ntt": 17, "grid_y": 2}),
    fcase("f2_cin8_cout1920", 2, (8, 16), [seg(8)], [seg(1920)], B=3, sw="bias", plan={"ntt": 120, "grid_y": 8}),
    # input segments: a boundary inside a chunk at a quad that is no 16-multiple (20 | 28), three segments as channel-slice views
    fcase("f_in2_20_28", 1, (7, 9), [seg(20), seg(28)], [seg(64)], B=2, sw="bias"),
    fcase("f_in3_slices", 1, (7, 9), [seg(8), seg(12, 16, 4), seg(28, 36, 4)], [seg(64)], B=2, sw="relu_in rep"),
    fcase("f2_in3_slices", 2, (7, 9), [seg(36, 40, 4), seg(4, 8, 4), seg(64)], [seg(144)], B=2, sw="bias"),
    # output segments with boundaries inside a 16-channel tile
    fcase("f_out2", 1, (7, 9), [seg(8)], [seg(20), seg(44, 48, 4)], B=2, sw="bias rep"),
    fcase("f_out3", 1, (7, 9), [seg(8)], [seg(24), seg(20, 24, 4), seg(28)], B=2, sw="relu_in"),
    fcase("f2_out3", 2, (7, 9), [seg(20)], [seg(40), seg(68, 72, 4), seg(36, 44, 8)], B=2, sw="bias"),
    # the bf16 parts 2 and 3: V (activations up to 200) and U (weights up to 300) with more than 8 significant bits
    fcase("bf3_parts_v", 1, (7, 9), [seg(16)], [seg(64)], B=1, amp=(200, 2), sw="bias"),
    fcase("bf3_parts_u", 2, (7, 9), [seg(32)], [seg(132)], B=1, amp=(2, 300)),
]
for _i, (_h, _w) in enumerate(SMALL_HW):
    for _rep in (0, 1):
        FWD_CASES.append(fcase("f%s_hw%dx%d_%s" % ("2" if _i % 2 else "", _h, _w, "rep" if _rep else "zero"), 2 if _i % 2 else 1, (_h, _w),
                               [seg(8)], [seg(132 if _i % 2 else 64)], B=3, sw=("rep " if _rep else "") + ("bias" if _i % 3 else "relu_in")))
FWD_CASES += [
    # the persistent tile loop (one 8x16-pixel tile per image: a block's consecutive tiles lie in different images); integer mode only
    # block 0 two tiles, the others one; one chunk (odd stage totals)
    fcase("p_fwdp_two_tiles", 1, (8, 16), [seg(16)], [seg(64)], B=2, cap=400, sw="bias", gauss=False,
          plan={"max_tiles": 2, "unequal": True, "nchunks": 1}),
    # three chunks, the last half full (72 -> 80 = 32 + 32 + 16), two tiles in block 0
    fcase("p_fwdp_chunks3_half", 1, (7, 16), [seg(72)], [seg(64)], B=2, cap=400, sw="relu_in rep", gauss=False,
          plan={"max_tiles": 2, "unequal": True, "nchunks": 3}),
    # three tiles in some blocks, two in the others (partial tiles of 3 x 5 pixels keep it small)
    fcase("p_fwdp_three_tiles", 1, (3, 5), [seg(48)], [seg(68)], B=2, cap=800, sw="bias", gauss=False,
          plan={"max_tiles": 3, "unequal": True, "nchunks": 2}),
    fcase("p_fwd2_two_tiles", 2, (8, 16), [seg(16)], [seg(256)], B=2, cap=400, sw="bias", gauss=False,
          plan={"max_tiles": 2, "unequal": True, "nchunks": 1, "grid_y": 1}),
    fcase("p_fwd2_chunks3_half_gy2", 2, (7, 16), [seg(72)], [seg(260)], B=2, cap=400, sw="rep", gauss=False,
          plan={"max_tiles": 2, "unequal": True, "nchunks": 3, "grid_y": 2}),
    fcase("p_fwd2_three_tiles_gy2", 2, (5, 9), [seg(16)], [seg(264)], B=2, cap=800, sw="bias relu_in", gauss=False,
          plan={"max_tiles": 3, "unequal": True, "grid_y": 2}),
    # 33+ tiles at Cout = 1920 (gy = 8, 32 blocks per row)
    fcase("p_fwd2_cout1920", 2, (4, 6), [seg(8)], [seg(1920)], B=2, cap=100, sw="bias", gauss=False,
          plan={"max_tiles": 2, "unequal": True, "grid_y": 8}),
]
FWD_BY_NAME = {c["name"]: c for c in FWD_CASES}
assert len(FWD_BY_NAME) == len(FWD_CASES)

NARROW_CASES = [
    fcase("n1_cin64_cout4", 1, (9, 17), [seg(64)], [seg(4)], B=2, sw="bias", narrow=True, plan={"nchunks": 2}),
    fcase("n1_cin80_cout16", 1, (9, 17), [seg(80)], [seg(16)], B=2, sw="relu_in rep relu_out", narrow=True, plan={"nchunks": 3}),
    fcase("n2_cin64_cout20", 2, (9, 17), [seg(64)], [seg(20)], B=2, sw="bias relu_out", narrow=True),
    fcase("n2_cin112_cout32", 2, (9, 17), [seg(48), seg(64, 72, 4)], [seg(32)], B=2, sw="bias rep", narrow=True, plan={"last_groups": 1}),
    fcase("n3_cin64_cout36", 3, (9, 17), [seg(64)], [seg(36)], B=2, sw="relu_in", narrow=True),
    fcase("n3_cin80_cout48_out3", 3, (9, 17), [seg(80)], [seg(20), seg(8, 16, 4), seg(20, 24, 4)], B=2, sw="bias relu_in rep relu_out",
          narrow=True),
    # the mode-1 operand: K = 72 weight output channels (K % 16 = 8: Cin_pad 80), the first 36 / 12 of 40 input channels
    fcase("n3_dgrad_k72_nvalid36", 3, (9, 17), [seg(72)], [seg(36)], B=2, narrow=True, dgrad=(40, 36)),
    fcase("n1_dgrad_k72_nvalid12", 1, (7, 9), [seg(72)], [seg(12)], B=2, sw="bias", narrow=True, dgrad=(40, 12)),
    fcase("p_nn_two_tiles", 2, (8, 16), [seg(64)], [seg(24)], B=2, cap=400, sw="bias relu_out", gauss=False, narrow=True,
          plan={"max_tiles": 2, "unequal": True}),
    fcase("p_nn_three_tiles_chunks3", 3, (3, 5), [seg(80)], [seg(40)], B=2, cap=800, sw="rep relu_in", gauss=False, narrow=True,
          plan={"max_tiles": 3, "unequal": True, "nchunks": 3, "last_groups": 1}),
    # the other (NTN, tile count) pairs on 3 x 5-pixel images
    fcase("p_nn1_two_tiles", 1, (3, 5), [seg(64)], [seg(16)], B=2, cap=400, sw="bias", gauss=False, narrow=True,
          plan={"max_tiles": 2, "unequal": True}),
    fcase("p_nn1_three_tiles", 1, (3, 5), [seg(112)], [seg(4)], B=2, cap=800, sw="relu_out", gauss=False, narrow=True,
          plan={"max_tiles": 3, "unequal": True}),
    fcase("p_nn2_three_tiles", 2, (3, 5), [seg(64)], [seg(32)], B=2, cap=800, sw="bias rep", gauss=False, narrow=True,
          plan={"max_tiles": 3, "unequal": True}),
    fcase("p_nn3_two_tiles", 3, (3, 5), [seg(64)], [seg(48)], B=2, cap=400, sw="relu_in", gauss=False, narrow=True,
          plan={"max_tiles": 2, "unequal": True}),
]
for _i, (_h, _w) in enumerate(SMALL_HW):
    for _rep in (0, 1):
        NARROW_CASES.append(fcase("n%d_hw%dx%d_%s" % (1 + _i % 3, _h, _w, "rep" if _rep else "zero"), 1 + _i % 3, (_h, _w), [seg(64)],
                                  [seg((8, 28, 44)[_i % 3])], B=3, narrow=True,
                                  sw=("rep " if _rep else "") + ("bias relu_out" if _i % 2 else "relu_in")))
NARROW_BY_NAME = {c["name"]: c for c in NARROW_CASES}
assert len(NARROW_BY_NAME) == len(NARROW_CASES)


def fwd_args(case, B):
    Hh, Ww = case["hw"]
    ins = [CC.descr((B, Hh, Ww), sp, i) for i, sp in enumerate(case["ins"])]
    outs = [CC.descr((B, Hh, Ww), sp, 4 + i) for i, sp in enumerate(case["outs"])]
    kw = dict(bias="bias" in case["sw"], relu_in="relu_in" in case["sw"], pad_rep="rep" in case["sw"])
    if case["narrow"]:
        kw["relu_out"] = "relu_out" in case["sw"]
    return ins, case["cout"], outs, kw


def fwd_plan_fn(Hm, case, arith):
    return Hm.conv_wino_narrow_plan if case["narrow"] else (Hm.conv_wino_fwd3_plan if arith == "bf16x3" else Hm.conv_wino_fwd_plan)


def fwd_plan_ok(case, arith, p):
    if p["rc"] != 0 or p["kernel"] != want_kernel(case, arith) or p["NPW"] != case["npw"] or p["Cin_pad"] != cin_pad(case, arith):
        return False
    for f, v in case["plan"].items():
        if f == "unequal":
            if (p["ntiles"] % p["grid_x"] != 0) != v:
                return False
        elif f == "last_groups" and arith == "bf16x3":
            continue          # the 32-channel granule: always 2
        elif p[f] != v:
            return False
    return True


def resolve_fwd(Hm, case, arith="f32"):
    """(B, plan): the smallest batch in [case B, cap] whose queried plan is on the instance and plan fields the case names."""
    fn, p = fwd_plan_fn(Hm, case, arith), None
    for B in range(case["B"], case["cap"] + 1):
        ins, cout, outs, kw = fwd_args(case, B)
        p = fn(ins, cout, outs, **kw)
        if fwd_plan_ok(case, arith, p):
            return B, p
    raise AssertionError("%s (%s): no batch in [%d, %d] reaches kernel %d NPW %d %s (last plan %s)" % (
        case["name"], arith, case["B"], case["cap"], want_kernel(case, arith), case["npw"], case["plan"], p))


def fwd_data(case, B, mode, seed=0):
    g = torch.Generator().manual_seed(6000 + seed)
    Hh, Ww = case["hw"]
    ax, aw = case["amp"]
    d = dict(x=CC.rnd(g, (B, Hh, Ww, case["cin"]), mode, ax), bias=None)
    if case["dgrad"]:
        cw, nv = case["dgrad"]
        d["w"] = CC.rnd(g, (case["cin"], cw, 3, 3), mode, aw)                  # [K = Cout of the conv][its Cin]
        d["w_eff"] = d["w"][:, :nv].flip(2, 3).permute(1, 0, 2, 3).contiguous()
    else:
        d["w"] = CC.rnd(g, (case["cout"], case["cin"], 3, 3), mode, aw)
        d["w_eff"] = d["w"]
    if "bias" in case["sw"]:
        d["bias"] = CC.rnd(g, (case["cout"],), mode, 8)
    return d


def fwd_ref(case, d, fault=None, winograd=False):
    """(ref, S^W) NHWC fp64.  ref is the plain F.conv2d unless a fault is injected or `winograd` asks for the restatement."""
    sw = case["sw"]
    xp = activate(d["x"], "relu_in" in sw, "rep" in sw)
    if fault is None and not winograd:
        y = F.conv2d(xp, d["w_eff"], d["bias"]).permute(0, 2, 3, 1)
    else:
        y = wino_fwd(xp, d["w_eff"], d["bias"], fault=fault)
    S = wino_fwd(xp, d["w_eff"], d["bias"], absolute=True)
    if "relu_out" in sw:
        y = y.clamp(min=0)
    return y.contiguous(), S


# ---------------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases (tmg_conv_wino_wgrad) and grouped ones (tmg_conv_wino_wgrad_grouped)
# ---------------------------------------------------------------------------------------------------------------------------------
def wcase(name, want, shape, cin, cout, ins=None, dy=None, plan=None, sw="dbias", layout=None, gauss=True, cap=None):
    """want = (CIT, NCO, DB); shape = (B, H, W) with B the first batch tried and cap the last (resolve_wg); layout = (cin_dst, cin_valid,
    ci_split, ci_off0, ci_off1); sw of: dbias relu_in rep.  dW and dbias always start from known non-zero values."""
    sw = set(sw.split())
    assert sw <= {"dbias", "relu_in", "rep"}
    ins = ins or [seg(cin)]
    assert sum(i[0] for i in ins) == cin
    return dict(name=name, want=tuple(want), shape=shape, cin=cin, cout=cout, k=3, s=1, ins=ins, dy=dy or seg(cout), plan=plan or {}, sw=sw,
                layout=layout or (0, 0, 0, 0, 0), gauss=gauss, cap=cap or shape[0])


W3 = (2, 9, 17)          # 8 tiles of 8x16 pixels (partial ones), 90 dy tiles
WG_CASES = [
    # every (CIT, NCO); DB = 0 only on (4, 4)
    wcase("w_cit2_nco2", (2, 2, 1), W3, 32, 32),
    wcase("w_cit2_nco3", (2, 3, 1), W3, 20, 36, sw="dbias rep"),
    wcase("w_cit2_nco4", (2, 4, 1), W3, 32, 64, sw="relu_in"),
    wcase("w_cit3_nco2", (3, 2, 1), W3, 36, 20, sw="dbias relu_in"),
    wcase("w_cit3_nco3", (3, 3, 1), W3, 48, 48, sw=""),
    wcase("w_cit3_nco4_gz2", (3, 4, 1), W3, 68, 52, plan={"gz": 2}, sw="dbias rep"),
    wcase("w_cit4_nco2", (4, 2, 1), W3, 64, 32),
    wcase("w_cit4_nco3_gy2", (4, 3, 1), W3, 52, 80, plan={"gy": 2, "gz": 1}, sw="dbias relu_in rep"),
    wcase("w_cit4_nco4_single_buffer", (4, 4, 0), W3, 64, 64),
    wcase("w_cit4_nco4_gz2_gy4", (4, 4, 0), (1, 9, 17), 104, 256, plan={"gz": 2, "gy": 4}, sw="dbias rep"),
    # gx: one block for 1 - 3 tiles; an odd share (7 tiles on 3 blocks: 3, 2, 2)
    wcase("w_gx1_one_tile", (2, 2, 1), (1, 5, 9), 32, 32, plan={"gx": 1, "ntiles": 1}),
    wcase("w_gx1_three_tiles", (4, 4, 0), (3, 1, 1), 64, 64, plan={"gx": 1, "ntiles": 3}, sw="dbias rep"),
    wcase("w_gx3_seven_tiles", (2, 2, 1), (7, 8, 16), 32, 32, plan={"gx": 3, "ntiles": 7}, sw="dbias relu_in"),
    # the reduce widths: NG = 8 from 32 slabs, 16 from 64 (batch from the planner)
    wcase("w_ng8", (2, 2, 1), (64, 8, 16), 32, 32, plan={"NG": 8}, cap=80),
    wcase("w_ng8_cit4_nco4", (4, 4, 0), (64, 7, 9), 64, 64, plan={"NG": 8}, cap=80, sw="dbias rep"),
    wcase("w_ng16", (2, 2, 1), (128, 8, 16), 32, 32, plan={"NG": 16}, cap=160, gauss=False),
    wcase("w_ng16_cit3_nco3", (3, 3, 1), (128, 3, 5), 36, 44, plan={"NG": 16}, cap=160, sw="dbias relu_in rep"),
    # operands: three input segments (slices), a dy slice (stride > Cout, offset 4)
    wcase("w_in3_slices", (3, 2, 1), W3, 48, 32, ins=[seg(8), seg(12, 16, 4), seg(28, 36, 4)], sw="dbias relu_in"),
    wcase("w_dy_slice_off4", (2, 3, 1), W3, 32, 44, dy=seg(44, 52, 4), sw="dbias rep"),
    # destination layouts: 32 source channels into rows of 40 at offset 5; 28 valid of 32 split 12 | 16 at offsets 1 and 9; 24 valid
    wcase("w_cin_dst_off0", (2, 2, 1), W3, 32, 32, layout=(40, 32, 0, 5, 0)),
    wcase("w_ci_split_off1", (2, 2, 1), W3, 32, 32, layout=(40, 28, 12, 1, 9), sw=""),
    wcase("w_cin_valid", (2, 2, 1), W3, 32, 32, layout=(32, 24, 0, 0, 0), sw="dbias rep"),
    # small images
    wcase("w_hw1x1", (2, 2, 1), (5, 1, 1), 32, 32, sw="dbias rep"),
    wcase("w_hw2x3_zero", (2, 2, 1), (4, 2, 3), 32, 32),
    wcase("w_hw17x1", (2, 2, 1), (2, 17, 1), 32, 32, sw="dbias relu_in rep"),
    wcase("w_hw7x9", (2, 2, 1), (3, 7, 9), 32, 32, sw="dbias rep"),
]
WG_BY_NAME = {c["name"]: c for c in WG_CASES}
assert len(WG_BY_NAME) == len(WG_CASES)
WG_INSTANCES = tuple((c, n, 0 if (c, n) == (4, 4) else 1) for c in (2, 3, 4) for n in (2, 3, 4))


def wg_dy_tiles(shape):
    B, Hh, Ww = shape
    return B * ((Hh + 1) // 2) * ((Ww + 1) // 2)


def wg_args(case, B):
    _, Hh, Ww = case["shape"]
    cd, cv, cs, o0, o1 = case["layout"]
    ins = [CC.descr((B, Hh, Ww), sp, i) for i, sp in enumerate(case["ins"])]
    kw = dict(dbias="dbias" in case["sw"], relu_in="relu_in" in case["sw"], pad_rep="rep" in case["sw"], cin_dst=cd, cin_valid=cv,
              ci_split=cs, ci_off0=o0, ci_off1=o1)
    return ins, CC.descr((B, Hh, Ww), case["dy"], 4), kw


def wg_plan_ok(case, p):
    return p["rc"] == 0 and (p["CIT"], p["NCO"], p["DB"]) == case["want"] and all(p[f] == v for f, v in case["plan"].items())


def resolve_wg(Hm, case, ngroups=1):
    p = None
    for B in range(case["shape"][0], case["cap"] + 1):
        ins, dy, kw = wg_args(case, B)
        p = Hm.conv_wino_wgrad_plan(ins, dy, ngroups=ngroups, **kw)
        if wg_plan_ok(case, p):
            return B, p
    raise AssertionError("%s: no batch in [%d, %d] reaches %s %s (last plan %s)" % (case["name"], case["shape"][0], case["cap"], case["want"],
                                                                                 case["plan"], p))


def wg_c(p):
    return 2 + 2 + 1 + (p["gx"] + p["NG"] - 1) // p["NG"] + (p["NG"] - 1) + 4 + 1


def wg_kb(p):
    """The chain length of a dbias element (module docstring)."""
    kd = 8 if p["NCO"] <= 2 else 16
    return (128 * kd // 512) * ((p["ntiles"] + p["gx"] - 1) // p["gx"]) + 512 // kd + p["gx"]


def wg_data(case, B, mode, seed=0, cout=None):
    g = torch.Generator().manual_seed(7000 + seed)
    _, Hh, Ww = case["shape"]
    cin, cout = case["cin"], cout or case["cout"]
    a = 2 if B * Hh * Ww > 8192 else 3
    cd = case["layout"][0] or cin
    return dict(x=CC.rnd(g, (B, Hh, Ww, cin), mode, a), dy=CC.rnd(g, (B, Hh, Ww, cout), mode, a), prevW=CC.rnd(g, (cout, cd, 9), mode, 8),
                prevb=CC.rnd(g, (cout,), mode, 8))


def wg_ref(case, d, off1_fault=False, winograd=False):
    """(dW, S^W, dbias, S_dbias, touched columns) fp64, dW as [Cout][cin_dst][9] on top of the previous contents."""
    xp = activate(d["x"], "relu_in" in case["sw"], "rep" in case["sw"])
    dense = wino_wg(xp, d["dy"]) if winograd else CC.wg_dense(xp, d["dy"], 3, 1)
    dabs = wino_wg(xp, d["dy"], absolute=True)
    c = dict(case, cout=d["dy"].shape[3])
    dW, touched = CC.wg_scatter(c, dense, d["prevW"], 1.0, off1_fault)
    SW, _ = CC.wg_scatter(c, dabs, d["prevW"].abs(), 1.0)
    db = d["dy"].sum((0, 1, 2)) + d["prevb"]
    Sb = d["dy"].abs().sum((0, 1, 2)) + d["prevb"].abs()
    return dW, SW, db, Sb, touched


# grouped: (name, G, Cin, Cg, want, (B, H, W), sw); group g's input: even g a channel-slice view of a wider tensor, odd g a tensor of
# its own (different pixel strides in one launch); dy: one tensor of G Cg (+ 8) channels, a slice at offset 4 when `dy_slice`
def gcase(name, G_, cin, cg, want, shape, sw="dbias", dy_slice=False, layout=None, plan=None):
    c = wcase(name, want, shape, cin, cg, sw=sw, layout=layout, plan=plan)
    c.update(G=G_, dy_slice=dy_slice)
    return c


GROUPED_CASES = [
    gcase("g2_cin20_cg32", 2, 20, 32, (2, 2, 1), W3, plan={"bpg": 1, "gy": 2}),
    gcase("g3_cin36_cg64", 3, 36, 64, (3, 4, 1), W3, sw="dbias relu_in", dy_slice=True, plan={"bpg": 1, "gy": 3}),
    gcase("g2_cin68_cg64", 2, 68, 64, (3, 4, 1), W3, sw="rep", plan={"gz": 2}),
    gcase("g3_cin20_cg32_layout", 3, 20, 32, (2, 2, 1), (3, 7, 9), sw="dbias rep", layout=(28, 16, 8, 2, 10), dy_slice=True),
    gcase("g2_cin36_cg32_ng8", 2, 36, 32, (3, 2, 1), (64, 3, 5), sw="dbias", plan={"NG": 8}),
]
GROUPED_CASES.append(gcase("g2_cin20_cg80_bpg2", 2, 20, 80, (2, 3, 1), W3, sw="dbias rep", plan={"bpg": 2, "gy": 4}))   # two block rows per group
GROUPED_BY_NAME = {c["name"]: c for c in GROUPED_CASES}


def grouped_data(case, mode, seed=0):
    B = case["shape"][0]
    return [wg_data(case, B, mode, seed=100 * (g + 1) + seed) for g in range(case["G"])]


def grouped_ref(case, ds, goff_fault=None):
    """Per group (dW, S^W, dbias, S_dbias, touched); goff_fault = g: group g reads group 0's dy channels (its dy_goff term dropped)."""
    out = []
    for g, d in enumerate(ds):
        if goff_fault is not None and g == goff_fault:
            d = dict(d, dy=ds[0]["dy"])
        out.append(wg_ref(case, d))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# pack references (the layouts documented above tmg_conv_wino_pack / tmg_conv_wino_pack3)
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_operand(w, mode, nvalid=0):
    """(g[N][K][3][3], K, N): the weight the operand is built from - mode 0: w itself; mode 1: transposed, taps flipped, the first
    nvalid (0: all) input channels."""
    cout, cin = w.shape[0], w.shape[1]
    if mode == 0:
        return w, cin, cout
    n = nvalid if 0 < nvalid < cin else cin
    return w[:, :n].flip(2, 3).permute(1, 0, 2, 3).contiguous(), cout, n


def pack_ref(w, mode, nvalid=0, absolute=False):
    """U[16 pos][Kpad / 16][Npad][16] = (G g G^T)[n][k] at [pos][k / 16][n][k % 16]; padding zero.  absolute: |G| |g| |G^T|."""
    g, K, N = pack_operand(w, mode, nvalid)
    Kp, Np = (K + 15) // 16 * 16, (N + 15) // 16 * 16
    U = torch.zeros(Np, Kp, 16, dtype=torch.float64)
    U[:N, :K] = (_two_sided(G.abs(), g.abs()) if absolute else _two_sided(G, g)).reshape(N, K, 16)
    return U.reshape(Np, Kp // 16, 16, 16).permute(3, 1, 0, 2).contiguous().reshape(-1)


def pack3_unpack(U3, K, N):
    """The bf16x3 operand [16][Kpad32 / 32][Npad / 16][3][64 lanes][8] (int16 bit patterns; lane = 16 ((k % 32) / 8) + n % 16, element
    k % 8) -> three fp32 parts in pack_ref's order with Kpad32: [3][16][Kpad32 / 16][Npad][16]."""
    nch, ntt = (K + 31) // 32, (N + 15) // 16
    t = (U3.to(torch.int32) << 16).view(torch.float32).reshape(16, nch, ntt, 3, 4, 16, 8)      # pos, ch, nt, part, q, li, j
    t = t.permute(3, 0, 1, 4, 6, 2, 5).reshape(3, 16, nch * 32, ntt * 16)                     # part, pos, k, n
    return t.reshape(3, 16, nch * 2, 16, ntt * 16).permute(0, 1, 2, 4, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# declined calls: every envelope condition of wino_fwd_setup and wino_wgrad_impl, with the code it must return BEFORE any launch.
# A segment is conv_cases.seg(n, width, off, mis): mis = 1 puts the base address 4 bytes off 16-byte alignment.
# forward: (name, entry, ins, outs, Cin in dims (None: the sum), Cout in dims, bias misalignment in floats (None: no bias), code)
# ---------------------------------------------------------------------------------------------------------------------------------
DECLINED_FWD = [
    ("wide_cout32", "fwd", [seg(8)], [seg(32)], None, None, None, -100),
    ("wide3_cout60", "fwd3", [seg(8)], [seg(60)], None, None, None, -100),
    ("narrow_cout52", "narrow", [seg(64)], [seg(52)], None, None, None, -100),
    ("narrow_cin60", "narrow", [seg(60)], [seg(16)], None, None, None, -100),
    ("cin6", "fwd", [seg(6)], [seg(64)], None, None, None, -100),
    ("cin6_two_segments_sum8", "fwd", [seg(6), seg(2)], [seg(64)], None, None, None, -100),
    ("cout66", "fwd", [seg(8)], [seg(66)], None, None, None, -100),
    ("in_stride10", "fwd", [seg(8, 10)], [seg(64)], None, None, None, -100),
    ("in_offset2", "fwd3", [seg(8, 12, 2)], [seg(64)], None, None, None, -100),
    ("in_misaligned", "narrow", [seg(64, 64, 0, 1)], [seg(16)], None, None, None, -100),
    ("out_stride66", "fwd", [seg(8)], [seg(64, 66)], None, None, None, -100),
    ("out_misaligned", "fwd", [seg(8)], [seg(64, 64, 0, 1)], None, None, None, -100),
    ("bias_misaligned", "fwd", [seg(8)], [seg(64)], None, None, 1, -100),
    ("bias_misaligned_narrow", "narrow", [seg(64)], [seg(16)], None, None, 2, -100),
    ("no_input_segment", "fwd", [], [seg(64)], 8, None, None, -3),
    ("four_input_segments", "fwd", [seg(4), seg(4), seg(4), seg(4)], [seg(64)], None, None, None, -3),
    ("no_output_segment", "narrow", [seg(64)], [], None, 16, None, -3),
    ("four_output_segments", "fwd3", [seg(8)], [seg(16), seg(16), seg(16), seg(16)], None, None, None, -3),
    ("cin_sum_disagrees", "fwd", [seg(8)], [seg(64)], 12, None, None, -3),
    ("cout_sum_disagrees", "fwd", [seg(8)], [seg(64)], None, 68, None, -3),
    # the order of the tests: the channel sums (-3) come before the envelope (-100)
    ("cout_sum_disagrees_outside_envelope", "fwd", [seg(8)], [seg(32)], None, 36, None, -3),
    ("cin_sum_disagrees_misaligned", "narrow", [seg(64, 64, 0, 1)], [seg(16)], 68, None, None, -3),
]
# weight gradient: (name, ins, dy, Cin in dims (None: the sum), workspace ("ok", "null", "short", "misaligned"), ngroups (0: ungrouped
# entry; "nogtab": grouped entry without a table), code)
DECLINED_WG = [
    ("cit1", [seg(16)], seg(32), None, "ok", 0, -100),
    ("cot1", [seg(32)], seg(16), None, "ok", 0, -100),
    ("cin30", [seg(30)], seg(32), None, "ok", 0, -100),
    ("cout34", [seg(32)], seg(34, 36), None, "ok", 0, -100),
    ("in_misaligned", [seg(32, 32, 0, 1)], seg(32), None, "ok", 0, -100),
    ("dy_stride34", [seg(32)], seg(32, 34), None, "ok", 0, -100),
    ("dy_misaligned", [seg(32)], seg(32, 32, 0, 1), None, "ok", 0, -100),
    ("ws_null", [seg(32)], seg(32), None, "null", 0, -100),
    ("ws_short", [seg(32)], seg(32), None, "short", 0, -100),
    ("ws_misaligned", [seg(32)], seg(32), None, "misaligned", 0, -100),
    ("no_input_segment", [], seg(32), 32, "ok", 0, -3),
    ("four_input_segments", [seg(8), seg(8), seg(8), seg(8)], seg(32), None, "ok", 0, -3),
    ("cin_sum_disagrees", [seg(32)], seg(32), 36, "ok", 0, -3),
    ("cin_sum_disagrees_dy_misaligned", [seg(32)], seg(32, 32, 0, 1), 36, "ok", 0, -3),
    ("grouped_without_table", [seg(32)], seg(32), None, "ok", "nogtab", -3),
]
DECL_SHAPE = (2, 5, 6)


def _tab(ctypes, addrs_strides_n):
    n = len(addrs_strides_n)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[a for a, _, _ in addrs_strides_n])
    desc = (ctypes.c_int64 * (3 * max(n, 1)))(*[v for _, s, c in addrs_strides_n for v in (s, 0, c)])
    return ptrs, desc, ctypes.c_int64(n)


def raw_fwd(Hm, entry, ins, outs, U, bias, cin, cout, plan=False, stream=None):
    """tmg_conv_wino_<entry>[_plan] on hand-built tables; ins / outs: [(address, pixel stride, channels)].  Returns (code, plan buffer)."""
    import ctypes
    B, Hh, Ww = DECL_SHAPE
    ip, idesc, n_in = _tab(ctypes, ins)
    op, odesc, n_out = _tab(ctypes, outs)
    dims = (ctypes.c_int64 * 8)(B, Hh, Ww, cin, cout, 0, 0, 0)
    args = [ip, idesc, n_in, ctypes.c_void_p(U), ctypes.c_void_p(bias), op, odesc, n_out, dims, stream]
    buf = (ctypes.c_int64 * len(Hm.WINO_FWD_PLAN_FIELDS))()
    if plan:
        return getattr(Hm.lib(), "tmg_conv_wino_%s_plan" % entry)(*(args + [buf])), list(buf)
    fn = getattr(Hm.lib(), "tmg_conv_wino_%s" % entry)
    return fn(*args), None


def raw_wg(Hm, ins, dy, dW, dbias, ws, ws_floats, cin, cout, ngroups=0, gtab=0, plan=False, stream=None):
    """tmg_conv_wino_wgrad / _grouped / _plan on hand-built tables; dy = (address, pixel stride, channels)."""
    import ctypes
    c_vp, c_i64 = ctypes.c_void_p, ctypes.c_int64
    B, Hh, Ww = DECL_SHAPE
    ip, idesc, n_in = _tab(ctypes, ins)
    dims = (c_i64 * 12)(B, Hh, Ww, cin, cout, 0, 0, 0, 0, 0, 0, 0)
    dyd = (c_i64 * 2)(dy[1], 0)
    tail = [c_vp(dy[0]), dyd, c_vp(dW), c_vp(dbias), c_vp(ws), c_i64(ws_floats), dims, stream]
    if plan:
        buf = (c_i64 * len(Hm.WINO_WGRAD_PLAN_FIELDS))()
        return Hm.lib().tmg_conv_wino_wgrad_plan(*([ip, idesc, n_in] + tail + [c_i64(max(int(ngroups or 1), 1)), buf])), list(buf)
    if ngroups:
        gd = (c_i64 * 3)(cout, cout * cin * 9, cout)
        return Hm.lib().tmg_conv_wino_wgrad_grouped(*([ip, idesc, n_in, c_vp(gtab), c_i64(2), gd] + tail)), None
    return Hm.lib().tmg_conv_wino_wgrad(*([ip, idesc, n_in] + tail)), None


def spec_addr(spec, slot):
    """(made-up address, pixel stride, channels) of a segment spec, for the plan queries."""
    n, width, off, mis = spec
    return (CC.BASE * (slot + 1) + 4 * (off + mis), width, n)
