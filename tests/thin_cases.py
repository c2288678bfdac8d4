"""Case tables, fp64 references and error measures of the growth-layer forwards (c1x2_fwd_kernel<CG>, c1_fwd_kernel: tmg_pointwise.hip),
the thin and mix weight gradients and the layer planes (tmg_thin.hip) and the AFF = 0 channel mixes (mix32_kernel<NT, NP, 0>,
mix16_kernel<NT, NP>: tmg_mix16.hip), shared by test_thin_plans_cpu.py (plan coverage, budgets, sensitivity of the measures; no device)
and test_thin_kernels.py (the kernels).  Segment specs (n, width, off, mis), descriptors, data generators and bit_equal / int_terms_ok
are conv_cases.py's.

A case has a name and builds its operands from a seed in either mode (`*_data`); its plan is what the library's own query answers for
its descriptors (`*_plan`; the mixes and the layer planes have no query: mix_plan restates grid = clamp(ceil(npix / (64 NP)), 1, 2048)
with the instance chosen by (C + 15) / 16).  The references are plain fp64 torch formulas (F.conv2d, einsum, matmul) that run wherever
their operands live: on the CPU, or - for the cases marked big (more than BIG_ELEMS operand elements) - on the device.

Two measures (u = 2^-24):
  integer mode  every operand is a small integer (exact in fp16 for mix_f16) and S, the same operation on absolute values, stays below
    2^24 (for c1x2 the second convolution runs over the BOUND of d1): every partial sum of every order - CG split, wave split, atomic
    order - is an exact fp32 integer and the kernel must equal fp64 bit for bit.
  Gaussian mode  elementwise |a - ref| <= bound, applied where K <= KMAX_GAUSS (a dropped product must stand out of K u S):
    c1_fwd      (K + 4) u S,  K = 9 Cpad (the padded channel count: the products one thread accumulates, zero ones included), 4 = the
                rounding of a product that is not fused, the `add` operand, the store's none + two for the factor (1 - K u)^-1 and slack.
    c1x2  d1    (K + 6) u S1: as c1_fwd plus the two xor-shuffle additions of the CG lanes.
          d2    (K + 16) u S2 + (K + 6) u (|w2_d1| * S1),  S2 = |w2| * |x| + |w2_d1| * S1 + |add2|: its own chain (K products, the two
                shuffles, nine d1 taps, add2, one product rounding, slack 2) plus the error d1 arrives with (ReLU is 1-Lipschitz).
    thin        (K + 4) u S,  K = B H W (the pixels an element sums over, in any order: waves, blocks, atomics), 4 = product, previous
                contents, slack 2.
    mix wgrad   (K + 4) u S,  K = npix, for dW and db alike.
    mix_f32     (K + 3) u S,  K = 16 NT (the accumulator's chain, bias included as its start value), 3 = product + slack 2.
    mix_f16     the same against the reference whose operands are rounded to fp16 first; and the result must differ from the fp32
                product by fp16's rounding and not by more: |a - y32| <= (2 * 2^-11 + 2^-22) S + (K + 3) u S.
  K and c were fixed from the kernels' code before the first device run.
The layer planes are a permutation: exact equality in both modes.
"""
import math

import torch
import torch.nn.functional as F

import conv_cases as CC
from conv_cases import seg, descr, rnd, U24, KMAX_GAUSS, bit_equal, int_terms_ok   # noqa: F401

BIG_ELEMS = 1 << 22          # operand elements above which a case's reference runs on the device
BYTES_CAP = 320 << 20        # operand bytes of one case
REF_FLOP_CAP = 2.5e10        # fp64 multiply-adds of one case's reference
NAN = float("nan")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def share(a, ref, bound):
    """max_i |a_i - ref_i| / bound_i: <= 1 passes.  Elements with bound 0 must be exact; NaN is infinite."""
    a = a.detach().double().to(ref.device)
    assert a.shape == ref.shape == bound.shape, (a.shape, ref.shape, bound.shape)
    dlt = (a - ref).abs()
    if bool(torch.isnan(dlt).any()):
        return math.inf
    r = torch.where(bound > 0, dlt / bound.clamp(min=1e-300), torch.where(dlt > 0, torch.full_like(dlt, math.inf), torch.zeros_like(dlt)))
    return float(r.max()) if r.numel() else 0.0


def exact(a, ref):
    """fp32 result == fp64 reference exactly (NaN never equal), on whichever device the reference lives."""
    a = a.detach().double().to(ref.device)
    return a.shape == ref.shape and bool((a == ref).all())


# =================================================================================================================================
# c1x2: d1 = conv3x3_zero(act(x); W1) + add1,  d2 = conv3x3_zero(act(x); W2) + conv3x3_zero(relu(d1); w2[w2_d1]) + add2
# =================================================================================================================================
CC_ROWS = 4      # conditioning channels between the t0 rows and the d1 row of the production weights (w2_d1_row = ch + Cc)


def c1x2_case(name, cg, B, hw, ins, sw="add1 add2 relu_in", plan=None, gauss=True):
    """ins: segment specs of the inputs; sw of: add1 add2 relu_in split (rows of channels >= the first segment's read w_gap = Cc further
    down) rows (w_rows = the first segment only: the other segments carry zero weight).  Weight rows: production form."""
    sw = set(sw.split())
    assert sw <= {"add1", "add2", "relu_in", "split", "rows"}, sw
    cin = sum(i[0] for i in ins)
    return dict(name=name, CG=cg, B=B, hw=hw, ins=ins, sw=sw, plan=plan or {}, cin=cin, K=9 * ((cin + 3) & ~3), gauss=gauss, fam="c1x2")


def _x1(ch):
    return seg(ch, 2 * ch, 0)       # x1: the first half of a [.., 2 ch] tensor


SMALL = (5, 7)
C1X2_CASES = [
    # CG = 1 above one channel quad: 1024 tiles of 256 pixels and more (the benchmarked batch sizes' plan)
    c1x2_case("x_cg1_cq2_b1024", 1, 1024, SMALL, [_x1(8)], plan={"t256": 1024, "nchunks": 1}),
    c1x2_case("x_cg1_chunks2_cin36", 1, 1024, SMALL, [_x1(32), seg(4)], sw="add1 add2 relu_in split", plan={"nchunks": 2, "KCH": 32}),
    c1x2_case("x_cg1_chunks2_cin64", 1, 1024, SMALL, [_x1(64)], plan={"nchunks": 2}),
    # few large images: TW = 32, TH = 8, 64 tiles per image, tile runs inside one image (16 images: 4 give 256 tiles and CG = 2)
    c1x2_case("x_cg1_large_images", 1, 16, (128, 128), [_x1(8)], plan={"TW_log2": 5, "TH": 8, "grid": 1024}),
    c1x2_case("x_cg2_large_images", 2, 4, (128, 128), [_x1(8)], sw="add2 relu_in", plan={"TW_log2": 5, "TH": 4, "grid": 512}),
    # uneven XCD remap (1027 % 8 = 3) with the ring outside the 5 x 7 image on two sides
    c1x2_case("x_cg1_cq2_xcd_uneven", 1, 1027, SMALL, [_x1(8)], sw="add1 relu_in", plan={"grid": 1027}),
    # CG = 2 at four quads and more: 512 <= t256 < 1024
    c1x2_case("x_cg2_cq4_b512", 2, 512, SMALL, [_x1(16)], plan={"t256": 512}),
    c1x2_case("x_cg2_chunks2_cin36", 2, 515, SMALL, [_x1(32), seg(4)], sw="add1 add2", plan={"nchunks": 2, "grid": 515}),
    # CG = 2 at two and three quads
    c1x2_case("x_cg2_cin8", 2, 3, (9, 12), [_x1(8)], plan={"TW_log2": 4, "TH": 8}),
    c1x2_case("x_cg2_cin12_seg3", 2, 2, (9, 12), [_x1(4), seg(4, 8, 4), seg(4)], sw="add1 relu_in rows"),
    # CG = 4 at TW_log2 3 and 4 (W = 33: the launcher reduces 5 to 4), two chunks, two segments
    c1x2_case("x_cg4_twl3", 4, 3, (9, 8), [_x1(16)], plan={"TW_log2": 3, "TH": 8}),
    c1x2_case("x_cg4_twl4_w33", 4, 2, (6, 33), [_x1(16)], sw="add2 relu_in", plan={"TW_log2": 4, "TH": 4, "tiles_x": 3}),
    c1x2_case("x_cg4_xcd_even", 4, 8, (6, 33), [_x1(16)], sw="add1 add2", plan={"grid": 48}),
    c1x2_case("x_cg4_cin36_seg2", 4, 2, (9, 12), [_x1(32), seg(4, 8, 4)], sw="add1 add2 relu_in split", plan={"nchunks": 2}),
    c1x2_case("x_cg4_cin64_norelu", 4, 2, (7, 19), [_x1(64)], sw="add1", plan={"nchunks": 2}),
    c1x2_case("x_cg4_cin44", 4, 2, (5, 9), [_x1(32), seg(12)], sw="relu_in", plan={"nchunks": 2}),
    # CG = 1 at one quad
    c1x2_case("x_cg1_cq1", 1, 3, (9, 12), [_x1(4)]),
    c1x2_case("x_cg1_cq1_noadd", 1, 2, (9, 12), [_x1(4)], sw=""),
    # scalar staging (Cin % 4 != 0: the padded channels must carry zero weight; a misaligned segment)
    c1x2_case("x_cg2_scalar_cin6", 2, 3, (9, 12), [seg(6)], plan={"vec4": 0}),
    c1x2_case("x_cg2_scalar_cin10", 2, 2, (5, 33), [seg(6, 8, 1), seg(4)], sw="add1 add2 relu_in split", plan={"vec4": 0}),
    c1x2_case("x_cg4_scalar_cin18", 4, 2, (9, 12), [seg(18, 20, 1)], sw="add2 relu_in", plan={"vec4": 0}),
    c1x2_case("x_cg1_scalar_cin3", 1, 2, (9, 12), [seg(3)], sw="add1", plan={"vec4": 0}),
    c1x2_case("x_cg4_scalar_misaligned", 4, 2, (9, 12), [seg(16, 16, 0, 1)], plan={"vec4": 0}),
]
# geometry in every CG (Cin = 4 / 8 / 16 select CG = 1 / 2 / 4 at these tile counts): H = W = 1; W < 8; H and W one more than a tile
# multiple with grid >= 16, grid % 8 != 0 and a last tile whose ring lies outside the image on two sides; an image of exactly one tile
for _cg, _ch, _plus1, _one in ((1, 4, (9, 33), (8, 32)), (2, 8, (5, 33), (4, 32)), (4, 16, (5, 33), (4, 16))):
    C1X2_CASES += [
        c1x2_case("x_cg%d_h1w1" % _cg, _cg, 3, (1, 1), [_x1(_ch)]),
        c1x2_case("x_cg%d_w5" % _cg, _cg, 2, (11, 5), [_x1(_ch)], sw="add1 relu_in"),
        c1x2_case("x_cg%d_plus1_xcd_uneven" % _cg, _cg, 5, _plus1, [_x1(_ch)], plan={"grid": 20 if _cg < 4 else 30}),
        c1x2_case("x_cg%d_one_tile" % _cg, _cg, 2, _one, [_x1(_ch)], sw="add2 relu_in", plan={"tiles_x": 1, "tiles_y": 1}),
    ]
C1X2_BY_NAME = {c["name"]: c for c in C1X2_CASES}
assert len(C1X2_BY_NAME) == len(C1X2_CASES)


def _w_params(case):
    """(w_rows, w_split, w_gap, w2_d1_row, weight rows) of a forward case in the production form."""
    n0, cin, sw = case["ins"][0][0], case["cin"], case["sw"]
    w_rows = n0 if "rows" in sw else cin
    split, gap = (n0, CC_ROWS) if "split" in sw else (0, 0)
    d1row = w_rows + gap + (0 if "split" in sw else CC_ROWS)
    return w_rows, split, gap, d1row, d1row + 1


def c1x2_plan(Hm, case):
    B, (Hh, Ww) = case["B"], case["hw"]
    ins = [descr((B, Hh, Ww), sp, i) for i, sp in enumerate(case["ins"])]
    w_rows, split, gap, d1row, _ = _w_params(case)
    a = lambda on, slot: descr((B, Hh, Ww), seg(1, 2, slot & 1), slot) if on else None      # noqa: E731
    return Hm.c1x2_fwd_plan(ins, descr((B, Hh, Ww), seg(4), 6), add1=a("add1" in case["sw"], 4), add2=a("add2" in case["sw"], 5),
                            w_rows=w_rows, w2_d1_row=d1row, w_split=split, w_gap=gap, relu_in="relu_in" in case["sw"])


def c1x2_features(p):
    """The (instance, plan feature) pairs of a c1x2 plan."""
    f = {"twl%d" % p["TW_log2"], "chunks%d" % p["nchunks"], "vec4" if p["vec4"] else "scalar",
         "one_tile_images" if p["tiles_x"] * p["tiles_y"] == 1 else "tiled_images",
         "xcd_off" if p["grid"] < 16 else ("xcd_even" if p["grid"] % 8 == 0 else "xcd_uneven")}
    return {("c1x2<%d>" % p["CG"], x) for x in f}


def fwd_data(case, mode, seed=0):
    """x (all segments' channels), the weights by row (rows no channel reads hold NaN), the addends."""
    g = _gen(4000 + seed)
    B, (Hh, Ww), cin = case["B"], case["hw"], case["cin"]
    w_rows, split, gap, d1row, nrows = _w_params(case) if case["fam"] == "c1x2" else _c1_params(case)
    d = dict(x=rnd(g, (B, Hh, Ww, cin), mode))
    for k in ("w1", "w2"):
        w = torch.full((nrows, 9), NAN, dtype=torch.float64)
        for c in range(min(w_rows, cin)):
            w[c + (gap if split and c >= split else 0)] = rnd(g, (9,), mode, 2)
        if k == "w2" and case["fam"] == "c1x2":
            w[d1row] = rnd(g, (9,), mode, 2)
        d[k] = w
    for k in ("add1", "add2", "add"):
        d[k] = rnd(g, (B, Hh, Ww, 1), mode, 8) if k in case["sw"] else None
    return d


def _eff(w, case, cin, params):
    """[1][Cin][3][3]: the weight every input channel meets (zero for channels >= w_rows)."""
    w_rows, split, gap = params[:3]
    out = torch.zeros(cin, 9, dtype=torch.float64)
    for c in range(min(w_rows, cin)):
        out[c] = w[c + (gap if split and c >= split else 0)]
    return out.reshape(1, cin, 3, 3)


def _conv(x_nchw, w):
    return F.conv2d(x_nchw, w.to(x_nchw.device), padding=1).permute(0, 2, 3, 1)


def c1x2_ref(case, d, fault=None):
    """(ref, bound factors) with ref [B,H,W,4] = (d1, d2, 0, 0) fp64 and the dict S1, S2, P21 = |w2_d1| * S1 (module docstring).
    fault: ("ring",) d1 is NOT zeroed outside the image (its values there are what the convolution formula gives on the zero-padded
    input); ("lane", CG, l) the channel quads q with q % CG == l dropped from both sums; ("quad", c0) channels c0 .. c0 + 3 dropped."""
    cin = case["cin"]
    P = _w_params(case)
    x = d["x"].permute(0, 3, 1, 2)
    a = x.clamp(min=0) if "relu_in" in case["sw"] else x
    W1, W2 = _eff(d["w1"], case, cin, P), _eff(d["w2"], case, cin, P)
    wd = d["w2"][P[3]].reshape(1, 1, 3, 3)
    F1, F2 = W1, W2
    if fault and fault[0] in ("lane", "quad"):
        keep = torch.ones(cin, dtype=torch.float64)
        for c in range(cin):
            if (fault[0] == "lane" and (c // 4) % fault[1] == fault[2]) or (fault[0] == "quad" and fault[1] <= c < fault[1] + 4):
                keep[c] = 0
        F1, F2 = W1 * keep.view(1, -1, 1, 1), W2 * keep.view(1, -1, 1, 1)
    zero = torch.zeros((), dtype=torch.float64)
    a1 = d["add1"] if d["add1"] is not None else zero
    a2 = d["add2"] if d["add2"] is not None else zero
    d1 = _conv(a, F1) + a1
    if fault and fault[0] == "ring":
        ap = F.pad(a, (1, 1, 1, 1))
        a1p = F.pad(d["add1"].permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1) if d["add1"] is not None else zero
        d1e = (_conv(ap, F1) + a1p).clamp(min=0).permute(0, 3, 1, 2)                  # d1 on the image plus a one-pixel ring
        second = F.conv2d(d1e, wd).permute(0, 2, 3, 1)
    else:
        second = _conv(d1.clamp(min=0).permute(0, 3, 1, 2), wd)
    d2 = _conv(a, F2) + second + a2
    S1 = _conv(a.abs(), W1.abs()) + a1.abs()
    P21 = _conv(S1.permute(0, 3, 1, 2), wd.abs())
    S2 = _conv(a.abs(), W2.abs()) + P21 + a2.abs()
    z = torch.zeros_like(d1)
    return torch.cat([d1, d2, z, z], 3).contiguous(), dict(S1=S1, S2=S2, P21=P21)


def c1x2_bound(case, S):
    K = case["K"]
    z = torch.zeros_like(S["S1"])
    return torch.cat([(K + 6) * U24 * S["S1"], (K + 16) * U24 * S["S2"] + (K + 6) * U24 * S["P21"], z, z], 3)


# =================================================================================================================================
# c1_fwd: out = conv3x3_zero(act(x); W) + add  (one channel; fill4: (value, 0, 0, 0))
# =================================================================================================================================
def c1_case(name, B, hw, ins, sw="add relu_in", w_rows=0, plan=None, gauss=True):
    """sw of: add relu_in fill4 split (channels >= the first segment's read rows w_gap = Cc further down) inplace (the production
    second layer: the last segment is D = (d1, 0, 0, 0), the output its channel 1, w_rows = Cin - 3)."""
    sw = set(sw.split())
    assert sw <= {"add", "relu_in", "fill4", "split", "inplace"}, sw
    cin = sum(i[0] for i in ins)
    assert "inplace" not in sw or (ins[-1][0] == 4 and "fill4" not in sw)
    return dict(name=name, B=B, hw=hw, ins=ins, sw=sw, w_rows=cin - 3 if "inplace" in sw else w_rows, plan=plan or {}, cin=cin,
                K=9 * ((cin + 3) & ~3), gauss=gauss, fam="c1")


C1_CASES = [
    c1_case("c_cin4_twl3", 3, (9, 8), [_x1(4)], sw="add relu_in fill4", plan={"TW_log2": 3, "vec4": 1}),
    c1_case("c_cin6_scalar_twl4", 2, (17, 12), [seg(6)], sw="relu_in", plan={"TW_log2": 4, "vec4": 0, "tiles_y": 2}),
    c1_case("c_cin36_twl5", 2, (9, 33), [_x1(32), seg(4)], sw="add relu_in split", plan={"TW_log2": 5, "nchunks": 2, "tiles_x": 2}),
    c1_case("c_cin44_seg3", 2, (5, 7), [_x1(32), seg(8, 12, 4), seg(4)], sw="add", plan={"nchunks": 2, "KCH": 32}),
    c1_case("c_cin64_fill4", 2, (9, 12), [_x1(64)], sw="relu_in fill4", plan={"nchunks": 2}),
    c1_case("c_cin44_rows36", 2, (9, 12), [_x1(32), seg(12)], sw="add relu_in", w_rows=36),
    c1_case("c_inplace_ch8", 3, (9, 12), [_x1(8), seg(4)], sw="add relu_in inplace split"),
    c1_case("c_inplace_ch64", 2, (9, 33), [_x1(64), seg(4)], sw="add relu_in inplace split", plan={"nchunks": 3}),
    c1_case("c_inplace_ch6_scalar", 2, (7, 19), [seg(6, 12, 0), seg(4)], sw="relu_in inplace split", plan={"vec4": 0}),
    c1_case("c_scalar_cin38", 2, (5, 9), [seg(38, 40, 1)], sw="add relu_in", plan={"vec4": 0, "nchunks": 2}),
    c1_case("c_scalar_cin70", 1, (5, 9), [seg(66), seg(4)], sw="add", plan={"vec4": 0, "nchunks": 3}),
    c1_case("c_h1w1", 3, (1, 1), [_x1(8)], sw="add relu_in fill4"),
    c1_case("c_cin4_b40_xcd_free", 40, (33, 9), [_x1(4)], sw="relu_in", plan={"TW_log2": 4, "tiles_y": 3, "grid": 120}),
]
C1_BY_NAME = {c["name"]: c for c in C1_CASES}
assert len(C1_BY_NAME) == len(C1_CASES)


def _c1_params(case):
    n0, cin, sw = case["ins"][0][0], case["cin"], case["sw"]
    w_rows = case["w_rows"] or cin
    split, gap = (n0, CC_ROWS) if "split" in sw else (0, 0)
    return w_rows, split, gap, -1, w_rows + gap + 1


def c1_plan(Hm, case):
    B, (Hh, Ww) = case["B"], case["hw"]
    ins = [descr((B, Hh, Ww), sp, i) for i, sp in enumerate(case["ins"])]
    w_rows, split, gap, _, _ = _c1_params(case)
    sw = case["sw"]
    return Hm.c1_fwd_plan(ins, descr((B, Hh, Ww), seg(1, 4, 1 if "inplace" in sw else 0), 6),
                          add=descr((B, Hh, Ww), seg(1, 2, 1), 4) if "add" in sw else None, w_rows=case["w_rows"],
                          fill4="fill4" in sw, w_split=split, w_gap=gap, relu_in="relu_in" in sw)


def c1_features(p):
    return {("c1_fwd", x) for x in ("twl%d" % p["TW_log2"], "chunks%d" % p["nchunks"], "vec4" if p["vec4"] else "scalar")}


def c1_data(case, mode, seed=0):
    d = fwd_data(case, mode, seed)
    if "inplace" in case["sw"]:
        d["x"][..., -3:] = 0          # D = (d1, 0, 0, 0) on entry
    return d


def c1_ref(case, d, fault=None):
    """(ref [B,H,W,1], S).  fault ("quad", c0): input channels c0 .. c0 + 3 dropped."""
    cin = case["cin"]
    P = _c1_params(case)
    x = d["x"].permute(0, 3, 1, 2)
    a = x.clamp(min=0) if "relu_in" in case["sw"] else x
    W = _eff(d["w1"], case, cin, P)
    Wf = W
    if fault:
        Wf = W.clone()
        Wf[:, fault[1]:fault[1] + 4] = 0
    ad = d["add"] if d["add"] is not None else torch.zeros((), dtype=torch.float64)
    return (_conv(a, Wf) + ad).contiguous(), (_conv(a.abs(), W.abs()) + ad.abs()).contiguous()


# =================================================================================================================================
# thin grouped weight gradient: dW[g][co][ci][ky][kx] += sum_{b,y,x} dy[b,y,x, dyc g + co] act(X_g[b, y + ky - 1, x + kx - 1, ci])
# =================================================================================================================================
THIN_INST = {12: (2, 12, 16), 20: (3, 20, 16), 36: (6, 36, 16), 68: (10, 68, 8)}


def thin_case(name, segs, shape, G, dyc, sw="relu_in", plan=None, rc=0, dy_mis=0, dy_slack=0):
    """segs: channels of the input segments (production: (ch, 4) = [x1 slice of a 2 ch tensor, D]); sw of: relu_in prev (dW non-zero on
    entry) dy_slice (dy a channel slice of a wider tensor); dy_mis: floats the dy pointer is off; dy_slack: extra pixel stride of dy."""
    sw = set(sw.split())
    assert sw <= {"relu_in", "prev", "dy_slice"}, sw
    B, Hh, Ww = shape
    return dict(name=name, segs=tuple(segs), shape=shape, G=G, dyc=dyc, sw=sw, plan=plan or {}, rc=rc, cin=sum(segs), K=B * Hh * Ww,
                gauss=B * Hh * Ww <= KMAX_GAUSS, dy_mis=dy_mis, dy_off=4 if "dy_slice" in sw else 0,
                dy_width=dyc * G + (8 if "dy_slice" in sw else 0) + dy_slack, fam="thin")


THIN_CASES = []
for _ch in (8, 16, 32, 64):
    _th = 8 if _ch == 64 else 16
    # P blocks per group at G = 15: (per_cu 256 + 14) / 15 rounded down to a multiple of 8 (per_cu = 7 / 5 / 3 / 3 by the LDS bytes)
    _P = {8: 120, 16: 80, 32: 48, 64: 48}[_ch]
    THIN_CASES += [
        # few tiles (P < 8: plain block order), both dy forms, ragged tiles on both axes
        thin_case("t_ch%d_dyc4_few" % _ch, (_ch, 4), (2, _th + 3, 21), 2, 4, plan={"xcd": 1, "P": 8}),
        thin_case("t_ch%d_dyc2_p4" % _ch, (_ch, 4), (1, _th + 3, 21), 2, 2, sw="relu_in dy_slice prev", plan={"xcd": 0, "P": 4}),
        # P >= 8 and a block that walks more than one tile with a ragged last round: P + 10 one-tile images, G = 15
        thin_case("t_ch%d_dyc2_walk_g15" % _ch, (_ch, 4), (_P + 10, 3, 5), 15, 2, plan={"xcd": 1, "P": _P, "ntiles": _P + 10}),
        thin_case("t_ch%d_walk_even_g15" % _ch, (_ch, 4), (2 * _P, 3, 5), 15, 2, sw="", plan={"xcd": 1, "P": _P, "ntiles": 2 * _P}),
        thin_case("t_ch%d_dyc4_walk_g15" % _ch, (_ch, 4), (_P + 3, 2, 17), 15, 4, sw="prev", plan={"xcd": 1, "P": _P, "ntiles": 2 * _P + 6}),
    ]
THIN_CASES += [
    thin_case("t_g1_one_segment", (12,), (3, 20, 24), 1, 4, sw="", plan={"xcd": 1, "P": 8, "ntiles": 12}),
    thin_case("t_g1_three_segments", (8, 8, 4), (2, 9, 40), 1, 2, sw="relu_in dy_slice", plan={"xcd": 0, "P": 6}),
    thin_case("t_three_segments_ch32", (16, 16, 4), (1, 5, 7), 3, 4, sw="prev", plan={"xcd": 0, "P": 1}),
    thin_case("t_h1w1", (8, 4), (3, 1, 1), 2, 2, plan={"xcd": 0, "P": 3}),
    thin_case("t_w_below_tile", (16, 4), (2, 37, 3), 2, 4, sw="", plan={"xcd": 0, "P": 6}),
    thin_case("t_h_below_tile_ch64", (64, 4), (2, 3, 37), 2, 2, sw="relu_in prev", plan={"xcd": 0, "P": 6}),
    thin_case("t_dy_stride_wider", (8, 4), (2, 9, 12), 3, 2, dy_slack=2, plan={"xcd": 0, "P": 2}),
    # multi-tile images on an uneven walk: 2 x 40 x 40 = 18 tiles over P = 16 blocks
    thin_case("t_walk_in_images", (8, 4), (2, 40, 40), 2, 2, plan={"xcd": 1, "P": 16, "ntiles": 18}),
    # declined: -100, outputs untouched
    thin_case("t_declined_cin16", (12, 4), (2, 9, 12), 2, 4, rc=-100),
    thin_case("t_declined_segment6", (6, 6), (2, 9, 12), 2, 4, rc=-100),
    thin_case("t_declined_four_segments", (4, 4, 8, 4), (2, 9, 12), 2, 4, rc=-100),
    thin_case("t_declined_dy_misaligned", (8, 4), (2, 9, 12), 2, 4, rc=-100, dy_mis=1),
    thin_case("t_declined_dy_stride_odd", (8, 4), (2, 9, 12), 2, 2, rc=-100, dy_slack=1),
]
THIN_BY_NAME = {c["name"]: c for c in THIN_CASES}
assert len(THIN_BY_NAME) == len(THIN_CASES)


def thin_plan(Hm, case):
    return Hm.conv_wgrad_thin_grouped_plan(case["shape"], case["segs"], case["G"], CC.BASE + 4 * (case["dy_off"] + case["dy_mis"]),
                                           case["dy_width"], case["dyc"], relu_in="relu_in" in case["sw"])


def thin_features(p):
    f = {"dyc%d" % p["dyc"], "xcd_order" if p["xcd"] else "plain_order"}
    if p["ntiles"] > p["P"]:
        f.add("walk_ragged" if p["ntiles"] % p["P"] else "walk_even")
    else:
        f.add("one_tile_per_block")
    return {("thin<%d,%d,%d>" % (p["SL"], p["CS"], p["TH"]), x) for x in f}


def thin_block_group(b, G, P, wrong=False):
    """(group, partition) of block b, as wgrad_thin_kernel maps it (wrong: the plain mapping where the XCD-aware one applies)."""
    if P % 8 == 0 and not wrong:
        xcd, slot = b & 7, b >> 3
        return slot % G, xcd + 8 * (slot // G)
    return b % G, b // G


def thin_data(case, mode, seed=0):
    g = _gen(5000 + seed)
    B, Hh, Ww = case["shape"]
    G, dyc, cin = case["G"], case["dyc"], case["cin"]
    d = dict(x=[rnd(g, (B, Hh, Ww, cin), mode) for _ in range(G)], dy=rnd(g, (B, Hh, Ww, dyc * G), mode),
             prev=rnd(g, (G, 4, cin, 3, 3), mode, 8) if "prev" in case["sw"] else None)
    return d


def thin_ref(case, d, fault=None, plan=None):
    """(dW [G][4][Cin][3][3], S).  fault (needs the plan): ("map",) every block takes its group from the PLAIN mapping and its partition
    from the kernel's: where P % 8 == 0 and G shares a factor with 8 some (group, partition) pairs are then computed twice and others
    never (for odd G, 8 slot + xcd mod G still visits every group once per partition: the same numbers);
    ("zw",) rows 2, 3 of a compact dy pair are not zeroed: they take the next group's pair (the bytes behind it)."""
    B, Hh, Ww = case["shape"]
    G, dyc, cin = case["G"], case["dyc"], case["cin"]
    relu = "relu_in" in case["sw"]
    out = d["prev"].clone() if d["prev"] is not None else torch.zeros(G, 4, cin, 3, 3, dtype=torch.float64)
    S = out.abs()
    dyq = torch.zeros(B, Hh, Ww, G, 4, dtype=torch.float64)
    dyq[..., :dyc] = d["dy"].reshape(B, Hh, Ww, G, dyc)
    if fault and fault[0] == "zw" and dyc == 2:
        dyq[..., :-1, 2:] = d["dy"].reshape(B, Hh, Ww, G, 2)[..., 1:, :]
    if fault and fault[0] == "map":
        P, tx_n, ty_n, th = plan["P"], plan["tiles_x"], plan["tiles_y"], plan["TH"]
        for b in range(P * G):
            _, part = thin_block_group(b, G, P)              # the block's partition, by the kernel's mapping
            gi, _ = thin_block_group(b, G, P, wrong=True)    # its group, by the plain one
            go = gi
            xp = F.pad((d["x"][gi].clamp(min=0) if relu else d["x"][gi]).permute(0, 3, 1, 2), (1, 1, 1, 1))
            m = torch.zeros(B, Hh, Ww, 1, dtype=torch.float64)
            for t in range(part, plan["ntiles"], P):
                tx, ty, bb = t % tx_n, (t // tx_n) % ty_n, t // (tx_n * ty_n)
                m[bb, ty * th:(ty + 1) * th, tx * 16:(tx + 1) * 16] = 1
            out[go] += CC.wg_dense(xp, dyq[..., gi, :] * m, 3, 1)
        return out, None
    for gi in range(G):
        xa = d["x"][gi].permute(0, 3, 1, 2)
        xp = F.pad(xa.clamp(min=0) if relu else xa, (1, 1, 1, 1))
        out[gi] += CC.wg_dense(xp, dyq[..., gi, :], 3, 1)
        S[gi] += CC.wg_dense(F.pad(xa.abs(), (1, 1, 1, 1)), dyq[..., gi, :].abs(), 3, 1)
    return out, S


# =================================================================================================================================
# mix weight gradient: dW[g][o][i] += sum_px dy_g[px][o] y_g[px][i],  db[g][o] += sum_px dy_g[px][o]
# =================================================================================================================================
def mixwg_case(name, C, npix, G, segs=None, sw="db", plan=None, rc=0, sets=None):
    """segs: channels of the input segments; sw of: db pair (dy as two halves at different pixel strides) prev; sets: the number of
    distinct (input, dy) operand sets the G groups cycle through (default G: every group its own)."""
    sw = set(sw.split())
    assert sw <= {"db", "pair", "prev"}, sw
    return dict(name=name, C=C, npix=npix, G=G, segs=tuple(segs or (C,)), sw=sw, plan=plan or {}, rc=rc, sets=sets or G, K=npix,
                gauss=npix <= KMAX_GAUSS, big=2 * (sets or G) * npix * C > BIG_ELEMS, fam="mixwg")


def PAIR_STRIDES(C):
    """Pixel strides of the two halves of a dy pair: different on purpose (the kernel reads table entries 13 and 15)."""
    return C // 2 + 4, C // 2 + 8


MIXWG_CASES = [
    mixwg_case("m16_p1_px1", 16, 1, 1, plan={"P": 1}),
    mixwg_case("m16_p1_px511_pair", 16, 511, 2, segs=(8, 8), sw="db pair", plan={"P": 1}),
    mixwg_case("m32_p1_px510_nodb", 32, 510, 2, segs=(16, 16), sw="pair prev", plan={"P": 1}),
    mixwg_case("m32_p1_three_segments", 32, 77, 3, segs=(16, 12, 4), sw="db", plan={"P": 1}),
    mixwg_case("m16_three_segments_pair", 16, 130, 2, segs=(8, 4, 4), sw="db pair prev", plan={"P": 1}),
    # P > 1 with a last partition of 1, 2 and 3 valid pixels: P = ceil(npix / 512) partitions of per = 512 pixels need
    # ceil(npix / P) > 512 - 16 U, i.e. P >= 4 at C = 16 (U = 8) and P >= 8 at C = 32 (U = 4); pixel counts that are no multiple of 4
    mixwg_case("m16_p4_last1", 16, 1537, 1, sw="db", plan={"P": 4, "per": 512}),
    mixwg_case("m16_p4_last2_pair", 16, 1538, 2, segs=(8, 8), sw="db pair", plan={"P": 4, "per": 512}),
    mixwg_case("m32_p8_last3_pair", 32, 3587, 2, segs=(16, 16), sw="db pair prev", plan={"P": 8, "per": 512}),
    mixwg_case("m32_p8_last1", 32, 3585, 1, segs=(16, 12, 4), sw="", plan={"P": 8, "per": 512}),
    mixwg_case("m16_p2_px770_pair", 16, 770, 2, segs=(8, 8), sw="db pair", plan={"P": 2}),
    mixwg_case("m16_p2_full", 16, 1024, 1, sw="db", plan={"P": 2, "per": 512}),
    mixwg_case("m32_p2_full_pair", 32, 1024, 2, segs=(16, 16), sw="db pair", plan={"P": 2, "per": 512}),
    mixwg_case("m32_p3_px1030", 32, 1030, 1, sw="", plan={"P": 3}),
    # G = 15: P = ceil(2048 / 15) = 137 against ceil(npix / 512)
    mixwg_case("m16_g15_p2", 16, 600, 15, segs=(8, 8), sw="db pair", plan={"P": 2}),
    mixwg_case("m32_g15_p137_pair", 32, 512 * 137 + 3, 15, segs=(16, 16), sw="db pair", plan={"P": 137}, sets=2),
    # empty partitions (p0 >= npix: the sweep reaches them whenever P = ceil(2048 / G) and npix / P is just above a 16 U multiple)
    mixwg_case("m16_g16_empty_partitions", 16, 65600, 16, segs=(8, 8), sw="db pair", plan={"P": 128, "per": 640}, sets=2),
    mixwg_case("m32_g16_empty_partitions", 32, 65600, 16, sw="db prev", plan={"P": 128, "per": 576}, sets=2),
    mixwg_case("m_declined_c24", 24, 100, 2, rc=-100),
    mixwg_case("m_declined_npix0", 16, 0, 2, rc=-100),
]
MIXWG_BY_NAME = {c["name"]: c for c in MIXWG_CASES}
assert len(MIXWG_BY_NAME) == len(MIXWG_CASES)


def mixwg_plan(Hm, case):
    return Hm.mix_wgrad_grouped_plan(case["npix"], case["C"], case["G"], db="db" in case["sw"])


def mixwg_features(p, npix):
    last = npix - (p["P"] - 1) * p["per"]
    f = {"P1" if p["P"] == 1 else "Pmany"}
    if p["P"] > 1:
        f.add("empty_partitions" if last <= 0 else ("last_partial" if last < p["per"] else "last_full"))
        if 0 < last < 4:
            f.add("last_below_4")
    if npix % 4:
        f.add("px_mod4")
    return {("mix_wgrad<%d>" % p["CT"], x) for x in f}


def mixwg_data(case, mode, seed=0):
    g = _gen(6000 + seed)
    n, C = case["npix"], case["C"]
    amp = 2 if n > 60000 else 3
    return dict(x=[rnd(g, (n, C), mode, amp) for _ in range(case["sets"])], dy=[rnd(g, (n, C), mode, amp) for _ in range(case["sets"])],
                prevW=rnd(g, (case["G"], C, C), mode, 8) if "prev" in case["sw"] else None,
                prevb=rnd(g, (case["G"], C), mode, 8) if "prev" in case["sw"] and "db" in case["sw"] else None)


def mixwg_ref(case, d, fault=None, plan=None):
    """(dW, S_W, db, S_b).  fault: ("ragged",) the last non-empty partition's pixels past its last multiple of 4 dropped;
    ("stride", s1, s2) the second dy half of pixel px read s1 / s2 pixels further on (the first half's stride), i.e. from pixel
    px s1 / s2 when that is a whole pixel of the same tensor, else zero."""
    G, C, n = case["G"], case["C"], case["npix"]
    dev = d["x"][0].device
    dW = d["prevW"].clone() if d["prevW"] is not None else torch.zeros(G, C, C, dtype=torch.float64, device=dev)
    db = d["prevb"].clone() if d["prevb"] is not None else torch.zeros(G, C, dtype=torch.float64, device=dev)
    SW, Sb = dW.abs(), db.abs()
    per_set = []
    for x, dy in zip(d["x"], d["dy"]):
        dyf = dy
        if fault and fault[0] == "ragged":
            p0 = ((n - 1) // plan["per"]) * plan["per"]
            keep = p0 + (n - p0) // 4 * 4
            dyf = dy.clone()
            dyf[keep:] = 0
        if fault and fault[0] == "stride":
            dyf = dy.clone()
            src = torch.arange(n) * fault[1]
            ok = (src % fault[2] == 0) & (src // fault[2] < n)
            dyf[:, C // 2:] = 0
            dyf[ok, C // 2:] = dy[(src // fault[2])[ok], C // 2:]
        per_set.append((dyf.t() @ x, dy.abs().t() @ x.abs(), dyf.sum(0), dy.abs().sum(0)))
    for gi in range(G):
        a, b, c, e = per_set[gi % case["sets"]]
        dW[gi] += a
        SW[gi] += b
        db[gi] += c
        Sb[gi] += e
    return dW, SW, db, Sb


# =================================================================================================================================
# layer planes: [npix][CP] -> [CP / 2][npix][2]
# =================================================================================================================================
PLANES_CP_MAX = 512
PLANES_CASES = [dict(name="lp_cp%d_px%d" % (cp, n), CP=cp, npix=n, rc=0) for cp in (4, 8, 32) for n in (1, 63, 64, 65)] + [
    dict(name="lp_cp30x_px200", CP=28, npix=200, rc=0),
    dict(name="lp_cp256_px65", CP=256, npix=65, rc=0),            # the first CP above 64 KB of LDS
    dict(name="lp_cp512_px130", CP=PLANES_CP_MAX, npix=130, rc=0),
    dict(name="lp_refused_cp516", CP=516, npix=5, rc=-1),
    dict(name="lp_refused_cp6", CP=6, npix=5, rc=-1),
    dict(name="lp_refused_cp0", CP=0, npix=5, rc=-1),
    dict(name="lp_refused_npix0", CP=8, npix=0, rc=-1),
]


def planes_ref(src):
    n, cp = src.shape
    return src.reshape(n, cp // 2, 2).permute(1, 0, 2).contiguous()


# =================================================================================================================================
# channel mixes: y[p][o] = sum_i W[o][i] x[p][i] + bias[o]  (transposed: W^T)
# =================================================================================================================================
MIX32_INST = {1: (1, 8), 2: (2, 4), 3: (3, 2), 4: (4, 2), 5: (6, 1), 6: (6, 1), 7: (8, 1), 8: (8, 1)}
MIX16_INST = {1: (1, 8), 2: (2, 8), 3: (3, 4), 4: (4, 4), 5: (6, 2), 6: (6, 2), 7: (8, 2), 8: (8, 2), 9: (12, 1), 10: (12, 1), 11: (12, 1),
              12: (12, 1), 13: (16, 1), 14: (16, 1), 15: (16, 1), 16: (16, 1)}
GRID_CAP = 2048


def mix_plan(kind, C, npix):
    """(NT, NP, grid, rounds): the instance by (C + 15) / 16, grid = clamp(ceil(npix / (64 NP)), 1, 2048); rounds a block loops."""
    NT, NP = (MIX32_INST if kind == "f32" else MIX16_INST)[(C + 15) // 16]
    groups = (npix + 64 * NP - 1) // (64 * NP)
    grid = min(max(groups, 1), GRID_CAP)
    return NT, NP, grid, (groups + grid - 1) // grid if groups else 0


def mix_case(name, kind, C, npix, sw="bias", xw=None, yw=None, rc=0):
    """sw of: bias transposed; xw / yw = (width, off): input / output as channel slices of wider tensors."""
    sw = set(sw.split())
    assert sw <= {"bias", "transposed"}, sw
    c = dict(name=name, kind=kind, C=C, npix=npix, sw=sw, xw=xw or (C, 0), yw=yw or (C, 0), rc=rc, K=16 * ((C + 15) // 16),
             big=npix * C > BIG_ELEMS, gauss=True, fam="mix")
    if rc == 0:
        c["NT"], c["NP"], c["grid"], c["rounds"] = mix_plan(kind, C, npix)
    return c


MIX_CASES = []
for _kind, _cs in (("f32", (12, 16, 20, 32, 40, 48, 56, 64, 68, 96, 100, 128)),
                   ("f16", (12, 16, 20, 32, 40, 48, 56, 64, 68, 96, 100, 128, 180, 192, 244, 256))):
    for _i, _c in enumerate(_cs):
        _n = (1, 15, 17, 333)[_i % 4]
        MIX_CASES.append(mix_case("mx_%s_c%d_px%d" % (_kind, _c, _n), _kind, _c, _n, sw="bias" if _i % 2 else "",
                                  xw=(_c + 8, 4) if _i % 3 == 0 else None, yw=(_c + 4, 4) if _i % 3 == 1 else None))
        _n = (333, 17, 1, 15)[_i % 4]
        MIX_CASES.append(mix_case("mx_%s_c%d_t_px%d" % (_kind, _c, _n), _kind, _c, _n, sw="transposed" if _i % 2 else "bias transposed",
                                  xw=(_c + 4, 0) if _i % 3 == 1 else None, yw=(_c + 8, 4) if _i % 3 == 2 else None))
MIX_CASES += [
    # the grid cap (blocks loop with stride gridDim.x 4 group), once per distinct loop
    mix_case("mx_f32_cap_np1_c68", "f32", 68, GRID_CAP * 64 + 64 + 37, sw="bias"),
    mix_case("mx_f16_cap_6x2_c96", "f16", 96, GRID_CAP * 128 + 128 + 37, sw="bias transposed"),
    mix_case("mx_f16_cap_nt12_c192", "f16", 192, GRID_CAP * 64 + 64 + 37, sw="bias"),
    mix_case("mx_f32_cap_np8_c16", "f32", 16, GRID_CAP * 512 + 512 + 37, sw="bias", xw=(20, 4)),
    # refused: -1, nothing written
    mix_case("mx_f32_refused_c6", "f32", 6, 20, rc=-1),
    mix_case("mx_f32_refused_c132", "f32", 132, 20, rc=-1),
    mix_case("mx_f16_refused_c260", "f16", 260, 20, rc=-1),
    mix_case("mx_f16_refused_c10", "f16", 10, 20, rc=-1),
    mix_case("mx_f32_refused_stride", "f32", 16, 20, xw=(18, 0), rc=-1),
    mix_case("mx_f16_refused_stride", "f16", 16, 20, yw=(22, 0), rc=-1),
]
MIX_BY_NAME = {c["name"]: c for c in MIX_CASES}
assert len(MIX_BY_NAME) == len(MIX_CASES)


def mix_features(case):
    f = {"transposed" if "transposed" in case["sw"] else "plain", "bias" if "bias" in case["sw"] else "no_bias",
         "full_tiles" if case["C"] % 16 == 0 else "partial_tile", "loops" if case["rounds"] > 1 else "one_round"}
    inst = ("mix32<%d,%d,0>" if case["kind"] == "f32" else "mix16<%d,%d>") % (case["NT"], case["NP"])
    # the pixel loop is one piece of source per kernel template (mix16_kernel: a second one for NT > 8): a looping block is a feature of
    # the loop, not of the instance
    loop = "mix32 loop" if case["kind"] == "f32" else ("mix16 loop NT > 8" if case["NT"] > 8 else "mix16 loop")
    return {(loop if x in ("loops", "one_round") else inst, x) for x in f}


def mix_data(case, mode, seed=0):
    g = _gen(7000 + seed)
    n, C = case["npix"], case["C"]
    if mode == "int":
        x, W = rnd(g, (n, C), mode, 3), rnd(g, (C, C), mode, 2)
    else:
        x, W = rnd(g, (n, C), mode), rnd(g, (C, C), mode) / math.sqrt(C)
        W = W.float().double()
    return dict(x=x, W=W, bias=rnd(g, (C,), mode, 8) if "bias" in case["sw"] else None)


def f16(t):
    return t.float().half().double()


def mix_ref(case, d, fault=None, half=None):
    """(y, S) fp64.  half: operands rounded to fp16 first (default: for kind f16).  fault ("round", grid, NP): the pixels of every
    block's second round dropped."""
    half = case["kind"] == "f16" if half is None else half
    x, W = (f16(d["x"]), f16(d["W"])) if half else (d["x"], d["W"])
    Wm = W if "transposed" in case["sw"] else W.t()
    y, S = x @ Wm.to(x.device), x.abs() @ Wm.abs().to(x.device)
    if d["bias"] is not None:
        y, S = y + d["bias"].to(x.device), S + d["bias"].abs().to(x.device)
    if fault:
        _, grid, NP = fault
        px = torch.arange(y.shape[0], device=y.device)
        rnd2 = (px // (16 * NP)) // (4 * grid) == 1
        y = torch.where(rnd2.view(-1, 1), torch.full_like(y, NAN), y)
    return y, S


def mix_bound(case, S):
    return (case["K"] + 3) * U24 * S


# =================================================================================================================================
# budgets
# =================================================================================================================================
def case_cost(case):
    """(operand bytes, fp64 multiply-adds of the reference incl. the absolute-value pass) of a case."""
    fam = case.get("fam", "planes")
    if fam in ("c1x2", "c1"):
        px = case["B"] * case["hw"][0] * case["hw"][1]
        return 4 * px * (case["cin"] + 8), 2 * 9 * px * (2 * case["cin"] + 2)
    if fam == "thin":
        px = case["K"]
        return 4 * px * (case["G"] * case["cin"] + case["dy_width"]), 2 * 9 * px * case["G"] * case["cin"] * 4
    if fam == "mixwg":
        return 4 * 2 * case["sets"] * case["npix"] * case["C"], 2 * case["sets"] * case["npix"] * case["C"] ** 2
    if fam == "mix":
        return 4 * case["npix"] * (case["xw"][0] + case["yw"][0]), 2 * case["npix"] * case["C"] ** 2
    return 8 * case["npix"] * case["CP"], 0
