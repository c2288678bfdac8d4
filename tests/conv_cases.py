"""Case tables, fp64 references and error measures of the direct convolution kernels (tmg_conv.hip), shared by
test_conv_plans_cpu.py (plan coverage and the sensitivity of the measures; no device) and test_conv_kernels.py (the kernels).

A segment spec is (n, width, off, mis): n channels at channel offset `off` of an NHWC parent with `width` channels per pixel whose base
address is `mis` floats off 16-byte alignment.  `descr` turns one into the descriptor the plan queries take (a made-up address: the
queries dereference nothing); test_conv_kernels.alloc builds the tensor.  A case names the kernel instance it must run on; `resolve`
asks the library's own planner (tmg_hip.conv_*_plan) for the smallest batch that lands there.

Error measures (u = 2^-24, the fp32 unit roundoff):
  integer mode: every operand is a small integer (in_scale in {0.5, 1, 2}: multiples of 1/2), and the fp64 sum of the absolute values
    of an element's terms, in units of the data's granularity, stays below 2^24.  Every partial sum of every summation order is then
    an integer multiple of that granularity below 2^24: exact in fp32.  The kernel must equal the reference bit for bit.
  Gaussian mode: |a_i - ref_i| <= (K + 8) u S_i with S_i the fp64 sum of the absolute values of element i's own terms and K the
    number of accumulated products.  Derivation: a sum of K + 1 fp32 terms (K products, exact in the matrix pipe's fp32 multiply-add
    up to one rounding each, folded into the additions below) accumulated in ANY order errs by at most gamma_K S = K u S / (1 - K u)
    (Higham, Accuracy and Stability, eq. 4.4); the epilogue adds bias, `add` and the previous contents (3 roundings), multiplies by
    exp(clamp(kappa)) (1 rounding, __expf within 2 ulp) and rounds the result: 8 u S covers them and the (1 - K u)^-1 factor for
    K <= 2048.  A dropped product moves an element by |x w| ~ S / K >> K u S only while K^2 u << 1, hence K <= 2048 (K^2 u = 0.25).
"""
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
KMAX_GAUSS = 2048
BASE = 0x10000000
LOG4 = math.log(4.0)


def seg(n, width=None, off=0, mis=0):
    return (n, width if width is not None else n, off, mis)


def descr(shape3, spec, slot):
    n, width, off, mis = spec
    return (tuple(shape3), BASE * (slot + 1) + 4 * (off + mis), width, n)


def out_hw(Hh, Ww, s):
    return (Hh - 1) // s + 1, (Ww - 1) // s + 1


SWITCHES = ("add", "acc", "bias", "kappa", "aff", "relu_in", "relu_out", "rep")


# ---------------------------------------------------------------------------------------------------------------------------------
# forward cases
# ---------------------------------------------------------------------------------------------------------------------------------
def fwd_case(name, want, hw, ins, outs, k=3, s=1, sw=(), add=None, B=1, cap=64, plan=None, gauss=True):
    """want = (kernel, MT, NTW, WM, WN); B: first batch tried, cap: last; plan: further plan fields the case is about."""
    sw = set(sw.split()) if isinstance(sw, str) else set(sw)
    assert sw <= set(SWITCHES), sw
    if "add" in sw and add is None:
        add = seg(sum(o[0] for o in outs))
    cin = sum(i[0] for i in ins)
    return dict(name=name, want=tuple(want), hw=hw, ins=ins, outs=outs, k=k, s=s, sw=sw, add=add if "add" in sw else None, B=B, cap=cap,
                plan=plan or {}, gauss=gauss and k * k * cin <= KMAX_GAUSS, K=k * k * cin)


LEAN_INST = {(1, 8, 1): 16, (2, 8, 1): 32, (3, 8, 1): 48, (4, 8, 1): 64, (3, 4, 2): 96, (4, 4, 2): 128, (3, 2, 4): 192, (4, 2, 4): 256}
FB_INST = {(1, 4, 1): 16, (2, 4, 1): 32, (3, 4, 1): 48, (4, 4, 1): 64, (3, 2, 2): 96, (4, 2, 2): 128, (3, 1, 4): 192, (4, 1, 4): 256}
# compiled by TMG_FWD_CASE but never selected: the lean planner takes NTW = 3 or 4 whenever WN > 1
FWD_UNREACHABLE = ((0, 2, 4, 2), (0, 1, 4, 2), (0, 2, 2, 4), (0, 1, 2, 4))

FWD_CASES = []
for (ntw, wm, wn), cout in LEAN_INST.items():
    # every (instance, MT): 4 input channels; MT = 2, 4 need 16 MT WM 256 / gy pixels or more (128 x 128 images, batch from the planner)
    FWD_CASES.append(fwd_case("lean_%dx%dx%d_mt1" % (ntw, wm, wn), (0, 1, ntw, wm, wn), (24, 40), [seg(4)], [seg(cout)], B=2, sw="bias rep"))
    for mt in (2, 4):
        FWD_CASES.append(fwd_case("lean_%dx%dx%d_mt%d" % (ntw, wm, wn, mt), (0, mt, ntw, wm, wn), (128, 128), [seg(4)], [seg(cout)], cap=16,
                                  gauss=False, sw="bias" if mt == 2 else "rep relu_in"))
for (ntw, wm, wn), cout in FB_INST.items():
    # the fallback through Cin % 4 != 0 (6 input channels)
    FWD_CASES.append(fwd_case("fb_%dx%dx%d_mt1" % (ntw, wm, wn), (1, 1, ntw, wm, wn), (24, 40), [seg(6)], [seg(cout)], B=2, sw="bias rep"))
    for mt in (2, 4):
        FWD_CASES.append(fwd_case("fb_%dx%dx%d_mt%d" % (ntw, wm, wn, mt), (1, mt, ntw, wm, wn), (128, 128), [seg(6)], [seg(cout)], cap=16,
                                  gauss=False, sw="bias" if mt == 2 else "rep relu_in"))
ALL_SW = " ".join(SWITCHES)
FWD_CASES += [
    # channel chunks of the lean kernel: 104 -> 64 + 48 (40 valid), 136 -> 3 x 48 (40 valid in the last)
    fwd_case("lean_chunks2_cin104", (0, 1, 1, 8, 1), (9, 40), [seg(104)], [seg(16)], B=2, plan={"nchunks": 2, "KCH": 64}, sw="rep bias"),
    fwd_case("lean_chunks3_cin136", (0, 1, 2, 8, 1), (9, 40), [seg(136)], [seg(32)], B=2, plan={"nchunks": 3, "KCH": 48}, sw="add relu_in"),
    # 64 channels fit one chunk on a 128-pixel tile; the 256-pixel tile of MT = 2 (patch 34 x 10) needs two
    fwd_case("lean_chunks_by_patch", (0, 2, 1, 8, 1), (128, 128), [seg(64)], [seg(4)], cap=8, plan={"nchunks": 2, "KCH": 32}, sw="bias"),
    fwd_case("lean_k1", (0, 1, 1, 8, 1), (13, 21), [seg(16)], [seg(16)], k=1, B=2, sw="bias kappa acc"),
    fwd_case("lean_k1_all", (0, 1, 2, 8, 1), (7, 19), [seg(24)], [seg(32)], k=1, B=3, sw=ALL_SW),
    fwd_case("lean_in3_slices", (0, 1, 1, 8, 1), (11, 37), [seg(8), seg(4, 12, 4), seg(4, 8, 4)], [seg(16)], B=2, sw="aff relu_in rep"),
    fwd_case("lean_out2", (0, 1, 2, 8, 1), (11, 37), [seg(8)], [seg(20), seg(12, 16, 4)], B=2, sw="kappa relu_out add"),
    fwd_case("lean_out3", (0, 1, 3, 8, 1), (11, 37), [seg(8)], [seg(16), seg(8, 16, 4), seg(16, 24, 8)], B=2, sw="acc bias"),
    fwd_case("lean_all_switches", (0, 1, 2, 8, 1), (11, 37), [seg(8), seg(8, 16, 4)], [seg(16), seg(16, 24, 4)], B=2, sw=ALL_SW),
    fwd_case("lean_ovec0_cout18", (0, 1, 2, 8, 1), (11, 37), [seg(8)], [seg(18)], B=2, plan={"ovec4": 0}, sw="add acc bias relu_out"),
    fwd_case("lean_ovec0_out_off2", (0, 1, 1, 8, 1), (11, 37), [seg(8)], [seg(16, 24, 2)], B=2, plan={"ovec4": 0}, sw="kappa aff"),
    fwd_case("lean_ovec0_add_misaligned", (0, 1, 1, 8, 1), (11, 37), [seg(8)], [seg(16)], B=2, plan={"ovec4": 0}, sw="add relu_out",
             add=seg(16, 16, 0, 1)),
    fwd_case("lean_h1", (0, 1, 1, 8, 1), (1, 45), [seg(8)], [seg(16)], B=3, sw="rep"),
    fwd_case("lean_w1", (0, 1, 1, 8, 1), (45, 1), [seg(8)], [seg(16)], B=3, sw="rep acc"),
    fwd_case("lean_w33", (0, 1, 1, 8, 1), (9, 33), [seg(8)], [seg(16)], B=2, plan={"tiles_x": 2}, sw="relu_in"),
    fwd_case("lean_tiny_image", (0, 1, 1, 8, 1), (3, 5), [seg(8)], [seg(16)], B=1, sw="add kappa"),
    # 12 tiles per image, 24 images on 256 blocks: a block's second tile lies in another image
    fwd_case("lean_persistent", (0, 1, 1, 8, 1), (24, 40), [seg(4)], [seg(16)], B=24, cap=24, plan={"grid_x": 256, "tiles_x": 2, "tiles_y": 6},
             sw="bias relu_out"),
    # the fallback kernel through each cause
    fwd_case("fb_stride2_even", (1, 1, 2, 4, 1), (16, 24), [seg(8)], [seg(32)], s=2, B=2, sw="bias relu_in"),
    fwd_case("fb_stride2_odd", (1, 1, 1, 4, 1), (13, 9), [seg(8)], [seg(16)], s=2, B=3, sw=ALL_SW),
    fwd_case("fb_stride2_k1", (1, 1, 1, 4, 1), (13, 10), [seg(8)], [seg(12)], s=2, k=1, B=2, sw="add kappa"),
    fwd_case("fb_in_off2", (1, 1, 1, 4, 1), (11, 37), [seg(8, 12, 2)], [seg(16)], B=2, plan={"vec4": 0}, sw="aff relu_out acc"),
    fwd_case("fb_in_misaligned", (1, 1, 1, 4, 1), (11, 37), [seg(8, 8, 0, 1)], [seg(16)], B=2, plan={"vec4": 0}, sw="rep kappa"),
    fwd_case("fb_out3_in3", (1, 1, 3, 4, 1), (11, 37), [seg(5), seg(4, 12, 4), seg(1)], [seg(16), seg(8, 16, 4), seg(17, 24, 3)], B=2,
             sw="add relu_in bias"),
    # 112 padded channels under the 40 000-byte budget: 64 + 48; 160 under the 65 536-byte budget (stride-2 patch): 144 + 16
    fwd_case("fb_chunks_40k", (1, 1, 1, 4, 1), (6, 40), [seg(102)], [seg(16)], B=2, plan={"KCH": 64, "nchunks": 2}, sw="rep bias"),
    fwd_case("fb_chunks_64k", (1, 1, 3, 1, 4), (7, 33), [seg(150)], [seg(192)], s=2, B=2, plan={"KCH": 144, "nchunks": 2}, sw="acc relu_in"),
]
FWD_BY_NAME = {c["name"]: c for c in FWD_CASES}
assert len(FWD_BY_NAME) == len(FWD_CASES)


def fwd_args(case, B):
    """Descriptors of a forward case for tmg_hip.conv_fwd_plan."""
    Hh, Ww = case["hw"]
    Ho, Wo = out_hw(Hh, Ww, case["s"])
    sw = case["sw"]
    ins = [descr((B, Hh, Ww), sp, i) for i, sp in enumerate(case["ins"])]
    outs = [descr((B, Ho, Wo), sp, 4 + i) for i, sp in enumerate(case["outs"])]
    kw = dict(bias="bias" in sw, kappa="kappa" in sw, in_scale="aff" in sw, in_shift="aff" in sw, relu_in="relu_in" in sw,
              pad_rep="rep" in sw, relu_out="relu_out" in sw, accumulate="acc" in sw,
              add=descr((B, Ho, Wo), case["add"], 8) if case["add"] is not None else None)
    return ins, sum(o[0] for o in case["outs"]), case["k"], case["s"], outs, kw


def fwd_instance(p):
    return (p["kernel"], p["MT"], p["NTW"], p["WM"], p["WN"])


def _matches(p, want, inst, extra):
    return p["rc"] == 0 and inst(p) == tuple(want) and all(p[f] == v for f, v in extra.items())


def resolve_fwd(Hm, case):
    """(B, plan): the smallest batch in [case B, cap] whose queried plan is the instance the case names."""
    for B in range(case["B"], case["cap"] + 1):
        ins, cout, k, s, outs, kw = fwd_args(case, B)
        p = Hm.conv_fwd_plan(ins, cout, k, s, outs, **kw)
        if _matches(p, case["want"], fwd_instance, case["plan"]):
            return B, p
    raise AssertionError("%s: no batch in [%d, %d] reaches %s %s (last plan %s)" % (case["name"], case["B"], case["cap"], case["want"],
                                                                                 case["plan"], p))


# ---------------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# ---------------------------------------------------------------------------------------------------------------------------------
def wg_case(name, want, shape, cin, cout, k=3, s=1, ins=None, dy=None, plan=None, ws=True, sw="dbias", layout=None, gauss=True):
    """want = (NP, NCO, LEAN); shape = (B, H, W); layout = (cin_dst, cin_valid, ci_split, ci_off0, ci_off1);
    sw of: dbias kappa aff relu_in rep prev (accumulate onto a non-zero dW)."""
    B, Hh, Ww = shape
    Ho, Wo = out_hw(Hh, Ww, s)
    K = B * Ho * Wo
    sw = set(sw.split())
    ins = ins or [seg(cin)]
    assert sum(i[0] for i in ins) == cin
    return dict(name=name, want=tuple(want), shape=shape, cin=cin, cout=cout, k=k, s=s, ins=ins, dy=dy or seg(cout), plan=plan or {},
                ws=ws, sw=sw, layout=layout or (0, 0, 0, 0, 0), gauss=gauss and K <= KMAX_GAUSS, K=K)


S3 = (3, 20, 24)
WG_CASES = [
    # every (NP, NCO) on the lean path
    wg_case("wg_np3_nco1", (3, 1, 1), S3, 4, 4, k=1, plan={"ksplit": 1}),
    wg_case("wg_np3_nco2", (3, 2, 1), (4, 64, 64), 4, 112, k=1, plan={"gx": 64}),
    wg_case("wg_np3_nco4", (3, 4, 1), (4, 64, 64), 4, 480, plan={"ksplit": 0}, sw=""),
    wg_case("wg_np5_nco1", (5, 1, 1), S3, 64, 4, k=1, sw="dbias prev"),
    wg_case("wg_np5_nco2_stride2", (5, 2, 1), S3, 256, 480, s=2, plan={"ksplit": 0, "gz": 8}, sw="rep"),
    wg_case("wg_np7_nco1", (7, 1, 1), S3, 256, 96, plan={"ksplit": 0, "gz": 6}, sw="dbias relu_in"),
    wg_case("wg_np7_nco2", (7, 2, 1), (4, 64, 64), 72, 48, plan={"gx": 64}),
    wg_case("wg_np8_nco1_k1", (8, 1, 1), S3, 256, 480, k=1, plan={"ksplit": 1, "gz": 2}, sw="dbias kappa"),
    wg_case("wg_np8_nco2_ppg32", (8, 2, 1), (4, 64, 64), 104, 48, plan={"PPG": 32, "gz": 2, "ksplit": 0}),
    wg_case("wg_np9_nco1", (9, 1, 1), S3, 4, 4, plan={"ksplit": 1, "gz": 1}, sw="dbias kappa aff relu_in rep prev"),
    wg_case("wg_np9_nco2", (9, 2, 1), S3, 136, 112, plan={"ksplit": 1, "gz": 9}, sw="aff relu_in"),
    # the same kernels finished by atomics (no workspace), one per NP
    wg_case("wg_np3_atomics", (3, 1, 1), S3, 4, 4, k=1, ws=False, plan={"slab": 0}),
    wg_case("wg_np5_atomics", (5, 1, 1), S3, 64, 4, k=1, ws=False, plan={"slab": 0}, sw="prev"),
    wg_case("wg_np7_atomics", (7, 1, 1), S3, 256, 96, ws=False, plan={"slab": 0}, sw="dbias kappa"),
    wg_case("wg_np8_atomics", (8, 1, 1), S3, 256, 480, k=1, ws=False, plan={"slab": 0}),
    wg_case("wg_np9_atomics", (9, 1, 1), S3, 4, 4, ws=False, plan={"slab": 0}, sw="dbias rep prev"),
    wg_case("wg_atomics_large", (9, 1, 1), (4, 64, 64), 4, 4, ws=False, plan={"slab": 0, "gx": 64}),
    # the non-lean staging path through each cause, one per NP
    wg_case("wg_np9_dy_off2", (9, 1, 0), S3, 4, 4, dy=seg(4, 8, 2), sw="dbias rep"),
    wg_case("wg_np3_cin6", (3, 1, 0), S3, 6, 4, k=1),
    wg_case("wg_np5_cout6", (5, 1, 0), S3, 64, 6, k=1, sw="dbias kappa"),
    wg_case("wg_np7_cin254", (7, 1, 0), S3, 254, 96, sw="aff relu_in"),
    wg_case("wg_np8_dy_off2", (8, 1, 0), S3, 256, 480, k=1, dy=seg(480, 484, 2), ws=False, plan={"slab": 0}),
    wg_case("wg_in_off2_stride2", (9, 1, 0), S3, 8, 8, s=2, ins=[seg(8, 12, 2)], sw="dbias prev"),
    # plan edges
    wg_case("wg_ppg_rebalanced", (5, 1, 1), (2, 32, 32), 104, 124, plan={"PPG": 16, "ksplit": 0, "gz": 4}),
    wg_case("wg_gx_two_chunks", (9, 1, 1), (4, 64, 64), 4, 4, plan={"gx": 64, "slab": 1}),
    wg_case("wg_gx1", (9, 1, 1), (1, 1, 7), 4, 4, s=2, plan={"gx": 1}),
    wg_case("wg_mpix128", (5, 1, 1), (16, 128, 128), 20, 4, plan={"MPIX": 128}),
    wg_case("wg_mpix256", (9, 1, 1), (16, 128, 128), 4, 4, plan={"MPIX": 256}, sw="dbias rep"),
    wg_case("wg_stride2_odd", (9, 1, 1), (3, 13, 9), 8, 8, s=2, sw="dbias rep aff"),
    wg_case("wg_k1_stride2", (3, 1, 1), (3, 13, 10), 8, 8, k=1, s=2),
    wg_case("wg_in3", (9, 1, 1), S3, 16, 8, ins=[seg(8), seg(4, 12, 4), seg(4, 8, 4)], sw="dbias relu_in"),
    # destination layouts: 8 source channels into rows of 14 at offset 3; 6 valid of 8 split 2 | 4 at offsets 1 and 5
    wg_case("wg_cin_dst_off0", (9, 1, 1), S3, 8, 8, layout=(14, 8, 0, 3, 0), sw="dbias prev"),
    wg_case("wg_ci_split_off1", (9, 1, 1), S3, 8, 8, layout=(14, 6, 2, 1, 5), sw=""),
    wg_case("wg_ci_split_off1_atomics", (9, 1, 1), S3, 8, 8, layout=(14, 6, 2, 1, 5), ws=False, plan={"slab": 0}, sw="kappa"),
]
# every (NP, NCO) on the non-lean staging path too: the 11 instance cases above with dy as a channel slice at offset 2
for _c in list(WG_CASES[:11]):
    _n = dict(_c, name=_c["name"] + "_nonlean", want=_c["want"][:2] + (0,), dy=seg(_c["cout"], _c["cout"] + 4, 2))
    WG_CASES.append(_n)
WG_BY_NAME = {c["name"]: c for c in WG_CASES}
assert len(WG_BY_NAME) == len(WG_CASES)
WG_INSTANCES = tuple((np_, nco) for np_ in (3, 5, 7, 8, 9) for nco in (1, 2)) + ((3, 4),)


def wg_instance(p):
    return (p["NP"], p["NCO"], p["LEAN"])


def wg_args(case):
    B, Hh, Ww = case["shape"]
    Ho, Wo = out_hw(Hh, Ww, case["s"])
    sw = case["sw"]
    cd, cv, cs, o0, o1 = case["layout"]
    ins = [descr((B, Hh, Ww), sp, i) for i, sp in enumerate(case["ins"])]
    kw = dict(dbias="dbias" in sw, kappa="kappa" in sw, in_scale="aff" in sw, in_shift="aff" in sw, relu_in="relu_in" in sw,
              pad_rep="rep" in sw, use_ws=case["ws"], cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    return ins, descr((B, Ho, Wo), case["dy"], 4), case["k"], case["s"], kw


def wg_plan(Hm, case):
    ins, dy, k, s, kw = wg_args(case)
    p = Hm.conv_wgrad_plan(ins, dy, k, s, **kw)
    assert _matches(p, case["want"], wg_instance, case["plan"]), "%s: wanted %s %s, planned %s" % (case["name"], case["want"], case["plan"], p)
    return p


def wino_routed(Hm, case, mode):
    """Whether tmg_hip.conv_wgrad would try the Winograd kernel for the operands this case passes in this data mode (integer mode
    passes no kappa), by the wrapper's own thresholds.  test_conv_kernels also replaces conv_wino_wgrad by a function that fails."""
    B, Hh, Ww = case["shape"]
    kappa = "kappa" in case["sw"] and mode != "int"
    return (case["k"] == 3 and case["s"] == 1 and not kappa and "aff" not in case["sw"] and case["ws"] and case["cin"] >= 32
            and (case["cout"] >= 128 or (case["cout"] >= 32 and case["cin"] >= Hm._WINO_WGRAD_CIN_MIN
                                         and B * Hh * Ww >= Hm._WINO_WGRAD_PIX_MIN)))


# ---------------------------------------------------------------------------------------------------------------------------------
# replicate-border cases: (name, want (mfma, NT), (B, H, W), Cdy, outs, dy spec, plan extras, kappa)
# ---------------------------------------------------------------------------------------------------------------------------------
def bd_case(name, want, shape, cdy, outs, dy=None, plan=None, kappa=False):
    return dict(name=name, want=tuple(want), shape=shape, cdy=cdy, outs=outs, dy=dy or seg(cdy), plan=plan or {}, kappa=kappa,
                K=9 * cdy, gauss=9 * cdy <= KMAX_GAUSS)


BD_CASES = [bd_case("bd_nt%d" % nt, (1, nt), (2, 6, 9), 16, [seg(16 * nt - 4)], plan={"S": 1}) for nt in range(1, 9)] + [
    bd_case("bd_split_k", (1, 2), (1, 4, 5), 192, [seg(32)], plan={"S": 3}),
    bd_case("bd_split_k_kappa", (1, 1), (2, 3, 3), 128, [seg(16)], plan={"S": 2}, kappa=True),
    bd_case("bd_h2_w2", (1, 1), (3, 2, 2), 16, [seg(16)]),          # no edge pixels: four classes with a zero count
    bd_case("bd_h2", (1, 1), (2, 2, 7), 16, [seg(8)]),
    bd_case("bd_w3", (1, 1), (2, 9, 3), 24, [seg(12)], kappa=True),
    bd_case("bd_h3_w2", (1, 2), (2, 3, 2), 16, [seg(20)]),
    bd_case("bd_scalar_h1", (0, 0), (2, 1, 9), 16, [seg(16)]),
    bd_case("bd_scalar_w1", (0, 0), (2, 7, 1), 16, [seg(8)], kappa=True),
    bd_case("bd_scalar_1x1", (0, 0), (3, 1, 1), 8, [seg(8)]),
    bd_case("bd_scalar_dy_misaligned", (0, 0), (2, 5, 6), 16, [seg(16)], dy=seg(16, 16, 0, 1)),
    bd_case("bd_scalar_dy_off2", (0, 0), (2, 5, 6), 12, [seg(16)], dy=seg(12, 16, 2)),
    bd_case("bd_scalar_cx136", (0, 0), (1, 4, 5), 16, [seg(136)]),
    bd_case("bd_scalar_cx6", (0, 0), (2, 4, 5), 10, [seg(6)]),
    bd_case("bd_out2", (1, 2), (2, 6, 9), 16, [seg(12), seg(8, 16, 4)]),
    bd_case("bd_out3_kappa", (1, 3), (2, 6, 9), 32, [seg(16), seg(8, 16, 4), seg(16, 24, 8)], kappa=True),
    # 5 images x 6 edge pixels = 30: the second 16-row tile of the edge classes holds 14 rows; corners 5 of 16
    bd_case("bd_partial_tile", (1, 1), (5, 8, 8), 16, [seg(16)], plan={"S": 1}),
]
BD_BY_NAME = {c["name"]: c for c in BD_CASES}
assert len(BD_BY_NAME) == len(BD_CASES)


def bd_args(case):
    B, Hh, Ww = case["shape"]
    return descr((B, Hh, Ww), case["dy"], 0), [descr((B, Hh, Ww), sp, 4 + i) for i, sp in enumerate(case["outs"])]


def bd_plan(Hm, case):
    dy, outs = bd_args(case)
    p = Hm.conv_rep_border_plan(dy, outs)
    assert _matches(p, case["want"], lambda q: (q["mfma"], q["NT"]), case["plan"]), "%s: wanted %s %s, planned %s" % (
        case["name"], case["want"], case["plan"], p)
    return p


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, shape, mode, amp=3):
    """fp64 tensor of fp32-representable values: integers in [-amp, amp] or Gaussians rounded to fp32."""
    if mode == "int":
        return torch.randint(-amp, amp + 1, shape, generator=g).double()
    return torch.randn(shape, generator=g, dtype=torch.float32).double()


def affine(g, cin, mode):
    if mode == "int":
        sc = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (cin,), generator=g)]
        return sc, torch.randint(-2, 3, (cin,), generator=g).double()
    return (0.5 + torch.rand(cin, generator=g, dtype=torch.float32)).double(), (0.3 * torch.randn(cin, generator=g, dtype=torch.float32)).double()


def osc_of(kappa):
    """out_scale_of: exp(clamp(kappa, -4, ln 4)) in fp64 of the fp32 kappa."""
    return math.exp(min(max(float(kappa), -4.0), LOG4))


def fwd_data(case, B, mode, seed=0):
    g = _gen(1000 + seed)
    Hh, Ww = case["hw"]
    Ho, Wo = out_hw(Hh, Ww, case["s"])
    cin, cout, k, sw = sum(i[0] for i in case["ins"]), sum(o[0] for o in case["outs"]), case["k"], case["sw"]
    d = dict(x=rnd(g, (B, Hh, Ww, cin), mode), w=rnd(g, (cout, cin, k, k), mode, 2), bias=None, add=None, prev=None, scale=None,
             shift=None, kappa=None)
    if "bias" in sw:
        d["bias"] = rnd(g, (cout,), mode, 8)
    if "add" in sw:
        d["add"] = rnd(g, (B, Ho, Wo, cout), mode, 8)
    if "acc" in sw:
        d["prev"] = rnd(g, (B, Ho, Wo, cout), mode, 8)
    if "aff" in sw:
        d["scale"], d["shift"] = affine(g, cin, mode)
    if "kappa" in sw and mode != "int":          # integer mode: no kappa (exp is not exact)
        d["kappa"] = float(torch.tensor(0.37, dtype=torch.float32))
    return d


def prep_input(x, scale, shift, relu_in, pad_rep, k):
    """NHWC fp64 -> (operand, magnitude), padded NCHW: affine, then ReLU, then padding (zero padding is not touched by the affine).
    The magnitude of an operand element is the sum of the absolute values of ITS terms: |x| |scale| + |shift|."""
    xp = x.permute(0, 3, 1, 2)
    xa = xp.abs()
    if scale is not None:
        xp = xp * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        xa = xa * scale.abs().view(1, -1, 1, 1) + shift.abs().view(1, -1, 1, 1)
    if relu_in:
        xp = xp.clamp(min=0)
    h = k // 2
    if h:
        xp = F.pad(xp, (h, h, h, h), mode="replicate" if pad_rep else "constant")
        xa = F.pad(xa, (h, h, h, h), mode="replicate" if pad_rep else "constant")
    return xp, xa


def fwd_ref(case, d, fault=None):
    """(ref, S) NHWC fp64: out = [relu]((conv + add + bias) osc) (+ previous contents); S the sum of the absolute terms.
    fault: ("tap", ci, ky, kx) one (tap, channel) product dropped; ("chunk", c0, c1) input channels [c0, c1) dropped;
    ("quad", q) output channels 4q .. 4q + 3 take the values of the next quad."""
    sw, k, s = case["sw"], case["k"], case["s"]
    xp, xa = prep_input(d["x"], d["scale"], d["shift"], "relu_in" in sw, "rep" in sw, k)
    w = d["w"]
    if fault and fault[0] == "tap":
        w = w.clone()
        w[:, fault[1], fault[2], fault[3]] = 0
    if fault and fault[0] == "chunk":
        w = w.clone()
        w[:, fault[1]:fault[2]] = 0
    y = F.conv2d(xp, w, stride=s).permute(0, 2, 3, 1)
    S = F.conv2d(xa, d["w"].abs(), stride=s).permute(0, 2, 3, 1)
    osc = osc_of(d["kappa"]) if d["kappa"] is not None else 1.0
    if d["add"] is not None:
        y, S = y + d["add"], S + d["add"].abs()
    if d["bias"] is not None:
        y, S = y + d["bias"], S + d["bias"].abs()
    y, S = y * osc, S * osc
    if "relu_out" in sw:
        y = y.clamp(min=0)
    if d["prev"] is not None:
        y, S = y + d["prev"], S + d["prev"].abs()
    if fault and fault[0] == "quad":
        q = fault[1]
        y = y.clone()
        y[..., 4 * q:4 * q + 4] = y[..., 4 * q + 4:4 * q + 8]
    return y.contiguous(), S.contiguous()


def wg_data(case, mode, seed=0):
    g = _gen(2000 + seed)
    B, Hh, Ww = case["shape"]
    Ho, Wo = out_hw(Hh, Ww, case["s"])
    cin, cout, k, sw = case["cin"], case["cout"], case["k"], case["sw"]
    big = B * Ho * Wo > 65536      # keep the sums of the absolute terms below 2^24
    d = dict(x=rnd(g, (B, Hh, Ww, cin), mode, 2 if big else 3), dy=rnd(g, (B, Ho, Wo, cout), mode, 2 if big else 3), scale=None,
             shift=None, kappa=None, prevW=None, prevb=None)
    if "aff" in sw:
        d["scale"], d["shift"] = affine(g, cin, mode)
    if "kappa" in sw and mode != "int":
        d["kappa"] = float(torch.tensor(-0.61, dtype=torch.float32))
    cd = case["layout"][0] or cin
    if "prev" in sw:
        d["prevW"] = rnd(g, (cout, cd, k * k), mode, 8)
        d["prevb"] = rnd(g, (cout,), mode, 8)
    return d


def wg_dense(xp, dy, k, s):
    """dW[co][ci][ky][kx] = sum_p xp(p s + tap)[ci] dy(p)[co]; xp padded NCHW, dy NHWC."""
    B, Ho, Wo, cout = dy.shape
    dyn = dy.permute(0, 3, 1, 2)
    out = torch.zeros(cout, xp.shape[1], k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s]
            out[:, :, ky, kx] = torch.einsum("bchw,bohw->oc", xs, dyn)
    return out


def wg_scatter(case, dense, prev, osc, off1_fault=False):
    cin, cout, k = case["cin"], case["cout"], case["k"]
    cd, cv, cs, o0, o1 = case["layout"]
    cd = cd or cin
    cv = cv or min(cd, cin)
    cs = cs or 0x7fffffff
    out = prev.clone() if prev is not None else torch.zeros(cout, cd, k * k, dtype=torch.float64)
    touched = torch.zeros(cd, dtype=torch.bool)
    for ci in range(cv):
        dst = ci + (o0 if ci < cs else (0 if off1_fault else o1))
        out[:, dst] += dense[:, ci].reshape(cout, k * k) * osc
        touched[dst] = True
    return out, touched


def wg_ref(case, d, fault=None):
    """(dW, S_dW, dbias, S_dbias, touched columns) fp64.  fault: ("unit16", b, y, x0) the 16 pixels x0 .. x0 + 15 of row y of image b
    dropped from the sum; ("off1",) the ci_off1 term of the destination column dropped."""
    sw, k, s = case["sw"], case["k"], case["s"]
    xp, xa = prep_input(d["x"], d["scale"], d["shift"], "relu_in" in sw, "rep" in sw, k)
    dy = d["dy"]
    dyf = dy
    if fault and fault[0] == "unit16":
        dyf = dy.clone()
        dyf[fault[1], fault[2], fault[3]:fault[3] + 16] = 0
    osc = osc_of(d["kappa"]) if d["kappa"] is not None else 1.0
    dense, dabs = wg_dense(xp, dyf, k, s), wg_dense(xa, dy.abs(), k, s)
    dW, touched = wg_scatter(case, dense, d["prevW"], osc, bool(fault and fault[0] == "off1"))
    SW, _ = wg_scatter(case, dabs, d["prevW"].abs() if d["prevW"] is not None else None, osc)
    db = dyf.sum((0, 1, 2)) * osc + (d["prevb"] if d["prevb"] is not None else 0)
    Sb = dy.abs().sum((0, 1, 2)) * osc + (d["prevb"].abs() if d["prevb"] is not None else 0)
    return dW, SW, db, Sb, touched


def bd_data(case, mode, seed=0):
    g = _gen(3000 + seed)
    B, Hh, Ww = case["shape"]
    cx = sum(o[0] for o in case["outs"])
    return dict(dy=rnd(g, (B, Hh, Ww, case["cdy"]), mode), w=rnd(g, (case["cdy"], cx, 3, 3), mode, 2), prev=rnd(g, (B, Hh, Ww, cx), mode, 8),
                kappa=float(torch.tensor(0.21, dtype=torch.float32)) if case["kappa"] and mode != "int" else None)


def _dx_of(dy, w, Hh, Ww, pad_mode):
    x = torch.zeros(dy.shape[0], w.shape[1], Hh, Ww, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode=pad_mode), w)
    y.backward(dy.permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1)


def bd_ref(case, d, fault=None):
    """(ref, S): previous contents + osc (input gradient of the replicate-padded 3x3 conv - that of the zero-padded one): the kernel
    ADDS the fold (conv_rep_border_fix_kernel: *dst += acc * osc).  fault "corners": the four corner pixels get no fold."""
    B, Hh, Ww = case["shape"]
    osc = osc_of(d["kappa"]) if d["kappa"] is not None else 1.0
    fold = _dx_of(d["dy"], d["w"], Hh, Ww, "replicate") - _dx_of(d["dy"], d["w"], Hh, Ww, "constant")
    fabs = _dx_of(d["dy"].abs(), d["w"].abs(), Hh, Ww, "replicate") - _dx_of(d["dy"].abs(), d["w"].abs(), Hh, Ww, "constant")
    if fault == "corners":
        fold = fold.clone()
        for y in (0, Hh - 1):
            for x in (0, Ww - 1):
                fold[:, y, x] = 0
    return d["prev"] + fold * osc, d["prev"].abs() + fabs * osc


def dgrad_ref(dy, w, shape_in, k, s):
    """(dx, S) NHWC fp64 of conv_transpose2d semantics: the input gradient of conv2d(x, w, stride s, padding k // 2)."""
    B, Hin, Win, cin = shape_in

    def one(dy_, w_):
        x = torch.zeros(B, cin, Hin, Win, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w_, stride=s, padding=k // 2).backward(dy_.permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous()
    return one(dy, w), one(dy.abs(), w.abs())


def pack_ref(w, mode, cin_eff=0, cmap=None):
    """The documented layout, from the comment above conv_pack_kernel: wpk[tap][K_pad / 16][N_pad][16];
    mode 0: K = operand input channels (cin_eff), N = Cout: wpk[tap][c / 16][n][c % 16] = W[n][src(c)][tap];
    mode 1: K = Cout, N = operand input channels: wpk[tap][co / 16][c][co % 16] = W[co][src(c)][ntaps - 1 - tap];
    src(c) = c (+ cgap when c >= csplit) for c < cvalid, zero beyond; every padding entry zero."""
    cout, cin, k, _ = w.shape
    nt = k * k
    ce = int(cin_eff) if cmap is not None else max(int(cin_eff), cin)
    cvalid, csplit, cgap = cmap if cmap is not None else (cin, 0x7fffffff, 0)
    K, N = (ce, cout) if mode == 0 else (cout, ce)
    Kp, Np = (K + 15) // 16 * 16, (N + 15) // 16 * 16
    out = torch.zeros(nt, Kp // 16, Np, 16, dtype=w.dtype)
    wf = w.reshape(cout, cin, nt)
    for c in range(min(cvalid, ce)):
        src = c + (cgap if c >= csplit else 0)
        for tap in range(nt):
            if mode == 0:
                out[tap, c // 16, :cout, c % 16] = wf[:, src, tap]
            else:
                col = wf[:, src, nt - 1 - tap]
                for co in range(cout):
                    out[tap, co // 16, c, co % 16] = col[co]
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# measures
# ---------------------------------------------------------------------------------------------------------------------------------
def int_terms_ok(S, gran=1.0):
    """The condition of the integer mode: sum |terms| / granularity < 2^24 everywhere."""
    return float(S.max()) / gran < 2.0 ** 24


def gran_of(d):
    return 0.5 if d.get("scale") is not None else 1.0


def bit_equal(a, ref):
    """fp32 result == fp64 reference exactly (NaN never equal)."""
    a = a.detach().cpu().double()
    return a.shape == ref.shape and bool((a == ref).all())


def gauss_share(a, ref, S, K):
    """max_i |a_i - ref_i| / ((K + 8) u S_i): <= 1 passes.  Elements with S_i = 0 must be exact; NaN is infinite."""
    a = a.detach().cpu().double()
    assert a.shape == ref.shape == S.shape, (a.shape, ref.shape, S.shape)
    if a.numel() == 0:
        return 0.0
    dlt = (a - ref).abs()
    if bool(torch.isnan(dlt).any()):
        return math.inf
    bound = (K + 8) * U24 * S
    r = torch.where(bound > 0, dlt / bound.clamp(min=1e-300), torch.where(dlt > 0, torch.full_like(dlt, math.inf), torch.zeros_like(dlt)))
    return float(r.max())


def affected_shares(ref_fault, ref, S, K):
    """Per affected element (faulted reference != reference): |fault_i - ref_i| / ((K + 8) u S_i)."""
    m = ref_fault != ref
    return (ref_fault - ref).abs()[m] / ((K + 8) * U24 * S[m])
