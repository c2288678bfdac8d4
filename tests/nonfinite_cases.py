"""Non-finite inputs ("Non-finite values"): the poison table, the judge of the three rules, the Winograd footprint and the
case list, shared by test_nonfinite_cpu.py (the references and the judge; no device) and test_nonfinite_gpu.py (the kernels).

A case poisons ONE element (of an activation, or of one parameter) of the data its home file already builds, with NaN, +Inf or -Inf,
and hands back the fp64 reference R of the home file on the poisoned data next to the bound of the home file on the CLEAN data:
  rule 1  wherever R is NaN / +-Inf the library's output A is NaN / +-Inf (which of them does not matter);
  rule 2  wherever R is finite A is finite and within the home file's bound (clean data); the Winograd kernels alone may be
          non-finite on the 2x2 output tiles whose 4x4 input patch holds the poisoned pixel (wino_footprint: at most 16 pixels);
  rule 3  everything outside the output views stays NaN (the device file checks it).
No reference is built here: conv_cases / wino_cases / the formulas of the home test files are called as they are.  Two refinements,
both stated in DESIGN.md: where a reference is non-finite only through a STRUCTURAL ZERO (0 * NaN at the zero taps of a derivative
stencil, in a fold formed as a difference, at the masked-out entries of l and u) the same formula on an indicator of the poisoned
element names the elements that do depend on it and the clean reference stands elsewhere; and where the poison leaves the reference
finite by design (+-Inf behind a clamp) the bound comes from the poisoned data, whose scales are finite.

A case is a dict (family, name, entry points, poison labels, build); build(label, tmg_hip) returns the run: the poisoned inputs `d`, the
references `R`, the bounds, `allowed` (the Winograd footprint), `expect` (the geometric non-finite set, `exact` when R must equal it),
`finite` (R must stay finite), `glob` (no finite element is required), `trips` and `mutated` (the reference as the kernels behaved
before: it must trip rule 1).

A poison label is "<target>.<placement>.<value>": target x (an activation), dy, kappa, w (one weight), gamma (one in_scale entry), g
(one gradient element); placement a (a channel inside a float4 body), b (the last channel of a segment whose width is no multiple of 4:
the scalar tail), c (a corner pixel under replicate padding: the halo reads it three more times), d (a channel of the second input
segment), p (the one entry of a parameter)."""
import math

import torch
import torch.nn.functional as F

import conv_cases as CC
import wino_cases as WC

NAN, INF = float("nan"), float("inf")
POISONS = {"nan": NAN, "pinf": INF, "ninf": -INF}


def nonfinite(t):
    return ~torch.isfinite(t)


# ---------------------------------------------------------------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------------------------------------------------------------
def verdict(A, R, bound, allowed=None):
    """Counts of one output: swallowed (rule 1: R non-finite, A finite), leaked (rule 2: R finite, A non-finite, outside `allowed`),
    off (rule 2: both finite, |A - R| above `bound`, outside `allowed`) and the worst share of the bound.  bound: fp64 tensor or float,
    absolute, per element; an element with bound 0 must be exact."""
    A = A.detach().cpu().double()
    R = R.detach().double()
    assert A.shape == R.shape, (A.shape, R.shape)
    nfR, nfA = nonfinite(R), nonfinite(A)
    free = allowed if allowed is not None else torch.zeros_like(nfR)
    free = free.expand_as(nfR) if free.shape != nfR.shape else free
    both = ~nfR & ~nfA & ~free
    b = bound if torch.is_tensor(bound) else torch.full_like(R, float(bound))
    dlt = torch.where(both, (A - R).abs(), torch.zeros_like(R))
    bb = torch.where(both, b.expand_as(R), torch.ones_like(R))
    share = torch.where(bb > 0, dlt / bb.clamp(min=1e-300), torch.where(dlt > 0, torch.full_like(dlt, INF), torch.zeros_like(dlt)))
    return dict(swallowed=int((nfR & ~nfA).sum()), leaked=int((~nfR & nfA & ~free).sum()), off=int((share > 1).sum()),
                share=float(share.max()) if share.numel() else 0.0, nonfinite_ref=int(nfR.sum()), finite_ref=int((~nfR).sum()))


def judge(run, got):
    """Every output of a run under rules 1 and 2 -> {output: verdict}; `got` maps the run's output names to the library's tensors."""
    out = {}
    for name, R in run["R"].items():
        out[name] = verdict(got[name], R, run["bound"][name], run.get("allowed", {}).get(name))
    return out


def failures(verdicts):
    return ["%s: swallowed %d, leaked %d, off %d (share %.3g)" % (n, v["swallowed"], v["leaked"], v["off"], v["share"])
            for n, v in verdicts.items() if v["swallowed"] or v["leaked"] or v["off"]]


def assert_not_vacuous(run):
    """The run's reference has a non-finite element (unless it is one the poison cannot reach: -Inf behind a ReLU, run["finite"]),
    and, unless the operation is global, a finite one."""
    nf = sum(int(nonfinite(R).sum()) for R in run["R"].values())
    fin = sum(int(torch.isfinite(R).sum()) for R in run["R"].values())
    if run.get("finite"):
        assert nf == 0, "the reference was expected to stay finite"
    else:
        assert nf > 0, "vacuous: the reference has no non-finite element"
    if not run.get("glob"):
        assert fin > 0, "vacuous: the reference has no finite element"


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_reach(shape3, pix, k, s, pad_rep):
    """(B, Ho, Wo) bool: the outputs of a k x k stride-s convolution (padding k // 2, zero or replicate) that read input pixel pix."""
    B, Hh, Ww = shape3
    ind = torch.zeros(B, 1, Hh, Ww, dtype=torch.float64)
    ind[pix[0], 0, pix[1], pix[2]] = 1
    h = k // 2
    if h:
        ind = F.pad(ind, (h, h, h, h), mode="replicate" if pad_rep else "constant")
    return F.conv2d(ind, torch.ones(1, 1, k, k, dtype=torch.float64), stride=s)[:, 0] > 0


def wino_footprint(shape3, pix, pad_rep):
    """(B, H, W) bool: every pixel of the 2x2 output tiles whose 4x4 input patch (rows 2 ty - 1 .. 2 ty + 2, clamped to the image under
    replicate padding, zero outside it otherwise) holds input pixel pix.  The input transform B^T d B mixes the whole patch, so a
    non-finite pixel may reach all four outputs of such a tile: the one exception of rule 2."""
    B, Hh, Ww = shape3
    b, py, px = pix
    m = torch.zeros(B, Hh, Ww, dtype=torch.bool)

    def holds(t, n, q):
        rows = range(2 * t - 1, 2 * t + 3)
        return any((min(max(r, 0), n - 1) if pad_rep else r) == q for r in rows)
    for ty in range((Hh + 1) // 2):
        for tx in range((Ww + 1) // 2):
            if holds(ty, Hh, py) and holds(tx, Ww, px):
                m[b, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2] = True
    return m


WINO_FOOTPRINT_CAP = 16


def wg_taps(shape3, pix, k, s, pad_rep):
    """(k * k) bool: the taps of a weight gradient whose sum reads input pixel pix (some output pixel sees it through that tap)."""
    _, Hh, Ww = shape3
    Ho, Wo = CC.out_hw(Hh, Ww, s)

    def reads(n, no, q, t):
        for o in range(no):
            i = o * s + t - k // 2
            if (min(max(i, 0), n - 1) if pad_rep else i) == q:
                return True
        return False
    return torch.tensor([reads(Hh, Ho, pix[1], ky) and reads(Ww, Wo, pix[2], kx) for ky in range(k) for kx in range(k)])


# ---------------------------------------------------------------------------------------------------------------------------------
# placements
# ---------------------------------------------------------------------------------------------------------------------------------
def placements(segs, shape3, pad_rep):
    """{placement: (b, y, x, concatenated channel)} of an activation made of the segment specs `segs` (conv_cases.seg)."""
    B, Hh, Ww = shape3
    out = {"a": (0, Hh // 2, Ww // 2, min(1, segs[0][0] - 1))}
    c0 = 0
    for n, _, _, _ in segs:
        if n % 4 and n > 4:
            out["b"] = (B - 1, Hh // 2, max(Ww // 2 - 1, 0), c0 + n - 1)
            break
        c0 += n
    if pad_rep:
        out["c"] = (B - 1, 0, 0, min(2, segs[0][0] - 1))
    if len(segs) > 1:
        out["d"] = (0, min(1, Hh - 1), min(1, Ww - 1), segs[0][0] + min(1, segs[1][0] - 1))
    return out


def _poisoned(t, idx, value):
    t = t.clone()
    t[idx] = value
    return t


def _label(target, place, value):
    return "%s.%s.%s" % (target, place, value)


def _parse(label):
    target, place, value = label.split(".")
    return target, place, POISONS[value]


def _trips(target, value, sw):
    """Whether a reference mutated the way the kernels behaved (fmaxf / fminf) must trip rule 1 under this poison."""
    return math.isnan(value) and ((target == "x" and "relu_in" in sw) or target == "kappa")


def _case(family, name, entry, labels, build, sites, glob=()):
    """entry: the tmg_hip wrappers the case launches; sites: which of today's swallowing forms its data path holds (relu, clamp, vmax,
    std, mask) - the mutated references of test_nonfinite_cpu.py must trip rule 1 on every case that names one; glob: the labels under
    which the operation is global (every output element depends on the poisoned one)."""
    return dict(family=family, name=name, entry=tuple(entry), labels=tuple(labels), build=build, sites=tuple(sites), glob=tuple(glob))


CASES = []


# ---------------------------------------------------------------------------------------------------------------------------------
# direct convolutions (conv_cases.py, test_conv_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def _osc(kappa, mutate):
    if kappa is None:
        return 1.0
    if mutate and math.isnan(kappa):
        kappa = -4.0                       # fminf(fmaxf(nan, -4), ln 4)
    return CC.osc_of(kappa)


def _mut_relu(t):
    return torch.where(torch.isnan(t), torch.zeros_like(t), t.clamp(min=0))


def conv_fwd_ref_mutated(case, d):
    """conv_cases.fwd_ref with the ReLUs and the kappa clamp as the kernels had them (fmaxf / fminf: NaN -> 0 / the lower limit)."""
    sw, k, s = case["sw"], case["k"], case["s"]
    xp = d["x"].permute(0, 3, 1, 2)
    if d["scale"] is not None:
        xp = xp * d["scale"].view(1, -1, 1, 1) + d["shift"].view(1, -1, 1, 1)
    if "relu_in" in sw:
        xp = _mut_relu(xp)
    if k // 2:
        xp = F.pad(xp, (k // 2,) * 4, mode="replicate" if "rep" in sw else "constant")
    y = F.conv2d(xp, d["w"], stride=s).permute(0, 2, 3, 1)
    if d["add"] is not None:
        y = y + d["add"]
    if d["bias"] is not None:
        y = y + d["bias"]
    y = y * _osc(d["kappa"], True)
    if "relu_out" in sw:
        y = _mut_relu(y)
    if d["prev"] is not None:
        y = y + d["prev"]
    return y.contiguous()


def _conv_fwd_labels(case):
    sw = case["sw"]
    places = placements(case["ins"], (2,) + tuple(case["hw"]), "rep" in sw)
    labels = [_label("x", p, v) for p in places for v in POISONS]
    labels.append("w.p.nan")
    if "kappa" in sw:
        labels.append("kappa.p.nan")
    if "aff" in sw:
        labels.append("gamma.p.nan")
    return labels


def build_conv_fwd(case, label, H):
    """H: tmg_hip (its planner names the batch that lands on the case's kernel instance; no device is needed for that)."""
    target, place, value = _parse(label)
    B, _ = CC.resolve_fwd(H, case)
    Hh, Ww = case["hw"]
    sw, k, s = case["sw"], case["k"], case["s"]
    clean = CC.fwd_data(case, B, "gauss")
    _, S = CC.fwd_ref(case, clean)
    d = dict(clean)
    Ho, Wo = CC.out_hw(Hh, Ww, s)
    cout = clean["w"].shape[0]
    expect, finite = None, False
    if target == "x":
        idx = placements(case["ins"], (B, Hh, Ww), "rep" in sw)[place]
        d["x"] = _poisoned(clean["x"], idx, value)
        expect = conv_reach((B, Hh, Ww), idx[:3], k, s, "rep" in sw).unsqueeze(-1).expand(B, Ho, Wo, cout)
        finite = value == -INF and "relu_in" in sw and (clean["scale"] is None or float(clean["scale"][idx[3]]) > 0)
    elif target == "w":
        d["w"] = _poisoned(clean["w"], (1, 1, k // 2, k // 2), value)
        expect = torch.zeros(B, Ho, Wo, cout, dtype=torch.bool)
        expect[..., 1] = True
    elif target == "kappa":
        d["kappa"] = value
        expect = torch.ones(B, Ho, Wo, cout, dtype=torch.bool)
    elif target == "gamma":
        d["scale"] = _poisoned(clean["scale"], (1,), value)
        expect = torch.ones(B, Ho, Wo, 1, dtype=torch.bool).expand(B, Ho, Wo, cout)
    R, _ = CC.fwd_ref(case, d)
    return dict(d=d, B=B, R={"out": R}, bound={"out": (case["K"] + 8) * CC.U24 * S}, expect={"out": expect}, exact=math.isnan(value),
                finite=finite, glob=target in ("kappa", "gamma"), trips=_trips(target, value, sw), mutated=lambda: {"out": conv_fwd_ref_mutated(case, d)})


for _n in ("lean_all_switches", "fb_out3_in3", "lean_k1_all", "fb_stride2_odd"):
    _c = CC.FWD_BY_NAME[_n]
    CASES.append(_case("conv_fwd", _n, ["conv_fwd"], _conv_fwd_labels(_c), (lambda c: lambda label, H: build_conv_fwd(c, label, H))(_c),
                       ["relu"] + (["clamp"] if "kappa" in _c["sw"] else [])))


def conv_wg_ref_mutated(case, d):
    sw, k, s = case["sw"], case["k"], case["s"]
    xp = d["x"].permute(0, 3, 1, 2)
    if d["scale"] is not None:
        xp = xp * d["scale"].view(1, -1, 1, 1) + d["shift"].view(1, -1, 1, 1)
    if "relu_in" in sw:
        xp = _mut_relu(xp)
    if k // 2:
        xp = F.pad(xp, (k // 2,) * 4, mode="replicate" if "rep" in sw else "constant")
    osc = _osc(d["kappa"], True)
    dW, _ = CC.wg_scatter(case, CC.wg_dense(xp, d["dy"], k, s), d["prevW"], osc)
    db = d["dy"].sum((0, 1, 2)) * osc + (d["prevb"] if d["prevb"] is not None else 0)
    return dW, db


def build_conv_wgrad(case, label, H):
    target, place, value = _parse(label)
    B, Hh, Ww = case["shape"]
    sw, k, cin, cout = case["sw"], case["k"], case["cin"], case["cout"]
    clean = CC.wg_data(case, "gauss")
    _, SW, _, Sb, _ = CC.wg_ref(case, clean)
    d = dict(clean)
    eW = torch.zeros(cout, case["layout"][0] or cin, k * k, dtype=torch.bool)
    eb = torch.zeros(cout, dtype=torch.bool)
    finite = False
    if target == "x":
        idx = placements(case["ins"], (B, Hh, Ww), "rep" in sw)[place]
        d["x"] = _poisoned(clean["x"], idx, value)
        eW[:, idx[3]] = wg_taps((B, Hh, Ww), idx[:3], k, case["s"], "rep" in sw)
        finite = value == -INF and "relu_in" in sw and (clean["scale"] is None or float(clean["scale"][idx[3]]) > 0)
    elif target == "dy":
        d["dy"] = _poisoned(clean["dy"], (0, 1, 1, 1), value)
        eW[1] = True
        eb[1] = True
    elif target == "kappa":
        d["kappa"] = value
        eW[:], eb[:] = True, True
    Wr, _, br, _, _ = CC.wg_ref(case, d)
    K = case["K"]
    run = dict(d=d, R={"dW": Wr}, bound={"dW": (K + 8) * CC.U24 * SW}, expect={"dW": eW}, exact=math.isnan(value), finite=finite,
               glob=target == "kappa", trips=_trips(target, value, sw), mutated=lambda: dict(zip(("dW", "dbias"), conv_wg_ref_mutated(case, d))))
    if "dbias" in sw:
        run["R"]["dbias"] = (br if clean["prevb"] is not None else br.expand(cout)).contiguous()
        run["bound"]["dbias"] = (K + 8) * CC.U24 * (Sb if clean["prevb"] is not None else Sb.expand(cout)).contiguous()
        run["expect"]["dbias"] = eb
    return run


def _wg_labels(case):
    B, Hh, Ww = case["shape"]
    places = placements(case["ins"], (B, Hh, Ww), "rep" in case["sw"])
    return [_label("x", p, v) for p in places for v in POISONS] + ["dy.a.nan"] + (["kappa.p.nan"] if "kappa" in case["sw"] else [])


for _n in ("wg_np9_nco1", "wg_in3"):
    _c = CC.WG_BY_NAME[_n]
    CASES.append(_case("conv_wgrad", _n, ["conv_wgrad"], _wg_labels(_c), (lambda c: lambda label, H: build_conv_wgrad(c, label, H))(_c),
                       ["relu"] + (["clamp"] if "kappa" in _c["sw"] else [])))


# conv_dgrad_direct: (name, (B, Hin, Win), Cin, Cout, k, stride) of test_conv_kernels.DG_CASES "dg_s2_k3_odd" / "dg_s1_k3_slices"
DGRAD = {"dg_s2_k3_odd": ((2, 13, 9), 6, 10, 3, 2, None, None), "dg_s1_k3_slices": ((2, 7, 11), 5, 7, 3, 1, (7, 12, 3, 0), (5, 9, 2, 0))}


def build_conv_dgrad(name, label, H):
    target, place, value = _parse(label)
    (B, Hin, Win), cin, cout, k, s, dys, dxs = DGRAD[name]
    Ho, Wo = CC.out_hw(Hin, Win, s)
    g = torch.Generator().manual_seed(4000)
    dy, w = CC.rnd(g, (B, Ho, Wo, cout), "gauss"), CC.rnd(g, (cout, cin, k, k), "gauss", 2)
    _, S = CC.dgrad_ref(dy, w, (B, Hin, Win, cin), k, s)
    d = dict(dy=dy, w=w, dys=dys, dxs=dxs, shape=(B, Hin, Win, cin), k=k, s=s)
    if target == "dy":
        idx = (0, Ho // 2, Wo // 2, 1) if place == "a" else (B - 1, 0, 0, cout - 1)
        d["dy"] = _poisoned(dy, idx, value)
        # dx(p) reads dy(o) when o s + tap - k // 2 == p for some tap
        e = torch.zeros(B, Hin, Win, dtype=torch.bool)
        for ky in range(k):
            for kx in range(k):
                y, x = idx[1] * s + ky - k // 2, idx[2] * s + kx - k // 2
                if 0 <= y < Hin and 0 <= x < Win:
                    e[idx[0], y, x] = True
        expect = e.unsqueeze(-1).expand(B, Hin, Win, cin)
    else:
        d["w"] = _poisoned(w, (1, 1, 1, 1), value)
        expect = None
    R, _ = CC.dgrad_ref(d["dy"], d["w"], (B, Hin, Win, cin), k, s)
    return dict(d=d, R={"dx": R}, bound={"dx": (k * k * cout + 8) * CC.U24 * S}, expect={"dx": expect}, exact=math.isnan(value), finite=False,
                glob=False, trips=False, mutated=None)


for _n in DGRAD:
    CASES.append(_case("conv_dgrad", _n, ["conv_dgrad_direct"], ["dy.a.nan", "dy.b.pinf", "dy.b.ninf", "w.p.nan"],
                       (lambda n: lambda label, H: build_conv_dgrad(n, label, H))(_n), []))


def build_conv_border(case, label, H):
    target, place, value = _parse(label)
    B, Hh, Ww = case["shape"]
    clean = CC.bd_data(case, "gauss")
    _, S = CC.bd_ref(case, clean)
    d = dict(clean)
    if target == "kappa":
        d["kappa"] = value
    else:
        d["dy"] = _poisoned(clean["dy"], (B - 1, 0, 0, 1), value)
    R, _ = CC.bd_ref(case, d)
    if target == "dy":
        # bd_ref forms the fold as a difference of two input gradients: a pixel that the poisoned dy reaches only through in-bounds
        # taps gets NaN - NaN there although the fold has no term from it.  The same formula on an indicator of the poisoned element
        # (absolute weights) names the pixels the fold does depend on; elsewhere the clean reference is the reference.
        ind = torch.zeros_like(clean["dy"])
        ind[B - 1, 0, 0, 1] = 1
        _, dep = CC.bd_ref(case, dict(clean, dy=ind, prev=torch.zeros_like(clean["prev"]), kappa=None))
        R = torch.where(dep > 0, R, CC.bd_ref(case, clean)[0])

    def mutated():
        return {"out": CC.bd_ref(case, dict(d, kappa=-4.0 if math.isnan(d["kappa"]) else d["kappa"]))[0]}
    return dict(d=d, R={"out": R}, bound={"out": (case["K"] + 8) * CC.U24 * S}, expect={"out": None}, exact=False, finite=False,
                glob=target == "kappa", trips=target == "kappa", mutated=mutated if target == "kappa" else None)


# every pixel of these images lies on the border (the fold of an interior pixel is 0 and the kernel never touches it, while the
# reference's 0 * exp(nan) would be NaN there): bd_h2_w2 on the matrix-core kernel, bd_scalar_w1 on the scalar one, both with kappa
for _n in ("bd_h2_w2", "bd_scalar_w1"):
    _c = dict(CC.BD_BY_NAME[_n], kappa=True)
    CASES.append(_case("conv_border", _n, ["conv_rep_border_fix"], ["kappa.p.nan", "dy.c.nan", "dy.c.pinf"],
                       (lambda c: lambda label, H: build_conv_border(c, label, H))(_c), ["clamp"], glob=["kappa.p.nan"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# Winograd (wino_cases.py, test_wino_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def wino_fwd_ref_mutated(case, d):
    sw = case["sw"]
    xp = d["x"].permute(0, 3, 1, 2)
    if "relu_in" in sw:
        xp = _mut_relu(xp)
    xp = F.pad(xp, (1, 1, 1, 1), mode="replicate" if "rep" in sw else "constant")
    y = F.conv2d(xp, d["w_eff"], d["bias"]).permute(0, 2, 3, 1)
    if "relu_out" in sw:
        y = _mut_relu(y)
    return y.contiguous()


def build_wino_fwd(case, arith, label, H):
    target, place, value = _parse(label)
    B, p = WC.resolve_fwd(H, case, arith)
    Hh, Ww = case["hw"]
    sw = case["sw"]
    clean = WC.fwd_data(case, B, "gauss")
    _, S = WC.fwd_ref(case, clean)
    d = dict(clean)
    cout = case["cout"]
    allowed, expect, finite = None, None, False
    if target == "x":
        idx = placements(case["ins"], (B, Hh, Ww), "rep" in sw)[place]
        d["x"] = _poisoned(clean["x"], idx, value)
        finite = value == -INF and "relu_in" in sw
        if not finite:
            allowed = wino_footprint((B, Hh, Ww), idx[:3], "rep" in sw).unsqueeze(-1).expand(B, Hh, Ww, cout)
        expect = conv_reach((B, Hh, Ww), idx[:3], 3, 1, "rep" in sw).unsqueeze(-1).expand(B, Hh, Ww, cout)
    else:
        d["w"] = _poisoned(clean["w"], (1, 1, 1, 1), value)
        d["w_eff"] = d["w"]
        expect = torch.zeros(B, Hh, Ww, cout, dtype=torch.bool)
        expect[..., 1] = True
    R, _ = WC.fwd_ref(case, d)
    c = WC.fwd_c(p["kernel"], p["nchunks"])
    return dict(d=d, B=B, R={"out": R}, bound={"out": (p["Cin_pad"] + c) * CC.U24 * S}, allowed={"out": allowed} if allowed is not None else {},
                expect={"out": expect}, exact=math.isnan(value) and "relu_out" not in sw, finite=finite, glob=False,
                trips=_trips(target, value, sw), mutated=lambda: {"out": wino_fwd_ref_mutated(case, d)})


def _wino_labels(case):
    places = placements(case["ins"], (2,) + tuple(case["hw"]), "rep" in case["sw"])
    return [_label("x", p, v) for p in places for v in POISONS] + ([] if case["dgrad"] else ["w.p.nan"])


WINO_FWD = ("f_cin20_cout68", "f_in3_slices", "f2_hw3x2_rep", "f2_cin20_cout264")
WINO_NARROW = ("n3_cin80_cout48_out3", "n1_hw17x1_rep")
for _n in WINO_FWD:
    for _a in ("f32", "bf16x3"):
        _c = WC.FWD_BY_NAME[_n]
        CASES.append(_case("wino_fwd", "%s-%s" % (_n, _a), ["conv_wino_fwd" if _a == "f32" else "conv_wino_fwd3"], _wino_labels(_c),
                           (lambda c, a: lambda label, H: build_wino_fwd(c, a, label, H))(_c, _a), ["relu"] if "relu_in" in _c["sw"] else []))
for _n in WINO_NARROW:
    _c = WC.NARROW_BY_NAME[_n]
    CASES.append(_case("wino_narrow", _n, ["conv_wino_narrow"], _wino_labels(_c),
                       (lambda c: lambda label, H: build_wino_fwd(c, "f32", label, H))(_c), ["relu"]))


def wino_wg_ref_mutated(case, d):
    xp = d["x"].permute(0, 3, 1, 2)
    if "relu_in" in case["sw"]:
        xp = _mut_relu(xp)
    xp = F.pad(xp, (1, 1, 1, 1), mode="replicate" if "rep" in case["sw"] else "constant")
    c = dict(case, cout=d["dy"].shape[3])
    return CC.wg_scatter(c, CC.wg_dense(xp, d["dy"], 3, 1), d["prevW"], 1.0)[0]


def _wino_wg_run(case, clean, label, p, K):
    """One group's run: (d, R, bound, expect, finite)."""
    target, place, value = _parse(label)
    B, Hh, Ww = clean["x"].shape[:3]
    _, SW, _, Sb, _ = WC.wg_ref(case, clean)
    d = dict(clean)
    cout = clean["dy"].shape[3]
    eW = torch.zeros(cout, case["layout"][0] or case["cin"], 9, dtype=torch.bool)
    eb = torch.zeros(cout, dtype=torch.bool)
    finite = False
    if target == "x":
        idx = placements(case["ins"], (B, Hh, Ww), "rep" in case["sw"])[place]
        d["x"] = _poisoned(clean["x"], idx, value)
        eW[:, idx[3]] = True
        assert bool(wg_taps((B, Hh, Ww), idx[:3], 3, 1, "rep" in case["sw"]).all())
        finite = value == -INF and "relu_in" in case["sw"]
    else:
        d["dy"] = _poisoned(clean["dy"], (0, Hh // 2, Ww // 2, 1), value)
        eW[1], eb[1] = True, True
    Wr, _, br, _, _ = WC.wg_ref(case, d)
    R, bound, expect = {"dW": Wr}, {"dW": (K + WC.wg_c(p)) * CC.U24 * SW}, {"dW": eW}
    if "dbias" in case["sw"]:
        R["dbias"], bound["dbias"], expect["dbias"] = br, (WC.wg_kb(p) + 1) * CC.U24 * Sb, eb
    return d, R, bound, expect, finite


def build_wino_wgrad(case, label, H):
    B, p = WC.resolve_wg(H, case)
    _, Hh, Ww = case["shape"]
    clean = WC.wg_data(case, B, "gauss")
    d, R, bound, expect, finite = _wino_wg_run(case, clean, label, p, WC.wg_dy_tiles((B, Hh, Ww)))
    # a Winograd weight gradient transforms the 4x4 patch too, but it SUMS over every tile: the poisoned input channel's column is
    # non-finite in the reference already (all taps), so no exception is needed
    return dict(d=d, B=B, R=R, bound=bound, expect=expect, exact=math.isnan(_parse(label)[2]), finite=finite, glob=False,
                trips=_trips(_parse(label)[0], _parse(label)[2], case["sw"]), mutated=lambda: {"dW": wino_wg_ref_mutated(case, d)})


def build_wino_wgrad_grouped(case, label, H):
    """The poison goes into group 1; every other group must stay clean."""
    B, Hh, Ww = case["shape"]
    ds = WC.grouped_data(case, "gauss")
    one = CC.descr((B, Hh, Ww), CC.seg(case["cout"]), 4)
    kw = WC.wg_args(case, B)[2]
    p = H.conv_wino_wgrad_plan([CC.descr((B, Hh, Ww), CC.seg(case["cin"]), 0)], one, ngroups=case["G"], **kw)
    assert WC.wg_plan_ok(case, p), p
    K = WC.wg_dy_tiles((B, Hh, Ww))
    R, bound, expect, out_ds, finite = {}, {}, {}, [], False
    for g, clean in enumerate(ds):
        if g == 1:
            d, Rg, bg, eg, fg = _wino_wg_run(case, clean, label, p, K)
        else:
            d, (Rg, bg, eg, fg) = clean, _clean_group(case, clean, p, K)
        out_ds.append(d)
        finite = finite or fg
        for n in Rg:
            R["%s%d" % (n, g)], bound["%s%d" % (n, g)], expect["%s%d" % (n, g)] = Rg[n], bg[n], eg[n]
    return dict(d=out_ds, R=R, bound=bound, expect=expect, exact=math.isnan(_parse(label)[2]), finite=finite, glob=False,
                trips=_trips(_parse(label)[0], _parse(label)[2], case["sw"]), mutated=lambda: {"dW1": wino_wg_ref_mutated(case, out_ds[1])})


def _clean_group(case, clean, p, K):
    Wr, SW, br, Sb, _ = WC.wg_ref(case, clean)
    R, bound = {"dW": Wr}, {"dW": (K + WC.wg_c(p)) * CC.U24 * SW}
    expect = {"dW": torch.zeros_like(Wr, dtype=torch.bool)}
    if "dbias" in case["sw"]:
        R["dbias"], bound["dbias"], expect["dbias"] = br, (WC.wg_kb(p) + 1) * CC.U24 * Sb, torch.zeros_like(br, dtype=torch.bool)
    return R, bound, expect, False


def _wino_wg_labels(case):
    """The output transform A'^T M A' spreads a non-finite (co, ci) product over all nine taps, so the poisoned pixel is one that every
    tap reads (an interior one; not the corner): the reference's column is then non-finite on all nine as well."""
    B, Hh, Ww = case["shape"]
    places = {p: i for p, i in placements(case["ins"], (B, Hh, Ww), "rep" in case["sw"]).items()
              if bool(wg_taps((B, Hh, Ww), i[:3], 3, 1, "rep" in case["sw"]).all())}
    return [_label("x", p, v) for p in places for v in POISONS] + ["dy.a.nan"]


for _n in ("w_cit3_nco2", "w_in3_slices", "w_hw17x1"):
    _c = WC.WG_BY_NAME[_n]
    CASES.append(_case("wino_wgrad", _n, ["conv_wino_wgrad"], _wino_wg_labels(_c),
                       (lambda c: lambda label, H: build_wino_wgrad(c, label, H))(_c), ["relu"]))
_c = WC.GROUPED_BY_NAME["g3_cin36_cg64"]
CASES.append(_case("wino_wgrad_grouped", "g3_cin36_cg64", ["conv_wgrad_grouped"], _wino_wg_labels(_c),
                   (lambda c: lambda label, H: build_wino_wgrad_grouped(c, label, H))(_c), ["relu"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the home files of the bandwidth-bound kernels are test modules; importing them runs no test and needs no device
# ---------------------------------------------------------------------------------------------------------------------------------
import test_ensemble_gpu as EG      # noqa: E402
import test_param_kernels as PK     # noqa: E402
import test_pointwise_kernels as PW  # noqa: E402
import test_turbulence_gpu as TG    # noqa: E402


def _pw_bound(ref, s, tol):
    """The bound of test_pointwise_kernels.share: tol (|ref| + s) + TINY."""
    return tol * (ref.abs() + torch.as_tensor(s, dtype=torch.float64)) + PW.TINY


# ---------------------------------------------------------------------------------------------------------------------------------
# diagonal Gaussian (test_pointwise_kernels.GAUSS_CASES, test_param_kernels.DRAW_CASES)
# ---------------------------------------------------------------------------------------------------------------------------------
GAUSS = {c[0]: c for c in PW.GAUSS_CASES}


def gauss_ref_mutated(hz, Ch, clip, lim):
    """hz with the clamps as fminf(fmaxf(.)) had them: a NaN mean (when clipped) / log-std becomes its lower limit."""
    hz = hz.clone()
    if clip:
        hz[..., :Ch] = torch.nan_to_num(hz[..., :Ch], nan=lim[0] - 1.0)
    hz[..., Ch:] = torch.nan_to_num(hz[..., Ch:], nan=lim[2] - 1.0)
    return hz


def _gauss_outputs(case, hz, v, dz, g, lp0, lim):
    name, B, Hh, Ww, Ch, mode, clip, has_zout, has_dzin, has_dzout, has_g = case[:11]
    out, so, lpt, slp, dzr, sdz, dhr, sdh = PW.gauss_ref(hz, v, dz if has_dzin else None, g if has_g else None, mode, clip, lim)
    K = Hh * Ww * Ch
    tol_lp = 2 * PW.TOL_GAUSS + 4 * PW.U + math.sqrt(K) * PW.U
    res = {"logp": (lp0.double() + lpt, lp0.double().abs() + slp, tol_lp), "dhz": (dhr, sdh, PW.TOL_GAUSS_B)}
    if has_zout:
        res["zout"] = (out, so, PW.TOL_GAUSS)
    if mode == 0 and has_dzout:
        res["dzout"] = (dzr, sdz, PW.TOL_GAUSS_B)
    return res


def build_gauss(name, label, H):
    case = GAUSS[name]
    _, B, Hh, Ww, Ch, mode, clip = case[:7]
    target, place, value = _parse(label)
    hz0, v0, dz0, g0, lp0, lim = PW._gauss_data(B, Hh, Ww, Ch, clip, 500 + Ch + B)
    j = min(1, Ch - 1) if place == "a" else Ch - 1
    hz = _poisoned(hz0, (B - 1, Hh // 2, Ww // 2, j + (Ch if target == "lsd" else 0)), value)
    finite = math.isinf(value) and (target == "lsd" or bool(clip))          # a clamp maps +-Inf to its limit
    pois = _gauss_outputs(case, hz, v0, dz0, g0, lp0, lim)
    R = {n: r for n, (r, _, _) in pois.items()}
    # the bound comes from the clean data, except where the poison leaves every output finite: the clamped element then takes its
    # limit, a finite value that is not the clean one, and the home file's scales of THAT data are finite too
    bound = {n: _pw_bound(r, s, tol) for n, (r, s, tol) in (pois if finite else _gauss_outputs(case, hz0, v0, dz0, g0, lp0, lim)).items()}

    def mutated():
        return {n: r for n, (r, _, _) in _gauss_outputs(case, gauss_ref_mutated(hz, Ch, clip, lim), v0, dz0, g0, lp0, lim).items()}
    return dict(d=dict(hz=hz, v=v0, dz=dz0, g=g0, lp0=lp0, lim=lim), R=R, bound=bound, expect={}, exact=False, finite=finite, glob=False,
                trips=math.isnan(value) and (target == "lsd" or bool(clip)), mutated=mutated)


for _n in ("m0c1", "m0c0", "m1c1", "m1c0"):
    CASES.append(_case("gauss", _n, ["gauss_fwd", "gauss_bwd"],
                       ["mean.a.nan", "mean.b.pinf", "mean.b.ninf", "lsd.a.nan", "lsd.b.pinf", "lsd.b.ninf"],
                       (lambda n: lambda label, H: build_gauss(n, label, H))(_n), ["clamp"]))


DRAW = {c[0]: c for c in PK.DRAW_CASES}


def build_gauss_sample(name, label, H):
    """tmg_gauss_sample with eps given (nothing is drawn): v8 on the float4 instance, s5 on the scalar one."""
    _, B, Hh, Ww, Ch = DRAW[name][:5]
    target, place, value = _parse(label)
    clip = Ch % 2
    hz0, z10, eps0, _, lp0, lim = PW._gauss_data(B, Hh, Ww, Ch, clip, 900 + Ch + B)
    j = min(1, Ch - 1) if place == "a" else Ch - 1
    hz = _poisoned(hz0, (B - 1, Hh // 2, Ww // 2, j + (Ch if target == "lsd" else 0)), value)

    def outs(h):
        out, so, lpt, slp = PW.gauss_ref(h, eps0, None, None, 1, clip, lim)[:4]
        tol_lp = 2 * PW.TOL_GAUSS + 4 * PW.U + math.sqrt(Hh * Ww * Ch) * PW.U
        return {"out": (out, so, PW.TOL_GAUSS), "logp": (lp0.double() + lpt, lp0.double().abs() + slp, tol_lp)}
    finite = math.isinf(value) and (target == "lsd" or bool(clip))
    return dict(d=dict(hz=hz, eps=eps0, z1=z10, lp0=lp0, lim=lim, clip=clip), R={n: r for n, (r, _, _) in outs(hz).items()},
                bound={n: _pw_bound(r, s, tol) for n, (r, s, tol) in outs(hz if finite else hz0).items()},   # see build_gauss
                expect={}, exact=False, finite=finite, glob=False,
                trips=math.isnan(value) and (target == "lsd" or bool(clip)),
                mutated=lambda: {n: r for n, (r, _, _) in outs(gauss_ref_mutated(hz, Ch, clip, lim)).items()})


for _n in ("v8", "s5"):
    CASES.append(_case("gauss_sample", _n, ["gauss_sample"], ["mean.a.nan", "mean.b.pinf", "lsd.a.nan", "lsd.b.ninf"],
                       (lambda n: lambda label, H: build_gauss_sample(n, label, H))(_n), ["clamp"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam (test_param_kernels.adam_ref: the header's formula, which is torch.optim.Adam's; test_nonfinite_cpu.py checks that the two
# have the same non-finite set)
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = [1, 255, 4097]
ADAM_POISON = 1 + 255 + 4096          # the last element of the last tensor: a chunk of one element
ADAM = {"ams1-wd0-s1": (0.0, 1, 1), "ams0-wd-s1000": (0.05, 0, 1000), "ams1-wd-s1000": (0.05, 1, 1000)}
ADAM_OUT = {"adam m": "m", "adam v": "v", "adam p": "p", "adam vmax": "vm"}


def adam_vals():
    g = torch.Generator().manual_seed(1234)
    nl = sum(ADAM_SIZES)
    vals = dict(p=torch.randn(nl, generator=g), g=torch.randn(nl, generator=g), m=0.1 * torch.randn(nl, generator=g),
                v=0.01 * torch.rand(nl, generator=g) + 1e-6)
    vals["vm"] = vals["v"] * torch.where(torch.rand(nl, generator=g) < 0.5, 0.5, 2.0)
    return vals


def adam_ref_mutated(vals, wd, ams, bc1, bc2s):
    """adam_ref with vmax = fmaxf(vmax, v): vmax kept when v is NaN."""
    ref = PK.adam_ref(vals, wd, ams, bc1, bc2s)
    out = {ADAM_OUT[k]: r for k, (r, _) in ref.items()}
    if ams:
        out["vm"] = torch.where(torch.isnan(out["v"]), vals["vm"].double(), out["vm"])
    return out


def build_adam(name, label, H):
    wd, ams, step = ADAM[name]
    target, place, value = _parse(label)
    clean = adam_vals()
    vals = dict(clean, g=_poisoned(clean["g"], (ADAM_POISON if place == "b" else 100,), value))
    bc1, bc2s = 1.0 - PK.B1 ** step, (1.0 - PK.B2 ** step) ** 0.5
    rc = PK.adam_ref(clean, wd, ams, bc1, bc2s)
    rp = PK.adam_ref(vals, wd, ams, bc1, bc2s)
    R = {ADAM_OUT[k]: r for k, (r, _) in rp.items()}
    bound = {ADAM_OUT[k]: _pw_bound(r, s, PK.U) for k, (r, s) in rc.items()}
    return dict(d=dict(vals=vals, wd=wd, ams=ams, step=step, bc1=bc1, bc2s=bc2s), R=R, bound=bound, expect={}, exact=False, finite=False,
                glob=False, trips=bool(ams) and math.isnan(value), mutated=lambda: adam_ref_mutated(vals, wd, ams, bc1, bc2s))


for _n in ADAM:
    CASES.append(_case("adam", _n, ["adam_step"], ["g.a.nan", "g.b.nan", "g.a.pinf", "g.b.ninf"],
                       (lambda n: lambda label, H: build_adam(n, label, H))(_n), ["vmax"] if ADAM[_n][1] else []))


# ---------------------------------------------------------------------------------------------------------------------------------
# basic ensemble statistics (test_ensemble_gpu._ref_stats, test_turbulence_gpu._ref_turb): one poisoned member at one pixel
# ---------------------------------------------------------------------------------------------------------------------------------
ENS = {"s7_b1_c3_5x7": (7, 1, 3, (5, 7), 4, 1, 2, True), "s2_b3_c4_5x7": (2, 3, 4, (5, 7), 3, 0, 1, False)}      # S, B, C, hw, T, t_start, chunks, u
ENS_STD = ("std", "mag_std", "time_mean_std", "time_rms_std", "vort_std", "time_uv_std", "time_tke_std", "time_vort_std")


def ens_refs(ys, u, mu, sd, t_start):
    ref, ymax = EG._ref_stats(ys, u, mu, sd, t_start)
    rt, _, fl = TG._ref_turb(ys, u, mu, sd, t_start, TG.DX, TG.DY)
    ref.update(rt)
    return ref, ymax, fl


def build_ensemble(name, label, H):
    S, B, Cc, (Hh, Ww), T, t_start, nchunks, u_given = ENS[name]
    target, place, value = _parse(label)
    g = torch.Generator().manual_seed(77)
    ys = torch.randn(T, S, B, Cc, Hh, Ww, generator=g) * 0.8 + 0.1
    mu = torch.tensor([0.3, -0.2, 0.5, 1.0][:Cc])
    sd = torch.tensor([1.7, 0.6, 2.5, 0.9][:Cc])
    u = (0.5 + torch.rand(B, Cc, generator=g)) if u_given else None
    rc, ymax, fl = ens_refs(ys, u, mu, sd, t_start)
    # the last step lies in the time window of both cases; channel 0 feeds the magnitude, the vorticity and the Reynolds stress
    yp = _poisoned(ys, (T - 1, S - 1, B - 1, 0 if place == "a" else Cc - 1, Hh // 2, Ww // 2), value)
    R, _, _ = ens_refs(yp, u, mu, sd, t_start)
    # The reference convolves with the full 3x3 stencils, whose centre row (d/dy) and centre column (d/dx) are zero: 0 * NaN makes the
    # three pixels of that row / column non-finite although the vorticity there has no term from the poisoned value (the kernel adds
    # the six non-zero taps).  The same stencils on an indicator name the pixels that do depend on it; elsewhere the clean reference
    # is the reference ("Non-finite values": structural zeros).
    ind = torch.zeros(1, 2, Hh, Ww, dtype=torch.float64)
    ch = 0 if place == "a" else Cc - 1
    if ch < 2:
        ind[0, ch, Hh // 2, Ww // 2] = 1
    dep = TG._vorticity(ind, TG.DX, TG.DY)[0] != 0
    for n in ("vort_mean", "vort_std", "time_vort_mean", "time_vort_std"):
        keep = torch.ones_like(R[n], dtype=torch.bool)
        keep[B - 1] = dep
        R[n] = torch.where(keep, R[n], rc[n])
    scales = TG._scales(ymax, fl, TG.DX, TG.DY)
    bound = {n: 4e-6 * scales.get(n, ymax) + 1e-5 * r.abs() for n, r in rc.items()}

    def mutated():
        # std = sqrt(fmaxf(m2, 0) / n): a NaN second moment gives a spread of exactly 0
        return {n: (torch.where(torch.isnan(r), torch.zeros_like(r), r) if n in ENS_STD else r) for n, r in R.items()}
    return dict(d=dict(ys=yp, u=u, mu=mu, sd=sd, t_start=t_start, nchunks=nchunks), R=R, bound=bound, expect={}, exact=False, finite=False,
                glob=False, trips=True, mutated=mutated)


for _n in ENS:
    CASES.append(_case("ensemble", _n, ["ens_accum", "ens_time_finalize", "ens_turb_accum", "ens_turb_finalize"],
                       ["y.a.nan", "y.b.nan", "y.a.pinf"], (lambda n: lambda label, H: build_ensemble(n, label, H))(_n), ["std"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole model (common.CFG_TINY, tests/golden/tiny_model.npz): reverse loss and parameter gradients of the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def model_inputs(label):
    """(cfg, state dict, x, h_in, eps) of the tiny model with one input pixel or one parameter element set to NaN; eps: the latents of the
    oracle's clean forward pass (fp32), fed to both sides."""
    import common as C
    from oracle import tmglow_oracle as O
    target, place, value = _parse(label)
    cfg = C.CFG_TINY
    d = C.load_npz("tiny_model.npz")
    L = len(cfg["glow_blocks"])
    sd = {k: torch.from_numpy(v).clone() for k, v in C.sub(d, "sd.").items()}
    x, y = torch.from_numpy(d["x"]).clone(), torch.from_numpy(d["y"])
    h_in = C.states_from(d, "h_in.", L)
    with torch.no_grad():
        _, _, _, eps = O.tmglow_forward(O.params_from_state_dict(sd, requires_grad=False), cfg, x, y, h_in, return_eps=True)
    eps = [e.detach().float() if e is not None else None for e in eps]
    if target == "x":
        x[0, 0, x.shape[2] // 2, x.shape[3] // 2] = value
    else:
        key = sorted(k for k, v in sd.items() if v.dim() == 4 and k.endswith(".weight"))[0]
        sd[key].view(-1)[1] = value
    return cfg, sd, x, h_in, eps


def build_model(label, H):
    import common as C
    from oracle import tmglow_oracle as O
    cfg, sd, x, h_in, eps = model_inputs(label)
    P = O.params_from_state_dict(sd, dtype=torch.float64)
    yo, ldo, _ = O.tmglow_reconstruct(P, cfg, x.double(), [(h.double(), c.double()) for h, c in h_in],
                                      [e.double() if e is not None else None for e in eps])
    loss = C.loss_reverse(yo, ldo)
    loss.backward()
    R = {"loss": loss.detach().reshape(1)}
    R.update({"grad " + k: v.grad.detach() for k, v in P.items() if v.requires_grad and v.grad is not None})
    # l and u enter the weight as l * l_mask and u * u_mask: the oracle's gradient of a masked-out entry is 0 * NaN, a structural zero
    # (lu_fold_bwd writes 0 there, as its header says)
    for k in list(R):
        for f in ("l", "u"):
            if k.endswith(".conv." + f):
                R[k] = torch.where(sd[k[len("grad "):] + "_mask"].double() != 0, R[k], torch.zeros_like(R[k]))
    # only rule 1 is asked of the whole model: where the oracle is finite under a NaN input nothing is stated
    return dict(d=dict(cfg=cfg, sd=sd, x=x, h_in=h_in, eps=eps), R=R, bound={n: INF for n in R}, expect={}, exact=False, finite=False,
                glob=True, trips=False, mutated=None)


CASES.append(_case("model", "tiny", ["TMGlow.reconstruct"], ["x.a.nan", "w.p.nan"], build_model, [], glob=["x.a.nan", "w.p.nan"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm chain (test_pointwise_kernels.test_chan_reduce_and_batchnorm): chan_moments -> bn_finalize64, the two-pass
# chan_reduce -> bn_finalize, chan_reduce mode 1 -> bn_bwd_apply, against nn.BatchNorm2d + ReLU in fp64 (train mode: a poisoned
# element makes its whole channel non-finite, the other channels stay within their bounds)
# ---------------------------------------------------------------------------------------------------------------------------------
BN = {"C12": (12, 3, 29, 23), "C3": (3, 2, 67, 41)}
BN_ROWS = ("mean", "var", "rstd", "a", "bsh")


def bn_reference(x0, gamma, beta, gy0, rm0, rv0):
    """{output: (ref, s, tol)} with the scales and tolerances of test_chan_reduce_and_batchnorm (fp64 moments path; `32` suffix: the
    fp32 two-pass path)."""
    B, Hh, Ww, Cn = x0.shape
    n = B * Hh * Ww
    U, EPS32, MOM32 = PW.U, PW.EPS32, PW.MOM32
    st = PW.bn_stats(x0, gamma, beta)
    xd = x0.double().flatten(0, 2)
    mean, var, rstd, a, bsh = (st[k] for k in BN_ROWS)
    gam, bet = gamma.double(), beta.double()
    sd = xd.abs() + mean.abs()
    s_mean, s_var = st["absx"] / n, (sd * sd).sum(0) / n
    s_rstd = 0.5 * rstd * s_var / (var + EPS32)
    tr = PW.tol_sum(n, 8)
    rmr, srm, rvr, srv = PW._run_stats_ref(st, rm0, rv0, n)
    out = {"mean": (mean, 0.0, 2 * U), "var": (var, 0.0, 2 * U), "rstd": (rstd, 0.0, 8 * U), "a": (a, 0.0, 9 * U),
           "bsh": (bsh, bet.abs() + (mean * a).abs(), 12 * U),
           "mean32": (mean, s_mean, tr + U), "var32": (var, s_var, tr + U), "rstd32": (rstd, s_rstd, tr + 8 * U),
           "a32": (a, gam.abs() * s_rstd, tr + 9 * U),
           "bsh32": (bsh, bet.abs() + (mean * a).abs() + a.abs() * s_mean + mean.abs() * gam.abs() * s_rstd, tr + 12 * U),
           "running_mean32": (rmr, srm + MOM32 * s_mean, tr + 9 * U), "running_var32": (rvr, srv + MOM32 * s_var * n / (n - 1), tr + 9 * U)}
    bn = torch.nn.BatchNorm2d(Cn, eps=EPS32, momentum=MOM32).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    bn.train()
    xg = x0.double().permute(0, 3, 1, 2).requires_grad_(True)
    (F.relu(bn(xg)) * gy0.double().permute(0, 3, 1, 2)).sum().backward()
    out["running_mean"] = (bn.running_mean.detach().clone(), srm, 9 * U)
    out["running_var"] = (bn.running_var.detach().clone(), srv, 9 * U)
    du_abs = (gy0.double().flatten(0, 2) * ((xd * a + bsh) > 0)).abs()
    xh_abs = (xd.abs() + mean.abs()) * rstd
    S0, S1 = du_abs.sum(0), (du_abs * xh_abs).sum(0)
    out["dbeta"] = (bn.bias.grad.clone(), S0, PW.tol_sum(n, 8))
    out["dgamma"] = (bn.weight.grad.clone(), S1, PW.tol_sum(n, 8) + 12 * U)
    s_dx = (gam.abs() * rstd * (gy0.double().flatten(0, 2).abs() + S0 / n + xh_abs * S1 / n)).view(B, Hh, Ww, Cn)
    out["dx"] = (xg.grad.permute(0, 2, 3, 1).contiguous(), s_dx, PW.tol_sum(n, 12))
    return out


def build_bn(name, label, H):
    Cn, B, Hh, Ww = BN[name]
    target, place, value = _parse(label)
    x0, gamma, beta, gy0, rm0, rv0 = PW._bn_data(Cn, B, Hh, Ww, 600 + Cn)
    clean = bn_reference(x0, gamma, beta, gy0, rm0, rv0)
    ch = 1 if place == "a" else Cn - 1
    x, gm = x0, gamma
    if target == "x":
        x = _poisoned(x0, (B - 1, Hh // 2, Ww // 2, ch), value)
    else:
        gm = _poisoned(gamma, (ch,), value)
    R = {n: r for n, (r, _, _) in bn_reference(x, gm, beta, gy0, rm0, rv0).items()}

    def mutated():
        # the mask as `u > 0 ? g : 0`: the gradient is dropped where the pre-activation is NaN, so the poisoned channel's dbeta, which
        # the reference keeps finite (the sum of all g), becomes the sum over no pixel at all: rule 2 (off), not rule 1
        m = dict(R)
        bad = nonfinite(R["a"])
        m["dbeta"] = torch.where(bad, torch.zeros_like(R["dbeta"]), R["dbeta"])
        return m
    return dict(d=dict(x=x, gamma=gm, beta=beta, gy=gy0, rm0=rm0, rv0=rv0), R=R, bound={n: _pw_bound(r, s, tol) for n, (r, s, tol) in clean.items()},
                expect={}, exact=False, finite=False, glob=False, trips=False, mutated=mutated, mask_off="dbeta")


for _n in BN:
    CASES.append(_case("batchnorm", _n, ["chan_moments", "bn_finalize64", "chan_reduce", "bn_finalize", "bn_bwd_apply"],
                       ["x.a.nan", "x.b.pinf", "x.b.ninf", "gamma.p.nan"], (lambda n: lambda label, H: build_bn(n, label, H))(_n), ["mask"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# physics loss (test_phys_kernels.py): the clamped residual fields of phys_fwd and the statistics of phys_rms
# ---------------------------------------------------------------------------------------------------------------------------------
import test_phys_kernels as PH     # noqa: E402

PHYS = {"2x9x7": (2, 9, 7), "1x5x6": (1, 5, 6)}


def phys_fwd_ref_mutated(r):
    """The clamps as fminf(fmaxf(raw, -1), 1): a NaN raw residual becomes -1."""
    return {"us": torch.nan_to_num(r["rd"], nan=-1.0).clamp(-1, 1), "ps": torch.nan_to_num(r["rp"], nan=-1.0).clamp(-1, 1)}


def build_phys_fwd(name, label, H):
    """One poisoned velocity (channel 0) or pressure (channel 2) value.  The stencils have zero centre rows / columns; the reference
    (a dense convolution) and the kernel both multiply every tap, zero ones included, so the plain reference is the reference."""
    N_, Hh, Ww = PHYS[name]
    target, place, value = _parse(label)
    y0, t = PH.make_y(N_, Hh, Ww, 1.5)
    y = _poisoned(y0, (N_ - 1, 0 if target == "u" else 2, Hh // 2, Ww // 2), value)
    rc, rp = PH.fwd_ref(y0, t), PH.fwd_ref(y, t)
    bound = {"us": _pw_bound(rc["us"], rc["Sd"], PH.TOL_US), "ps": _pw_bound(rc["ps"], rc["Sp"], PH.TOL_PS)}
    return dict(d=dict(y=y, t=t), R={"us": rp["us"], "ps": rp["ps"]}, bound=bound, expect={}, exact=False, finite=False, glob=False,
                trips=True, mutated=lambda: phys_fwd_ref_mutated(rp), sums=rp["sums"])


for _n in PHYS:
    CASES.append(_case("phys_fwd", _n, ["phys_fwd"], ["u.a.nan", "p.a.nan"], (lambda n: lambda label, H: build_phys_fwd(n, label, H))(_n),
                       ["clamp"]))


def build_phys_rms(name, label, H):
    """mean, coef = (rms - trms) / (T rms) (the statement of test_phys_kernels.bwd_ref; every series here has rms > 0) and the sum."""
    B, T, (Hh, Ww) = 2, 5, PHYS[name][1:]
    target, place, value = _parse(label)
    g = PH._gen(B * 100 + T * 10 + Hh)
    y0 = torch.randn(B, T, 3, Hh, Ww, generator=g)
    trms = torch.randn(B, 3, Hh, Ww, generator=g).abs()
    y = _poisoned(y0, (B - 1, T - 1, 1, Hh // 2, Ww // 2), value)
    rc = PH.rms_ref(y0, trms)

    def stats(yy):
        y64 = yy.double()
        m = y64.mean(1)
        rms = ((y64 - m.unsqueeze(1)) ** 2).mean(1).sqrt()
        return m, (rms - trms.double()) / (T * rms)
    m, coef = stats(y)
    assert bool((rc["rms"] > 0).all())
    bound = {"mean": _pw_bound(rc["mean"], rc["M1"], T * PH.U), "coef": rc["b_coef"] + PW.TINY}

    def mutated():
        return {"mean": m, "coef": torch.where(torch.isnan(coef), torch.zeros_like(coef), coef)}       # rms > 0 ? .. : 0
    return dict(d=dict(y=y, trms=trms), R={"mean": m, "coef": coef}, bound=bound, expect={}, exact=False, finite=False, glob=False,
                trips=True, mutated=mutated)


CASES.append(_case("phys_rms", "1x5x6", ["phys_rms"], ["y.a.nan", "y.a.pinf"], lambda label, H: build_phys_rms("1x5x6", label, H), ["clamp"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# growth-layer forwards (thin_cases.py, test_thin_kernels.py): c1_fwd and c1x2_fwd with relu_in (3x3, zero padding)
# ---------------------------------------------------------------------------------------------------------------------------------
import thin_cases as T     # noqa: E402


def _thin_mut(case, d, two):
    """c1_ref / c1x2_ref on an input whose NaN the staging ReLU turned into 0 (fmaxf)."""
    dm = dict(d, x=torch.where(torch.isnan(d["x"]), torch.zeros_like(d["x"]), d["x"]))
    return {"out": (T.c1x2_ref(case, dm)[0] if two else T.c1_ref(case, dm)[0])}


def build_thin(case, label, H):
    target, place, value = _parse(label)
    two = case["fam"] == "c1x2"
    B, (Hh, Ww) = case["B"], case["hw"]
    clean = T.fwd_data(case, "gauss") if two else T.c1_data(case, "gauss")
    idx = placements(case["ins"], (B, Hh, Ww), False)[place]
    d = dict(clean, x=_poisoned(clean["x"], idx, value))
    reach = conv_reach((B, Hh, Ww), idx[:3], 3, 1, False).unsqueeze(-1)
    if two:
        _, S = T.c1x2_ref(case, clean)
        R, _ = T.c1x2_ref(case, d)
        bound = T.c1x2_bound(case, S)
        # d1 reads the pixel's 3x3 neighbourhood, d2 reads x there and relu(d1) one ring further out
        far = F.max_pool2d(reach.permute(0, 3, 1, 2).double(), 3, 1, 1).permute(0, 2, 3, 1) > 0
        expect = torch.cat([reach, far, torch.zeros_like(reach), torch.zeros_like(reach)], 3)
    else:
        _, S = T.c1_ref(case, clean)
        R, _ = T.c1_ref(case, d)
        bound = (case["K"] + 4) * T.U24 * S
        expect = reach
    finite = value == -INF and "relu_in" in case["sw"]
    return dict(d=d, R={"out": R}, bound={"out": bound}, expect={"out": expect}, exact=False, finite=finite, glob=False,
                trips=_trips(target, value, case["sw"]), mutated=lambda: _thin_mut(case, d, two))


def _thin_labels(case):
    places = placements(case["ins"], (case["B"],) + tuple(case["hw"]), False)
    return [_label("x", p, v) for p in places for v in POISONS]


for _c in (T.C1_BY_NAME["c_cin6_scalar_twl4"], T.C1_BY_NAME["c_cin36_twl5"], T.C1X2_BY_NAME["x_cg2_cin8"], T.C1X2_BY_NAME["x_cg2_scalar_cin6"]):
    CASES.append(_case("thin", _c["name"], ["c1x2_fwd" if _c["fam"] == "c1x2" else "c1_fwd"], _thin_labels(_c),
                       (lambda c: lambda label, H: build_thin(c, label, H))(_c), ["relu"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the autograd nodes (node_cases.py, test_nodes_fp64.py): forward and backward on each node's smallest shape, one poisoned input
# element, kappa (the zero conv's scale) or upstream-gradient element.  The reference is node_cases' own fp64 run on the poisoned
# data; the bound is the node's bound in node_cases' measure, tol max(1, max|clean reference|) per element (the log-det: tol times
# max(1, sum_image |sg|)).
# ---------------------------------------------------------------------------------------------------------------------------------
import copy                 # noqa: E402

import node_cases as NC     # noqa: E402


def _node_ref(kind, d):
    if kind == "coupling":
        return NC._coupling_run(d.sd, d.t, d.reverse, d.use_ld, NC.F64, lambda P, x, c, r, m, rc: NC.O.coupling(P, "", x, c, r))
    if kind == "cell":
        return NC._cell_run(d.t, d.variant, NC.F64)
    if kind == "dense":
        return NC._dense_run(d, NC.F64)
    if kind == "mix":
        return NC._mix_run(d.t, d.with_b, NC.F64)
    B, Hh, Ww, segs, Cout, k, stride, relu_in = d.shape          # conv: the statement of node_cases.conv_data
    xr, wr = [NC._leaf(v, NC.F64) for v in d.t["xs"]], NC._leaf(d.t["w"], NC.F64)
    inp = torch.cat(xr, 1)
    yr = NC._conv(None, "conv", F.relu(inp) if relu_in else inp, wr, None, 1, stride)
    (yr * d.t["gy"].double()).sum().backward()
    ref = {"y": yr.detach(), "dW": wr.grad}
    ref.update({"dx%d" % i: x.grad for i, x in enumerate(xr)})
    return ref


NODES = {
    "coupling-c8-fwd": ("coupling", lambda: NC.coupling_data("c8", False)),
    "coupling-c12_odd-rev": ("coupling", lambda: NC.coupling_data("c12_odd", True)),
    "cell-r4": ("cell", lambda: NC.cell_data("r4", "c_none")),
    "cell-r4-first_seg": ("cell", lambda: NC.cell_data("r4", "first_seg_only")),
    "dense-d6-train": ("dense", lambda: NC.dense_data("d6", "train")),
    "dense-d6-eval": ("dense", lambda: NC.dense_data("d6", "eval")),
    "mix-16": ("mix", lambda: NC.mix_data(16, "9x7", True)),
    "mix-6": ("mix", lambda: NC.mix_data(6, "9x7", False)),
    "conv-s2_5x5": ("conv", lambda: NC.conv_data("s2_5x5")),
}
NODE_IN = {"coupling": "x", "cell": "xs", "dense": "x", "mix": "x", "conv": "xs"}
NODE_GY = {"coupling": "gy", "cell": "gh", "dense": "gy", "mix": "gy", "conv": "gy"}


def _mid(t):
    return tuple(s // 2 for s in t.shape)


def build_node(name, label, H):
    kind, data = NODES[name]
    d = data()
    target, place, value = _parse(label)
    dp = copy.copy(d)
    dp.t = dict(d.t)
    if target == "x":
        key = NODE_IN[kind]
        if isinstance(d.t[key], list):
            dp.t[key] = [_poisoned(d.t[key][0], _mid(d.t[key][0]), value)] + list(d.t[key][1:])
        else:
            dp.t[key] = _poisoned(d.t[key], _mid(d.t[key]), value)
    elif target == "g":
        key = "gc" if (kind == "cell" and d.variant == "c_only") else NODE_GY[kind]
        dp.t[key] = _poisoned(d.t[key], _mid(d.t[key]), value)
    else:
        dp.sd = dict(d.sd)
        dp.sd["coupling_nn.zero_conv.scale"] = torch.full_like(d.sd["coupling_nn.zero_conv.scale"], value)
    clean = d.ref
    R = {k: v for k, v in _node_ref(kind, dp).items() if v is not None and v.is_floating_point()}
    bound = {}
    for k in R:
        if k == "ld":
            bound[k] = d.tol_ld * d.rec.sg_abs.clamp(min=1.0).reshape(clean[k].shape)
        else:
            tol = NC.mix_tol(d, k) if kind == "mix" else NC.tol_of(d, k)
            bound[k] = tol * max(1.0, float(clean[k].abs().max()))
    finite = kind == "conv" and target == "x" and value == -INF          # ConvFn rectifies its input
    return dict(d=dp, kind=kind, R=R, bound=bound, expect={}, exact=False, finite=finite, glob=target == "kappa", trips=False, mutated=None)


for _n, (_k, _) in NODES.items():
    CASES.append(_case("node", _n, [{"coupling": "CouplingTailFn", "cell": "ConvLSTMCellFn", "dense": "DenseBlockFn", "mix": "MixFn",
                                     "conv": "ConvFn"}[_k]],
                       ["x.a.nan", "x.a.pinf", "x.a.ninf", "g.a.nan"] + (["kappa.p.nan"] if _k == "coupling" else []),
                       (lambda n: lambda label, H: build_node(n, label, H))(_n), [], glob=["kappa.p.nan"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# fused coupling kernels (test_coupling_kernels.py): coupling_fwd (the staging ReLU of x1 | D, kappa) and coupling_bwd (the masks on
# x1 | D, kappa), in the home file's max-norm measure: TOL max(1, max|clean reference|) per element
# ---------------------------------------------------------------------------------------------------------------------------------
import test_coupling_kernels as CK      # noqa: E402

# name: (C, reverse / density, B, H, W, layout, mix or g)
CPL_FWD = {"f8_halves": (8, 0, 2, 9, 7, "halves", False), "f16_slice_mix": (16, 1, 2, 9, 7, "slice", True)}
CPL_BWD = {"b8_halves_dens": (8, True, 2, 9, 7, "halves", True), "b16_slice_gen": (16, False, 2, 9, 7, "slice", True)}


def _cpl_poison(inp, label):
    target, place, value = _parse(label)
    B, Hh, Ww, C_ = inp["x"].shape
    p = dict(inp)
    mid = (B - 1, Hh // 2, Ww // 2)
    if target == "x":           # a: a channel of x1 (rectified, feeds the zero conv); b: a channel of x2 (transformed)
        p["x"] = _poisoned(inp["x"], mid + (1 if place == "a" else C_ // 2 + 1,), value)
    elif target == "D":
        p["D"] = _poisoned(inp["D"], mid + (0,), value)
    elif target == "g":
        p["dout"] = _poisoned(inp["dout"], mid + (1,), value)
    else:
        p["kappa"] = torch.tensor([value])
    return p


def _maxnorm(tol, clean):
    return tol * max(1.0, float(clean.abs().max()))


def cpl_fwd_outputs(inp, reverse, mix):
    with torch.no_grad():
        R = CK.cpl_ref(inp, reverse, mix, "cpu")
    return {"out": CK._nhwc(R["out"]), "r": CK._nhwc(R["hh"][:, 1::2]), "y2": CK._nhwc(R["y2"]), "logdet": inp["ld0"].double() + R["ld"]}, R


def build_cpl_fwd(name, label, H):
    C_, reverse, B, Hh, Ww, layout, mix = CPL_FWD[name]
    inp = CK.cpl_inputs(C_, B, Hh, Ww, 7 + C_)
    clean, Rc = cpl_fwd_outputs(inp, reverse, mix)
    p = _cpl_poison(inp, label)
    R, _ = cpl_fwd_outputs(p, reverse, mix)
    scale = (inp["ld0"].abs().double() + Rc["sg"].abs().sum((1, 2, 3))).clamp(min=1.0)
    bound = {"out": _maxnorm(CK.TOL_OUT, clean["out"]), "r": _maxnorm(CK.TOL_R, clean["r"]), "y2": _maxnorm(CK.TOL_OUT, clean["y2"]),
             "logdet": CK.TOL_LD * scale}
    target, _, value = _parse(label)
    finite = value == -INF and target == "D"           # relu(-Inf) = 0 in the staging
    place = label.split(".")[1]

    def mutated():
        # the staging ReLU as fmaxf (NaN -> 0) and the kappa clamp as fminf(fmaxf(.)) (NaN -> -4)
        q = dict(p, x=torch.cat([torch.nan_to_num(p["x"][..., :C_ // 2], nan=0.0), p["x"][..., C_ // 2:]], 3), D=torch.nan_to_num(p["D"], nan=0.0),
                 kappa=torch.nan_to_num(p["kappa"], nan=-4.0))
        return cpl_fwd_outputs(q, reverse, mix)[0]
    trips = math.isnan(value) and (target in ("kappa", "D") or (target == "x" and place == "a"))
    return dict(d=p, R=R, bound=bound, expect={}, exact=False, finite=finite, glob=target == "kappa", trips=trips, mutated=mutated)


def build_cpl_bwd(name, label, H):
    C_, dens, B, Hh, Ww, layout, with_g = CPL_BWD[name]
    inp = CK.cpl_inputs(C_, B, Hh, Ww, 11 + C_)
    clean, _ = CK.cpl_bwd_ref(inp, dens, with_g, "cpu")
    p = _cpl_poison(inp, label)
    R, fw = CK.cpl_bwd_ref(p, dens, with_g, "cpu")
    bound = {k: _maxnorm(CK.TOL_BWD, clean[k]) for k in R}
    target = _parse(label)[0]
    return dict(d=p, fw=fw, R={k: v.contiguous() for k, v in R.items()}, bound=bound, expect={}, exact=False, finite=False,
                glob=target == "kappa", trips=target == "kappa",
                mutated=lambda: {k: v.contiguous() for k, v in CK.cpl_bwd_ref(dict(p, kappa=torch.tensor([-4.0])), dens, with_g, "cpu")[0].items()})


for _n in CPL_FWD:
    CASES.append(_case("coupling_fwd", _n, ["coupling_fwd"], ["x.a.nan", "x.a.pinf", "x.b.nan", "D.a.nan", "D.a.ninf", "kappa.p.nan"],
                       (lambda n: lambda label, H: build_cpl_fwd(n, label, H))(_n), ["relu", "clamp"], glob=["kappa.p.nan"]))
for _n in CPL_BWD:
    CASES.append(_case("coupling_bwd", _n, ["coupling_bwd"], ["x.a.nan", "x.b.nan", "D.a.nan", "g.a.nan", "g.a.pinf", "kappa.p.nan"],
                       (lambda n: lambda label, H: build_cpl_bwd(n, label, H))(_n), ["mask", "clamp"], glob=["kappa.p.nan"]))


# dense2_bwd on the lean kernel (test_coupling_kernels.check_d2_lean): the mask on d2 (given by D) and the upstream gradients.
# x1 and d1 are not poisoned here: d2_ref rebuilds d1 as conv(relu(x1)) + a detached constant and d2 as conv(relu([x1, d1])) + one,
# which a non-finite x1 / d1 turns into NaN over a 3x3 neighbourhood although the kernel is handed d1 and d2 themselves (seen on the
# device: finite results off the rebuilt reference); the x1 and d1 masks are reached through the CouplingTailFn node cases.
D2_LEAN = {"ch4": (4, 3, 9, 7, False), "ch12_quad": (12, 2, 9, 7, True)}


def _d2_outputs(inp, ch):
    cc = CK.CC
    W2 = torch.cat([inp["w2"][:, :ch], inp["w2"][:, ch + cc:ch + cc + 1]], 1)
    gt, g1, g2, _, _ = CK.d2_ref(inp["x1"], inp["D"], inp["G0"][..., :ch], inp["GD"], inp["w1"][:, :ch], W2, "cpu")
    return {"out": (gt + inp["add0"].double()).contiguous(), "dd1": g1.contiguous(), "dd2": g2.contiguous()}


def build_d2(name, label, H):
    ch, B, Hh, Ww, quad = D2_LEAN[name]
    target, place, value = _parse(label)
    inp = CK.d2_inputs(ch, CK.CC, B, Hh, Ww, 31 + ch)
    clean = _d2_outputs(inp, ch)
    # a pixel at which d1, d2 and x1's channels 0, 1 are positive: an upstream gradient poisoned there is not masked away
    live = (inp["D"][..., 0] > 0) & (inp["D"][..., 1] > 0) & (inp["x1"][..., 0] > 0) & (inp["x1"][..., 1] > 0)
    live[:, 0], live[:, -1], live[:, :, 0], live[:, :, -1] = False, False, False, False
    mid = tuple(int(i) for i in live.nonzero()[0])
    p = dict(inp)
    key = {"D": "D", "g": "GD", "G0": "G0"}[target]
    p[key] = _poisoned(inp[key], mid + (0 if place == "a" else 1,), value)
    R = _d2_outputs(p, ch)
    # a non-finite d1 / d2 enters the backward through its mask alone: the reference stays finite and passes the gradient there
    # (threshold_backward), which rule 2 then asks of the kernel
    return dict(d=p, R=R, bound={k: _maxnorm(CK.TOL_D2, clean[k]) for k in R}, expect={}, exact=False, finite=target == "D", glob=False,
                trips=False, mutated=None)


for _n in D2_LEAN:
    CASES.append(_case("dense2_bwd", _n, ["dense2_bwd"], ["D.b.nan", "D.b.pinf", "g.a.nan", "g.b.pinf", "G0.b.nan"],
                       (lambda n: lambda label, H: build_d2(n, label, H))(_n), ["mask"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# pointwise coupling pieces (test_pointwise_kernels.py): affine_apply, affine_bwd (kappa), masked_add
# ---------------------------------------------------------------------------------------------------------------------------------
AFF_F = {c[0]: c for c in PW.AFF_FWD if c[0] in ("f8", "s6")}
AFF_B = {c[0]: c for c in PW.AFF_BWD if c[0] in ("b8", "b6", "dodd8")}
MADD = {c[0]: c for c in PW.MADD_CASES if c[0] in ("v8", "s6")}


def build_aff_fwd(name, label, H):
    _, B, Hh, Ww, Ch, rev = AFF_F[name][:6]
    target, place, value = _parse(label)
    g = PW._gen(100 + Ch + Hh + rev)
    hh0 = 1.5 * torch.randn(B, Hh, Ww, 2 * Ch, generator=g)
    x0 = torch.randn(B, Hh, Ww, 2 * Ch, generator=g)
    ld0 = torch.randn(B, generator=g) * 3 + 1.0
    mid = (B - 1, Hh // 2, Ww // 2)
    hh, x = hh0, x0
    if target == "hh":          # a: a shift (even channel), b: a log-scale pre-activation (odd channel)
        hh = _poisoned(hh0, mid + (2 if place == "a" else 3,), value)
    else:
        x = _poisoned(x0, mid + (Ch + 1,), value)

    def outs(h, xx):
        yr, s, sg = PW.aff_ref(h, xx[..., Ch:], rev)
        K = Hh * Ww * Ch
        return {"y2": (yr, s, PW.TOL_AFF), "ld": (ld0.double() + sg.sum((1, 2, 3)), ld0.double().abs() + sg.abs().sum((1, 2, 3)), PW.tol_sum(K, 2))}
    clean = outs(hh0, x0)
    return dict(d=dict(hh=hh, x=x, ld0=ld0), R={n: r for n, (r, _, _) in outs(hh, x).items()},
                bound={n: _pw_bound(r, s, tol) for n, (r, s, tol) in clean.items()}, expect={}, exact=False, finite=False, glob=False,
                trips=False, mutated=None)


def build_aff_bwd(name, label, H):
    _, B, Hh, Ww, Ch, rev, has_g, kappa = AFF_B[name][:8]
    target, place, value = _parse(label)
    g_ = PW._gen(200 + Ch + Hh + rev)
    dy0 = torch.randn(B, Hh, Ww, 2 * Ch, generator=g_)
    y0 = torch.randn(B, Hh, Ww, 2 * Ch, generator=g_)
    r0 = 1.5 * torch.randn(B, Hh, Ww, Ch, generator=g_)
    gv = torch.randn(B, generator=g_) if has_g else None
    mid = (B - 1, Hh // 2, Ww // 2)
    d = dict(dy=dy0, y=y0, r=r0, g=gv, kappa=kappa)
    if target == "g":
        d["dy"] = _poisoned(dy0, mid + (Ch + 1,), value)
    elif target == "r":
        d["r"] = _poisoned(r0, mid + (1,), value)
    else:
        d["kappa"] = value

    def outs(q):
        gi, dhh, sdh = PW.aff_bwd_ref(q["dy"][..., Ch:], q["y"][..., Ch:], q["r"], q["g"], q["kappa"], rev)
        return {"gin": (gi, 0.0, PW.TOL_AFFB), "dhh": (dhh, sdh, PW.TOL_AFFB)}
    clean = outs(dict(dy=dy0, y=y0, r=r0, g=gv, kappa=kappa))

    def mutated():
        return {n: r for n, (r, _, _) in outs(dict(d, kappa=-4.0)).items()}
    return dict(d=d, R={n: r for n, (r, _, _) in outs(d).items()}, bound={n: _pw_bound(r, s, tol) for n, (r, s, tol) in clean.items()},
                expect={}, exact=False, finite=False, glob=False, trips=target == "kappa", mutated=mutated if target == "kappa" else None)


def build_madd(name, label, H):
    """dst += [ref > 0] src + add.  The home file states the mask as torch.where(ref > 0, v, 0); on a NaN mask operand the kernel
    follows threshold_backward, which passes the value (x <= 0 is false), so the statement here is where(ref <= 0, 0, v): the same
    on every finite operand."""
    _, B, Hh, Ww, n = MADD[name][:5]
    target, place, value = _parse(label)
    g = PW._gen(700 + n)
    shape = (B, Hh, Ww, n)
    src0, add0, dst0 = (torch.randn(shape, generator=g) for _ in range(3))
    ref0 = torch.randn(shape, generator=g)
    ref0.view(-1)[::5] = 0.0
    ref0.view(-1)[2::7] = -0.0
    pos = tuple(int(i) for i in (ref0 > 0).nonzero()[7]) if place == "a" else tuple(int(i) for i in (ref0 < 0).nonzero()[7])
    d = dict(src=src0, add=add0, dst=dst0, ref=ref0)
    key = {"src": "src", "ref": "ref", "add": "add"}[target]
    d[key] = _poisoned(d[key], pos, value)
    R = d["dst"].double() + torch.where(d["ref"].double() <= 0, torch.zeros(shape, dtype=torch.float64), d["src"].double()) + d["add"].double()
    # the result is one fp32 rounding of an exact three-term sum formed in two steps: 2 u of the magnitudes
    S = dst0.double().abs() + src0.double().abs() + add0.double().abs()
    finite = target == "ref" or (target == "src" and place == "b")          # a NaN mask passes a finite value; a masked-out NaN is dropped
    return dict(d=d, R={"dst": R}, bound={"dst": 2 * PW.U * S}, expect={}, exact=False, finite=finite, glob=False, trips=False, mutated=None)


for _n in AFF_F:
    CASES.append(_case("affine_apply", _n, ["affine_apply"], ["hh.a.nan", "hh.b.nan", "hh.b.pinf", "x.a.nan", "x.a.ninf"],
                       (lambda n: lambda label, H: build_aff_fwd(n, label, H))(_n), []))
for _n in AFF_B:
    CASES.append(_case("affine_bwd", _n, ["affine_bwd"], ["g.a.nan", "g.a.pinf", "r.a.nan", "kappa.p.nan"],
                       (lambda n: lambda label, H: build_aff_bwd(n, label, H))(_n), ["clamp"], glob=["kappa.p.nan"]))
for _n in MADD:
    CASES.append(_case("masked_add", _n, ["masked_add"], ["ref.a.nan", "ref.b.nan", "src.a.nan", "src.b.nan", "src.a.pinf", "add.b.nan"],
                       (lambda n: lambda label, H: build_madd(n, label, H))(_n), ["mask"]))


# phys_fields (test_phys_kernels.test_phys_fields): the clamped divergence / pressure residual for the 3x3 and 5x5 stencils
PHYS_FIELDS = {"k33_scaled_3x5x5": (3, 5, 5, 3, 3, True), "k55_raw_2x9x7": (2, 9, 7, 5, 5, False)}


def build_phys_fields(name, label, H):
    N_, Hh, Ww, k1, k2, scale = PHYS_FIELDS[name]
    target, place, value = _parse(label)
    u0, p0 = PH.field_inputs(N_, Hh, Ww, scale)
    mid = (N_ - 1, 0, Hh // 2, Ww // 2)
    u, p = (_poisoned(u0, mid, value), p0) if target == "u" else (u0, _poisoned(p0, mid, value))
    rd0, rp0, Sd, Sp = PH.fields_ref(u0, p0, k1, k2, scale)
    rd, rp, _, _ = PH.fields_ref(u, p, k1, k2, scale)
    R = {"us": rd.clamp(-1, 1), "ps": rp.clamp(-1, 1)}
    bound = {"us": _pw_bound(rd0.clamp(-1, 1), Sd, PH.tol_d(k1)), "ps": _pw_bound(rp0.clamp(-1, 1), Sp, PH.tol_p(k1, k2))}
    return dict(d=dict(u=u, p=p, k1=k1, k2=k2, scale=scale), R=R, bound=bound, expect={}, exact=False, finite=False, glob=False, trips=True,
                mutated=lambda: {"us": torch.nan_to_num(rd, nan=-1.0).clamp(-1, 1), "ps": torch.nan_to_num(rp, nan=-1.0).clamp(-1, 1)})


for _n in PHYS_FIELDS:
    CASES.append(_case("phys_fields", _n, ["phys_fields"], ["u.a.nan", "p.a.nan"],
                       (lambda n: lambda label, H: build_phys_fields(n, label, H))(_n), ["clamp"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# thin grouped weight gradient (thin_cases.THIN_CASES, dyc = 4: the compact pair's rows 2, 3 are zeros that the reference multiplies
# and the kernel never forms) and c1_bwd (the statement of test_hip_ops.test_c1_forward_and_backward, its mask written as
# where(dref <= 0, 0, dd): threshold_backward, the same on finite operands)
# ---------------------------------------------------------------------------------------------------------------------------------
THIN_WG = ("t_ch8_dyc4_few", "t_ch16_dyc4_few")


def build_thin_wg(name, label, H):
    case = T.THIN_BY_NAME[name]
    target, place, value = _parse(label)
    B, Hh, Ww = case["shape"]
    clean = T.thin_data(case, "gauss")
    _, S = T.thin_ref(case, clean)
    d = dict(clean)
    if target == "x":               # group 1; a: a channel of the first segment, d: the D segment's first channel
        ci = 1 if place == "a" else case["segs"][0]
        d["x"] = [clean["x"][0], _poisoned(clean["x"][1], (B - 1, Hh // 2, Ww // 2, ci), value)] + list(clean["x"][2:])
    else:
        d["dy"] = _poisoned(clean["dy"], (0, Hh // 2, Ww // 2, 1), value)
    R, _ = T.thin_ref(case, d)
    finite = target == "x" and value == -INF and "relu_in" in case["sw"]

    def mutated():
        return {"dW": T.thin_ref(case, dict(d, x=[torch.nan_to_num(t, nan=0.0) for t in d["x"]]))[0]}
    return dict(d=d, R={"dW": R}, bound={"dW": (case["K"] + 4) * T.U24 * S}, expect={}, exact=False, finite=finite, glob=False,
                trips=_trips(target, value, case["sw"]), mutated=mutated)


for _n in THIN_WG:
    CASES.append(_case("thin_wgrad", _n, ["conv_wgrad_thin_grouped"], ["x.a.nan", "x.d.nan", "x.a.pinf", "x.a.ninf", "dy.a.nan"],
                       (lambda n: lambda label, H: build_thin_wg(n, label, H))(_n), ["relu"]))

C1_BWD = {"6_5": (1, 7, 9, [6, 5]), "8_32": (2, 16, 16, [8, 32])}
C1_BWD_TOL = 5e-5


def _c1_bwd_ref(xs, w, dd, dref):
    xr = [t.double().requires_grad_(True) for t in xs]
    wr = w.double().requires_grad_(True)
    act = F.relu(torch.cat(xr, 1))
    act.retain_grad()
    yr = F.conv2d(act, wr, padding=1)
    (yr * torch.where(dref.double() <= 0, torch.zeros_like(yr), dd.double())).sum().backward()
    return {"dW": wr.grad, "gin": act.grad}


def build_c1_bwd(name, label, H):
    B, Hh, Ww, segs = C1_BWD[name]
    target, place, value = _parse(label)
    g = torch.Generator().manual_seed(17)
    xs = [torch.randn(B, c, Hh, Ww, generator=g) for c in segs]
    cin = sum(segs)
    w = 0.2 * torch.randn(1, cin, 3, 3, generator=g)
    dref = torch.randn(B, 1, Hh, Ww, generator=g)
    dd = torch.randn(B, 1, Hh, Ww, generator=g)
    clean = _c1_bwd_ref(xs, w, dd, dref)
    d = dict(xs=xs, w=w, dd=dd, dref=dref)
    live = (dref[:, 0] > 0)
    live[:, 0], live[:, -1], live[:, :, 0], live[:, :, -1] = False, False, False, False
    b, y, x = (int(i) for i in live.nonzero()[0])           # an interior pixel whose produced channel is active
    if target == "x":
        seg = 0 if place == "a" else 1
        d["xs"] = list(xs)
        d["xs"][seg] = _poisoned(xs[seg], (b, segs[seg] - 1, y, x), value)      # the segment's last channel (the scalar tail of 6 | 5)
    elif target == "g":
        d["dd"] = _poisoned(dd, (b, 0, y, x), value)
    else:
        d["dref"] = _poisoned(dref, (b, 0, y, x), value)
    R = _c1_bwd_ref(d["xs"], w, d["dd"], d["dref"])
    finite = target == "dref" or (target == "x" and value == -INF)

    def mutated():
        return _c1_bwd_ref([torch.nan_to_num(t, nan=0.0) for t in d["xs"]], w, d["dd"], d["dref"])
    return dict(d=d, R=R, bound={k: _maxnorm(C1_BWD_TOL, clean[k]) for k in R}, expect={}, exact=False, finite=finite, glob=False,
                trips=target == "x" and math.isnan(value), mutated=mutated)


for _n in C1_BWD:
    CASES.append(_case("c1_bwd", _n, ["c1_bwd"], ["x.a.nan", "x.d.nan", "x.a.ninf", "g.a.nan", "dref.a.nan"],
                       (lambda n: lambda label, H: build_c1_bwd(n, label, H))(_n), ["relu", "mask"]))


# phys_bwd (test_phys_kernels.bwd_ref: fp64 autograd of the four loss terms through clamp): one poisoned velocity / pressure value.
# The clamp's backward is a select, so the adjoint sources of a NaN residual are 0; autograd still forms 2 ux_x * 0 with a NaN
# derivative, so a poisoned VELOCITY makes the velocity gradients non-finite over the 5x5 reach (stencil, then adjoint stencil), while
# a poisoned PRESSURE, which enters linearly, leaves everything finite but its own L2 / rms terms.  Reference and kernel both multiply
# every tap, zero ones included, so no indicator treatment is needed here.  The home file leaves out the pixels within reach of a
# residual that is within 1e-4 of the clamp (`keep`): they are `allowed` here as there.
#                 B, T, H, W, coef / mean given
PHYS_BWD = {"2x9x7": (1, 2, 9, 7, True), "1x5x6": (1, 1, 5, 6, False)}


def build_phys_bwd(name, label, H):
    B, T, Hh, Ww, coef_given = PHYS_BWD[name]
    target, place, value = _parse(label)
    co = (PH.CP, PH.CD, PH.CL, PH.CR)
    y0, t, trms = PH.bwd_inputs(Hh, Ww, B, T, 1.5)
    rc = PH.bwd_ref(y0, t, trms, B, T, co, coef_given, None)
    assert rc["out_share"] <= 0.05, rc["out_share"]
    y = _poisoned(y0, (B * T - 1, 0 if target == "u" else 2, Hh // 2, Ww // 2), value)
    rp = PH.bwd_ref(y, t, trms, B, T, co, coef_given, None)
    return dict(d=dict(y=y, t=t, mean=rp["mean"] if coef_given else None, coef=rp["coef"] if coef_given else None, T=T, co=co),
                R={"dy": rp["ref"]}, bound={"dy": rc["bound"] + PW.TINY}, allowed={"dy": ~rc["keep"]}, expect={}, exact=False, finite=False,
                glob=False, trips=False, mutated=None)


for _n in PHYS_BWD:
    CASES.append(_case("phys_bwd", _n, ["phys_bwd"], ["u.a.nan", "u.a.pinf", "p.a.nan", "p.a.ninf"],
                       (lambda n: lambda label, H: build_phys_bwd(n, label, H))(_n), []))


# dense2_bwd on the general kernel (test_coupling_kernels.check_d2_general: three input segments, two gradient / output segments,
# dW1 / dW2 accumulated): the same poisons as the lean cases, for the same reason
D2_GENERAL = {"ch8_wg": (8, 2, 9, 7, True)}


def _d2g_outputs(inp, ch):
    t0 = torch.cat([inp["x1"], inp["cond"]], 3)
    gt, g1, g2, gw1, gw2 = CK.d2_ref(t0, inp["D"], inp["G0"], inp["GD"], inp["w1"], inp["w2"], "cpu")
    return {"out0": (gt[..., :ch] + inp["add0"].double()).contiguous(), "out1": gt[..., ch:].contiguous(), "dd1": g1.contiguous(),
            "dd2": g2.contiguous(), "dW1": gw1 + inp["dW1"].double(), "dW2": gw2 + inp["dW2"].double()}


def build_d2_general(name, label, H):
    ch, B, Hh, Ww, _ = D2_GENERAL[name]
    target, place, value = _parse(label)
    inp = CK.d2_inputs(ch, CK.CC, B, Hh, Ww, 41 + ch)
    clean = _d2g_outputs(inp, ch)
    live = (inp["D"][..., 0] > 0) & (inp["D"][..., 1] > 0) & (inp["x1"][..., 0] > 0) & (inp["x1"][..., 1] > 0)
    live[:, 0], live[:, -1], live[:, :, 0], live[:, :, -1] = False, False, False, False
    mid = tuple(int(i) for i in live.nonzero()[0])
    p = dict(inp)
    key = {"D": "D", "g": "GD", "G0": "G0"}[target]
    p[key] = _poisoned(inp[key], mid + (0 if place == "a" else 1,), value)
    R = _d2g_outputs(p, ch)
    return dict(d=p, R=R, bound={k: _maxnorm(CK.TOL_D2, clean[k]) for k in R}, expect={}, exact=False, finite=target == "D", glob=False,
                trips=False, mutated=None)


for _n in D2_GENERAL:
    CASES.append(_case("dense2_bwd", _n, ["dense2_bwd"], ["D.b.nan", "D.b.pinf", "g.a.nan", "g.b.pinf", "G0.b.nan"],
                       (lambda n: lambda label, H: build_d2_general(n, label, H))(_n), ["mask"]))


# coupling_bwd in the summed form (test_coupling_presum.py: G0 == NULL, the first half of dtin receives dto1 + [x1 > 0] G0 and GD carries
# the packed mask bits that dense2_bwd(g0_masked) selects by): the mask as threshold_backward states it, where(x1 <= 0, 0, G0), and a
# bit that is SET for a NaN x1
CPL_BWD_SUM = {"b8_halves_dens_sum": CPL_BWD["b8_halves_dens"], "b16_slice_gen_sum": CPL_BWD["b16_slice_gen"]}


def build_cpl_bwd_sum(name, label, H):
    C_, dens, B, Hh, Ww, layout, with_g = CPL_BWD_SUM[name]
    ch = C_ // 2
    run = build_cpl_bwd(name[:-4], label, H)

    def summed(ref, x):
        x1 = x[..., :ch].double()
        return {"sum1": (ref["dtin"][..., :ch] + torch.where(x1 <= 0, torch.zeros_like(ref["G0"]), ref["G0"])).contiguous(),
                "dtin2": ref["dtin"][..., ch:].contiguous(), "DH": ref["DH"], "GD01": ref["GD"][..., :2].contiguous()}
    inp = CK.cpl_inputs(C_, B, Hh, Ww, 11 + C_)
    clean = summed(CK.cpl_bwd_ref(inp, dens, with_g, "cpu")[0], inp["x"])
    R = summed(run["R"], run["d"]["x"])
    # x1 = -Inf is rectified away in the forward and masked out here: every gradient stays finite
    return dict(run, R=R, bound={k: _maxnorm(CK.TOL_BWD, clean[k]) for k in R}, finite=label == "x.a.ninf", trips=False, mutated=None)


for _n in CPL_BWD_SUM:
    CASES.append(_case("coupling_bwd", _n, ["coupling_bwd"], ["x.a.nan", "x.a.pinf", "x.a.ninf", "D.a.nan", "g.a.nan", "kappa.p.nan"],
                       (lambda n: lambda label, H: build_cpl_bwd_sum(n, label, H))(_n), ["mask"], glob=["kappa.p.nan"]))
