"""The growth-layer forwards (c1x2_fwd_kernel<CG>, c1_fwd_kernel), the thin and mix weight gradients (wgrad_thin_kernel<SL, CS, TH>,
mix_wgrad_kernel<CT>), layer_planes_kernel and the plain channel mixes (mix32_kernel<NT, NP, 0>, mix16_kernel<NT, NP>) against fp64
on every launch plan: every case of thin_cases.py in integer mode (bit-exact) and, where K <= 2048, in Gaussian mode (elementwise
bound).  Case tables, references, K and c of the bounds: thin_cases.py; that the tables reach every instance and plan feature, and
which case catches which defect: test_thin_plans_cpu.py.

The weight gradients are called through tmg_hip.conv_wgrad_thin_grouped / mix_wgrad_grouped, which return the library's code: a
declined launch (-100) cannot pass as a tested one.  Before every launch the plan of the ACTUAL operands (their addresses and strides)
is queried and must equal the plan the case was chosen for.  Every output is a view inside a NaN-filled buffer - pixel stride wider
than the channels, guard rows before and after - and every float outside the view must be bit-identical afterwards; declined and
refused calls run on NaN-filled outputs, which must stay NaN.

Observed on an MI355X (LAB_NOTES.md, "The growth-layer, thin and mix kernels against fp64 on every launch plan"): 341 passed in 6.4 s,
integer mode bit-exact everywhere; largest / median share of the Gaussian bound over a family's cases (the SHARE lines this module
prints): c1x2 0.0452 / 0.0117 (35 cases), c1_fwd 0.0716 / 0.0052 (13), thin 0.2094 / 0.0009 (23; 0.1333 in another run: the atomics'
order), mix_wgrad 0.1829 / 0.0011 (12), mix_f32 0.2965 / 0.0488 (26), mix_f16 0.3984 / 0.1757 (34).  K and c of the bounds were fixed
before the first device run and not touched afterwards.
"""
import statistics

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import thin_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SHARES = {}
MODES = ("int", "gauss")


def _H():
    import tmg_hip as H
    return H


@pytest.fixture(scope="module", autouse=True)
def _report_shares():
    yield
    for fam in sorted(SHARES):
        v = sorted(SHARES[fam].values())
        print("SHARE %-12s max %.4f median %.4f over %d cases" % (fam, v[-1], statistics.median(v), len(v)))


def _record(fam, name, v):
    SHARES.setdefault(fam, {})[name] = max(SHARES.get(fam, {}).get(name, 0.0), v)


# ---------------------------------------------------------------------------------------------------------------------------------
# buffers: a view of n channels at channel offset `off` of rows of `width` floats, `mis` floats off 16-byte alignment, GUARD rows of
# NaN before and after
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 4


class Buf:
    def __init__(self, shape, width=None, off=0, mis=0, data=None):
        n = shape[-1]
        npix = 1
        for s in shape[:-1]:
            npix *= s
        width = width or n
        self.base = torch.full(((npix + 2 * GUARD) * width + 4,), NAN, dtype=torch.float32, device=DEV)
        lo = GUARD * width + mis
        rows = self.base[lo:lo + npix * width].view(*shape[:-1], width)
        self.view = rows[..., off:off + n]
        m = torch.zeros_like(self.base, dtype=torch.bool)
        m[lo:lo + npix * width].view(*shape[:-1], width)[..., off:off + n] = True
        self.mask = m
        if data is not None:
            self.view.copy_(data.to(DEV).float().reshape(shape))
        self.snap = None

    def arm(self):
        self.snap = self.base.clone()
        return self

    def intact(self, written=True):
        """Every float outside the view (written = False: every float) is bit-identical to what it was when armed."""
        a, b = self.base.view(torch.int32), self.snap.view(torch.int32)
        if written:
            return bool((a[~self.mask] == b[~self.mask]).all())
        return bool((a == b).all())


def _in(t64, spec):
    n, width, off, mis = spec
    return Buf(tuple(t64.shape), width, off, mis, data=t64).view


def _segments(x, specs):
    out, c = [], 0
    for sp in specs:
        out.append(_in(x[..., c:c + sp[0]], sp))
        c += sp[0]
    return out


def _same_plan(got, want):
    assert got == want, "the launch's plan differs from the case's:\n  %s\n  %s" % (got, want)


def _judge(fam, case, mode, pairs):
    """pairs: (result, reference, bound or None).  Integer mode: bit-exact; Gaussian mode: share <= 1 (printed before asserted)."""
    if mode == "int":
        for a, ref, _ in pairs:
            assert T.exact(a, ref), "%s: not bit-equal to fp64 in integer mode (%d of %d elements differ)" % (
                case["name"], int((a.detach().double().to(ref.device) != ref).sum()), ref.numel())
        return
    v = max(T.share(a, ref, b) for a, ref, b in pairs)
    print("share %s %.4f" % (case["name"], v))
    _record(fam, case["name"], v)
    assert v <= 1.0, "%s: %.3g of its bound" % (case["name"], v)


def _params(cases):
    return [pytest.param(c, m, id="%s-%s" % (c["name"], m)) for c in cases for m in MODES if m == "int" or c["gauss"]]


# ---------------------------------------------------------------------------------------------------------------------------------
# c1x2
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _params(T.C1X2_CASES))
def test_c1x2(case, mode):
    H = _H()
    d = T.fwd_data(case, mode)
    ref, S = T.c1x2_ref(case, d)
    if mode == "int":
        assert T.int_terms_ok(S["S2"]) and T.int_terms_ok(S["S1"])
    B, (Hh, Ww) = case["B"], case["hw"]
    ins = _segments(d["x"], case["ins"])
    w1, w2 = d["w1"].float().to(DEV).contiguous(), d["w2"].float().to(DEV).contiguous()
    a1 = _in(d["add1"], T.seg(1, 2, 0)) if d["add1"] is not None else None
    a2 = _in(d["add2"], T.seg(1, 2, 1)) if d["add2"] is not None else None
    out = Buf((B, Hh, Ww, 4), width=8).arm()
    w_rows, split, gap, d1row, _ = T._w_params(case)
    kw = dict(w_rows=w_rows, w2_d1_row=d1row, add1=a1, add2=a2, w_split=split, w_gap=gap, relu_in="relu_in" in case["sw"])
    _same_plan(H.c1x2_fwd_plan(ins, out.view, **kw), T.c1x2_plan(H, case))
    H.c1x2_fwd(ins, w1, w2, out.view, **kw)           # raises unless the library returns 0
    torch.cuda.synchronize()
    assert out.intact(), "%s: wrote outside its output view" % case["name"]
    got = out.view
    assert bool((got[..., 2:] == 0).all()), "%s: channels 2, 3 of the output are not exactly 0" % case["name"]
    _judge("c1x2", case, mode, [(got, ref, T.c1x2_bound(case, S))])


# ---------------------------------------------------------------------------------------------------------------------------------
# c1_fwd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _params(T.C1_CASES))
def test_c1_fwd(case, mode):
    H = _H()
    sw = case["sw"]
    d = T.c1_data(case, mode)
    ref, S = T.c1_ref(case, d)
    if mode == "int":
        assert T.int_terms_ok(S)
    B, (Hh, Ww) = case["B"], case["hw"]
    w = d["w1"].float().to(DEV).contiguous()
    ad = _in(d["add"], T.seg(1, 2, 1)) if d["add"] is not None else None
    z3 = torch.zeros(B, Hh, Ww, 3, dtype=torch.float64)
    if "inplace" in sw:
        # the production second layer: inputs [x1, D], output D[..., 1:2]
        ins = _segments(d["x"][..., :-4], case["ins"][:-1])
        D = Buf((B, Hh, Ww, 1), width=4, off=1)
        Dfull = D.base[GUARD * 4:GUARD * 4 + B * Hh * Ww * 4].view(B, Hh, Ww, 4)
        Dfull.copy_(d["x"][..., -4:].float())
        ins.append(Dfull)
        out, ov = D.arm(), D.view
    elif "fill4" in sw:
        ins = _segments(d["x"], case["ins"])
        out = Buf((B, Hh, Ww, 4), width=8).arm()
        ov = out.view[..., 0:1]
        ref, S = torch.cat([ref, z3], 3), torch.cat([S, z3], 3)
    else:
        ins = _segments(d["x"], case["ins"])
        out = Buf((B, Hh, Ww, 1), width=4).arm()
        ov = out.view
    _, split, gap, _, _ = T._c1_params(case)
    kw = dict(w_rows=case["w_rows"], fill4="fill4" in sw, add=ad, w_split=split, w_gap=gap, relu_in="relu_in" in sw)
    _same_plan(H.c1_fwd_plan(ins, ov, **kw), T.c1_plan(H, case))
    H.c1_fwd(ins, w, ov, **kw)
    torch.cuda.synchronize()
    assert out.intact(), "%s: wrote outside its output view" % case["name"]
    _judge("c1_fwd", case, mode, [(out.view, ref, (case["K"] + 4) * T.U24 * S)])


# ---------------------------------------------------------------------------------------------------------------------------------
# thin grouped weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _params(T.THIN_CASES))
def test_thin_wgrad(case, mode):
    H = _H()
    G, dyc, cin = case["G"], case["dyc"], case["cin"]
    d = T.thin_data(case, mode)
    groups = []
    for g in range(G):
        # production: the first group's first segment is a channel slice of a twice as wide tensor, the others tensors of their own
        # (different pixel strides per table row); widths are multiples of 4 so that only the LIBRARY can decline a 6-channel segment
        specs = [T.seg(n, 2 * n if (g == 0 and i == 0) else (n + 3) // 4 * 4, 0) for i, n in enumerate(case["segs"])]
        groups.append(_segments(d["x"][g], specs))
    dy = _in(d["dy"], (dyc * G, case["dy_width"], case["dy_off"], case["dy_mis"]))
    declined = case["rc"] != 0
    dW = Buf((1, G * 4 * cin * 9), data=None if declined else (d["prev"] if d["prev"] is not None else torch.zeros(G * 4 * cin * 9))).arm()
    plan = H.conv_wgrad_thin_grouped_plan(case["shape"], case["segs"], G, dy.data_ptr(), dy.stride(2), dyc, relu_in="relu_in" in case["sw"])
    _same_plan(plan, T.thin_plan(H, case))
    rc = H.conv_wgrad_thin_grouped(groups, dy, dyc, dW.view.view(G, 4, cin, 3, 3), relu_in="relu_in" in case["sw"])
    torch.cuda.synchronize()
    assert rc == case["rc"] == plan["rc"], "%s: returned %d" % (case["name"], rc)
    if declined:
        assert dW.intact(written=False) and bool(torch.isnan(dW.view).all()), "%s: a declined call wrote" % case["name"]
        return
    assert dW.intact()
    ref, S = T.thin_ref(case, d)
    if mode == "int":
        assert T.int_terms_ok(S)
    got = dW.view.view(G, 4, cin, 3, 3)
    if dyc == 2:
        prev = d["prev"][:, 2:].float().to(DEV) if d["prev"] is not None else torch.zeros(G, 2, cin, 3, 3, device=DEV)
        assert bool((got[:, 2:] == prev).all()), "%s: rows 2, 3 of a compact group's dW changed" % case["name"]
    _judge("thin", case, mode, [(got, ref, (case["K"] + 4) * T.U24 * S)])


# ---------------------------------------------------------------------------------------------------------------------------------
# mix weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _params(T.MIXWG_CASES))
def test_mix_wgrad(case, mode):
    H = _H()
    G, Cn, n = case["G"], case["C"], case["npix"]
    d = T.mixwg_data(case, mode)
    h = Cn // 2
    s1, s2 = T.PAIR_STRIDES(Cn)
    sets = []
    for k in range(case["sets"]):
        x, dy = d["x"][k].reshape(1, 1, n, Cn), d["dy"][k].reshape(1, 1, n, Cn)
        xin = _segments(x, [T.seg(c, 2 * c if i == 0 else c + 4, 0 if i == 0 else 4) for i, c in enumerate(case["segs"])])
        if "pair" in case["sw"]:
            dyt = (_in(dy[..., :h], T.seg(h, s1, 0)), _in(dy[..., h:], T.seg(h, s2, 4)))
        else:
            dyt = _in(dy, T.seg(Cn, Cn + 4, 4))
        sets.append((xin, dyt))
    groups = [sets[g % case["sets"]][0] for g in range(G)]
    gdy = [sets[g % case["sets"]][1] for g in range(G)]
    declined = case["rc"] != 0
    zW, zb = torch.zeros(G * Cn * Cn), torch.zeros(G * Cn)
    dW = Buf((1, G * Cn * Cn), data=None if declined else (d["prevW"] if d["prevW"] is not None else zW)).arm()
    db = Buf((1, G * Cn), data=None if declined else (d["prevb"] if d["prevb"] is not None else zb)).arm()
    use_db = "db" in case["sw"] or declined
    plan = H.mix_wgrad_grouped_plan(n, Cn, G, db=use_db)
    _same_plan(plan, T.mixwg_plan(H, case))
    rc = H.mix_wgrad_grouped(groups, gdy, dW.view.view(G, Cn, Cn), db.view.view(G, Cn) if use_db else None)
    torch.cuda.synchronize()
    assert rc == case["rc"] == plan["rc"], "%s: returned %d" % (case["name"], rc)
    if declined:
        assert dW.intact(written=False) and db.intact(written=False) and bool(torch.isnan(dW.view).all()), "%s: a declined call wrote" % case["name"]
        return
    assert dW.intact() and db.intact(written=use_db)
    if case["big"]:
        d = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else (v.to(DEV) if v is not None else None)) for k, v in d.items()}
    rW, SW, rb, Sb = T.mixwg_ref(case, d)
    if mode == "int":
        assert T.int_terms_ok(SW) and T.int_terms_ok(Sb)
    pairs = [(dW.view.view(G, Cn, Cn), rW, (case["K"] + 4) * T.U24 * SW)]
    if use_db:
        pairs.append((db.view.view(G, Cn), rb, (case["K"] + 4) * T.U24 * Sb))
    _judge("mix_wgrad", case, mode, pairs)


# ---------------------------------------------------------------------------------------------------------------------------------
# layer planes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.PLANES_CASES, ids=lambda c: c["name"])
def test_layer_planes(case):
    H = _H()
    n, cp = case["npix"], case["CP"]
    g = torch.Generator().manual_seed(8000 + n + cp)
    src = torch.randn(max(n, 1), max(cp, 4), generator=g).to(DEV)
    dst = Buf((1, max(n, 1) * max(cp, 4))).arm()
    rc = H.lib().tmg_layer_planes(H._ptr(src), H._ptr(dst.view), H.c_i64(n), H.c_i64(cp), H._stream())
    torch.cuda.synchronize()
    assert rc == case["rc"], "%s: returned %d" % (case["name"], rc)
    if rc != 0:
        assert dst.intact(written=False), "%s: a refused call wrote" % case["name"]
        return
    assert dst.intact()
    ref = T.planes_ref(src)
    assert bool((dst.view.view(cp // 2, n, 2) == ref).all()), case["name"]
    if n * cp <= 65 * 32:
        assert bool((H.layer_planes(src.view(1, 1, n, cp)).reshape(cp // 2, n, 2) == ref).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# channel mixes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _params(T.MIX_CASES))
def test_mix(case, mode):
    H = _H()
    n, Cn, f16 = case["npix"], case["C"], case["kind"] == "f16"
    d = T.mix_data(case, mode)
    x = _in(d["x"].reshape(1, 1, n, Cn), T.seg(Cn, *case["xw"]))
    W = d["W"].float().to(DEV).contiguous()
    bias = d["bias"].float().to(DEV) if d["bias"] is not None else None
    y = Buf((1, 1, n, Cn), *case["yw"]).arm()
    tr = "transposed" in case["sw"]
    if case["rc"] != 0:
        fn = H.lib().tmg_mix_f16 if f16 else H.lib().tmg_mix_f32
        rc = fn(H._ptr(x), H._i64(x.stride(2), 0), H._ptr(W), H._ptr(bias), H._ptr(y.view), H._i64(y.view.stride(2), 0),
                H._i64(n, Cn, 1 if tr else 0), H._stream())
        torch.cuda.synchronize()
        assert rc == case["rc"], "%s: returned %d" % (case["name"], rc)
        assert y.intact(written=False), "%s: a refused call wrote" % case["name"]
        if not f16:
            assert Cn % 4 == 0 and Cn <= 128 or H.mix_f32(x, W, bias, y.view, transposed=tr) is False
        return
    assert (case["NT"], case["NP"], case["grid"], case["rounds"]) == T.mix_plan(case["kind"], Cn, n)
    if f16:
        H.mix_f16(x, W, bias, y.view, transposed=tr)          # raises unless the library returns 0
    else:
        assert H.mix_f32(x, W, bias, y.view, transposed=tr) is True
    torch.cuda.synchronize()
    assert y.intact(), "%s: wrote outside its output view" % case["name"]
    if case["big"]:
        d = {k: (v.to(DEV) if v is not None else None) for k, v in d.items()}
    ref, S = T.mix_ref(case, d)
    if mode == "int":
        assert T.int_terms_ok(S)
    pairs = [(y.view.reshape(n, Cn), ref, T.mix_bound(case, S))]
    if f16 and mode == "gauss":
        # the result differs from the fp32 product by fp16's rounding of the two operands, and not by more
        r32, S32 = T.mix_ref(case, d, half=False)
        pairs.append((y.view.reshape(n, Cn), r32, (2 * 2.0 ** -11 + 2.0 ** -22) * S32 + T.mix_bound(case, S32)))
    _judge("mix_f16" if f16 else "mix_f32", case, mode, pairs)
