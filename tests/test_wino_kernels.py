"""The Winograd kernels of tmg_wino.hip, each called through its tmg_hip wrapper and compared with a plain fp64 reference of the same
operation (wino_cases.py), on every kernel instance and at the edges of the launch plans - among them the persistent tile loop (a block's
second and third tile), the reduce widths NG = 8 / 16, the grouped weight gradient and the destination mappings, which the case lists of
test_hip_ops.py::test_winograd_* never reach.

Every case first asserts, through the library's own plan query on the very tensors it is about to pass, that it runs on the kernel
instance and plan fields its name states (where that depends on the compute-unit count the batch is the smallest one the planner sends
there).  Every operand is a view inside a NaN parent (test_conv_kernels.Buf), outputs are NaN-prefilled (the accumulating dW / dbias:
known values inside a NaN parent), and everything outside the views must stay as it was.

Two data modes (wino_cases.py derives both, with the counts c):
  int    small integers, 4 S^W < 2^24: every kernel, bf16x3 included, must equal fp64 BIT FOR BIT (carries the many-pixel plans);
  gauss  |a_i - ref_i| <= (K + c) 2^-24 S^W_i elementwise, S^W the fp64 Winograd sum of absolute values; only where K <= 2048.

Case map (wino_cases.py):
  test_wino_fwd       FWD_CASES on tmg_conv_wino_fwd (f32: wino_fwdp_kernel<1> up to 128 output channels, wino_fwd_kernel<2> above) and
                      tmg_conv_wino_fwd3 (bf16x3: wino_fwd3_kernel<1> / <2>): f_cin* / f2_cin* channel counts, chunk fills, gy, odd
                      Npad / 16, Cout % 16; f*_in2 / in3 / out2 / out3 segments; bf3_parts_v / _u; f*_hwHxW_zero / _rep small images;
                      p_* the persistent loop (two and three tiles per block, unequal counts, 1 and 3 chunks, a half-full last chunk).
  test_wino_narrow    NARROW_CASES on tmg_conv_wino_narrow: NTN 1 - 3, switches, three output segments, the mode-1 operand, small
                      images, p_nn_* the persistent loop.
  test_wino_wgrad     WG_CASES: every (CIT, NCO) with DB = 0 on (4, 4), gy / gz > 1, gx 1 / odd share, NG 4 / 8 / 16, operands, layouts.
  test_wino_wgrad_grouped  GROUPED_CASES through tmg_hip.conv_wgrad_grouped: G = 2, 3, strides per group, dy slice, bpg 1 and 2.
  test_wino_pack*, test_declined_calls_write_nothing.
Measured shares of the bounds: LAB_NOTES.md."""
import ctypes
import functools

import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import conv_cases as CC
import wino_cases as WC
from test_conv_kernels import Buf, _dev, _split

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _H():
    import tmg_hip as H
    return H


def _check(got, ref, S, K, c, mode, what):
    if mode == "int":
        assert CC.bit_equal(got, ref), "%s: integer mode is not bit-exact (max |diff| %g)" % (
            what, float((got.detach().cpu().double() - ref).abs().nan_to_num(float("inf")).max()))
        return
    share = CC.gauss_share(got, ref, S, K + c - 8)          # conv_cases.gauss_share bounds by (its K + 8) u S
    print("SHARE %s %.4f" % (what, share))
    assert share <= 1.0, "%s: %.3f of the bound (K + c) 2^-24 S^W, K = %d, c = %d" % (what, share, K, c)


class Flat:
    """A contiguous tensor of known values with 4 NaN floats in front and behind (dW, dbias: the kernels accumulate onto them)."""

    def __init__(self, init):
        self.flat = torch.full((init.numel() + 8,), NAN, device=DEV)
        self.t = self.flat[4:4 + init.numel()].view(init.shape)
        self.t.copy_(init.to(DEV, torch.float32))

    def intact(self):
        return int(torch.isnan(self.flat).sum()) == 8


@functools.lru_cache(maxsize=2)
def _fwd_ref(name, narrow, B, mode):
    """Data and reference of a forward case, computed once for the f32 and the bf16x3 run; nobody writes to them."""
    case = (WC.NARROW_BY_NAME if narrow else WC.FWD_BY_NAME)[name]
    d = WC.fwd_data(case, B, mode)
    return (d,) + WC.fwd_ref(case, d)


def _params(cases, ariths):
    return [pytest.param(c, a, m, id="%s-%s-%s" % (c["name"], a, m)) for c in cases for m in (("int", "gauss") if c["gauss"] else ("int",))
            for a in ariths]


def _run_fwd(case, arith, mode):
    H = _H()
    B, _ = WC.resolve_fwd(H, case, arith)
    Hh, Ww = case["hw"]
    d, ref, S = _fwd_ref(case["name"], case["narrow"], B, mode)
    if mode == "int":
        assert CC.int_terms_ok(S, WC.GRAN)
    ins = _split(d["x"], case["ins"], (B, Hh, Ww))
    outs = _split(None, case["outs"], (B, Hh, Ww))
    _, cout, _, kw = WC.fwd_args(case, B)
    kw["bias"] = _dev(d["bias"])
    p = WC.fwd_plan_fn(H, case, arith)([b.view for b in ins], cout, [b.view for b in outs], **kw)
    assert WC.fwd_plan_ok(case, arith, p), (case["name"], arith, p)
    pmode, nvalid = (1, case["dgrad"][1]) if case["dgrad"] else (0, 0)
    wd = _dev(d["w"])
    if case["narrow"]:
        ok = H.conv_wino_narrow([b.view for b in ins], H.conv_wino_pack(wd, pmode, nvalid), cout, [b.view for b in outs], **kw)
    elif arith == "bf16x3":
        ok = H.conv_wino_fwd3([b.view for b in ins], H.conv_wino_pack3(wd, pmode, nvalid), cout, [b.view for b in outs], **kw)
    else:
        ok = H.conv_wino_fwd([b.view for b in ins], H.conv_wino_pack(wd, pmode, nvalid), cout, [b.view for b in outs], **kw)
    torch.cuda.synchronize()
    assert ok, "the launcher declined the case"
    got = torch.cat([b.view for b in outs], 3)
    _check(got, ref, S, p["Cin_pad"], WC.fwd_c(p["kernel"], p["nchunks"]), mode, "%s %s" % (case["name"], arith))
    assert all(b.intact() for b in outs), "written outside the output segments"
    assert all(b.intact() for b in ins)


@pytest.mark.parametrize("case,arith,mode", _params(WC.FWD_CASES, ("f32", "bf16x3")))
def test_wino_fwd(case, arith, mode):
    _run_fwd(case, arith, mode)


@pytest.mark.parametrize("case,arith,mode", _params(WC.NARROW_CASES, ("f32",)))
def test_wino_narrow(case, arith, mode):
    _run_fwd(case, arith, mode)


# ---------------------------------------------------------------------------------------------------------------------------------
def _modes(cases):
    return [pytest.param(c, m, id="%s-%s" % (c["name"], m)) for c in cases for m in (("int", "gauss") if c["gauss"] else ("int",))]


@pytest.mark.parametrize("case,mode", _modes(WC.WG_CASES))
def test_wino_wgrad(case, mode):
    H = _H()
    B, _ = WC.resolve_wg(H, case)
    _, Hh, Ww = case["shape"]
    sw = case["sw"]
    cd, cv, cs, o0, o1 = case["layout"]
    d = WC.wg_data(case, B, mode)
    Wr, SW, br, Sb, touched = WC.wg_ref(case, d)
    K = WC.wg_dy_tiles((B, Hh, Ww))
    if mode == "int":
        assert CC.int_terms_ok(SW, WC.GRAN) and CC.int_terms_ok(Sb)
    else:
        assert K <= CC.KMAX_GAUSS
    ins = _split(d["x"], case["ins"], (B, Hh, Ww))
    dy = Buf((B, Hh, Ww), case["dy"], d["dy"])
    dW = Flat(d["prevW"])
    db = Flat(d["prevb"]) if "dbias" in sw else None
    kw = dict(relu_in="relu_in" in sw, pad_rep="rep" in sw, cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    p = H.conv_wino_wgrad_plan([b.view for b in ins], dy.view, dbias=db.t if db else None, **kw)
    assert WC.wg_plan_ok(case, p), (case["name"], p)
    ok = H.conv_wino_wgrad([b.view for b in ins], dy.view, dW.t, db.t if db else None, **kw)
    torch.cuda.synchronize()
    assert ok, "the launcher declined the case"
    _check(dW.t, Wr, SW, K, WC.wg_c(p), mode, case["name"] + " dW")
    keep = ~touched.to(DEV)
    assert torch.equal(dW.t[:, keep], _dev(d["prevW"])[:, keep]), "columns outside the destination changed"
    if db is not None:
        _check(db.t, br, Sb, WC.wg_kb(p), 1, mode, case["name"] + " dbias")
    assert dW.intact() and (db is None or db.intact()) and dy.intact() and all(b.intact() for b in ins)


@pytest.mark.parametrize("case,mode", _modes(WC.GROUPED_CASES))
def test_wino_wgrad_grouped(case, mode, monkeypatch):
    H = _H()
    G, cin, cg = case["G"], case["cin"], case["cout"]
    B, Hh, Ww = case["shape"]
    sw = case["sw"]
    cd, cv, cs, o0, o1 = case["layout"]
    ds = WC.grouped_data(case, mode)
    refs = WC.grouped_ref(case, ds)
    K = WC.wg_dy_tiles((B, Hh, Ww))
    # group inputs with different pixel strides: even groups a channel-slice view at offset 4 of a wider tensor, odd ones their own
    ins = [Buf((B, Hh, Ww), CC.seg(cin, cin + 8, 4) if g % 2 == 0 else CC.seg(cin), d["x"]) for g, d in enumerate(ds)]
    assert len({b.view.stride(2) for b in ins}) == 2
    dy = Buf((B, Hh, Ww), CC.seg(G * cg, G * cg + 8, 4) if case["dy_slice"] else CC.seg(G * cg), torch.cat([d["dy"] for d in ds], 3))
    dW = Flat(torch.stack([d["prevW"] for d in ds]).reshape(G, cg, cd or cin, 3, 3))
    db = Flat(torch.stack([d["prevb"] for d in ds])) if "dbias" in sw else None
    kw = dict(relu_in="relu_in" in sw, pad_rep="rep" in sw, cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    one = ((B, Hh, Ww), dy.view.data_ptr(), dy.view.stride(2), cg)       # one group's dy channels
    p = H.conv_wino_wgrad_plan([ins[0].view], one, dbias=db.t if db else None, ngroups=G, **kw)
    assert WC.wg_plan_ok(case, p) and p["gy"] == G * p["bpg"], (case["name"], p)

    def _not_winograd(*a, **k):
        raise AssertionError("%s fell through to the direct grouped kernel" % case["name"])
    monkeypatch.setattr(H.lib(), "tmg_conv_wgrad_grouped", _not_winograd)
    ok = H.conv_wgrad_grouped([[b.view] for b in ins], dy.view, cg, dW.t, db.t if db else None, 3, 1, **kw)
    torch.cuda.synchronize()
    assert ok
    for g, (Wr, SW, br, Sb, touched) in enumerate(refs):
        if mode == "int":
            assert CC.int_terms_ok(SW, WC.GRAN) and CC.int_terms_ok(Sb)
        got = dW.t[g].reshape(cg, cd or cin, 9)
        _check(got, Wr, SW, K, WC.wg_c(p), mode, "%s dW[%d]" % (case["name"], g))
        keep = ~touched.to(DEV)
        assert torch.equal(got[:, keep], _dev(ds[g]["prevW"])[:, keep]), "columns outside the destination changed"
        if db is not None:
            _check(db.t[g], br, Sb, WC.wg_kb(p), 1, mode, "%s dbias[%d]" % (case["name"], g))
    assert dW.intact() and (db is None or db.intact()) and dy.intact() and all(b.intact() for b in ins)


# ---------------------------------------------------------------------------------------------------------------------------------
# (Cout, Cin, mode, nvalid) of a [Cout][Cin][3][3] weight
PACK_CASES = [(20, 24, 0, 0), (64, 104, 0, 0), (68, 40, 1, 36), (72, 40, 1, 12), (36, 20, 1, 0), (4, 64, 0, 0), (132, 8, 1, 40)]


def _raw_pack(H, name, w, out, mode, nvalid):
    """tmg_conv_wino_pack / _pack3 on a destination the TEST owns (the wrappers allocate theirs with torch.empty): every float of `out`
    starts as NaN, so padding the packer does not write stays NaN."""
    c_i64 = ctypes.c_int64
    rc = getattr(H.lib(), name)(H._ptr(w), H._ptr(out), c_i64(w.shape[0]), c_i64(w.shape[1]), c_i64(mode), c_i64(nvalid), H._stream())
    assert rc == 0, (name, rc)


@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_wino_pack_equals_the_documented_layout(kind):
    H = _H()
    g = torch.Generator().manual_seed(8000)
    for cout, cin, mode, nvalid in PACK_CASES:
        w = CC.rnd(g, (cout, cin, 3, 3), kind, 5)
        ref = WC.pack_ref(w, mode, nvalid)
        wd = _dev(w)
        out = torch.full((ref.numel() + 4,), NAN, device=DEV)
        _raw_pack(H, "tmg_conv_wino_pack", wd, out, mode, nvalid)
        got = H.conv_wino_pack(wd, mode, nvalid)
        assert got.numel() == ref.numel() and torch.equal(got, out[:-4]) and bool(torch.isnan(out[-4:]).all()), (cout, cin, mode, nvalid)
        gotd = got.cpu().double()
        Uabs = WC.pack_ref(w, mode, nvalid, absolute=True)
        assert bool((gotd[Uabs == 0] == 0).all()), "padding entries must be exactly zero"
        if kind == "int":
            assert torch.equal(gotd, ref), (cout, cin, mode, nvalid)       # multiples of 1/4: exact
        else:
            # four additions (two per pass of G g G^T) on the sum of the absolute terms
            assert bool(((gotd - ref).abs() <= 4 * CC.U24 * Uabs).all()), (cout, cin, mode, nvalid)


@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_wino_pack3_parts_sum_to_the_fp32_operand(kind):
    H = _H()
    g = torch.Generator().manual_seed(8100)
    for cout, cin, mode, nvalid in PACK_CASES:
        w = CC.rnd(g, (cout, cin, 3, 3), kind, 300)
        wd = _dev(w)
        _, K, N = WC.pack_operand(w, mode, nvalid)
        Kp16, Kp32, Np = (K + 15) // 16 * 16, (K + 31) // 32 * 32, (N + 15) // 16 * 16
        n3 = 16 * Kp32 * Np * 3
        out = torch.full((n3 + 8,), -1, device=DEV, dtype=torch.int16)          # 0xffff: a bf16 NaN
        _raw_pack(H, "tmg_conv_wino_pack3", wd, out, mode, nvalid)
        got = H.conv_wino_pack3(wd, mode, nvalid)
        assert got.numel() == n3 and torch.equal(got, out[:n3]) and bool((out[n3:] == -1).all()), (cout, cin, mode, nvalid)
        parts = WC.pack3_unpack(got.cpu(), K, N).double()                       # [3][16][Kp32 / 16][Np][16]
        U = H.conv_wino_pack(wd, mode, nvalid).cpu().double().reshape(16, Kp16 // 16, Np, 16)
        full = torch.zeros(16, Kp32 // 16, Np, 16, dtype=torch.float64)
        full[:, :Kp16 // 16] = U
        assert torch.equal(parts.sum(0), full), "the three bf16 parts must sum to the fp32 operand exactly"
        want = WC.split_bf16(full)
        assert all(torch.equal(parts[i], want[i]) for i in range(3)), "the parts are the successive truncations (tmg_split3)"
        assert bool((parts[1] != 0).any()) and bool((parts[2] != 0).any() or kind == "int")
        if kind == "int":
            ref = WC.pack_ref(w, mode, nvalid).reshape(16, Kp16 // 16, Np, 16)
            assert torch.equal(full[:, :Kp16 // 16], ref)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_declined_calls_write_nothing():
    """Every envelope condition of wino_fwd_setup and wino_wgrad_impl: the code of wino_cases.DECLINED_*, returned before any launch,
    and NaN-poisoned outputs untouched.  (The same codes without a device: test_wino_plans_cpu.test_declined_by_plan.)"""
    H = _H()
    shp = WC.DECL_SHAPE
    U = torch.zeros(1 << 20, device=DEV)
    every = []
    for name, entry, ins, outs, cin, cout, bias_mis, code in WC.DECLINED_FWD:
        ib = [Buf(shp, sp, torch.ones(shp + (sp[0],))) for sp in ins]
        ob = [Buf(shp, sp) for sp in outs]
        bias = torch.zeros(260, device=DEV)[bias_mis:] if bias_mis is not None else None
        rc, _ = WC.raw_fwd(H, entry, [(b.view.data_ptr(), b.view.stride(2), b.view.shape[3]) for b in ib],
                           [(b.view.data_ptr(), b.view.stride(2), b.view.shape[3]) for b in ob], U.data_ptr(),
                           bias.data_ptr() if bias is not None else 0, cin if cin is not None else sum(s[0] for s in ins),
                           cout if cout is not None else sum(s[0] for s in outs), stream=H._stream())
        assert rc == code, (name, rc, code)
        every += [b.flat for b in ob]
    B, Hh, Ww = shp
    ws_all = torch.full(((1 << 21) + 4,), NAN, device=DEV)
    gtab = torch.zeros(32, dtype=torch.int64, device=DEV)
    for name, ins, dys, cin, wsk, ng, code in WC.DECLINED_WG:
        ib = [Buf(shp, sp, torch.ones(shp + (sp[0],))) for sp in ins]
        dyb = Buf(shp, dys, torch.ones(shp + (dys[0],)))
        cin_ = cin if cin is not None else sum(s[0] for s in ins)
        cout = dys[0]
        dW = torch.full((cout, cin_, 9), NAN, device=DEV)
        db = torch.full((cout,), NAN, device=DEV)
        need = int(H.lib().tmg_conv_wino_wgrad_ws_floats(H._i64(B, Hh, Ww, cin_, cout, 0, 0, 0, 0, 0, 0, 0)))
        ws, wsn = {"ok": (ws_all.data_ptr(), 1 << 21), "null": (0, 1 << 21), "short": (ws_all.data_ptr(), max(need - 1, 0)),
                   "misaligned": (ws_all.data_ptr() + 4, 1 << 21)}[wsk]
        assert wsk != "short" or need > 1
        rc, _ = WC.raw_wg(H, [(b.view.data_ptr(), b.view.stride(2), b.view.shape[3]) for b in ib],
                          (dyb.view.data_ptr(), dyb.view.stride(2), cout), dW.data_ptr(), db.data_ptr(), ws, wsn, cin_, cout,
                          ngroups=2 if ng else 0, gtab=0 if ng == "nogtab" else gtab.data_ptr(), stream=H._stream())
        assert rc == code, (name, rc, code)
        every += [dW, db]
    # the launching wrappers report an envelope miss as False
    x, o = torch.randn(shp + (8,), device=DEV), torch.full(shp + (32,), NAN, device=DEV)
    assert H.conv_wino_fwd([x], U, 32, [o]) is False and H.conv_wino_fwd3([x], U.view(torch.int16), 32, [o]) is False
    assert H.conv_wino_narrow([x], U, 32, [o]) is False
    every.append(o)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in every), "a declined call wrote to an output"
    assert bool(torch.isnan(ws_all).all()), "a declined call wrote to the workspace"
