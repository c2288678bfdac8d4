"""The direct convolution kernels of tmg_conv.hip, each called through its tmg_hip wrapper and compared with a plain fp64 restatement
of the same operation (conv_cases.py), on every reachable kernel instance and at the edges of the launch plans.

Every case first asserts, through the library's own plan query on the very tensors it is about to pass, that it runs on the kernel
instance its name states (where that depends on the compute-unit count the batch is the smallest one the planner sends there).  Every
output buffer is NaN-prefilled (accumulating outputs: known values) inside a NaN parent, and the parent outside the view must stay NaN.

Two data modes (conv_cases.py derives both):
  int    small integers, sum |terms| < 2^24: the kernel must equal fp64 BIT FOR BIT whatever the summation order (carries the
         large-pixel plans and the atomics path);
  gauss  |a_i - ref_i| <= (K + 8) 2^-24 S_i elementwise, S_i the fp64 sum of the absolute values of element i's own terms,
         K = k^2 Cin forward, B Hout Wout for a weight gradient, k^2 Cdy for the adjoints; only where K <= 2048.

Case map (conv_cases.py):
  test_conv_fwd         FWD_CASES: lean_NxWMxWN_mtM / fb_NxWMxWN_mtM every reachable (kernel, MT, NTW, WM, WN); lean_chunks* channel
                        chunks 2 / 3 with a part-filled last one and by patch size; lean_k1*; lean_in3_slices; lean_out2 / out3;
                        lean_ovec0_* (Cout % 4, output slice at offset 2, misaligned add); lean_h1 / w1 / w33 / tiny_image;
                        lean_persistent (a block's tiles in two images); lean_all_switches, fb_stride2_odd (every operand switch);
                        fb_stride2_* / fb_in_off2 / fb_in_misaligned (causes of the fallback); fb_chunks_40k / 64k (KCH < Cin_pad).
  test_conv_wgrad       WG_CASES: wg_npN_ncoM every (NP, NCO) lean, *_nonlean the same through a dy slice at offset 2; *_atomics
                        (use_ws=False) per NP; non-lean through Cin % 4, Cout % 4, an input slice at offset 2; wg_ppg_rebalanced,
                        wg_gx_two_chunks, wg_gx1, wg_mpix128 / 256, stride 2, k = 1, three input segments, cin_dst / ci_split layouts.
  test_conv_rep_border  BD_CASES: NT = 1 .. 8, split K, H or W in {1, 2, 3}, the scalar kernel by misalignment / Cx > 128 / Cx % 4,
                        two and three output segments, kappa, a part-filled last 16-row tile.
  test_conv_dgrad_direct, test_pack*, test_declined_shapes_write_nothing.
Measured shares of the bounds: LAB_NOTES.md."""
import pytest
import torch

import common as C  # noqa: F401  (sets sys.path)
import conv_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _H():
    import tmg_hip as H
    return H


class Buf:
    """An NHWC tensor built from a segment spec (conv_cases.seg): the view the kernel gets, inside a NaN parent."""

    def __init__(self, shape3, spec, init=None):
        n, width, off, mis = spec
        B, Hh, Ww = shape3
        numel = B * Hh * Ww * width
        self.flat = torch.full((numel + 4,), NAN, device=DEV)
        self.view = self.flat[mis:mis + numel].view(B, Hh, Ww, width)[..., off:off + n]
        self.outside = self.flat.numel() - self.view.numel()
        if init is not None:
            self.view.copy_(init.to(DEV, torch.float32))

    def intact(self):
        """Everything outside the view is still NaN (and nothing inside is)."""
        return int(torch.isnan(self.flat).sum()) == self.outside


def _split(t, specs, shape3, fill=True):
    """One Buf per segment spec, holding consecutive channel ranges of t (None: NaN outputs)."""
    out, c0 = [], 0
    for sp in specs:
        out.append(Buf(shape3, sp, t[..., c0:c0 + sp[0]] if t is not None else None))
        c0 += sp[0]
    return out


def _dev(t):
    return t.to(DEV, torch.float32).contiguous() if t is not None else None


def _kappa(v):
    return torch.tensor([v], device=DEV, dtype=torch.float32) if v is not None else None


def _check(got, ref, S, K, mode, what):
    if mode == "int":
        assert CC.bit_equal(got, ref), "%s: integer mode is not bit-exact (max |diff| %g)" % (
            what, float((got.detach().cpu().double() - ref).abs().nan_to_num(float("inf")).max()))
        return
    share = CC.gauss_share(got, ref, S, K)
    print("SHARE %s %.4f" % (what, share))
    assert share <= 1.0, "%s: %.3f of the bound (K + 8) 2^-24 S, K = %d" % (what, share, K)


def _modes(cases):
    return [pytest.param(c, m, id="%s-%s" % (c["name"], m)) for c in cases for m in (("int", "gauss") if c["gauss"] else ("int",))]


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _modes(CC.FWD_CASES))
def test_conv_fwd(case, mode):
    H = _H()
    B, _ = CC.resolve_fwd(H, case)
    Hh, Ww = case["hw"]
    Ho, Wo = CC.out_hw(Hh, Ww, case["s"])
    sw, k, s = case["sw"], case["k"], case["s"]
    cout = sum(o[0] for o in case["outs"])
    d = CC.fwd_data(case, B, mode)
    ref, S = CC.fwd_ref(case, d)
    if mode == "int":
        assert CC.int_terms_ok(S, CC.gran_of(d))
    ins = _split(d["x"], case["ins"], (B, Hh, Ww))
    outs = _split(d["prev"], case["outs"], (B, Ho, Wo))
    add = Buf((B, Ho, Wo), case["add"], d["add"]) if case["add"] is not None else None
    kw = dict(bias=_dev(d["bias"]), kappa=_kappa(d["kappa"]), in_scale=_dev(d["scale"]), in_shift=_dev(d["shift"]),
              relu_in="relu_in" in sw, pad_rep="rep" in sw, relu_out="relu_out" in sw, accumulate="acc" in sw,
              add=add.view if add is not None else None)
    p = H.conv_fwd_plan([b.view for b in ins], cout, k, s, [b.view for b in outs], **kw)
    assert p["rc"] == 0 and CC.fwd_instance(p) == case["want"] and all(p[f] == v for f, v in case["plan"].items()), (case["name"], p)
    wpk = H.conv_pack(_dev(d["w"]), 0)
    H.conv_fwd([b.view for b in ins], wpk, cout, k, s, [b.view for b in outs], **kw)
    torch.cuda.synchronize()
    got = torch.cat([b.view for b in outs], 3)
    _check(got, ref, S, case["K"], mode, case["name"])
    assert all(b.intact() for b in outs), "written outside the output segments"
    assert all(b.intact() for b in ins) and (add is None or add.intact())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _modes(CC.WG_CASES))
def test_conv_wgrad(case, mode, monkeypatch):
    H = _H()

    def _no_winograd(*a, **k):
        raise AssertionError("%s was routed to the Winograd weight-gradient kernel" % case["name"])
    monkeypatch.setattr(H, "conv_wino_wgrad", _no_winograd)
    CC.wg_plan(H, case)
    B, Hh, Ww = case["shape"]
    Ho, Wo = CC.out_hw(Hh, Ww, case["s"])
    sw, k, s, cin, cout = case["sw"], case["k"], case["s"], case["cin"], case["cout"]
    cd, cv, cs, o0, o1 = case["layout"]
    d = CC.wg_data(case, mode)
    Wr, SW, br, Sb, touched = CC.wg_ref(case, d)
    if mode == "int":
        assert CC.int_terms_ok(SW, CC.gran_of(d)) and CC.int_terms_ok(Sb)
    ins = _split(d["x"], case["ins"], (B, Hh, Ww))
    dy = Buf((B, Ho, Wo), case["dy"], d["dy"])
    dW = _dev(d["prevW"]) if d["prevW"] is not None else torch.zeros(cout, cd or cin, k * k, device=DEV)
    dW0 = dW.clone()
    db = None
    if "dbias" in sw:
        db = _dev(d["prevb"]) if d["prevb"] is not None else torch.zeros(cout, device=DEV)
    kw = dict(kappa=_kappa(d["kappa"]), in_scale=_dev(d["scale"]), in_shift=_dev(d["shift"]), relu_in="relu_in" in sw,
              pad_rep="rep" in sw, use_ws=case["ws"], cin_dst=cd, cin_valid=cv, ci_split=cs, ci_off0=o0, ci_off1=o1)
    p = H.conv_wgrad_plan([b.view for b in ins], dy.view, k, s, dbias=db, **kw)
    assert p["rc"] == 0 and CC.wg_instance(p) == case["want"] and all(p[f] == v for f, v in case["plan"].items()), (case["name"], p)
    assert not CC.wino_routed(H, case, mode)
    H.conv_wgrad([b.view for b in ins], dy.view, dW, db, k, s, **kw)
    torch.cuda.synchronize()
    _check(dW, Wr, SW, case["K"], mode, case["name"] + " dW")
    assert torch.equal(dW[:, ~touched.to(DEV)], dW0[:, ~touched.to(DEV)]), "columns outside the destination changed"
    if db is not None:
        if d["prevb"] is None:
            br, Sb = br.expand(cout), Sb.expand(cout)
        _check(db, br.contiguous(), Sb.contiguous(), case["K"], mode, case["name"] + " dbias")
    assert dy.intact() and all(b.intact() for b in ins)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode", _modes(CC.BD_CASES))
def test_conv_rep_border(case, mode):
    H = _H()
    CC.bd_plan(H, case)
    B, Hh, Ww = case["shape"]
    d = CC.bd_data(case, mode)
    ref, S = CC.bd_ref(case, d)
    if mode == "int":
        assert CC.int_terms_ok(S)
    dy = Buf((B, Hh, Ww), case["dy"], d["dy"])
    outs = _split(d["prev"], case["outs"], (B, Hh, Ww))
    p = H.conv_rep_border_plan(dy.view, [b.view for b in outs])
    assert p["rc"] == 0 and (p["mfma"], p["NT"]) == case["want"] and all(p[f] == v for f, v in case["plan"].items()), (case["name"], p)
    wpk = H.conv_pack(_dev(d["w"]), 1)
    H.conv_rep_border_fix(dy.view, wpk, [b.view for b in outs], kappa=_kappa(d["kappa"]))
    torch.cuda.synchronize()
    _check(torch.cat([b.view for b in outs], 3), ref, S, case["K"], mode, case["name"])
    assert all(b.intact() for b in outs) and dy.intact()


# ---------------------------------------------------------------------------------------------------------------------------------
# (name, (B, Hin, Win), Cin, Cout, k, stride, accumulate, dy spec, dx spec); the last one: 2 162 688 elements > 8192 x 256
DG_CASES = [
    ("dg_s2_k3_odd", (2, 13, 9), 6, 10, 3, 2, False, None, None),
    ("dg_s2_k3_even_acc", (2, 16, 12), 8, 8, 3, 2, True, None, None),
    ("dg_s1_k3_slices", (2, 7, 11), 5, 7, 3, 1, False, (7, 12, 3, 0), (5, 9, 2, 0)),
    ("dg_s1_k1", (2, 7, 11), 8, 12, 1, 1, False, None, None),
    ("dg_s2_k1_acc_slices", (3, 9, 10), 4, 6, 1, 2, True, (6, 8, 1, 1), (4, 8, 4, 0)),
    ("dg_grid_stride", (2, 192, 176), 32, 4, 3, 2, False, None, None),
]


@pytest.mark.parametrize("mode", ["int", "gauss"])
@pytest.mark.parametrize("case", DG_CASES, ids=[c[0] for c in DG_CASES])
def test_conv_dgrad_direct(case, mode):
    H = _H()
    name, (B, Hin, Win), cin, cout, k, s, acc, dys, dxs = case
    Ho, Wo = CC.out_hw(Hin, Win, s)
    g = torch.Generator().manual_seed(4000)
    dyv, w, prev = CC.rnd(g, (B, Ho, Wo, cout), mode), CC.rnd(g, (cout, cin, k, k), mode, 2), CC.rnd(g, (B, Hin, Win, cin), mode, 8)
    ref, S = CC.dgrad_ref(dyv, w, (B, Hin, Win, cin), k, s)
    if acc:
        ref, S = ref + prev, S + prev.abs()
    assert B * Hin * Win * cin > 8192 * 256 or name != "dg_grid_stride"
    dy = Buf((B, Ho, Wo), dys or CC.seg(cout), dyv)
    dx = Buf((B, Hin, Win), dxs or CC.seg(cin), prev if acc else None)
    H.conv_dgrad_direct(dy.view, _dev(w), dx.view, k, s, accumulate=acc)
    torch.cuda.synchronize()
    if mode == "int":
        assert CC.int_terms_ok(S)
    _check(dx.view, ref, S, k * k * cout, mode, name)
    assert dx.intact() and dy.intact()


# ---------------------------------------------------------------------------------------------------------------------------------
def _raw_pack(H, kind, w, mode, ce, cmap, out):
    """The library entry behind conv_pack / conv_pack_map / conv_pack_batched / conv_pack_many on a destination the TEST owns (the
    wrappers allocate theirs with torch.empty, whose contents nobody controls): every float of `out` starts as NaN, so padding the
    packer does not write stays NaN."""
    import ctypes
    c_i64, L = ctypes.c_int64, H.lib()
    batched = w.dim() == 5
    cout, cin, k = w.shape[-4], w.shape[-3], w.shape[-1]
    m = cmap if cmap is not None else (cin, 0x7fffffff, 0)
    e = int(ce) if cmap is not None else max(int(ce), cin)
    if kind == "pack":
        rc = L.tmg_conv_pack(H._ptr(w), H._ptr(out), c_i64(cout), c_i64(cin), c_i64(e), c_i64(k), c_i64(mode), H._stream())
    elif kind == "map":
        rc = L.tmg_conv_pack_map(H._ptr(w), H._ptr(out), c_i64(cout), c_i64(cin), c_i64(e), c_i64(k), c_i64(mode), H._i64(*m), H._stream())
    elif kind == "batched":
        assert batched
        rc = L.tmg_conv_pack_batched(H._ptr(w), H._ptr(out), c_i64(w.shape[0]), c_i64(cout), c_i64(cin), c_i64(e), c_i64(k), c_i64(mode),
                                     H._i64(*m), H._stream())
    else:
        wp, op = (ctypes.c_void_p * 1)(w.data_ptr()), (ctypes.c_void_p * 1)(out.data_ptr())
        rc = L.tmg_conv_pack_many(wp, op, H._i64(cout, cin, e, k, mode, m[0], m[1], m[2]), c_i64(1), H._stream())
    assert rc == 0, (kind, rc)


PACK_CASES = [(20, 24, 3, 0, None), (36, 20, 1, 0, None), (6, 40, 1, 0, None), (16, 16, 3, 0, None), (20, 8, 3, 24, None),
              (12, 30, 3, 16, (10, 4, 6)), (33, 18, 1, 32, (14, 6, 3))]


@pytest.mark.parametrize("mode", [0, 1])
def test_pack_and_pack_map_equal_the_documented_layout(mode):
    H = _H()
    g = torch.Generator().manual_seed(5000 + mode)
    for cout, cin, k, ce, cmap in PACK_CASES:
        w = torch.randn(cout, cin, k, k, generator=g)
        ref = CC.pack_ref(w, mode, ce, cmap)
        wd = w.to(DEV)
        got = H.conv_pack(wd, mode, ce, cmap)
        assert got.numel() == ref.numel() and torch.equal(got.cpu(), ref), (cout, cin, k, ce, cmap)
        # the same entries on NaN-prefilled destinations (4 floats of slack behind, which must stay NaN): padding is written as zeros
        for kind in (("pack",) if cmap is None else ()) + ("map", "many"):
            out = torch.full((ref.numel() + 4,), NAN, device=DEV)
            _raw_pack(H, kind, wd, mode, ce, cmap, out)
            assert torch.equal(out[:-4].cpu(), ref) and bool(torch.isnan(out[-4:]).all()), (kind, cout, cin, k, ce, cmap)


@pytest.mark.parametrize("mode", [0, 1])
def test_pack_batched_equals_the_documented_layout(mode):
    H = _H()
    g = torch.Generator().manual_seed(5100 + mode)
    for n, cout, cin, k, ce, cmap in [(5, 20, 24, 3, 0, None), (3, 12, 30, 3, 16, (10, 4, 6)), (4, 6, 40, 1, 48, None)]:
        w = torch.randn(n, cout, cin, k, k, generator=g)
        ref = torch.stack([CC.pack_ref(w[i], mode, ce, cmap) for i in range(n)])
        wd = w.to(DEV)
        got = H.conv_pack_batched(wd, mode, ce, cmap)
        assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (n, cout, cin, k, ce, cmap)
        out = torch.full((ref.numel() + 4,), NAN, device=DEV)
        _raw_pack(H, "batched", wd, mode, ce, cmap, out)
        assert torch.equal(out[:-4].cpu(), ref.reshape(-1)) and bool(torch.isnan(out[-4:]).all()), (n, cout, cin, k, ce, cmap)


def test_pack_many_49_jobs_equal_the_single_packs():
    H = _H()
    g = torch.Generator().manual_seed(5200)
    jobs = []
    for i in range(49):
        cout, cin, k, ce, cmap = PACK_CASES[i % len(PACK_CASES)]
        jobs.append((torch.randn(cout + i % 3, cin, k, k, generator=g).to(DEV), i % 2, ce, cmap))
    outs = H.conv_pack_many(jobs)
    assert len(outs) == 49
    for (w, m, ce, cm), o in zip(jobs, outs):
        assert torch.equal(o.cpu(), CC.pack_ref(w.cpu(), m, ce, cm)) and torch.equal(o, H.conv_pack(w, m, ce, cm))
    short = H.conv_pack_many([(jobs[0][0], 0), (jobs[1][0], 1)])      # the (w, mode) job form
    assert torch.equal(short[0].cpu(), CC.pack_ref(jobs[0][0].cpu(), 0)) and torch.equal(short[1].cpu(), CC.pack_ref(jobs[1][0].cpu(), 1))


# ---------------------------------------------------------------------------------------------------------------------------------
def test_declined_shapes_write_nothing():
    H = _H()
    x = torch.randn(2, 8, 8, 8, device=DEV)
    out = torch.full((2, 8, 8, 16), NAN, device=DEV)
    wpk = torch.zeros(25 * 16 * 16, device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        H.conv_fwd([x], wpk, 16, 5, 1, [out])
    q = [x[..., 0:2], x[..., 2:4], x[..., 4:6], x[..., 6:8]]
    with pytest.raises(RuntimeError, match="code -3"):
        H.conv_fwd(q, wpk, 16, 3, 1, [out])
    with pytest.raises(RuntimeError, match="code -3"):
        H.conv_fwd([x], wpk, 16, 3, 1, [out[..., 0:4], out[..., 4:8], out[..., 8:12], out[..., 12:16]])
    dW = torch.full((16, 8, 25), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        H.conv_wgrad([x], torch.randn(2, 8, 8, 16, device=DEV), dW, None, 5, 1)
    # Two codes no launching wrapper can produce - conv_wgrad_grouped always passes a workspace, conv_fwd asserts the output channel
    # sum - are read from the plan queries only.  A query and its launch are one function body, which returns these codes before the
    # point where a launch would happen; "writes nothing" is observed by a launch only for the codes above.
    assert H.conv_wgrad_plan([x], out, 3, 1, use_ws=False, ngroups=2)["rc"] == -100
    assert H.conv_fwd_plan([x], 20, 3, 1, [out])["rc"] == -4
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dW).all())
