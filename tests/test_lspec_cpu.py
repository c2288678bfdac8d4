"""CPU-side checks of the line spectra: the kernel entries are declared in their own header, listed apart and exported; the plan
query's values and the codes the entries return before any launch; every argument error in its documented order, without a GPU; the
operand against its fp64 statement; the reference of tests/lspec_cases.py against its second statement and the Parseval identity;
tmg_ops.lspec_outputs against fp64 formulas written in lspec_cases; the float32 Welford mirror against the two-pass reference; and
the sensitivity of the comparison the GPU test uses: every named mutation of the reference is caught."""
import ctypes
import inspect
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import common as C
import lspec_cases as K

NAMES = ["tmg_ens_lspec_plan", "tmg_ens_lspec_chunk", "tmg_ens_lspec_step", "tmg_ens_lspec_finalize"]
c_i64 = ctypes.c_int64
P64 = ctypes.POINTER(c_i64)
vp = ctypes.c_void_p
PKG = os.path.join(C.ROOT, "deep-turbulence_amd")


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    hdr = open(os.path.join(inc, "tmglow_hip_lspec.h")).read()
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", hdr)
    assert decl == [("int", n) for n in NAMES] and tmg_hip.LSPEC_EXPORTS == NAMES
    assert "lspec" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    want = {"tmg_ens_lspec_plan": [P64, P64], "tmg_ens_lspec_chunk": [vp, P64] + [vp] * 7 + [P64, vp],
            "tmg_ens_lspec_step": [vp] * 4 + [P64, vp], "tmg_ens_lspec_finalize": [vp] * 7 + [P64, vp]}
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.LSPEC_ARGTYPES[name] == want[name]
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        kinds = [P64 if "int64_t*" in q.replace(" *", "*") else c_i64 if "int64_t" in q else vp for q in params]
        assert kinds == want[name], name
    assert "tmg_lspec.hip" in tmg_hip.SOURCES and "tmg_lspec.hip" in tmg_hip.NO_PACKED_F32
    assert "tmglow_hip_lspec.h" in inspect.getsource(tmg_hip.build)
    import __graft_entry__ as G
    assert "LSPEC_EXPORTS" in inspect.getsource(G.build)
    code = re.sub(r"//[^\n]*", "", open(os.path.join(tmg_hip.CSRC, "tmg_lspec.hip")).read())
    # no atomics, no inline assembly, nothing printed or asserted in a kernel, no memset; the matrix pipe's fp32 form is used
    assert not re.search(r"\basm\b|printf|assert\s*\(|atomic|hipMemset", code)
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in code


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredLineSpectra).parameters
    assert list(sig) == old + ["axis", "window", "per_member"]
    assert (sig["axis"].default, sig["window"].default, sig["per_member"].default) == ("x", "hann", False)
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleLineSpectra.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "grid", "axis", "window",
                          "per_member"]
    assert (init["u"].default, init["grid"].default, init["axis"].default, init["window"].default, init["per_member"].default) == \
        (None, (1.0, 1.0), "x", "hann", False)
    assert list(inspect.signature(tmg_ops.EnsembleLineSpectra.add).parameters) == ["self", "y", "m0", "time"]
    assert issubclass(tmg_ops.EnsembleLineSpectra, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.lspec_args).parameters) == ["C", "Hh", "Ww", "grid", "axis", "window", "members"]
    assert "channels, N, L, grid, axis, window, members" in tmg_ops.lspec_args.__doc__
    assert "44 S B L NQ" in tmg_ops.EnsembleLineSpectra.__doc__                  # the device memory is stated
    assert inspect.signature(tmg_hip.ens_lspec_plan).parameters["code"].default is False
    for c in (2, 3, 4):
        assert tmg_ops.lspec_fields(c) == K.fields(c) and len(K.fields(c)) == c + 2
    assert K.fields(3) == ("uu", "vv", "pp", "uv_co", "uv_quad")


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,S,B,Cc,L,N", [(1, 1, 1, 2, 1, 16), (2, 5, 2, 3, 17, 48), (1, 2, 1, 4, 33, 272), (8, 32, 8, 3, 256, 256),
                                          (1, 1024, 1, 2, 1, 512)])
def test_plan_values(k, S, B, Cc, L, N):
    import tmg_hip
    p = tmg_hip.ens_lspec_plan(k, S, B, Cc, L, N)
    nq = N // 2 + 1
    nqp = -(-nq // 16) * 16
    lt = -(-L // 16)
    assert (p["tiles"], p["mode_tiles"], p["nq"], p["nqp"]) == (lt, nqp // 16, nq, nqp)
    assert (p["grid_x"], p["grid_y"], p["threads"]) == (lt, k * B, 256)
    assert p["lds_bytes"] == 4 * Cc * 16 * (N + 4) <= 160 * 1024
    assert p["part_floats"] == k * B * lt * (Cc + 2) * nq
    assert p["mean_floats"] == 2 * S * B * Cc * L * nq and p["comom_floats"] == S * B * (Cc + 2) * L * nq
    assert 4 * (p["mean_floats"] + p["comom_floats"]) == 4 * (3 * Cc + 2) * S * B * L * nq      # 44 S B L NQ bytes at C = 3
    assert p["operand_floats"] == 2 * N * nqp
    assert {16: 1, 48: 2, 80: 3, 272: 9}.get(N, p["mode_tiles"]) == p["mode_tiles"]


def test_codes_come_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    code = lambda *a: tmg_hip.ens_lspec_plan(*a, code=True)[1]                  # noqa: E731
    assert code(1, 1, 1, 2, 1, 16) == 0
    for bad in ((0, 1, 1, 2, 1, 16), (1, 0, 1, 2, 1, 16), (1, 1, 0, 2, 1, 16), (1, 1, 1, 1, 1, 16), (1, 1, 1, 5, 1, 16), (1, 1, 1, 2, 0, 16),
                (1, 1, 1, 2, 1, 8), (1, 1, 1, 2, 1, 24), (1, 1, 1, 2, 1, 528), (2, 1, 1, 2, 1, 16)):
        assert code(*bad) == -1, bad
    for big in ((1, 1025, 1, 2, 1, 16), (1, 1, 65536, 2, 1, 16), (1, 1, 1, 2, 16 * 65536, 16), (1, 1024, 64, 3, 512, 512)):
        assert code(*big) == -2, big
    assert lib.tmg_ens_lspec_plan(None, _i64(*[0] * 12)) == -3 and lib.tmg_ens_lspec_plan(_i64(1, 1, 1, 2, 1, 16), None) == -3
    with pytest.raises(RuntimeError, match="tmg_ens_lspec_plan failed with code -1"):
        tmg_hip.ens_lspec_plan(1, 1, 1, 2, 1, 24)
    # the chunk: host pointers stand in for device ones; every code below is returned before the launch
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    k, S, B, Cc, L, N = 1, 2, 1, 3, 5, 16
    p = tmg_hip.ens_lspec_plan(k, S, B, Cc, L, N)
    sizes = (p["part_floats"], p["mean_floats"], p["comom_floats"], p["operand_floats"])

    def chunk(dims, y=a, yd=(3, 0), mu=a, sd=a, op=a, mean=a, comom=a, part=a):
        return lib.tmg_ens_lspec_chunk(y, _i64(*yd), None, mu, sd, op, mean, comom, part, _i64(*dims), None)

    good = (k, S, B, Cc, L, N, N, 1, 0, 0, 1) + sizes
    cols = (k, S, B, Cc, L, N, 1, L, 0, 0, 1) + sizes
    edit = lambda i, v, base=good: base[:i] + (v,) + base[i + 1:]               # noqa: E731
    for dims in (edit(6, N + 1), edit(7, 2), (k, S, B, Cc, L, N, 1, N, 0, 0, 1) + sizes, edit(8, -1), edit(8, 2), edit(9, -1), edit(10, 2),
                 edit(5, 24), edit(3, 5)):
        assert chunk(dims) == -1, dims
    assert chunk(good, yd=(2, 0)) == -1 and chunk(good, yd=(3, 1)) == -1 and chunk(cols, yd=(4, 2)) == -1
    assert chunk(good, yd=(2 ** 34, 0)) == -2
    assert chunk(good, y=None) == -3 and chunk(good, op=None) == -3 and chunk(good, part=None) == -3 and chunk(good, mean=None) == -3
    assert chunk(edit(10, 0), mean=None, comom=None, part=None) == -3           # an untimed chunk needs no state, but its partials
    for i in (11, 12, 13, 14):
        assert chunk(edit(i, good[i] - 1)) == -4, i
    step = lambda dims, part=a, state=a, mo=a, so=a: lib.tmg_ens_lspec_step(part, state, mo, so, _i64(*dims), None)     # noqa: E731
    sgood = (1, B, Cc + 2, L, N, 0, S, 3, 0, 0)
    for i, v in ((0, 0), (1, 0), (2, 3), (2, 7), (3, 0), (4, 24), (5, -1), (6, 0), (7, 0), (8, 3), (8, -1), (9, 2), (9, 1), (5, 2)):
        assert step(sgood[:i] + (v,) + sgood[i + 1:]) == -1, (i, v)
    assert step((1, B, Cc + 2, L, N, 1, S, 3, 0, 0)) == -1                       # the step's last chunk must say so
    assert step(sgood, part=None) == -3 and step(sgood, state=None) == -3
    assert step((1, B, Cc + 2, L, N, 1, S, 3, 0, 1), mo=None) == -3
    fin = lambda dims, **kw: lib.tmg_ens_lspec_finalize(kw.get("mean", a), a, a, a, a, kw.get("fs", a), None, _i64(*dims), None)  # noqa: E731
    for dims in ((0, B, Cc, L, N, 2), (S, B, 1, L, N, 2), (S, B, Cc, 0, N, 2), (S, B, Cc, L, 24, 2), (S, B, Cc, L, N, 0)):
        assert fin(dims) == -1, dims
    assert fin((1025, B, Cc, L, N, 2)) == -2
    assert fin((S, B, Cc, L, N, 2), mean=None) == -3 and fin((S, B, Cc, L, N, 2), fs=None) == -3


# ---- the argument checks ---------------------------------------------------------------------------------------------------------------
def test_every_argument_check_fires_in_its_documented_order():
    import tmg_ops as ops
    good = dict(C=3, Hh=16, Ww=32, grid=(0.1, 0.2), axis="x", window="hann", members=4)
    assert ops.lspec_args(**good) == ((0.1, 0.2), 32, 16, 0.1)
    assert ops.lspec_args(**dict(good, axis="y")) == ((0.1, 0.2), 16, 32, 0.2)
    assert ops.lspec_args(**dict(good, Hh=1, window=None))[1:3] == (32, 1)
    # one bad value per argument, in the documented order; each later one is also bad in every call, so the FIRST must win
    bad = [("C", 5, "2 <= C <= 4"), ("Ww", 24, "N a multiple of 16"), ("Hh", 0, "L >= 1 lines"), ("grid", (0.1, -1.0), "two positive finite"),
           ("axis", "z", "axis must be"), ("window", "hamming", "window must be"), ("members", 0, "1 <= members <= 1024")]
    for i, (name, value, msg) in enumerate(bad):
        kw = dict(good)
        for n, v, _ in bad[i:]:
            kw[n] = v
        with pytest.raises(ValueError, match=msg):
            ops.lspec_args(**kw)
    for kw, msg in ((dict(C=True), "integer number of channels"), (dict(C=1), "2 <= C <= 4"), (dict(Ww=528), "N a multiple of 16"),
                    (dict(Ww=16.0), "N a multiple of 16"), (dict(axis="y", Hh=24), "N a multiple of 16"), (dict(axis="y", Ww=0), "L >= 1"),
                    (dict(grid=(1.0,)), "two positive"), (dict(grid=None), "two positive"), (dict(grid=(float("inf"), 1.0)), "two positive"),
                    (dict(axis=0), "axis must be"), (dict(axis=None), "axis must be"), (dict(window="none"), "window must be"),
                    (dict(members=1025), "1 <= members"), (dict(members=2.0), "integer number of members")):
        with pytest.raises(ValueError, match=msg):
            ops.lspec_args(**dict(good, **kw))


def test_constructor_checks_come_before_the_device_and_a_cpu_device_raises_last():
    import tmg_ops as ops
    mk = lambda S=2, B=2, Cc=3, Hh=16, Ww=16, T=2, **kw: ops.EnsembleLineSpectra(S, B, Cc, Hh, Ww, T, kw.pop("device", "cpu"),   # noqa: E731
                                                                                 torch.zeros(Cc), kw.pop("sd", torch.ones(Cc)), **kw)
    for kw, msg in ((dict(Cc=5), "2 <= C <= 4"), (dict(Ww=24), "multiple of 16"), (dict(axis="y", Hh=8), "multiple of 16"),
                    (dict(grid=(0.0, 1.0)), "two positive"), (dict(axis="t"), "axis must be"), (dict(window="welch"), "window must be"),
                    (dict(S=0), "1 <= members"), (dict(T=0), "steps >= 1"), (dict(B=0), "B >= 1"), (dict(sd=torch.zeros(3)), "strictly positive"),
                    (dict(u=torch.zeros(2, 3)), "u must be finite")):
        with pytest.raises(ValueError, match=msg):
            mk(**kw)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        mk()
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        mk(Hh=5, axis="x", window=None, per_member=True)


def test_model_pred_line_spectra_on_a_cpu_model_raises():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from utils import utils
    log = SimpleNamespace(log=lambda *a, **k: None)
    args = SimpleNamespace(device=None, dx=0.1, dy=0.1)
    for kw, msg in ((dict(axis="z"), "axis must be"), (dict(window="boxcar"), "window must be"), (dict(samples=2000), "1 <= members")):
        with pytest.raises(ValueError, match=msg):
            utils.modelPredLineSpectra(args, torch.nn.Linear(1, 1), [], log, tmax=2, **kw)
    with pytest.raises(RuntimeError, match="modelPredLineSpectra runs on the HIP path"):
        utils.modelPredLineSpectra(args, torch.nn.Linear(1, 1), [], log, samples=2, tmax=2)


# ---- the operand -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 48, 80, 272, 512])
@pytest.mark.parametrize("win", ["hann", None])
def test_operand_is_the_fp64_statement_rounded_once(N, win):
    import tmg_ops as ops
    op = ops._lspec_operand(N, win)
    nq = N // 2 + 1
    nqp = -(-nq // 16) * 16
    assert op.dtype == torch.float32 and tuple(op.shape) == (2, N, nqp) and op.is_contiguous()
    cr, ci = K.operand64(N, win)
    assert np.array_equal(op[0, :, :nq].numpy(), cr.astype(np.float32)) and np.array_equal(op[1, :, :nq].numpy(), ci.astype(np.float32))
    assert nqp == nq or bool((op[:, :, nq:] == 0).all())                         # the padded columns are exactly zero
    assert nqp - nq == {16: 7, 48: 7, 80: 7, 272: 7, 512: 15}[N]
    # the statement itself: the plain complex exponential of the unreduced argument, in fp64
    n, q = np.arange(N)[:, None], np.arange(nq)[None, :]
    z = K.window(N, win)[:, None] * np.exp(-2j * math.pi * q * n / N) / N
    # (the unreduced argument q n 2 pi / N carries a rounding error of up to 2^-53 q n 2 pi / N radians: 1e-10 covers N = 512)
    assert float(np.abs(cr + 1j * ci - z).max()) < 1e-10 * float(K.window(N, win).max()) / N
    if win == "hann":
        w = K.window(N, win)
        assert abs(float(np.mean(w * w)) - 1.0) < 1e-14 and w[0] == 0.0


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 2, 1, 3, 3, 16), (4, 3, 2, 2, 5, 48), (6, 2, 1, 4, 17, 32), (40, 1, 1, 3, 4, 256)]     # (T, S, B, C, L, N)


def _field(shape, axis, seed, **kw):
    T, S, B, Cc, L, N = shape
    Hh, Ww = (L, N) if axis == "x" else (N, L)
    return K.synthetic(T, S, B, Cc, Hh, Ww, seed, **kw)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("axis,win,t_start", [("x", "hann", 0), ("y", None, 1)])
def test_the_reference_agrees_with_its_second_statement_and_with_parseval(shape, axis, win, t_start):
    f = _field(shape, axis, 11)
    ref = K.reference(f, axis, win, t_start)
    two = K.reference_direct(f, axis, win, t_start)
    T, S, B, Cc, L, N = shape
    nq = N // 2 + 1
    assert ref["lspec_mean"].shape == (B, T, Cc + 2, nq) and ref["time_lspec_fluct_mean"].shape == (B, Cc + 2, L, nq)
    assert ref["time_lspec_fluct_member"].shape == (B, S, Cc + 2, L, nq)
    for name in K.KEYS:
        scale = ref["_P"][name]
        assert ref[name].shape == two[name].shape, name
        assert float(np.abs(ref[name] - two[name]).max()) <= 1e-12 * scale, name
    tot = ref["time_lspec_fluct_member"][:, :, :Cc].sum(-1).transpose(1, 0, 2, 3)      # [S, B, C, L]
    var = K.parseval(f, axis, win, t_start)
    assert float(np.abs(tot - var).max()) <= 1e-12 * float(var.max())
    # the mean flow carries several times the power of the fluctuations: the case the one-pass form has to survive
    flow = ref["time_lspec_flow_mean"][:, :Cc].sum(-1).max()
    assert flow > 4 * ref["time_lspec_fluct_mean"][:, :Cc].sum(-1).max()
    assert float(np.abs(ref["time_lspec_fluct_mean"][:, Cc:]).max()) > 0.02 * scale_of(ref, Cc)


def scale_of(ref, Cc):
    return float(ref["time_lspec_fluct_mean"][:, :Cc].max())


def test_hand_case_one_cosine():
    """u = 3 + 2 cos(2 pi 3 n / N) cos(w t), v = sin(2 pi 3 n / N) cos(w t) over a full period of t: every number by hand."""
    N, T = 16, 8
    n = np.arange(N)
    ct = np.cos(2 * math.pi * np.arange(T) / T)
    f = np.zeros((T, 1, 1, 2, 1, N))
    f[:, 0, 0, 0, 0] = 3 + 2 * np.cos(2 * math.pi * 3 * n / N)[None, :] * ct[:, None]
    f[:, 0, 0, 1, 0] = np.sin(2 * math.pi * 3 * n / N)[None, :] * ct[:, None]
    ref = K.reference(f, "x", None, 0)
    want = np.zeros((4, N // 2 + 1))
    want[0, 3], want[1, 3] = 2 * 1.0 * 0.5, 2 * 0.25 * 0.5                       # a_q |X|^2 mean(cos^2): X_u = 1, X_v = -i / 2
    want[3, 3] = 2 * 0.5 * 0.5                                                   # Im(X_u conj X_v) = Im(1 * (i / 2)) = 1 / 2
    np.testing.assert_allclose(ref["time_lspec_fluct_mean"][0, :, 0], want, atol=1e-15)
    flow = np.zeros((4, N // 2 + 1))
    flow[0, 0] = 9.0
    np.testing.assert_allclose(ref["time_lspec_flow_mean"][0, :, 0], flow, atol=1e-14)
    assert float(np.abs(ref["time_lspec_fluct_std"]).max()) == 0.0


# ---- the host-formed outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_lspec_outputs_match_the_fp64_formulas(shape):
    import tmg_ops as ops
    T, S, B, Cc, L, N = shape
    ref = K.reference(_field(shape, "x", 12), "x", "hann", 0)
    fl = ref["time_lspec_fluct_mean"].astype(np.float32)                         # what the device hands over
    k = K.wavenumbers(N, 0.05)
    got = ops.lspec_outputs(torch.from_numpy(fl), torch.from_numpy(k), Cc)
    want = K.derived(fl.astype(np.float64), k, Cc)
    assert set(got) == set(K.DERIVED)
    for name in K.DERIVED:
        g = got[name]
        assert g.dtype == torch.float64 and g.device.type == "cpu" and tuple(g.shape) == want[name].shape, name
        err = np.abs(g.numpy() - want[name])
        assert bool((err <= 2.0 ** -24 * np.abs(want[name]) + 2.0 ** -40).all()), (name, float(err.max()))
    assert tuple(got["time_lspec_energy"].shape) == (B, Cc + 2, L) and tuple(got["time_lspec_centroid"].shape) == (B, Cc, L)
    assert tuple(got["time_lspec_coherence"].shape) == (B, L, N // 2 + 1)
    coh = got["time_lspec_coherence"].numpy()
    assert float(coh[np.isfinite(coh)].max()) <= 1.0 + 1e-6                      # Cauchy-Schwarz on the ensemble-mean planes


def test_lspec_outputs_conventions():
    import tmg_ops as ops
    k = K.wavenumbers(16, 1.0)
    P = torch.zeros(1, 4, 2, 9)
    P[0, 0, 0, 2], P[0, 1, 0, 2], P[0, 2, 0, 2] = 4.0, 1.0, 2.0
    o = ops.lspec_outputs(P, k, 2)
    assert o["time_lspec_centroid"][0, 0, 0] == k[2] and math.isnan(float(o["time_lspec_centroid"][0, 0, 1]))       # 0 / 0
    assert float(o["time_lspec_coherence"][0, 0, 2]) == 1.0 and math.isnan(float(o["time_lspec_coherence"][0, 0, 3]))
    assert float(o["time_lspec_energy"][0, 0, 0]) == 4.0
    with pytest.raises(ValueError, match="fluct is"):
        ops.lspec_outputs(P, k, 3)
    d = K.log_distance(np.ones((1, 4, 2, 9)) * 10.0, np.ones((1, 4, 2, 9)), 2)
    assert np.allclose(d, 10.0) and d.shape == (1, 2, 2)
    from utils import utils
    e, t = torch.ones(1, 4, 2, 9) * 10.0, torch.ones(1, 4, 2, 9)
    t[0, 1, 1, 4] = 0.0
    got = utils._lspec_log_distance(e, t, 2)
    assert got.dtype == torch.float64 and float(got[0, 0, 0]) == 10.0 and math.isnan(float(got[0, 1, 1]))
    e[0, 0, 0, 0] = -1.0                                                         # q = 0 is not part of the distance
    assert float(utils._lspec_log_distance(e, t, 2)[0, 0, 0]) == 10.0


# ---- the float32 mirror and the sensitivity of the comparison --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("axis,win,t_start", [("x", "hann", 1), ("y", None, 0)])
def test_the_float32_welford_mirror_stays_inside_the_bound(shape, axis, win, t_start):
    f32 = torch.from_numpy(_field(shape, axis, 13)).float()
    ref = K.reference(f32.double().numpy(), axis, win, t_start)
    y32 = K.mirror32(f32, axis, win, t_start)
    bad = K.compare(y32, ref, None, "mirror %s" % (shape,))                      # the bound without its e32 arm
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_the_comparison_catches_every_named_mutation(mutation):
    shape = (5, 2, 1, 3, 3, 16)
    f32 = torch.from_numpy(_field(shape, "x", 14)).float()
    f = f32.double().numpy()
    ref = K.reference(f, "x", "hann", 1)
    y32 = K.mirror32(f32, "x", "hann", 1)
    assert not K.compare(ref, ref, y32, "self", report=lambda s: None)
    bad = K.compare(K.reference(f, "x", "hann", 1, mutation=mutation), ref, y32, mutation, report=lambda s: None)
    assert bad, mutation
    hit = {b.split()[1].rstrip(":") for b in bad}
    expect = {"nyquist2": "lspec_mean", "no_1_over_N": "lspec_mean", "window_rms": "lspec_mean", "ddof1": "time_lspec_fluct_mean",
              "quad_conj": "time_lspec_fluct_mean", "line_mean": "time_lspec_fluct_mean", "swap": "lspec_mean"}[mutation]
    assert expect in hit, (mutation, hit)
    if mutation == "ddof1":                                                      # it touches the fluctuation alone
        assert not {"lspec_mean", "lspec_std", "time_lspec_flow_mean", "time_lspec_flow_std"} & hit
