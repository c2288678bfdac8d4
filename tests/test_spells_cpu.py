"""CPU-side checks of the ensemble event durations: the kernel entries are declared in their own header, listed apart and exported;
the signatures of the three Python layers; the plan query's values and the codes the entries return before any launch; every
argument error without a GPU; the reference of tests/spell_cases.py against its second statement (runs as regular-expression
matches) and against directly counted transitions; the four identities of the tables on every case; tmg_ops.spell_outputs against
independently written fp64 formulas; and the sensitivity of the comparison the GPU test uses: every named mutation is caught."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import common as C
import spell_cases as K

NAMES = ["tmg_ens_spell_plan", "tmg_ens_spell_step", "tmg_ens_spell_finalize"]
c_i64 = ctypes.c_int64


def _i64(*v):
    return (c_i64 * len(v))(*v)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_in_their_own_header_listed_apart_and_exported():
    import tmg_hip
    inc = os.path.join(C.ROOT, "include")
    decl = re.findall(r"\b(int|int64_t)\s+(tmg_\w+)\s*\(", open(os.path.join(inc, "tmglow_hip_spell.h")).read())
    assert decl == [("int", n) for n in NAMES] and tmg_hip.SPELL_EXPORTS == NAMES
    assert "spell" not in open(os.path.join(inc, "tmglow_hip.h")).read()
    lib = ctypes.CDLL(tmg_hip.build())
    P64 = ctypes.POINTER(c_i64)
    vp = ctypes.c_void_p
    want = {"tmg_ens_spell_plan": [P64, P64], "tmg_ens_spell_step": [vp, P64, vp, P64, vp, vp, vp, P64, vp],
            "tmg_ens_spell_finalize": [vp, vp, vp, P64, vp]}
    for name in NAMES:
        assert name not in tmg_hip.EXPORTS and name not in tmg_hip.PLAN_EXPORTS and name not in tmg_hip.RET_I64
        assert hasattr(lib, name)
        fn = getattr(tmg_hip.lib(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[name] and tmg_hip.SPELL_ARGTYPES[name] == want[name]
    assert "tmg_spell.hip" in tmg_hip.SOURCES and "tmg_spell.hip" not in tmg_hip.NO_PACKED_F32
    assert tmg_hip.SOURCES.index("tmg_spell.hip") < tmg_hip.SOURCES.index("tmg_lagr.hip")
    assert "tmglow_hip_spell.h" in inspect.getsource(tmg_hip.build)
    assert re.search(r"\btmg_spell\b", open(os.path.join(C.ROOT, "tools", "spill_report.sh")).read())
    src = open(os.path.join(tmg_hip.CSRC, "tmg_spell.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    # integer arithmetic only: no float atomics, no inline assembly, nothing printed or asserted in a kernel, no unbounded loop
    assert not re.search(r"\basm\b|printf|assert\s*\(|while\s*\(|atomicAdd\s*\(\s*\(float|double", code)
    # no lane leaves before the barriers: the kernels have no return statement
    for name, end in (("ens_spell_step_kernel", "ens_spell_final_kernel"), ("ens_spell_final_kernel", "static int spell_args")):
        body = code[code.index("void " + name):code.index(end, code.index("void " + name) + 10)]
        assert "__syncthreads" in body and not re.search(r"\breturn\b", body), name


def test_signatures():
    from utils import utils
    import tmg_hip
    import tmg_ops
    old = ["args", "model", "testing_loader", "log", "samples", "stride", "tmax", "t_start", "max_rows"]
    sig = inspect.signature(utils.modelPredSpells).parameters
    assert list(sig) == old + ["events", "max_len"] and sig["events"].default == ((0, 0.0, "<"),) and sig["max_len"].default == 32
    assert [sig[n].default for n in old[4:]] == [1, 1, 1, 0, 64]
    init = inspect.signature(tmg_ops.EnsembleSpells.__init__).parameters
    assert list(init) == ["self", "members", "B", "C", "Hh", "Ww", "steps", "device", "out_mu", "out_std", "u", "events", "max_len",
                          "max_state_bytes"]
    assert init["max_len"].default == 32 and init["max_state_bytes"].default == 2 ** 31
    assert list(inspect.signature(tmg_ops.EnsembleSpells.add).parameters) == ["self", "y", "m0", "target"]
    assert issubclass(tmg_ops.EnsembleSpells, tmg_ops.EnsembleFeed)
    assert list(inspect.signature(tmg_ops.spell_args).parameters) == ["events", "max_len", "C"]
    assert list(inspect.signature(tmg_ops.spell_outputs).parameters) == ["hist", "length", "cens", "cens_len", "S", "Tn", "HW"]
    plan = inspect.signature(tmg_hip.ens_spell_plan).parameters
    assert list(plan) == ["S", "B", "HW", "K", "L", "Tn", "code"] and plan["code"].default is False
    assert "(S + 1) B K HW 4 bytes" in tmg_ops.EnsembleSpells.__doc__                # the device memory is stated
    for word in ("excluded from the histograms", "stride", "censored"):
        assert word in utils.modelPredSpells.__doc__, word


# ---- the plan and the codes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B,HW,Kn,L,Tn", [(1, 1, 1, 1, 1, 2), (7, 3, 35, 4, 4, 9), (8, 2, 256, 1, 32, 40), (33, 3, 257, 4, 64, 9),
                                            (1024, 1, 561, 2, 64, 32767), (32, 4, 65536, 1, 32, 100)])
def test_plan_values(S, B, HW, Kn, L, Tn):
    import tmg_hip
    p = tmg_hip.ens_spell_plan(S, B, HW, Kn, L, Tn)
    G = K.group(Kn, L)
    assert 1 <= G <= 8 and p["group"] == G and p["threads"] == 256
    assert p["grid"] == (-(-HW // 256), B) and p["blocks"] == -(-HW // 256) * B
    assert p["lds_bytes"] == G * Kn * 2 * (L + 3) * 4 <= 16384 and p["fin_lds_bytes"] == G * Kn * 2 * 4 * 4
    assert G == 8 or (G + 1) * Kn * 2 * (L + 3) * 4 > 16384
    assert p["state_words"] == (S + 1) * B * Kn * HW and p["row_words"] == L + 7 and p["table_words"] == B * Kn * (S + 1) * 2 * (L + 7)


def test_the_group_sizes_the_gpu_cases_assume():
    import tmg_hip
    for S, B, Cc, hw, Kn, Tn, L, kind, padded in K.TABLE:
        assert tmg_hip.ens_spell_plan(S, B, hw[0] * hw[1], Kn, L, Tn)["group"] == K.group(Kn, L)
    assert K.group(4, 4) == 8 and K.group(4, 64) == 7
    sizes = {c[0] for c in K.TABLE}
    assert {1, 2, 7, 8, 9, 17} <= sizes and 15 in sizes                        # 1, 2, G - 1, G, G + 1, 2 G + 1, and 2 G + 1 at G = 7


def test_codes_before_any_launch():
    import tmg_hip
    lib = tmg_hip.lib()
    plan = (c_i64 * 10)()
    good = [5, 2, 72, 2, 8, 9]                                                # S, B, HW, K, L, Tn
    assert lib.tmg_ens_spell_plan(_i64(*good), plan) == 0
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 5), (4, 0), (4, 65), (5, 1), (5, 0)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_spell_plan(_i64(*d), plan) == -1, (pos, bad)
    for pos, bad in ((0, 1025), (1, 65536), (2, (1 << 31) - 256), (5, 32768)):
        d = list(good)
        d[pos] = bad
        assert lib.tmg_ens_spell_plan(_i64(*d), plan) == -2, (pos, bad)
    assert lib.tmg_ens_spell_plan(_i64(1024, 65535, 1 << 20, 4, 8, 9), plan) == -2  # the state is over the index range
    assert lib.tmg_ens_spell_plan(_i64(1024, 1, 35, 1, 64, 32767), plan) == 0       # both limits at once are fine
    assert lib.tmg_ens_spell_plan(None, plan) == -3 and lib.tmg_ens_spell_plan(_i64(*good), None) == -3
    assert tmg_hip.ens_spell_plan(0, 1, 5, 1, 4, 9, code=True)[1] == -1
    assert tmg_hip.ens_spell_plan(1, 1, 5, 1, 4, 40000, code=True)[1] == -2
    with pytest.raises(RuntimeError):
        tmg_hip.ens_spell_plan(1025, 1, 5, 1, 4, 9)
    nul = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                                                  # never dereferenced: every code comes before a launch
    k, B, HW, Cc, S, Kn, L, Tn = 2, 2, 72, 3, 5, 2, 8, 9
    base = [k, B, HW, Cc, S, 0, Kn, L, Tn, 0]                                  # k, B, HW, C, S, row0, K, L, Tn, t

    def step(dims=base, y=one, yd=(4, 1), thr=one, ev=(0, 0, 2, 1), state=one, table=one, maps=one):
        return lib.tmg_ens_spell_step(y, _i64(*yd) if yd else None, thr, _i64(*ev) if ev else None, state, table, maps, _i64(*dims), nul)

    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 1), (3, 5), (4, 0), (5, -1), (5, 4), (6, 0), (6, 5), (7, 0), (7, 65), (8, 1), (9, -1), (9, Tn)):
        d = list(base)
        d[pos] = bad
        assert step(d) == -1, (pos, bad)
    d = list(base)
    d[0], d[5] = 2, S                                                         # the target is a one-row chunk
    assert step(d) == -1
    for yd in ((2, 0), (4, -1), (4, 2)):
        assert step(yd=yd) == -1, yd
    for ev in ((3, 0, 2, 1), (0, 2, 2, 1), (-1, 0, 2, 1)):
        assert step(ev=ev) == -1, ev
    for pos, bad in ((4, 1025), (1, 65536), (2, (1 << 31) - 256), (8, 32768)):
        d = list(base)
        d[pos] = bad
        assert step(d) == -2, (pos, bad)
    assert step(yd=(1 << 31, 0)) == -2
    assert step(yd=None) == -3 and step(ev=None) == -3
    assert step(y=nul) == -3 and step(thr=nul) == -3 and step(state=nul) == -3 and step(table=nul) == -3 and step(maps=nul) == -3
    assert lib.tmg_ens_spell_step(one, _i64(4, 1), one, _i64(0, 0, 2, 1), one, one, one, None, nul) == -3

    def fin(dims=good, state=one, table=one, maps=one):
        return lib.tmg_ens_spell_finalize(state, table, maps, _i64(*dims) if dims else None, nul)

    for pos, bad, code in ((0, 0, -1), (3, 5, -1), (4, 65, -1), (5, 1, -1), (0, 1025, -2), (5, 32768, -2)):
        d = list(good)
        d[pos] = bad
        assert fin(d) == code, (pos, bad)
    assert fin(dims=None) == -3 and fin(state=nul) == -3 and fin(table=nul) == -3 and fin(maps=nul) == -3


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
def test_spell_args_follow_the_event_rules_and_check_max_len():
    import tmg_ops as ops
    ev, L = ops.spell_args([(0, 0.0, "<"), (2, 1.5, ">")], 7, 3)
    assert [tuple(e) for e in ev] == [(0, 0.0, "<"), (2, 1.5, ">")] and L == 7 and type(L) is int
    assert ops.spell_args(((0, 0.0, "<"),), np.int64(64), 3)[1] == 64
    for events in ((), ((3, 0.0, "<"),), ((0, float("nan"), "<"),), ((0, 0.0, "="),), ((True, 0.0, "<"),), ((0, 0.0, "<"),) * 5):
        with pytest.raises(ValueError) as a:
            ops.spell_args(events, 32, 3)
        with pytest.raises(ValueError) as b:
            ops.event_args(events, (1,), 3)
        assert str(a.value) == str(b.value)                                   # event_args' own messages
    for bad in (0, 65, -1, True, 4.0, "4", None):
        with pytest.raises(ValueError, match=r"max_len is an integer in 1\.\.64"):
            ops.spell_args(((0, 0.0, "<"),), bad, 3)


def test_constructor_limits_come_with_their_numbers_before_any_device_work():
    import tmg_ops as ops
    from utils import utils
    ok = dict(members=5, B=2, C=3, Hh=8, Ww=9, steps=4, device="cuda", out_mu=torch.zeros(3), out_std=torch.ones(3))
    for kw, msg in ((dict(C=1), "2 <= C <= 4"), (dict(C=5, out_mu=torch.zeros(5), out_std=torch.ones(5)), "2 <= C <= 4"),
                    (dict(steps=1), "steps >= 2"), (dict(steps=True), "steps >= 2"), (dict(steps=2.0), "steps >= 2"),
                    (dict(members=0), "members"), (dict(members=1025), "1024"), (dict(B=0), "B, H, W >= 1"), (dict(Hh=0), "B, H, W >= 1"),
                    (dict(B=65536), "at most 65535 cases, got 65536"), (dict(steps=32768), r"steps = 32768 exceeds 32767"),
                    (dict(steps=32767, Hh=256, Ww=257), r"Tn HW = 32767 \* 65792"),
                    (dict(max_state_bytes=1000), r"\(5 \+ 1\) \* 2 \* 1 \* 72 \* 4 = 3456 bytes exceeds max_state_bytes = 1000"),
                    (dict(members=1024, B=64, Hh=128, Ww=128, events=((0, 0.0, "<"), (1, 0.0, ">"))), r"8598323200 bytes exceeds max_state_bytes = 2147483648"),
                    (dict(max_len=0), "max_len"), (dict(max_len=65), "max_len"), (dict(events=()), "at least one"),
                    (dict(out_std=torch.tensor([1.0, 0.0, 1.0])), "strictly positive"), (dict(u=torch.zeros(2, 3)), "strictly positive")):
        with pytest.raises(ValueError, match=msg):
            ops.EnsembleSpells(**dict(ok, **kw))
    with pytest.raises(RuntimeError, match="not a GPU"):
        ops.EnsembleSpells(**dict(ok, device="cpu"))
    with pytest.raises(ValueError):                                           # the argument error wins over the device error
        ops.EnsembleSpells(**dict(ok, device="cpu", max_len=0))
    for kw in (dict(events=()), dict(events=((3, 0.0, "<"),)), dict(max_len=0), dict(max_len=2.0)):
        with pytest.raises(ValueError):
            utils.modelPredSpells(None, None, None, None, **kw)
    z = torch.zeros(1, 3, 2, 4, dtype=torch.int64)
    zl, zc = z[..., 0], z[..., :3]
    ops.spell_outputs(z, zl, zc, zc, 2, 5, 7)
    for a in ((z.double(), zl, zc, zc, 2, 5, 7), (z, zl, zc, zc, 3, 5, 7), (z, zl[..., :1], zc, zc, 2, 5, 7), (z, zl, zc[..., :2], zc, 2, 5, 7),
              (z, zl, zc, zc, 2, 1, 7), (z, zl, zc, zc, 2, 32767, 65792)):
        with pytest.raises(ValueError):
            ops.spell_outputs(*a)


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
SMALL = [(3, 2, 3, (2, 5), 4, 7, 3, "int", False), (2, 1, 2, (3, 3), 4, 2, 4, "ar1", False), (1, 2, 4, (2, 4), 1, 3, 1, "int", False),
         (4, 1, 3, (2, 4), 4, 12, 5, "ar1", False)]


@pytest.mark.parametrize("case", SMALL)
def test_the_reference_equals_the_regular_expression_statement_and_the_counted_transitions(case):
    S, B, Cc, hw, Kn, Tn, L, kind, _ = case
    xs, tgt = K.make_inputs(case, 7)
    if kind == "ar1":
        K.plant_nonfinite(xs, tgt, 8)
    ev = K.events_for(Cc, Kn)
    thr = K.thresholds(ev, B)
    ref = K.reference(xs, tgt, thr, ev, L)
    assert not K.mismatches(K.regex_tables(xs, tgt, thr, ev, L), ref, K.TABLE_KEYS + K.MAP_KEYS)
    K.check_identities(ref, Tn, hw[0] * hw[1], K.transitions(xs, tgt, thr, ev))


def test_run_list_on_series_written_by_hand():
    E = np.array([[1, 1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1]], dtype=bool)
    series, start, length, pol, cls = K.run_list(E)
    assert series.tolist() == [0, 0, 0, 0, 1, 2, 2, 2, 2, 2, 2, 2]
    assert start.tolist() == [0, 2, 5, 6, 0, 0, 1, 2, 3, 4, 5, 6] and length.tolist() == [2, 3, 1, 1, 7, 1, 1, 1, 1, 1, 1, 1]
    assert pol.tolist() == [1, 0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 1]
    assert cls.tolist() == [K.LEFT, K.COMPLETE, K.COMPLETE, K.RIGHT, K.BOTH, K.LEFT] + [K.COMPLETE] * 5 + [K.RIGHT]


def test_planted_pixels_give_the_known_runs():
    case = (2, 1, 2, (5, 7), 1, 9, 4, "ar1", False)
    xs, tgt = K.make_inputs(case, 3)
    ev = K.events_for(2, 1)
    ref = K.reference(xs, tgt, K.thresholds(ev, 1), ev, 4)
    flat = {k: ref[k].reshape(1, 1, 35) for k in K.MAP_KEYS}
    assert flat["target_longest"][0, 0, :6].tolist() == [9, 0, 1, 3, 4, 5]
    assert flat["target_spell_count"][0, 0, :6].tolist() == [1, 0, 5, 1, 1, 1]
    assert flat["target_in_count"][0, 0, :6].tolist() == [9, 0, 5, 3, 4, 5]
    # the target's planted complete spells of length 3, 4, 5 land in bins 2, 3, 3 (the last bin is open)
    only = np.zeros_like(xs), np.zeros_like(tgt)
    only[0][:], only[1][:] = 5.0, 5.0                                          # never in: one gap that covers the window
    K.plant(only[0], only[1], ev, 4)
    t = K.reference(only[0], only[1], K.thresholds(ev, 1), ev, 4)
    assert t["spell_hist"][0, 0, 2, 1].tolist() == [3, 0, 1, 2] and int(t["spell_len"][0, 0, 2, 1]) == 3 + 3 + 4 + 5
    assert t["spell_cens"][0, 0, 2, 1].tolist() == [1, 1, 1] and t["spell_cens_len"][0, 0, 2, 1].tolist() == [1, 1, 9]
    assert t["spell_cens"][0, 0, 2, 0].tolist() == [3, 3, 30]                  # gaps: before and after the three planted spells, and the
    #                                                                            never-in pixel with the 29 untouched ones


@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_the_four_identities_hold_on_every_case(idx):
    S, B, Cc, hw, Kn, Tn, L, kind, _ = K.TABLE[idx]
    xs, tgt = K.inputs(idx)
    ev = K.events_for(Cc, Kn)
    ref = K.case_reference(idx)
    assert ref["spell_hist"].shape == (B, Kn, S + 1, 2, L) and ref["spell_cens_len"].shape == (B, Kn, S + 1, 2, 3)
    assert ref["time_in_count"].shape == (B, Kn) + hw and all(ref[k].dtype == np.int64 for k in K.TABLE_KEYS + K.MAP_KEYS)
    K.check_identities(ref, Tn, hw[0] * hw[1], K.transitions(xs, tgt, K.thresholds(ev, B), ev))
    assert int(ref["time_longest_max"].max()) <= Tn and np.array_equal(ref["time_in_count"] == 0, ref["time_spell_count"] == 0)


# ---- spell_outputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(K.TABLE)))
def test_spell_outputs_agree_with_the_fp64_restatement(idx):
    import tmg_ops as ops
    S, B, Cc, hw, Kn, Tn, L, kind, _ = K.TABLE[idx]
    ref = K.case_reference(idx)
    got = {k: v.numpy() for k, v in ops.spell_outputs(*[torch.from_numpy(ref[k]) for k in K.TABLE_KEYS], S, Tn, hw[0] * hw[1]).items()}
    want = K.host_reference(ref, S)
    assert set(got) == set(K.INT_HOST_KEYS + K.FLOAT_HOST_KEYS)
    assert not K.mismatches(got, want, K.INT_HOST_KEYS)
    worst = K.check_floats(got, want, K.FLOAT_HOST_KEYS, "case %d" % idx)
    assert got["spell_w1"].shape == (B, Kn, S, 2) and got["spell_p11"].shape == (B, Kn, S + 1)
    print("case %d: worst share of the float tolerance %.3f" % (idx, worst))


def test_spell_outputs_known_answers():
    import tmg_ops as ops
    S, L = 2, 4
    hist = torch.zeros(1, 1, S + 1, 2, L, dtype=torch.int64)
    slen = torch.zeros(1, 1, S + 1, 2, dtype=torch.int64)
    cens = torch.zeros(1, 1, S + 1, 2, 3, dtype=torch.int64)
    clen = torch.zeros(1, 1, S + 1, 2, 3, dtype=torch.int64)
    # member 0: spells 1, 1, 2, 4+ (6); member 1: none complete; the target: spells 2, 2
    hist[0, 0, 0, 1] = torch.tensor([2, 1, 0, 1])
    slen[0, 0, 0, 1] = 10
    hist[0, 0, 2, 1] = torch.tensor([0, 2, 0, 0])
    slen[0, 0, 2, 1] = 4
    cens[0, 0, 1, 0, 2], clen[0, 0, 1, 0, 2] = 3, 30                           # member 1: three pixels never in the event
    o = ops.spell_outputs(hist, slen, cens, clen, S, 10, 3)
    assert o["spell_mean"][0, 0, :, 1].tolist()[0] == 2.5 and o["spell_mean"][0, 0, 2, 1] == 2.0 and torch.isnan(o["spell_mean"][0, 0, 1, 1])
    assert o["spell_survival"][0, 0, 0, 1].tolist() == [1.0, 0.5, 0.25, 0.25]
    assert o["spell_w1"][0, 0, 0, 1] == 1.0 and torch.isnan(o["spell_w1"][0, 0, 1, 1])      # |.5 - 0| + |.75 - 1| + |.75 - 1|
    assert o["spell_mean_valid"][0, 0].tolist() == [0, 1] and o["spell_mean_below"][0, 0].tolist() == [0, 0]
    assert o["spell_mean_equal"][0, 0].tolist() == [0, 0]
    assert float(o["spell_p01"][0, 0, 1]) == 0.0 and torch.isnan(o["spell_p11"][0, 0, 1]) and torch.isnan(o["spell_markov_mean"][0, 0, 1])
    # spells of 10 steps in 4 runs, none censored: n11 = 6, n10 = 4
    assert abs(float(o["spell_p11"][0, 0, 0]) - 0.6) < 1e-7 and abs(float(o["spell_markov_mean"][0, 0, 0]) - 2.5) < 1e-6
    assert all(v.dtype == (torch.int64 if k in K.INT_HOST_KEYS else torch.float32) for k, v in o.items())


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate", K.MUTATIONS)
def test_named_mutations_are_caught(mutate):
    """Every mutation changes at least one array the GPU test compares, on the case set; the ones that touch ties or NaN alone must
    change nothing on continuous finite data, which shows that they are mutations of that rule and nothing else."""
    keys = K.TABLE_KEYS + K.MAP_KEYS
    caught = []
    for idx, case in enumerate(K.TABLE):
        S, B, Cc, hw, Kn, Tn, L, kind, _ = case
        xs, tgt = K.inputs(idx)
        if mutate == "nan_in_event":
            xs, tgt = xs.copy(), tgt.copy()
            K.plant_nonfinite(xs, tgt, 50 + idx)
        ev = K.events_for(Cc, Kn)
        thr = K.thresholds(ev, B)
        ref = K.reference(xs, tgt, thr, ev, L)
        assert not K.mismatches(ref, ref, keys)
        bad = K.mismatches(K.reference(xs, tgt, thr, ev, L, mutate), ref, keys)
        if kind == "ar1" and mutate == "non_strict":
            assert not bad, (idx, bad)                                        # no ties on continuous data (the planted values are off it)
        caught.append(bool(bad))
    assert any(caught), mutate
    if mutate in ("censored_complete", "length_off_by_one", "left_right_swapped"):
        assert all(caught), (mutate, caught)


def test_the_comparison_sees_one_unit_one_dtype_and_one_key():
    ref = K.case_reference(1)
    keys = K.TABLE_KEYS + K.MAP_KEYS
    for k in keys:
        off = {n: v.copy() for n, v in ref.items()}
        off[k].reshape(-1)[-1] += 1
        assert K.mismatches(off, ref, keys) == [k]
        cast = dict(ref)
        cast[k] = ref[k].astype(np.int32)
        assert K.mismatches(cast, ref, keys) == [k]
    assert K.mismatches({k: v for k, v in ref.items() if k != "spell_cens"}, ref, keys) == ["spell_cens"]
