"""The launch plans that share the slice rounding of csrc/tmg_common.h (tmg_slices) and the symmetric-Gram plan of csrc/tmg_symgram.h
are pinned to what they were before the two were written once: tests/golden/symgram_plans.json holds the raw output of
tmg_ens_gram_plan, tmg_ens_spod_plan, tmg_ens_pod_plan and tmg_ens_sfun_plan over a grid (tests/golden/make_symgram_golden.py wrote it
from the library of the commit before), and every tuple must come out equal.  No device is needed: the plan entries are host code."""
import ctypes
import json
import os

import pytest

import common as C

GOLDEN = os.path.join(C.GOLDEN, "symgram_plans.json")
HWS = {1: (1, 1), 63: (7, 9), 64: (8, 8), 255: (15, 17), 256: (16, 16), 257: (1, 257), 4096: (64, 64), 65536: (256, 256),
       1048576: (1024, 1024)}
S_GRAM = [1, 2, 14, 15, 16, 47, 62, 63, 64, 127, 128, 130, 500, 1023, 1024]    # test_energy_cpu's member counts
S_SPOD = [1, 6, 7, 8, 30, 31, 32, 63, 64, 127, 128, 255]                       # test_spod_cpu's
BATCH = {1: (2, 1, 1), 3: (3, 2, 2), 16: (4, 4, 16)}                           # B -> (C of gram and sfun, Cg, NB)
LAGS = [[(1, 0)], [(1, 0), (0, 1), (2, -1), (3, 3)]]                           # a lag that does not fit the field: the code is recorded
OUT = {"gram": 7, "spod": 9, "pod": 4, "sfun": 88}


def grid(entry):
    """The tuples of one entry: the dims array it is called with (sfun: dims, then the flat lag list)."""
    out = []
    for S in (S_SPOD if entry == "spod" else S_GRAM):
        for HW, (Hh, Ww) in HWS.items():
            for B, (Cc, Cg, NB) in BATCH.items():
                if entry == "gram":
                    out.append([S, B, Cc, HW])
                elif entry == "spod":
                    out += [[S, B, Cg, HW, NB, addr] for addr in (0, 4)]
                elif entry == "pod":
                    out.append([S, B, Cg, HW, 5])
                else:
                    out += [[S, B, Cc, Hh, Ww, len(lg)] + [v for l in lg for v in l] for lg in LAGS]
    return out


def evaluate(entry, dims):
    """-> [return code, plan...]: the entry's raw output (the plan of a refused call is left out)."""
    import tmg_hip
    i64 = lambda v: (ctypes.c_int64 * max(1, len(v)))(*v)                      # noqa: E731
    plan = (ctypes.c_int64 * OUT[entry])()
    fn = getattr(tmg_hip.lib(), "tmg_ens_%s_plan" % entry)
    rc = fn(i64(dims[:6]), i64(dims[6:]), plan) if entry == "sfun" else fn(i64(dims), plan)
    used = 8 + 5 * dims[5] if entry == "sfun" else OUT[entry]                  # sfun: the head, then five numbers per lag
    return [int(rc)] + ([int(v) for v in plan[:used]] if rc == 0 else [])


def test_an_edit_of_the_shared_header_rebuilds_its_users():
    import inspect
    import tmg_hip
    assert "tmg_symgram.h" in inspect.getsource(tmg_hip.build) and os.path.isfile(os.path.join(tmg_hip.CSRC, "tmg_symgram.h"))
    for name in ("tmg_gram.hip", "tmg_spod.hip"):
        src = open(os.path.join(tmg_hip.CSRC, name)).read()
        assert '#include "tmg_symgram.h"' in src and "symgram_store<DIAG, NTL>" in src and "SYMGRAM_LAUNCH(" in src
        assert "_reduce_kernel(" not in src and "_LAUNCH(DIAG_" not in src    # written once, in the header


def test_pinned_bits_reach_every_branch_of_the_engine():
    """tests/golden/symgram_bits.json (compared on the device by test_energy_gpu.py and test_spod_gpu.py): what the recorded plans say."""
    rec = json.load(open(os.path.join(C.GOLDEN, "symgram_bits.json")))
    for part in ("gram", "spod"):
        plans = [v["plan"] for v in rec[part].values()]
        assert any(p["part"] == 256 for p in plans)                            # one 16-row tile: NTL = 1
        assert any(p["part"] == 4096 and p["NT"] == 1 for p in plans)          # NT = 1 with NTL = 4
        assert any(p["NT"] > 1 and p["P"] > 1 for p in plans)                  # the off-diagonal instance, with the slice reduction
        assert any(p["P"] == 1 for p in plans) and any(p["P"] > 1 and p["part"] == 256 for p in plans)
        assert any(p["vec"] for p in plans) and any(not p["vec"] for p in plans)
        assert any(p["HW"] % 16 for p in plans)
    assert any(p["plan"]["NT"] > 1 and p["plan"]["P"] == 1 for p in rec["gram"].values())      # and without it
    assert any(p["plan"]["Cg"] > 1 and p["plan"]["NT"] > 1 for p in rec["spod"].values())
    assert any(not p["plan"]["vec"] and p["plan"]["NT"] > 1 for p in rec["spod"].values())     # scalar loads off the 16-byte grid


@pytest.mark.parametrize("entry", sorted(OUT))
def test_plan_is_what_it_was(entry):
    gold = json.load(open(GOLDEN))[entry]
    tuples = grid(entry)
    assert [g[0] for g in gold] == tuples and 300 <= len(tuples) <= 900
    assert sum(1 for g in gold if g[1][0] == 0) >= len(gold) // 2             # most of the grid is accepted
    for dims, want in gold:
        assert evaluate(entry, dims) == want, (entry, dims)
