"""The case tables of the autograd-node tests (node_cases.py), checked without a GPU: every case is valid and every test can fail.

  test_constants_are_the_kernel_tests_own     the bounds restated in node_cases.py are the kernel tests' constants
  test_restatement_equals_the_oracle          ref_coupling / ref_lstm_coupling (recorder, mutation switches) = oracle.coupling /
                                              oracle.lstm_coupling bit for bit in fp64: outputs and every gradient
  test_seed_and_margin                        every case has a seed in 0 .. 15 whose rectified pre-activations keep |value| >= 1e-4;
                                              prints seed, margin, the fp32 CPU error of the same pre-activations, and the largest
                                              err / bound of an fp32 CPU evaluation of the whole reference (the bounds can be met)
  test_every_mutation_moves_an_output         each mutation of the reference moves at least one checked output to >= 10x its bound
                                              at every case of the node it applies to (the bounds can be missed)."""
import math

import pytest
import torch

import node_cases as N

SEEDED = N.seeded_cases()
UNSEEDED = N.unseeded_cases()
ALL = SEEDED + UNSEEDED


def test_constants_are_the_kernel_tests_own():
    import test_coupling_kernels as TC
    import test_pointwise_kernels as TP
    import conv_cases
    assert N.U == conv_cases.U24 == TP.U
    assert N.TOL_D2 == TC.TOL_D2
    assert (N.TOL_AFF, N.TOL_AFFB, N.TOL_LSTM_H, N.TOL_LSTM_B) == (TP.TOL_AFF, TP.TOL_AFFB, TP.TOL_LSTM_H, TP.TOL_LSTM_B)
    assert N.tol_sum(100, 2.0) == TP.tol_sum(100, 2.0)


@pytest.mark.parametrize("label,thunk", [(c[0], c[1]) for c in SEEDED if c[0].split()[0] in ("coupling", "lstm", "window")],
                         ids=[c[0] for c in SEEDED if c[0].split()[0] in ("coupling", "lstm", "window")])
def test_restatement_equals_the_oracle(label, thunk):
    d = thunk()
    assert set(d.mine) == set(d.ref)
    for k, r in d.ref.items():
        assert (d.mine[k] is None) == (r is None), k
        if r is not None:
            assert torch.equal(d.mine[k], r), "%s: %s differs from the oracle by %.3e" % (label, k, float((d.mine[k] - r).abs().max()))


def _fp32_floor(d):
    """max |fp32 - fp64| over the rectified pre-activations, both evaluated by torch on the CPU."""
    rec = N.Rec()
    out = d.run(None, torch.float32, rec)
    floor = max((float((z.double() - z64).abs().max()) for (_, z), (_, z64) in zip(rec.pre, d.rec.pre)), default=0.0)
    return floor, out


@pytest.mark.parametrize("label,thunk", [(c[0], c[1]) for c in SEEDED], ids=[c[0] for c in SEEDED])
def test_seed_and_margin(label, thunk):
    d = thunk()
    floor, out32 = _fp32_floor(d)
    share = N.moved(d, out32)
    print("NODECASE %-30s seed %2d  min|pre-activation| %.3e  fp32 CPU error of it %.2e  fp32 CPU err / bound %.3f"
          % (label, d.seed, d.margin, floor, share))
    assert d.seed_ok and d.margin >= N.MARGIN, "%s: no seed in 0 .. %d keeps the margin (best %.3e)" % (label, N.MAX_SEEDS - 1, d.margin)
    # a ReLU flips only where the fp32 error exceeds |pre-activation|: ten times the CPU's fp32 error must still fit under the smallest
    assert floor * 10 <= d.margin, "%s: the fp32 error %.2e of a pre-activation is within 10x of the smallest one" % (label, floor)
    assert share <= 1.0, "%s: an fp32 CPU evaluation of the reference misses the derived bound (%.2f of it)" % (label, share)


@pytest.mark.parametrize("label,thunk", [(c[0], c[1]) for c in UNSEEDED], ids=[c[0] for c in UNSEEDED])
def test_fp32_cpu_evaluation_meets_the_bounds(label, thunk):
    d = thunk()
    share = N.moved(d, d.run(None, torch.float32))
    print("NODECASE %-30s fp32 CPU err / bound %.3f" % (label, share))
    assert share <= 1.0, label


MUTS = [(c[0], c[1], m) for c in ALL for m in c[2]]


@pytest.mark.parametrize("label,thunk,mut", MUTS, ids=["%s-%s" % (c[0], c[2]) for c in MUTS])
def test_every_mutation_moves_an_output(label, thunk, mut):
    d = thunk()
    share = N.moved(d, d.run(mut))
    print("NODEMUT %-30s %-24s moves an output to %.3g x its bound" % (label, mut, share))
    assert share >= 10.0, "%s: mutation %s moves no checked output by 10x its bound (largest %.3g x)" % (label, mut, share)


def test_every_listed_mutation_is_exercised():
    used = {m for _, _, m in MUTS}
    listed = set(N.COUPLING_MUTATIONS) | set(N.LSTM_MUTATIONS) | set(N.LSTM_PAD_MUTATIONS) | set(N.WINDOW_MUTATIONS) | \
        set(N.CELL_MUTATIONS) | set(N.DENSE_MUTATIONS) | set(N.MIX_MUTATIONS)
    assert used == listed, sorted(listed - used)


def test_error_measures():
    a = torch.tensor([1.0, 2.0, 4.0])
    assert N.err(a, a) == 0.0
    assert N.err(torch.tensor([1.0, 2.0, 4.5]), a) == 0.125
    assert N.err(torch.tensor([1.0, math.nan, 4.0]), a) == math.inf
    assert N.ld_err(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0]), torch.tensor([0.5, 4.0]).double()) == 0.25
