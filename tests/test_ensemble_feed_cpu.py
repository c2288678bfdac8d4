"""The feeding protocol of the ensemble accumulators on its own (tmg_ops.EnsembleFeed): host bookkeeping, driven here without a
device and without a kernel.  S = 5 members of B = 2 cases of [3, 4, 6] over Tk = 3 steps, fed in chunks of 2, 2 and 1 members."""
import pytest
import torch

import common as C  # noqa: F401  (puts the package on the path)

S, B, CH, HH, WW, TK = 5, 2, 3, 4, 6, 3
CHUNKS = ((0, 2), (2, 2), (4, 1))


def _feed():
    import tmg_ops
    return tmg_ops.EnsembleFeed(S, B, CH, HH, WW, TK)


def _y(k, c=CH, h=HH, w=WW, rows=None):
    return torch.zeros(k * B if rows is None else rows, c, h, w)


TARGET = torch.zeros(B, CH, HH, WW)


def _step(f, time, chunks=CHUNKS):
    """Feed one step -> the (t_before, last) of its chunks."""
    seen = []
    for m0, k in chunks:
        yn, tn, kk, t_before, last = f.open_chunk(_y(k), m0, time)
        assert tuple(yn.shape) == (k * B, HH, WW, CH) and tn is None and kk == k
        seen.append((t_before, last))
        f.close_chunk(m0, k, time, last)
    return seen


def test_chunks_out_of_order_raise():
    f = _feed()
    with pytest.raises(ValueError, match="fed in order"):
        f.open_chunk(_y(2), 2)                                               # the wrong m0
    _step(f, True, CHUNKS[:2])
    with pytest.raises(ValueError, match="fed in order"):
        f.open_chunk(_y(2), 4)                                               # overruns S
    _step(f, True, CHUNKS[2:])
    _step(f, True)
    _step(f, True)
    with pytest.raises(ValueError, match="fed in order"):
        f.open_chunk(_y(2), 0)                                               # after the last step


@pytest.mark.parametrize("y", [_y(0, rows=3), _y(2, h=HH + 1), _y(2, c=CH - 1)], ids=["rows", "H", "C"])
def test_chunks_that_hold_no_whole_members_raise(y):
    with pytest.raises(ValueError, match="whole members"):
        _feed().open_chunk(y, 0)


def test_a_missing_or_misshaped_target_raises():
    f = _feed()
    with pytest.raises(ValueError, match="target shape None"):
        f.open_chunk(_y(2), 0, True, None, required=True)
    for required in (True, False):
        with pytest.raises(ValueError, match="target shape"):
            f.open_chunk(_y(2), 0, True, TARGET[:, :2], required=required)
    assert f.open_chunk(_y(2), 0, True, None)[1] is None                     # optional: none is fine
    tn = f.open_chunk(_y(2), 0, True, TARGET, required=True)[1]
    assert tuple(tn.shape) == (B, HH, WW, CH)
    assert (f._n, f._step) == (0, 0)                                         # opening alone counts nothing


def test_last_and_t_before_and_the_timed_steps():
    f = _feed()
    seen = [_step(f, time) for time in (False, True, True)]
    assert [[last for _, last in s] for s in seen] == [[False, False, True]] * 3
    assert [[t for t, _ in s] for s in seen] == [[0, 0, 0], [0, 0, 0], [1, 1, 1]]    # only the steps fed with time=True count
    assert f._timed == [1, 2]
    assert f.finalize_guard() == 2


def test_guard_before_any_step_and_without_a_timed_step():
    f = _feed()
    with pytest.raises(RuntimeError, match="0 of 3 steps"):
        f.finalize_guard()
    for _ in range(TK):
        _step(f, False)
    with pytest.raises(RuntimeError, match="no time statistics"):
        f.finalize_guard()


def test_the_variant_without_a_time_argument_counts_steps():
    f = _feed()
    _step(f, None)
    f.close_chunk(0, 2, None, f.open_chunk(_y(2), 0, None)[4])
    with pytest.raises(RuntimeError, match="1 of 3 steps fed"):              # a step is half fed
        f.finalize_guard(timed=False)
    assert f.open_chunk(_y(2), 2, None)[3] is None                           # no time statistics to count
    _step(f, None, CHUNKS[1:])
    with pytest.raises(ValueError, match="whole members"):
        f.open_chunk(_y(0), 0, None)                                         # and an empty chunk is none
    _step(f, None)
    assert f.finalize_guard(timed=False) == TK and f._timed == []
