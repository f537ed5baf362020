"""rein48_amd.ntuple.replica_steps without a GPU: the validation of NTupleReplicaTrainer's `replicas`
and `alphas`, and the per-replica step as the float32 the solo trainer's c_float(alpha / (8.0 * m))
is."""
import ctypes
import math

import pytest

from rein48_amd.ntuple import MAX_REPLICAS, replica_steps


def solo_step(alpha, m):
    """What ctypes hands r48_ntuple_apply for NTupleTrainer's float(alpha / (8.0 * m))."""
    return ctypes.c_float(alpha / (8.0 * m)).value


@pytest.mark.parametrize("m", [1, 2, 4, 5, 8])
def test_the_step_is_the_solo_trainers_float32(m):
    alphas = (1.0, 0.25, 0.1, 0.5, 0.0, 1e-3, 0.3, 2.0 / 3.0, 7.0)
    steps = replica_steps(len(alphas), alphas, 123.0, m)
    assert steps == [solo_step(a, m) for a in alphas]
    for s in steps:
        assert ctypes.c_float(s).value == s                     # a float32 value: a float32 tensor holds it exactly


def test_alpha_one_with_five_tuples_is_not_a_power_of_two():
    """1 / 40 is not a float32: the step is its nearest float32, not the double."""
    (step,) = replica_steps(1, (1.0,), 0.0, 5)
    assert step == solo_step(1.0, 5) and step != 1.0 / 40.0
    assert abs(step - 0.025) < 2.0 ** -29


def test_none_means_the_configs_alpha_everywhere():
    assert replica_steps(3, None, 0.25, 4) == [solo_step(0.25, 4)] * 3
    assert replica_steps(1, None, 1.0, 5) == [solo_step(1.0, 5)]
    assert len(replica_steps(MAX_REPLICAS, None, 0.1, 8)) == MAX_REPLICAS == 64


def test_alphas_may_be_any_sequence_of_numbers():
    want = [solo_step(0.5, 4), solo_step(1.0, 4)]
    assert replica_steps(2, [0.5, 1], 0.0, 4) == want
    assert replica_steps(2, iter((0.5, 1.0)), 0.0, 4) == want


def test_bad_replicas():
    for replicas in (0, -1, 65, 1000, 2.5, True):
        with pytest.raises(ValueError):
            replica_steps(replicas, None, 0.25, 4)


def test_bad_alphas():
    for replicas, alphas in ((2, (0.1,)), (2, (0.1, 0.2, 0.3)), (1, ()), (3, (0.1, 0.2))):
        with pytest.raises(ValueError, match="one alpha per replica"):
            replica_steps(replicas, alphas, 0.25, 4)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            replica_steps(2, (0.1, bad), 0.25, 4)
    with pytest.raises((ValueError, TypeError)):
        replica_steps(2, ("a", "b"), 0.25, 4)


def test_bad_tuple_count():
    for m in (0, 9):
        with pytest.raises(ValueError):
            replica_steps(2, None, 0.25, m)
