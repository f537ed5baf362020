"""Does the 2-ply expectimax search play better than the 1-ply greedy search on the same tables?

The recipe of test_ntuple_trainer_gpu.py's learning test: lines-squares, 1,024 boards, 1,000
train_step()s at alpha 0.25 from seed 0; then 512 whole episodes with policy(depth=1) and 512 with
policy(depth=2), same tables, same eval seed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_depth2_search_scores_above_depth1():
    """mean_2 - mean_1 > 3 * sqrt(var_1 / 512 + var_2 / 512). Measured on one MI355X: depth 1 mean
    1,917.7, depth 2 mean 4,171.9, 29.0 standard errors."""
    from rein48_amd.evaluate import play_episodes
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    tr = NTupleTrainer(NTupleConfig(n_boards=1024, layout="lines-squares", alpha=0.25, seed=0), device=DEV)
    for _ in range(1000):
        tr.train_step()
    one = play_episodes(tr.policy(depth=1), 512, device=DEV, seed=1, return_scores=True)
    two = play_episodes(tr.policy(depth=2), 512, device=DEV, seed=1, return_scores=True)
    assert one["finished"] == 1.0 and two["finished"] == 1.0
    s1, s2 = one["scores"].numpy(), two["scores"].numpy()
    se = float(np.sqrt(s1.var(ddof=1) / len(s1) + s2.var(ddof=1) / len(s2)))
    print("depth 1 mean %.1f, depth 2 mean %.1f, difference %.1f standard errors"
          % (s1.mean(), s2.mean(), (s2.mean() - s1.mean()) / se))
    assert s2.mean() - s1.mean() > 3 * se
