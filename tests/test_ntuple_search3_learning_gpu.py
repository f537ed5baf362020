"""Does the 3-ply expectimax search play better than the 2-ply one on the same tables?

The recipe of test_ntuple_search_learning_gpu.py: lines-squares, 1,024 boards, 1,000 train_step()s
at alpha 0.25 from seed 0; then 512 whole episodes with policy(depth=2) and 512 with
policy(depth=3), same tables, same eval seed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_depth3_search_scores_above_depth2():
    """mean_3 - mean_2 > 3 * sqrt(var_2 / 512 + var_3 / 512). Measured on one MI355X: depth 2 mean
    4,171.9, depth 3 mean 6,872.8, 21.2 standard errors; the depth-3 episodes take 2.7 s
    (BASELINE.md)."""
    from rein48_amd.evaluate import play_episodes
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    tr = NTupleTrainer(NTupleConfig(n_boards=1024, layout="lines-squares", alpha=0.25, seed=0), device=DEV)
    for _ in range(1000):
        tr.train_step()
    two = play_episodes(tr.policy(depth=2), 512, device=DEV, seed=1, return_scores=True)
    three = play_episodes(tr.policy(depth=3), 512, device=DEV, seed=1, return_scores=True)
    assert two["finished"] == 1.0 and three["finished"] == 1.0
    s2, s3 = two["scores"].numpy(), three["scores"].numpy()
    se = float(np.sqrt(s2.var(ddof=1) / len(s2) + s3.var(ddof=1) / len(s3)))
    print("depth 2 mean %.1f, depth 3 mean %.1f, difference %.1f standard errors"
          % (s2.mean(), s3.mean(), (s3.mean() - s2.mean()) / se))
    assert s3.mean() - s2.mean() > 3 * se
