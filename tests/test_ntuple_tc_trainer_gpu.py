"""NTupleTrainer with temporal-coherence learning rates (NTupleConfig.tc) on the GPU: its step against
the numpy restatement, checkpoint / resume bit for bit with the error sums, the refusals between
tc=True and tc=False, the default path unchanged, and that TC at alpha 1.0 learns clearly faster
than TD(0) at alpha 0.25."""
import numpy as np
import pytest
import torch

from test_ntuple_gpu import sums_numpy
from test_ntuple_tc_gpu import tc_numpy
from test_ntuple_trainer_gpu import _state, host, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tc_state(tr):
    return _state(tr) + [tr.net.tc_e.view(torch.int32), tr.net.tc_a.view(torch.int32)]


def test_tc_train_step_equals_the_numpy_restatement():
    """20 steps of a tc=True, alpha=1.0 lines-squares trainer at 65 boards from seeded random tables.
    delta is bit-equal to the float32 restatement from the step's own act outputs; tables, E and A
    agree with the restated rule within 1e-6 relative on |old| + |increment|; entries not hit keep
    their bits; later steps run entries at a rate below 1."""
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    n = 65
    tr = seeded(NTupleTrainer(NTupleConfig(n_boards=n, layout="lines-squares", alpha=1.0, seed=5, tc=True), device=DEV))
    assert tr.net.tc
    cells, m = tr.net.cells, tr.net.m
    worst, below = 0.0, 0
    for step in range(20):
        old, e, a = host(tr.net.tables).ravel(), host(tr.net.tc_e).ravel(), host(tr.net.tc_a).ravel()
        p_after, p_value, p_done, p_valid = host(tr.prev_after), host(tr.prev_value), host(tr.prev_done), host(tr.prev_valid)
        tr.train_step()
        v, r = host(tr.prev_value), host(tr.reward)          # this step's act outputs
        target = np.where(p_done != 0, np.float32(0), r.astype(np.float32) + v).astype(np.float32)
        delta = (target - p_value).astype(np.float32)
        np.testing.assert_array_equal(host(tr.delta), delta)
        acc, cnt = sums_numpy(p_after, delta, p_valid, cells)
        hit = cnt != 0
        assert hit.any() == (step > 0)
        got = [host(tr.net.tables).ravel(), host(tr.net.tc_e).ravel(), host(tr.net.tc_a).ravel()]
        for g, o in zip(got, (old, e, a)):
            np.testing.assert_array_equal(g[~hit], o[~hit])
        if hit.any():
            rate, mean, inc, *want = tc_numpy(old[hit], e[hit], a[hit], acc[hit], cnt[hit], 1.0 / (8 * m))
            below += int((rate < 1).sum())
            for g, w, o, d in zip(got, want, (old, e, a), (inc, mean, mean)):
                err, tol = np.abs(g[hit].astype(np.float64) - w), 1e-6 * (np.abs(o[hit]) + np.abs(d))
                worst = max(worst, float((err / np.maximum(tol, 1e-30)).max()))
                assert (err <= tol).all()
        assert not bool(tr.net.acc.any()) and not bool(tr.net.cnt.any())
    print("tc train_step parity: worst err / tol %.3g, %d entry updates at a rate below 1" % (worst, below))
    assert tr.updates == 20 and below > 0


def test_tc_checkpoint_resume_is_bit_identical_and_tc_must_match(tmp_path):
    from rein48_amd import checkpoint
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    cfg = dict(n_boards=257, layout="lines-squares", alpha=1.0, seed=21, tc=True)
    straight = seeded(NTupleTrainer(NTupleConfig(**cfg), device=DEV))
    for _ in range(6):
        straight.train_step()
    first = seeded(NTupleTrainer(NTupleConfig(**cfg), device=DEV))
    for _ in range(3):
        first.train_step()
    path = str(tmp_path / "nt_tc.pt")
    checkpoint.save(first, path)
    resumed = NTupleTrainer(NTupleConfig(**cfg), device=DEV)
    checkpoint.load(resumed, path)
    assert resumed.updates == 3 and resumed.env.counters == first.env.counters
    for x, y in zip(_tc_state(first), _tc_state(resumed)):
        assert torch.equal(x, y)
    assert bool(resumed.net.tc_a.any())
    for _ in range(3):
        resumed.train_step()
    for x, y in zip(_tc_state(straight), _tc_state(resumed)):
        assert torch.equal(x, y)
    assert resumed.updates == 6 and resumed.env.counters == straight.env.counters
    # a tc=True checkpoint into a tc=False trainer is refused, and the converse
    plain_cfg = dict(cfg, tc=False)
    plain = seeded(NTupleTrainer(NTupleConfig(**plain_cfg), device=DEV))
    with pytest.raises(ValueError):
        checkpoint.load(plain, path)
    plain.train_step()
    plain_path = str(tmp_path / "nt_plain.pt")
    checkpoint.save(plain, plain_path)
    assert "tc_e" not in torch.load(plain_path, map_location="cpu", weights_only=True)
    with pytest.raises(ValueError):
        checkpoint.load(NTupleTrainer(NTupleConfig(**cfg), device=DEV), plain_path)
    checkpoint.load(NTupleTrainer(NTupleConfig(**plain_cfg), device=DEV), plain_path)
    # a file from before the tc field reads as tc=False through the defaults
    st = torch.load(plain_path, map_location="cpu", weights_only=True)
    del st["cfg"]["tc"]
    old_path = str(tmp_path / "nt_old.pt")
    torch.save(st, old_path)
    checkpoint.load(NTupleTrainer(NTupleConfig(**plain_cfg), device=DEV), old_path)
    with pytest.raises(ValueError):
        checkpoint.load(NTupleTrainer(NTupleConfig(**cfg), device=DEV), old_path)


def test_default_trainer_is_td_and_reproducible():
    """tc defaults to False: no error sums are allocated, and two such trainers' 6 steps agree bit
    for bit (the default path inside this file)."""
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    cfg = dict(n_boards=257, layout="lines-squares", alpha=0.25, seed=21)
    assert NTupleConfig().tc is False
    out = []
    for _ in range(2):
        tr = seeded(NTupleTrainer(NTupleConfig(**cfg), device=DEV))
        assert tr.net.tc is False and tr.net.tc_e is None and tr.net.tc_a is None
        for _ in range(6):
            tr.train_step()
        out.append(_state(tr))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    # and TC from the same start departs from it once entries have history
    tc = seeded(NTupleTrainer(NTupleConfig(**dict(cfg, tc=True)), device=DEV))
    for _ in range(6):
        tc.train_step()
    assert not torch.equal(tc.net.tables.view(torch.int32), out[0][0])


def test_tc_learns_faster_than_td():
    """lines-squares, 1,024 boards, 1,000 train_step()s, seed 0: TC at alpha 1.0 against TD(0) at alpha
    0.25, 512 whole greedy episodes each with the same seed. The TC mean exceeds the TD mean by more
    than 5 standard errors of the difference (a CPU simulation of this trainer gives 2,870 +- 46
    against 1,861 +- 32, 18 standard errors, so a miss is a defect, not noise)."""
    from rein48_amd.evaluate import play_episodes
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    scores = {}
    for name, alpha, tc in (("tc", 1.0, True), ("td", 0.25, False)):
        tr = NTupleTrainer(NTupleConfig(n_boards=1024, layout="lines-squares", alpha=alpha, seed=0, tc=tc), device=DEV)
        for _ in range(1000):
            tr.train_step()
        ev = play_episodes(tr.net.policy(), 512, device=DEV, seed=1, return_scores=True)
        assert ev["finished"] == 1.0
        scores[name] = ev["scores"].numpy().astype(np.float64)
    s, b = scores["tc"], scores["td"]
    se = float(np.sqrt(s.var(ddof=1) / len(s) + b.var(ddof=1) / len(b)))
    print("TC mean %.1f, TD mean %.1f, ratio %.3f, difference %.1f standard errors"
          % (s.mean(), b.mean(), s.mean() / b.mean(), (s.mean() - b.mean()) / se))
    assert s.mean() - b.mean() > 5 * se
