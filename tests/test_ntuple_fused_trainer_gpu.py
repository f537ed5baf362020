"""NTupleTrainer's fused step (NTupleConfig.fused: td_act, apply, env.step) on the GPU against the
unfused step of the same build, bit for bit: 600 steps of lines-squares at 257 boards from the same
seed, for TD(0) at alpha 0.25 and for TC at alpha 1.0, with episodes ending (and boards auto-reset)
on the way; train_steps(k) against k train_step()s; and checkpoints crossing between the two paths
in both directions."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {"td": dict(alpha=0.25, tc=False), "tc": dict(alpha=1.0, tc=True)}


def trainer(mode, fused, **kw):
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    cfg = dict(n_boards=257, layout="lines-squares", seed=0, fused=fused, **MODES[mode])
    cfg.update(kw)
    return NTupleTrainer(NTupleConfig(**cfg), device=DEV)


def state(tr):
    """Everything that decides the trainer's next step, and this step's outputs."""
    out = {"tables": tr.net.tables.view(torch.int32), "boards": tr.env.boards, "prev_after": tr.prev_after,
           "prev_value": tr.prev_value.view(torch.int32), "prev_done": tr.prev_done, "prev_valid": tr.prev_valid,
           "actions": tr.actions, "reward": tr.reward, "legal": tr.legal, "delta": tr.delta.view(torch.int32)}
    if tr.net.tc:
        out.update(tc_e=tr.net.tc_e.view(torch.int32), tc_a=tr.net.tc_a.view(torch.int32))
    return out


def assert_same(a, b):
    sa, sb = state(a), state(b)
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.updates == b.updates and a.env.counters == b.env.counters
    for tr in (a, b):
        assert int(tr.prev_valid.max()) <= 1
        assert not bool(tr.net.acc.any()) and not bool(tr.net.cnt.any())


@pytest.mark.parametrize("mode", sorted(MODES))
def test_600_fused_steps_equal_600_unfused_steps(mode):
    from rein48_amd.ntuple import NTupleConfig
    assert NTupleConfig().fused is False
    fused, plain = trainer(mode, True), trainer(mode, False)
    assert fused.cfg.fused and not plain.cfg.fused
    ended = torch.zeros(257, dtype=torch.int32, device=DEV)
    for _ in range(600):
        fused.train_step()
        ended += fused.prev_done                                # read between steps; changes nothing
    for _ in range(600):
        plain.train_step()
    assert_same(fused, plain)
    episodes = int(ended.sum())
    print("%s: %d episodes ended in 600 steps of 257 boards" % (mode, episodes))
    assert episodes >= 1                                        # the prev_done branch and the auto-reset ran
    assert bool(fused.net.tables.any()) and fused.updates == 600
    if mode == "tc":
        assert bool(fused.net.tc_a.any())


@pytest.mark.parametrize("fused", [True, False])
def test_train_steps_is_k_train_steps(fused):
    one, many = trainer("tc", fused), trainer("tc", fused)
    for _ in range(50):
        one.train_step()
    many.train_steps(50)
    assert_same(one, many)
    assert many.updates == 50


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("first_fused", [True, False])
def test_a_checkpoint_crosses_between_the_two_paths(tmp_path, mode, first_fused):
    """200 steps on one path, saved, loaded into a trainer of the other path, 100 more steps: the
    state of a straight 300-step run. `fused` is not a field a checkpoint must agree on."""
    from rein48_amd import checkpoint
    first = trainer(mode, first_fused)
    first.train_steps(200)
    path = str(tmp_path / "nt.pt")
    checkpoint.save(first, path)
    second = trainer(mode, not first_fused)
    checkpoint.load(second, path)
    assert second.updates == 200 and second.env.counters == first.env.counters
    second.train_steps(100)
    straight = trainer(mode, first_fused)
    straight.train_steps(300)
    want, got = state(straight), state(second)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert second.updates == 300 and second.env.counters == straight.env.counters
    assert bool(straight.net.tables.any())
