"""NTupleTrainer with carousel shaping (NTupleConfig.carousel) on the GPU: carousel=() is the trainer
without the field bit for bit; fused and unfused steps agree bit for bit in the tables and in the
carousel's five buffers, with restarts from every stage; checkpoint / resume bit for bit with the cuts
and the buffers, across a run that restarts from the pool before and after the save; the refusal of
other cuts; and that a two-stage TC net trained with carousel learns to play clearly better than
greedy-merge (with the same recipe's score without carousel printed next to it)."""
import numpy as np
import pytest
import torch

from test_ntuple_trainer_gpu import _state, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAROUSEL = ("pool", "pool_has", "seen", "turn", "starts")


def _full_state(tr):
    net = tr.net
    st = _state(tr) + [getattr(net, k).view(torch.int32) for k in ("tc_e", "tc_a") if net.tc]
    st += [net.own] if net.cuts else []
    return st + ([getattr(tr, k) for k in CAROUSEL] if tr.carousel else [])


def start(cfg):
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    tr = seeded(NTupleTrainer(NTupleConfig(**cfg), device=DEV))
    if tr.net.cuts:
        tr.net.tables[1:] = tr.net.tables[0]
    return tr


@pytest.mark.parametrize("fused", [False, True])
def test_no_carousel_is_the_trainer_without_the_field(fused):
    """carousel=() allocates nothing, calls nothing and leaves every state tensor of a 40-step run equal
    to that of a trainer whose configuration never names the field."""
    cfg = dict(n_boards=257, layout="lines-squares", alpha=1.0, seed=8, tc=True, stages=(2, 3), fused=fused)
    a, b = start(cfg), start(dict(cfg, carousel=()))
    for tr in (a, b):
        tr.train_steps(40)
        assert tr.carousel == () and not any(hasattr(tr, k) for k in CAROUSEL)
        with pytest.raises(ValueError):
            tr.carousel_stats()
    assert a.env.counters == b.env.counters
    for x, y in zip(_full_state(a), _full_state(b)):
        assert torch.equal(x, y)
    for bad in ((0,), (16,), (4, 4), (5, 4), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            start(dict(cfg, carousel=bad))


@pytest.mark.parametrize("tc", [False, True])
def test_fused_and_unfused_steps_agree_bit_for_bit(tc):
    """lines-squares, 257 boards, carousel=(2, 3) on an unstaged net, 1,500 steps: tables, every trainer
    tensor and the five carousel buffers agree bit for bit, and boards have restarted in stage 1 and in
    stage 2 (asserted). Measured on an MI355X from these seeds (checked every 5 steps): starts[1] is
    non-zero from step 46 and starts[2] from step 155 without TC, from steps 55 and 470 with TC; after
    1,500 steps starts is [190, 326, 271] without TC and [1, 233, 60] with it (TC at alpha 1.0 learns to
    play longer games, so fewer episodes end), every pool slot filled in both."""
    cfg = dict(n_boards=257, layout="lines-squares", alpha=1.0 if tc else 0.25, seed=8, tc=tc, carousel=(2, 3))
    a, b = start(cfg), start(dict(cfg, fused=True))
    for tr in (a, b):
        tr.train_steps(1500)
    for x, y in zip(_full_state(a), _full_state(b)):
        assert torch.equal(x, y)
    stats = a.carousel_stats()
    print("carousel_stats after 1,500 steps (tc=%s): %r" % (tc, stats))
    assert stats == b.carousel_stats()
    assert stats["starts"][1] > 0 and stats["starts"][2] > 0
    assert len(stats["filled"]) == 3 and stats["filled"][0] == 1.0 and all(0.0 < f <= 1.0 for f in stats["filled"])
    # every start is counted once: the starts are the episodes that ended
    assert sum(stats["starts"]) > 0 and int(a.turn.max()) <= 2 and int(a.seen.max()) <= 2


def test_checkpoint_resume_is_bit_identical_and_the_cuts_must_match(tmp_path):
    """750 + 750 steps against 1,500 straight, a two-stage net with carousel=(2, 3). Measured on an MI355X from
    these seeds: boards restart from the pool from step 43 on; starts is [1, 154, 14] at the save and
    [6, 231, 106] at the end, so restarts from the pool happen on both sides of it (asserted)."""
    from rein48_amd import checkpoint
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    cfg = dict(n_boards=257, layout="lines-squares", alpha=1.0, seed=21, tc=True, stages=(3,), carousel=(2, 3), fused=True)
    straight = start(cfg)
    straight.train_steps(1500)
    first = start(cfg)
    first.train_steps(750)
    at_save = first.carousel_stats()["starts"]
    assert at_save[1] + at_save[2] > 0          # restarts from the pool before the save
    path = str(tmp_path / "nt_carousel.pt")
    checkpoint.save(first, path)
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert st["carousel"] == [2, 3] and st["cfg"]["carousel"] == [2, 3] and sorted(st["carousel_state"]) == sorted(CAROUSEL)
    assert st["carousel_state"]["pool"].dtype == torch.int8 and tuple(st["carousel_state"]["pool"].shape) == (2, 257, 16)
    resumed = NTupleTrainer(NTupleConfig(**cfg), device=DEV)
    checkpoint.load(resumed, path)
    assert resumed.updates == 750 and resumed.env.counters == first.env.counters
    for x, y in zip(_full_state(first), _full_state(resumed)):
        assert torch.equal(x, y)
    resumed.train_steps(750)
    for x, y in zip(_full_state(straight), _full_state(resumed)):
        assert torch.equal(x, y)
    end = resumed.carousel_stats()["starts"]
    assert end == straight.carousel_stats()["starts"]
    assert end[1] + end[2] > at_save[1] + at_save[2]   # and after it
    # other cuts, more cuts and no carousel are refused, as other stages are
    for other in ((2, 4), (2,), (2, 3, 4), ()):
        with pytest.raises(ValueError):
            checkpoint.load(NTupleTrainer(NTupleConfig(**dict(cfg, carousel=other)), device=DEV), path)
    # a checkpoint without carousel carries no key, loads into a trainer without and not into one with
    plain_cfg = dict(cfg, carousel=())
    plain = start(plain_cfg)
    plain.train_steps(3)
    plain_path = str(tmp_path / "nt_plain.pt")
    checkpoint.save(plain, plain_path)
    st = torch.load(plain_path, map_location="cpu", weights_only=True)
    assert "carousel" not in st and "carousel_state" not in st
    again = NTupleTrainer(NTupleConfig(**plain_cfg), device=DEV)
    checkpoint.load(again, plain_path)
    assert torch.equal(again.net.tables.view(torch.int32), plain.net.tables.view(torch.int32))
    with pytest.raises(ValueError):
        checkpoint.load(NTupleTrainer(NTupleConfig(**cfg), device=DEV), plain_path)
    # a file from before the carousel field reads as carousel=()
    del st["cfg"]["carousel"]
    old_path = str(tmp_path / "nt_old.pt")
    torch.save(st, old_path)
    checkpoint.load(NTupleTrainer(NTupleConfig(**plain_cfg), device=DEV), old_path)
    with pytest.raises(ValueError):
        checkpoint.load(NTupleTrainer(NTupleConfig(**cfg), device=DEV), old_path)


def test_a_two_stage_tc_net_learns_with_carousel():
    """The recipe of test_a_two_stage_tc_net_learns -- lines-squares, 1,024 boards, 1,000 train_step()s,
    seed 0, TC at alpha 1.0, stages=(7,) -- with carousel=(7,), then 512 whole greedy episodes at eval seed
    1: the mean exceeds greedy-merge's on the same seed by more than 5 standard errors of the difference
    (the project's gate). The same recipe's score without carousel and the difference in standard errors
    are printed, not gated: nobody has measured what the carousel buys at this budget."""
    from rein48_amd.evaluate import afterstate_policy, play_episodes
    from rein48_amd.ntuple import NTupleConfig, NTupleTrainer
    scores = {}
    for name, carousel in (("carousel", (7,)), ("plain", ())):
        tr = NTupleTrainer(NTupleConfig(n_boards=1024, layout="lines-squares", alpha=1.0, seed=0, tc=True, stages=(7,),
                                        carousel=carousel), device=DEV)
        tr.train_steps(1000)
        ev = play_episodes(tr.net.policy(), 512, device=DEV, seed=1, return_scores=True)
        assert ev["finished"] == 1.0
        scores[name] = ev["scores"].numpy().astype(np.float64)
        print("%s: own[1] set in %.4f of the entries" % (name, float(tr.net.own[1].float().mean())))
        if carousel:
            print("carousel_stats: %r" % (tr.carousel_stats(),))
    base = play_episodes(afterstate_policy(None), 512, device=DEV, seed=1, return_scores=True)
    assert base["finished"] == 1.0
    scores["greedy"] = base["scores"].numpy().astype(np.float64)

    def gap(x, y):
        se = float(np.sqrt(x.var(ddof=1) / len(x) + y.var(ddof=1) / len(y)))
        return (x.mean() - y.mean()) / se

    c, p, b = scores["carousel"], scores["plain"], scores["greedy"]
    print("two-stage TC with carousel mean %.1f, greedy-merge mean %.1f: %.1f standard errors" % (c.mean(), b.mean(), gap(c, b)))
    print("without carousel mean %.1f: the carousel is %+.1f standard errors from it (printed, not gated)" % (p.mean(), gap(c, p)))
    assert gap(c, b) > 5
