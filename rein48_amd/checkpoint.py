"""Checkpoint / resume of the trainers (SURVEY.md section 5 lists it as optional: the reference keeps no
`tf.train.Saver` in algorithm/a3c/a3c.py, so there is no reference format to match).

A checkpoint is everything that decides the trainer's next step, so that training resumed from it
is bit-identical to training that never stopped (tests/test_checkpoint_gpu.py):
  A3CTrainer  the net (flat parameters), the TF1 RMSProp slots (ms, momentum), the env's boards and
              its Philox step / reset counters, the policy's sampling counter, the update count
  DQNTrainer  online and target nets (parameters, BN running statistics, num_batches_tracked),
              Adam's m, v and step, the env's boards and counters, the env-step count, the update
              count, and the HBM replay ring (its counters and, unless replay=False, its contents in
              slot order: 38 B per stored transition)
  NTupleTrainer  the tables (with cfg.tc also the error sums tc_e / tc_a, with cfg.stages also the cuts and the own flags), the env's boards and counters, the previous step's afterstates, values,
              done and valid flags, and the step count (the update is deterministic: integer
              atomics, one plain table update per entry); with cfg.carousel also its cuts and its
              five buffers (pool, pool_has, seen, turn, starts)
Draws are keyed by counters, not by RNG state in memory, so restoring the
counters restores every later draw.

One file per rank: each rank owns its boards and its replay shard, so pass a
per-rank path (e.g. "ckpt.rank%d.pt" % rank). Files are written with torch.save and read back with
torch.load(weights_only=True): plain tensors, numbers and strings, nothing executable.

load() also reads format-1 files (round 4: no draw contract or shard recorded; contract 3 is
assumed, with a warning). It refuses (ValueError) a file whose resume could not be bit-identical: another kind or format,
another draw contract (R48_DRAW_CONTRACT: the same counters would give other draws), another rank's
shard (its first global board id, which keys every Philox draw), or a configuration that differs in a
field that fixes buffer shapes, the draws (seed), the network's inputs (features) or numerics (bf16),
the loss (mode), or which actions are taken and bootstrapped (the DQN's mask_illegal). Hyper-parameters
such as lr, gamma or epsilon may differ (a deliberate change).
"""
import dataclasses
import warnings

import torch

from ._lib import DRAW_CONTRACT

FORMAT = 2

# configuration fields a checkpoint must agree on: buffer shapes, draws, inputs, numerics, loss
_MATCH_FIELDS = {
    "a3c": ("n_boards", "max_steps", "net", "seed", "mode", "features", "bf16"),
    "dqn": ("n_boards", "replay_capacity", "channels", "blocks", "bn", "bf16", "seed", "reward_transform",
            "mask_illegal"),
    "ntuple": ("n_boards", "seed", "tc"),   # and the layout's cells, compared as cells (a name or a list in cfg)
}


def _gid0(trainer, kind):
    """Global id of the trainer's first board (rank * n_boards): keys the Philox draws of its shard."""
    return int(trainer.gid0) if kind == "a3c" else int(trainer.rank) * int(trainer.cfg.n_boards)


def _cells(net):
    return [list(t) for t in net.cells]


def _kind(trainer):
    from .a3c.trainer import A3CTrainer
    from .dqn.trainer import DQNLearner
    from .ntuple import NTupleTrainer
    if isinstance(trainer, NTupleTrainer):
        return "ntuple"
    if isinstance(trainer, A3CTrainer):
        return "a3c"
    if isinstance(trainer, DQNLearner):
        return "dqn"
    raise TypeError("checkpoint: expected an A3CTrainer, a DQNLearner / DQNTrainer or an NTupleTrainer, got %r" % type(trainer))


def _cpu(t):
    return t.detach().to("cpu", copy=True)


def _cpu_state(module):
    return {k: _cpu(v) for k, v in module.state_dict().items()}


def _env_state(env):
    step, reset = env.counters
    return {"boards": _cpu(env.boards), "step_ctr": int(step), "reset_ctr": int(reset)}


def _load_env(env, st):
    if tuple(st["boards"].shape) != tuple(env.boards.shape):
        raise ValueError("checkpoint: env has %s boards, the file %s" % (tuple(env.boards.shape), tuple(st["boards"].shape)))
    env.boards.copy_(st["boards"].to(env.boards.device))
    env.counters = (st["step_ctr"], st["reset_ctr"])


def _replay_state(rep, contents):
    size, head, ctr = rep.counters
    st = {"size": int(size), "head": int(head), "sample_ctr": int(ctr), "mode": rep.mode, "capacity": rep.capacity}
    if contents and size:
        rows = rep.gather(torch.arange(size, dtype=torch.int64, device=rep.device))
        st["rows"] = {k: _cpu(rows[k]) for k in ("state", "action", "reward", "next_state", "done")}
    return st


def _load_replay(rep, st):
    if st["mode"] != rep.mode or st["capacity"] != rep.capacity:
        raise ValueError("checkpoint: replay is %s/%d, the file %s/%d" % (rep.mode, rep.capacity, st["mode"],
                                                                          st["capacity"]))
    rep.clear()
    rows = st.get("rows")
    if rows is not None:   # slot k <- row k (a cleared ring stores from slot 0), then the counters
        d = rep.device
        rep.store(rows["state"].to(d), rows["action"].to(d), rows["reward"].to(d), rows["next_state"].to(d),
                  rows["done"].to(d))
        rep.set_counters(st["size"], st["head"], st["sample_ctr"])
    else:                  # contents not saved: an empty ring that refills (no stale rows sampled)
        rep.set_counters(0, 0, st["sample_ctr"])


def save(trainer, path, replay=True):
    """Write `trainer`'s state to `path` (replay=False leaves the DQN ring's contents out: the
    resumed ring starts empty and refills from the env before it is sampled again, so that resume
    is not bit-identical to uninterrupted training)."""
    kind = _kind(trainer)
    if trainer.device.type == "cuda":
        torch.cuda.synchronize(trainer.device)
    st = {"format": FORMAT, "kind": kind, "cfg": dataclasses.asdict(trainer.cfg), "updates": int(trainer.updates),
          "draw_contract": DRAW_CONTRACT, "gid0": _gid0(trainer, kind)}
    if kind == "ntuple":
        cfg = dict(st["cfg"], layout=_cells(trainer.net))     # a layout given as tuples is saved as lists
        st.update(cfg=cfg, cells=_cells(trainer.net), tables=_cpu(trainer.net.tables), env=_env_state(trainer.env),
                  prev_after=_cpu(trainer.prev_after), prev_value=_cpu(trainer.prev_value),
                  prev_done=_cpu(trainer.prev_done), prev_valid=_cpu(trainer.prev_valid))
        if trainer.cfg.tc:
            st.update(tc_e=_cpu(trainer.net.tc_e), tc_a=_cpu(trainer.net.tc_a))
        if trainer.net.cuts:
            st.update(cfg=dict(cfg, stages=list(trainer.net.cuts)), stages=list(trainer.net.cuts), own=_cpu(trainer.net.own))
        if trainer.carousel:
            st.update(cfg=dict(st["cfg"], carousel=list(trainer.carousel)), carousel=list(trainer.carousel),
                      carousel_state={k: _cpu(getattr(trainer, k)) for k in trainer.CAROUSEL_STATE})
    elif kind == "a3c":
        st.update(net=_cpu_state(trainer.net), ms=_cpu(trainer.opt.ms), mom=_cpu(trainer.opt.mom),
                  env=_env_state(trainer.env), sample_ctr=int(trainer.sample_ctr))
    else:
        st.update(net=_cpu_state(trainer.net), target=_cpu_state(trainer.target), adam_m=_cpu(trainer.opt.m),
                  adam_v=_cpu(trainer.opt.v), adam_t=int(trainer.opt.t))
        if hasattr(trainer, "env"):
            st.update(env=_env_state(trainer.env), steps=int(trainer.steps),
                      replay=_replay_state(trainer.replay, replay))
    torch.save(st, path)


def load(trainer, path):
    """Restore a checkpoint written by save() into a trainer built with a matching configuration."""
    kind = _kind(trainer)
    st = torch.load(path, map_location="cpu", weights_only=True)
    if st.get("format") not in (1, FORMAT) or st.get("kind") != kind:
        raise ValueError("checkpoint: %s is a %s checkpoint of format %s, not a %s one of format %d"
                         % (path, st.get("kind"), st.get("format"), kind, FORMAT))
    if st["format"] == 1:
        # format 1 (round 4) predates the recorded draw contract and shard: contract 3 (Philox4x32-7
        # step draws, commit 66448e8) is assumed -- a file written by a library from before that
        # commit resumes under other env draws -- and the shard cannot be checked
        warnings.warn("checkpoint: %s is format 1: draw contract 3 assumed (files from before it resume "
                      "under other draws), its rank shard is not recorded (pass this rank's own file)" % path,
                      stacklevel=2)
        st = dict(st, draw_contract=3, gid0=_gid0(trainer, kind))
    if st["draw_contract"] != DRAW_CONTRACT:
        raise ValueError("checkpoint: %s was written under draw contract %d, this library draws under %d"
                         % (path, st["draw_contract"], DRAW_CONTRACT))
    if st["gid0"] != _gid0(trainer, kind):
        raise ValueError("checkpoint: %s holds the shard starting at board %d, this trainer's starts at %d "
                         "(another rank's file?)" % (path, st["gid0"], _gid0(trainer, kind)))
    cfg = dataclasses.asdict(trainer.cfg)
    # a field the file's configuration predates (mask_illegal) had its default when the file was written
    defaults = {f.name: f.default for f in dataclasses.fields(trainer.cfg)}
    for f in _MATCH_FIELDS[kind]:
        theirs = st["cfg"].get(f, defaults[f])
        if cfg[f] != theirs:
            raise ValueError("checkpoint: %s = %r in the trainer, %r in %s" % (f, cfg[f], theirs, path))
    if kind == "ntuple" and st["cells"] != _cells(trainer.net):
        raise ValueError("checkpoint: layout cells %r in the trainer, %r in %s" % (_cells(trainer.net), st["cells"], path))
    # the cuts of a staged net, compared as cuts like the cells; a file without the key is an unstaged trainer's
    if kind == "ntuple" and tuple(st.get("stages", ())) != trainer.net.cuts:
        raise ValueError("checkpoint: stages %r in the trainer, %r in %s" % (trainer.net.cuts, tuple(st.get("stages", ())), path))
    # the carousel's cuts likewise; a file without the key is a trainer's without carousel
    if kind == "ntuple" and tuple(st.get("carousel", ())) != trainer.carousel:
        raise ValueError("checkpoint: carousel %r in the trainer, %r in %s" % (trainer.carousel, tuple(st.get("carousel", ())), path))
    dev = trainer.device
    with torch.no_grad():
        if kind == "ntuple":
            for k in trainer.CAROUSEL_STATE if trainer.carousel else ():
                getattr(trainer, k).copy_(st["carousel_state"][k].to(dev))
            trainer.net.tables.copy_(st["tables"].to(dev))
            if trainer.net.cuts:
                trainer.net.own.copy_(st["own"].to(dev))
            if trainer.cfg.tc:
                trainer.net.tc_e.copy_(st["tc_e"].to(dev))
                trainer.net.tc_a.copy_(st["tc_a"].to(dev))
            _load_env(trainer.env, st["env"])
            for k in ("prev_after", "prev_value", "prev_done", "prev_valid"):
                getattr(trainer, k).copy_(st[k].to(dev))
        elif kind == "a3c":
            trainer.net.load_state_dict(st["net"])   # copies into the flat buffers' views
            trainer.opt.ms.copy_(st["ms"].to(dev))
            trainer.opt.mom.copy_(st["mom"].to(dev))
            _load_env(trainer.env, st["env"])
            trainer.sample_ctr = st["sample_ctr"]
            trainer._rollout_v = None            # the rollout's values belong to the old weights
            trainer._wepoch += 1                 # repack the kernels' weight images
            trainer._mask = None
        else:
            trainer.net.load_state_dict(st["net"])
            trainer.target.load_state_dict(st["target"])
            trainer.opt.m.copy_(st["adam_m"].to(dev))
            trainer.opt.v.copy_(st["adam_v"].to(dev))
            trainer.opt.t = st["adam_t"]
            trainer._version += 1                # repack the fused-kernel weights of both nets
            if hasattr(trainer, "env"):
                if "env" not in st:
                    raise ValueError("checkpoint: %s holds a learner without env / replay" % path)
                _load_env(trainer.env, st["env"])
                trainer.steps = st["steps"]
                _load_replay(trainer.replay, st["replay"])
    trainer.updates = st["updates"]
    return st["cfg"]
