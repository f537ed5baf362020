"""N-tuple network on afterstates, trained by TD(0), optionally with temporal-coherence learning
rates (rein48_amd/csrc/r48_ntuple.hip).

The value of a board is a sum of lookup-table entries over `m` board patterns (tuples of `L`
cells) and their 8 symmetries: V(b) = sum_t sum_g tables[t][index(g . b, t)], index = sum_k
min(b[cell_k], 15) << 4k (DESIGN.md "N-tuple network"). It fills the `value` of
evaluate.afterstate_policy, fused: NTupleNet.act makes the four moves, evaluates the legal
afterstates and picks the best in one kernel.

The reference has no such learner (its value-based code is the unfinished DDPG); the method is the
TD-afterstate n-tuple network of Szubert & Jaskowski (CIG 2014) with its per-entry step
normalisation taken over the batch: every table entry moves by alpha / (8m) times the MEAN delta of
the boards that hit it, so one board alone moves V(s') by alpha * delta and 64 copies of it move it
by the same amount.

tc=True adds temporal-coherence (TC) learning rates (Beal & Smith; Jaskowski 2016): every entry keeps
the running sum E of the mean deltas it was updated with and the running sum A of their absolute
values, and its step is scaled by |E| / A -- 1 while its errors agree in sign, towards 0 once they
are noise. No step size is annealed by hand; alpha = 1.0 is the recommended setting with it.

stages=(c_1, ..., c_k) (1 to 3 strictly ascending exponents in 1..15) makes the net multi-stage with
lazy weight promotion (Jaskowski 2016): k + 1 copies of every table, and a board is evaluated in stage
#{j : its largest tile's exponent, clamped to 15, >= c_j} -- the stage of the afterstate being
evaluated. An entry of a higher stage that was never updated reads as the nearest lower stage's
current value (the update copies new values upwards until the first entry that has its own), so a
fresh stage does not read as 0, and its first update starts from there. Opt-in; stages=() is the
single-stage net, unchanged.

NTupleConfig.carousel=(c_1, ..., c_k) (cuts of the same form) turns on carousel shaping in the trainer
(Jaskowski 2016): episodes start in turn from every stage, from a remembered board with which a
recent episode entered it, so the late stages get as many episode starts as the first
(NTupleTrainer; the contract is in rein48_amd/csrc/r48_ntuple.h). Opt-in; carousel=() is off.

NTupleReplicaTrainer trains up to 64 independent unstaged nets -- seeds, or an alpha sweep -- in the
same three launches per step: each replica has its own tables, boards and alpha, and is bit for bit
the solo fused trainer on its boards (the contract is in r48_ntuple.h, "Replicas").
"""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import check, ptr
from .a3c.kernels import _dev, _stream
from .env import VecGame
from .moves import _boards, _out

LAYOUTS = {
    "4x6": ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10)),
    "lines-squares": ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 4, 5), (1, 2, 5, 6), (5, 6, 9, 10)),
}


# steps per launch of NTupleNet.play_episodes, by depth: a launch at 2^16 boards stays under 100 ms
# on an MI355X (DESIGN.md section 16 has the measured launch times)
PLAY_CHUNK = {1: 1000, 2: 100}

# board-steps per launch of play_ruled in play_episodes, by the rule's largest depth: a launch with
# every board alive stays under 100 ms on an MI355X (DESIGN.md "Whole games at a per-board depth"
# has the measured launch times: at 4,096 boards 25 ms, 29 ms, 74 ms from reset at depths 1, 2, 3 and
# 33 ms under depth_rule(16, 3), the costliest rule recorded, which depth 4 is sized for; a rule
# with depth 4 on roomier boards takes longer per step, in play_ruled as in search_ruled).
RULED_BUDGET = {1: 1 << 20, 2: 1 << 18, 3: 1 << 16, 4: 1 << 13}
# and the most steps per launch: with few boards a launch costs its steps times ONE board's step
# (~0.1 ms at depth 3: 1,024 steps of 64 boards measured 100 ms)
RULED_MAX_CHUNK = {1: 4096, 2: 1024, 3: 512, 4: 16}


def ruled_chunk(max_depth, n_boards):
    """Steps per launch of play_ruled in play_episodes: RULED_BUDGET[max_depth] board-steps over
    n_boards, at least 1 step and at most RULED_MAX_CHUNK[max_depth]."""
    d = int(max_depth)
    return max(1, min(RULED_BUDGET[d] // max(1, int(n_boards)), RULED_MAX_CHUNK[d]))


def layout_cells(layout):
    """A layout name or a sequence of equal-length cell tuples -> tuple of tuples of ints."""
    cells = LAYOUTS[layout] if isinstance(layout, str) else layout
    cells = tuple(tuple(int(c) for c in t) for t in cells)
    if not 1 <= len(cells) <= 8:
        raise ValueError("a layout has 1..8 tuples, got %d" % len(cells))
    L = len(cells[0])
    if not 2 <= L <= 6 or any(len(t) != L for t in cells):
        raise ValueError("the tuples of a layout have one length, 2..6 cells")
    for t in cells:
        if any(not 0 <= c < 16 for c in t) or len(set(t)) != L:
            raise ValueError("tuple %r: cells are distinct numbers 0..15" % (t,))
    return cells


# the outputs of act, td_act and the searches: (name, dtype, shape after [n])
_ACT_OUT = (("actions", torch.int8, ()), ("after", torch.int8, (16,)), ("value", torch.float32, ()),
            ("reward", torch.int32, ()), ("legal", torch.uint8, ()))
_TD_ACT_OUT = _ACT_OUT + (("valid", torch.uint8, ()), ("delta", torch.float32, ()))
_SEARCH_OUT = (("actions", torch.int8, ()), ("q", torch.float32, (4,)), ("legal", torch.uint8, ()))
_RULED_OUT = _SEARCH_OUT + (("depth", torch.uint8, ()),)


def _outs(spec, given, n, boards):
    """The output tensors of one call in the order of `spec`: the given ones checked, the rest allocated."""
    return tuple(_out(t, name, dtype, (n,) + tail, boards) for t, (name, dtype, tail) in zip(given, spec))


def stage_cuts(stages):
    """The cuts of a staged net as a tuple of ints: () or 1..3 strictly ascending exponents in 1..15."""
    cuts = tuple(int(c) for c in stages)
    if len(cuts) > 3:
        raise ValueError("a net has at most 3 cuts (4 stages), got %r" % (cuts,))
    if any(not 1 <= c <= 15 for c in cuts) or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError("cuts are strictly ascending exponents in 1..15, got %r" % (cuts,))
    return cuts


def _rule(rule):
    """A rule of search_ruled as a tuple of 17 ints, each 1..4."""
    rule = tuple(int(d) for d in rule)
    if len(rule) != 17:
        raise ValueError("a rule has 17 depths (blanks 0..16), got %d" % len(rule))
    if any(not 1 <= d <= 4 for d in rule):
        raise ValueError("a rule's depths are 1..4, got %r" % (rule,))
    return rule


class NTupleNet:
    """The tables float32 [m, 16^L] and the update's scratch (acc int64, cnt uint32 held as int32,
    same shape; zero between calls) on one GPU. With tc, also the error sums tc_e and tc_a of the
    temporal-coherence learning rates (float32, same shape, zero at the start: +512 MiB for "4x6").
    With stages (S - 1 cuts) every one of these is [S, m, 16^L] and `own` (uint8, same shape: own[0]
    all 1, the rest 0 at the start) records which entries of the higher stages have been updated;
    every method then goes through the library's _staged entry points."""

    def __init__(self, layout="4x6", device="cuda:0", tc=False, stages=()):
        self.cells = layout_cells(layout)
        self.m, self.L = len(self.cells), len(self.cells[0])
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("NTupleNet device must be a GPU, got %s" % self.device)
        flat = [c for t in self.cells for c in t]
        self._cells = (C.c_uint8 * len(flat))(*flat)
        self.cuts = stage_cuts(stages)
        self.S = len(self.cuts) + 1
        self._cuts = (C.c_uint8 * len(self.cuts))(*self.cuts)
        shape = (self.S, self.m, 16 ** self.L) if self.cuts else (self.m, 16 ** self.L)
        self.tables = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.acc = torch.zeros(shape, dtype=torch.int64, device=self.device)
        self.cnt = torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.tc = bool(tc)
        self.tc_e = torch.zeros(shape, dtype=torch.float32, device=self.device) if self.tc else None
        self.tc_a = torch.zeros(shape, dtype=torch.float32, device=self.device) if self.tc else None
        self.own = None
        if self.cuts:
            self.own = torch.zeros(shape, dtype=torch.uint8, device=self.device)
            self.own[0] = 1
        self._lib = _lib.load()

    @classmethod
    def _over(cls, layout, tables, acc, cnt, tc_e=None, tc_a=None):
        """An unstaged net over given tensors, each contiguous [m, 16^L] on one GPU (tc_e and tc_a
        both or neither): nothing is allocated, every method works on the caller's storage
        (NTupleReplicaTrainer.net)."""
        self = cls.__new__(cls)
        self.cells = layout_cells(layout)
        self.m, self.L = len(self.cells), len(self.cells[0])
        shape = (self.m, 16 ** self.L)
        for t, name, dtype in ((tables, "tables", torch.float32), (acc, "acc", torch.int64), (cnt, "cnt", torch.int32),
                               (tc_e, "tc_e", torch.float32), (tc_a, "tc_a", torch.float32)):
            if t is None and name in ("tc_e", "tc_a"):
                continue
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != tables.device:
                raise ValueError("%s must be a contiguous %s tensor %r on %s" % (name, dtype, shape, tables.device))
        if (tc_e is None) != (tc_a is None):
            raise ValueError("tc_e and tc_a come together")
        self.device = tables.device
        if self.device.type != "cuda":
            raise ValueError("NTupleNet device must be a GPU, got %s" % self.device)
        flat = [c for t in self.cells for c in t]
        self._cells = (C.c_uint8 * len(flat))(*flat)
        self.cuts, self.S, self._cuts, self.own = (), 1, (C.c_uint8 * 0)(), None
        self.tables, self.acc, self.cnt = tables, acc, cnt
        self.tc, self.tc_e, self.tc_a = tc_e is not None, tc_e, tc_a
        self._lib = _lib.load()
        return self

    def _fn(self, name):
        """The entry point `name`, or its _staged twin on a staged net."""
        return getattr(self._lib, name + "_staged" if self.cuts else name)

    def _lay(self):
        """What every entry point takes from cells on: (cells, m, L), and the cuts on a staged net."""
        if self.cuts:
            return self._cells, self.m, self.L, self._cuts, len(self.cuts)
        return self._cells, self.m, self.L

    def _own(self):
        """The trailing own argument of the updating entry points' staged twins."""
        return (ptr(self.own),) if self.cuts else ()

    def stage(self, boards):
        """uint8 [n]: the stage each board is evaluated in (0 on an unstaged net)."""
        top = boards.reshape(-1, 16).clamp(max=15).max(dim=1).values
        out = torch.zeros(top.shape, dtype=torch.uint8, device=boards.device)
        for c in self.cuts:
            out += (top >= c).to(torch.uint8)
        return out

    def value(self, boards, out=None):
        """float32 [n]: V of int8 boards [..., 16]."""
        n = _boards(boards)
        out = _out(out, "out", torch.float32, (n,), boards)
        check(self._fn("r48_ntuple_value")(ptr(boards), n, *self._lay(), ptr(self.tables), ptr(out), _stream(boards)))
        return out

    def act(self, boards, actions=None, after=None, value=None, reward=None, legal=None):
        """The one-ply afterstate search -> (actions int8 [n], after int8 [n, 16], value float32 [n],
        reward int32 [n], legal uint8 [n]) of the chosen move: argmax over the legal moves of
        reward + V(afterstate), ties to the lowest code. No legal move: action 0, the board itself,
        value 0, reward 0, legal 0."""
        n = _boards(boards)
        outs = _outs(_ACT_OUT, (actions, after, value, reward, legal), n, boards)
        check(self._fn("r48_ntuple_act")(ptr(boards), n, *self._lay(), ptr(self.tables), *map(ptr, outs), _stream(boards)))
        return outs

    def td_act(self, boards, prev_after, prev_value, prev_done, prev_valid, actions=None, after=None, value=None,
               reward=None, legal=None, valid=None, delta=None):
        """act on `boards` and, in the same kernel, the accumulate half of the TD update for the
        previous step's afterstates -> (actions, after, value, reward, legal) as act returns them,
        valid uint8 [n] = legal != 0, and delta float32 [n] = (0 where prev_done else reward +
        value) - prev_value for every board. Boards with prev_valid != 0 add delta over the hits of
        prev_after into the net's scratch; apply(prev_after, step, prev_valid) finishes the update.
        after / value / valid must not be the prev_ tensors: apply still reads those."""
        n = _boards(boards)
        if _boards(prev_after) != n:
            raise ValueError("prev_after must hold one afterstate per board (%d)" % n)
        for t, name, dtype in ((prev_value, "prev_value", torch.float32), (prev_done, "prev_done", torch.uint8),
                               (prev_valid, "prev_valid", torch.uint8)):
            if _dev(t, name, dtype).numel() != n:
                raise ValueError("%s must have one element per board (%d)" % (name, n))
        outs = _outs(_TD_ACT_OUT, (actions, after, value, reward, legal, valid, delta), n, boards)
        check(self._fn("r48_ntuple_td_act")(ptr(boards), n, *self._lay(), ptr(self.tables), ptr(prev_after),
                                          ptr(prev_value), ptr(prev_done), ptr(prev_valid), *map(ptr, outs),
                                          ptr(self.acc), ptr(self.cnt), *self._own(), _stream(boards)))
        return outs

    def accumulate(self, boards, delta, valid=None):
        """First half of td_update: per-entry hit counts and fixed-point delta sums into the scratch."""
        n = _boards(boards)
        _dev(delta, "delta", torch.float32)
        if delta.numel() != n or (valid is not None and _dev(valid, "valid", torch.uint8).numel() != n):
            raise ValueError("delta / valid must have one element per board (%d)" % n)
        check(self._fn("r48_ntuple_accumulate")(ptr(boards), n, ptr(delta), ptr(valid), *self._lay(), ptr(self.acc),
                                                      ptr(self.cnt), *self._own(), _stream(boards)))

    def apply(self, boards, step, valid=None):
        """Second half: every entry the boards hit moves by step * its mean delta (a TC net: times
        its rate |E| / A, and E, A take the mean delta in); scratch back to zero."""
        n = _boards(boards)
        if valid is not None and _dev(valid, "valid", torch.uint8).numel() != n:
            raise ValueError("valid must have one element per board (%d)" % n)
        if self.tc:
            check(self._fn("r48_ntuple_apply_tc")(ptr(boards), n, ptr(valid), *self._lay(), float(step),
                                                ptr(self.tables), ptr(self.tc_e), ptr(self.tc_a), ptr(self.acc),
                                                        ptr(self.cnt), *self._own(), _stream(boards)))
            return
        check(self._fn("r48_ntuple_apply")(ptr(boards), n, ptr(valid), *self._lay(), float(step), ptr(self.tables),
                                                 ptr(self.acc), ptr(self.cnt), *self._own(), _stream(boards)))

    def td_update(self, afterstates, delta, alpha, valid=None):
        """tables[e] += alpha / (8m) * mean over the valid boards hitting e of delta, for every entry
        hit (a TC net: times the entry's rate). Deterministic: integer atomics, then one plain update
        per entry."""
        self.accumulate(afterstates, delta, valid)
        self.apply(afterstates, alpha / (8.0 * self.m), valid)

    def tc_rate(self, boards, out=None):
        """float32 [n]: the mean TC learning rate |E| / A over each board's 8m hits (1 on a net
        without history) -- how settled the network is on these boards. TC nets only."""
        if not self.tc:
            raise ValueError("tc_rate needs a net built with tc=True")
        n = _boards(boards)
        out = _out(out, "out", torch.float32, (n,), boards)
        check(self._fn("r48_ntuple_tc_rate")(ptr(boards), n, *self._lay(), ptr(self.tc_e), ptr(self.tc_a), ptr(out),
                                           _stream(boards)))
        return out

    def search(self, boards, depth=2, actions=None, q=None, legal=None):
        """Expectimax over the afterstate values -> (actions int8 [n], q float32 [n, 4], legal uint8
        [n]). depth 1: q[a] = reward + V(afterstate), act's scores. depth 2: q[a] = reward + the mean
        over the tile spawns (every empty cell, a 2 with weight 0.9, a 4 with 0.1) of act's best
        score on the board after the spawn, 0 where that board has no move. Illegal moves have q =
        -inf; the action is the first maximiser, 0 where no move is legal. One board per wave."""
        if depth not in (1, 2):
            raise ValueError("search depth is 1 or 2, got %r (three plies: search3)" % (depth,))
        n = _boards(boards)
        outs = _outs(_SEARCH_OUT, (actions, q, legal), n, boards)
        check(self._fn("r48_ntuple_search")(ptr(boards), n, *self._lay(), ptr(self.tables), depth, *map(ptr, outs),
                                          _stream(boards)))
        return outs

    def search3(self, boards, actions=None, q=None, legal=None):
        """The 3-ply expectimax search -> (actions int8 [n], q float32 [n, 4], legal uint8 [n]):
        search's depth 2 with the leaf one level deeper. q[a] = reward + the mean over the tile
        spawns of the best depth-2 q on the board after the spawn, 0 where that board has no move.
        Illegal moves, the action and the summation order are search's; q is bitwise reproducible.
        One kernel, one board per workgroup: a depth-2 search of each of the board's 2 to 120
        children."""
        n = _boards(boards)
        outs = _outs(_SEARCH_OUT, (actions, q, legal), n, boards)
        check(self._fn("r48_ntuple_search3")(ptr(boards), n, *self._lay(), ptr(self.tables), *map(ptr, outs),
                                           _stream(boards)))
        return outs

    @staticmethod
    def depth_rule(d3, d4=-1, base=2):
        """A rule for search_ruled, a 17-tuple indexed by a board's number of blanks (0..16): 4
        where blanks <= d4, else 3 where blanks <= d3, else `base` (1..4). depth_rule(16) is three
        plies everywhere, depth_rule(-1) two; depth_rule(6, 2) searches boards with at most 2 blanks
        four plies deep, those with 3 to 6 blanks three, the roomier ones two."""
        base = int(base)
        if not 1 <= base <= 4:
            raise ValueError("base depth is 1..4, got %r" % (base,))
        return tuple(4 if k <= d4 else 3 if k <= d3 else base for k in range(17))

    def search_ruled(self, boards, rule, actions=None, q=None, legal=None, depth=None):
        """Expectimax at a depth chosen per board -> (actions int8 [n], q float32 [n, 4], legal
        uint8 [n], depth uint8 [n]). `rule` is 17 depths, each 1..4, indexed by the board's number
        of blanks (depth_rule builds the usual ones); board i is searched at depth[i] =
        rule[blanks(board i)] and gets exactly the actions, q and legal of search(depth 1 or 2),
        of search3 (3), or the same recursion one level deeper (4: a 3-ply search of each of the
        board's children, then the averaging step). depth is written for every board, one without
        a legal move included. One launch, one board per workgroup, bitwise reproducible.
        The rule is the cost guard: a 4-ply search of a roomy board costs about a hundred times
        its 3-ply search (a board with b blanks has about 2b children per move), so give depth 4
        to boards with few blanks only. Measured on an MI355X, 4,096 boards of running games,
        lines-squares / 4x6: three plies everywhere 1.7 / 1.9 ms a call;
        four plies on the boards with no blank (2 % of them) 2.0 / 2.2 ms, with at most 1 blank
        (10 %) 3.3 / 3.6 ms, at most 2 (25 %) 6.7 / 7.7 ms, at most 3 (45 %) 13 / 15 ms, at most
        4 (62 %) 21 / 23 ms. At 2^16 boards a launch stays under 100 ms up to depth_rule(16, 2)
        (58 / 74 ms) and not beyond (depth_rule(16, 3): 116 / 180 ms): give such rules smaller
        batches on a shared GPU."""
        rule = _rule(rule)
        n = _boards(boards)
        outs = _outs(_RULED_OUT, (actions, q, legal, depth), n, boards)
        check(self._fn("r48_ntuple_search_ruled")(ptr(boards), n, *self._lay(), ptr(self.tables), (C.c_uint8 * 17)(*rule),
                                                *map(ptr, outs), _stream(boards)))
        return outs

    def policy(self, depth=1, rule=None):
        """`policy(boards, t) -> actions` for evaluate.play_episodes: the fused greedy search (depth
        1, act), the 2-ply expectimax search (depth 2) or the 3-ply one (depth 3, search3). With a
        rule (search_ruled: 17 depths 1..4 by the board's blanks) it plays through search_ruled
        and `depth` is not used."""
        if rule is not None:
            rule = _rule(rule)

            def policy(boards, t):
                return self.search_ruled(boards.contiguous(), rule)[0]
            return policy
        if depth not in (1, 2, 3):
            raise ValueError("policy depth is 1, 2 or 3, got %r" % (depth,))
        if depth == 1:
            def policy(boards, t):
                return self.act(boards.contiguous())[0]
        elif depth == 2:
            def policy(boards, t):
                return self.search(boards.contiguous(), 2)[0]
        else:
            def policy(boards, t):
                return self.search3(boards.contiguous())[0]
        return policy

    def play(self, env, n_steps, depth=1, length=None, gain=None, done=None):
        """n_steps x (policy(depth), env.step) on env's boards in ONE launch, every board in registers
        throughout -> (boards, length int32 [n], gain int32 [n], done uint8 [n]). The boards, done
        and env.counters end exactly where n_steps calls of env.step(self.policy(depth)(...)) leave
        them (no auto-reset), bit for bit, so a following env.step draws the same spawns. length +=
        the steps that changed a board, gain += their merge rewards: pass the tensors of an earlier
        call and chunked calls add up (allocated zero where None). A board without a legal move is
        finished and costs nothing more; a wave stops once all its boards are. depth 1 or 2; play_ruled
        plays at depth 3 and under a rule."""
        if depth not in (1, 2):
            raise ValueError("play depth is 1 or 2, got %r (three plies and rules: play_ruled)" % (depth,))
        boards = env.boards
        if boards.device != self.device:
            raise ValueError("the env is on %s, the net on %s" % (boards.device, self.device))
        n = _boards(boards)
        n_steps = int(n_steps)
        length, gain, done = self._play_outs(n, boards, length, gain, done)
        step, reset = env.counters
        check(self._fn("r48_ntuple_play")(ptr(boards), n, *self._lay(), ptr(self.tables), depth, n_steps, env.seed,
                                        env.board_offset, step, ptr(length), ptr(gain), ptr(done), _stream(boards)))
        env.counters = ((step + n_steps) & 0xFFFFFFFF, reset)
        return boards, length, gain, done

    def play_ruled(self, env, n_steps, rule, length=None, gain=None, done=None):
        """n_steps x (policy(rule=rule), env.step) on env's boards in ONE launch -> (boards, length
        int32 [n], gain int32 [n], done uint8 [n]), play's tuple with play's meaning: every step
        searches a board at rule[its number of blanks] plies (1..4; depth_rule builds the usual
        rules, (3,) * 17 is three plies throughout), so the depth follows the game. The boards,
        done and env.counters end exactly where n_steps calls of env.step(self.search_ruled(boards,
        rule)[0]) leave them (no auto-reset), bit for bit; length and gain add up over chunked
        calls. One board per workgroup, which stays on it for all n_steps; a board without a legal
        move is finished and costs nothing more. search_ruled's cost guard applies to every step:
        keep depth 4 to boards with few blanks and n_steps small (play_episodes' chunks keep a
        launch under 100 ms)."""
        rule = _rule(rule)
        boards = env.boards
        if boards.device != self.device:
            raise ValueError("the env is on %s, the net on %s" % (boards.device, self.device))
        n = _boards(boards)
        n_steps = int(n_steps)
        length, gain, done = self._play_outs(n, boards, length, gain, done)
        step, reset = env.counters
        check(self._fn("r48_ntuple_play_ruled")(ptr(boards), n, *self._lay(), ptr(self.tables), (C.c_uint8 * 17)(*rule),
                                              n_steps, env.seed, env.board_offset, step, ptr(length), ptr(gain),
                                              ptr(done), _stream(boards)))
        env.counters = ((step + n_steps) & 0xFFFFFFFF, reset)
        return boards, length, gain, done

    def _play_outs(self, n, boards, length, gain, done):
        """play's in/out tensors: the given ones checked, zeros where None."""
        length = torch.zeros(n, dtype=torch.int32, device=self.device) if length is None else length
        gain = torch.zeros(n, dtype=torch.int32, device=self.device) if gain is None else gain
        length, gain = _out(length, "length", torch.int32, (n,), boards), _out(gain, "gain", torch.int32, (n,), boards)
        done = torch.zeros(n, dtype=torch.uint8, device=self.device) if done is None else done
        return length, gain, _out(done, "done", torch.uint8, (n,), boards)      # n_steps == 0 leaves done as it is

    @torch.no_grad()
    def play_episodes(self, n_boards, seed=0, depth=1, max_steps=20_000, chunk=None, return_scores=False, rule=None):
        """evaluate.play_episodes(self.policy(depth, rule), n_boards, seed=seed, ...) through play and
        play_ruled: the same dict, every value equal to the last bit except steps_run, which is a
        multiple of chunk, plus mean_gain (the mean sum of merge rewards). The boards are played in
        launches of `chunk` steps with one host check of done in between. Depths 1 and 2 go through
        play (default chunk PLAY_CHUNK[depth]); depth 3 and a rule (17 depths 1..4 by the board's
        blanks; `depth` is then not used) through play_ruled, depth 3 as the rule (3,) * 17, with
        the default chunk ruled_chunk(the rule's largest depth, n_boards)."""
        if rule is None and depth not in (1, 2, 3):
            raise ValueError("play_episodes depth is 1, 2 or 3, got %r" % (depth,))
        if rule is None and depth == 3:
            rule = (3,) * 17
        if rule is not None:
            rule = _rule(rule)
            default = ruled_chunk(max(rule), n_boards)
        else:
            default = PLAY_CHUNK[depth]
        chunk = default if chunk is None else int(chunk)
        if chunk <= 0:
            raise ValueError("chunk must be positive, got %r" % (chunk,))
        env = VecGame(n_boards, device=self.device, seed=seed)
        env.reset()
        length = torch.zeros(n_boards, dtype=torch.int32, device=self.device)
        gain = torch.zeros(n_boards, dtype=torch.int32, device=self.device)
        done = torch.zeros(n_boards, dtype=torch.uint8, device=self.device)
        t = 0
        while t < max_steps:
            k = min(chunk, max_steps - t)
            if rule is not None:
                self.play_ruled(env, k, rule, length, gain, done)
            else:
                self.play(env, k, depth, length, gain, done)
            t += k
            if bool((done != 0).all()):
                break
        score = env.score().double()
        top = env.boards.max(dim=1).values.long()
        hist = torch.bincount(top, minlength=18).double() / n_boards
        out = {"boards": n_boards, "mean_score": float(score.mean()), "max_score": float(score.max()),
               "mean_length": float(length.double().mean()), "finished": float((done != 0).double().mean()),
               "steps_run": t, "max_tile_exponent_hist": {int(e): float(f) for e, f in enumerate(hist) if f > 0},
               "mean_gain": float(gain.double().mean())}
        if return_scores:
            out["scores"] = score.cpu()
        return out

    def state_dict(self):
        st = {"cells": [list(t) for t in self.cells], "tables": self.tables.detach().to("cpu", copy=True)}
        if self.cuts:
            st.update(stages=list(self.cuts), own=self.own.detach().to("cpu", copy=True))
        if self.tc:
            st.update(tc_e=self.tc_e.detach().to("cpu", copy=True), tc_a=self.tc_a.detach().to("cpu", copy=True))
        return st

    def load_state_dict(self, st):
        if [list(t) for t in self.cells] != [list(t) for t in st["cells"]]:
            raise ValueError("NTupleNet: the layout is %r, the saved one %r" % (self.cells, st["cells"]))
        if self.cuts != tuple(st.get("stages", ())):   # a state without the key is an unstaged net's
            raise ValueError("NTupleNet: the stages are %r, the saved ones %r" % (self.cuts, tuple(st.get("stages", ()))))
        if self.tc and not ("tc_e" in st and "tc_a" in st):
            raise ValueError("NTupleNet: a tc=True net needs the saved tc_e / tc_a, the state has none")
        self.tables.copy_(st["tables"].to(self.device))
        if self.cuts:
            self.own.copy_(st["own"].to(self.device))
        if self.tc:
            self.tc_e.copy_(st["tc_e"].to(self.device))
            self.tc_a.copy_(st["tc_a"].to(self.device))

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))


@dataclass
class NTupleConfig:
    n_boards: int = 4096
    layout: object = "4x6"           # a name in LAYOUTS or a sequence of cell tuples
    alpha: float = 0.25
    seed: int = 0
    tc: bool = False                 # temporal-coherence learning rates; alpha = 1.0 is recommended with it
    fused: bool = False              # train_step in three launches (td_act, apply, env.step): the same bits
    stages: tuple = ()               # cuts of a multi-stage net with weight promotion: () or 1..3 ascending exponents in 1..15
    carousel: tuple = ()             # cuts of carousel shaping (episode starts in turn from every stage): () is off


class NTupleTrainer:
    """Board-synchronous TD(0) on afterstates, one env step of every board per train_step():
      1. act on the env boards: a_t, the afterstate s'_t, v_t = V(s'_t), the merge reward r_t
      2. boards with a previous afterstate: target = 0 if the previous step ended the episode, else
         r_t + v_t; delta = target - v_{t-1}, where v_{t-1} is the value act returned one step ago
         (one batch update old); td_update(s'_{t-1}, delta, alpha, valid)
      3. env.step(a_t, auto_reset=True); s'_t, v_t, done become the "previous"
    cfg.tc: the update scales every entry's step by its temporal-coherence rate (NTupleNet).
    cfg.fused: steps 1 and 2 up to the sums run in one kernel (NTupleNet.td_act), apply and the env
    step follow, and the "previous" buffers are swapped by reference: three launches and no torch
    kernel instead of about fourteen, the same bits in every tensor, so a checkpoint moves freely
    between the two paths.
    cfg.carousel: carousel shaping (Jaskowski 2016). The cuts split a game into stages by the env
    board's largest tile, as a staged net's cuts do (they need not be the net's, and the net may be
    unstaged). Every board slot remembers the board with which its game last entered each stage, and
    an episode that ends restarts in turn from stage 0 (the env's fresh board), 1, ..., S - 1, from
    the remembered entry board of a slot drawn by Philox -- or from the fresh board where that slot
    has none yet. One call (two launches) after the env step, in both paths; the TD chain is as it
    was: the step after a restart takes target 0 for the ended episode's last afterstate. Off, the
    trainer allocates and calls nothing more.
    No exploration: the spawns randomise. Single GPU (an all-reduce of the table updates is not
    built)."""

    def __init__(self, cfg: NTupleConfig, device="cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        self.rank = 0
        n = cfg.n_boards
        self.net = NTupleNet(cfg.layout, self.device, tc=cfg.tc, stages=cfg.stages)
        self.env = VecGame(n, device=self.device, seed=cfg.seed)
        self.device = self.env.device
        self.env.reset()
        d = self.device
        self.actions = torch.zeros(n, dtype=torch.int8, device=d)
        self.reward = torch.zeros(n, dtype=torch.int32, device=d)
        self.legal = torch.zeros(n, dtype=torch.uint8, device=d)
        # this step's outputs and the previous step's, swapped every step
        self.after, self.prev_after = (torch.zeros((n, 16), dtype=torch.int8, device=d) for _ in range(2))
        self.value, self.prev_value = (torch.zeros(n, dtype=torch.float32, device=d) for _ in range(2))
        self.prev_done = torch.zeros(n, dtype=torch.uint8, device=d)
        # 0/1; the first step has no previous afterstate. `valid` is the fused step's output, swapped with it
        self.valid, self.prev_valid = (torch.zeros(n, dtype=torch.uint8, device=d) for _ in range(2))
        self.delta = torch.zeros(n, dtype=torch.float32, device=d)
        self.updates = 0
        # carousel shaping: the entry boards per stage and slot, and where each slot's episode stands
        self.carousel = stage_cuts(cfg.carousel)
        if self.carousel:
            S = len(self.carousel) + 1
            self._carousel = (C.c_uint8 * len(self.carousel))(*self.carousel)
            self.pool = torch.zeros((S - 1, n, 16), dtype=torch.int8, device=d)
            self.pool_has = torch.zeros((S - 1, n), dtype=torch.uint8, device=d)
            self.seen, self.turn = (torch.zeros(n, dtype=torch.uint8, device=d) for _ in range(2))
            self.starts = torch.zeros(S, dtype=torch.int64, device=d)   # the library's uint64 words

    # the carousel's tensors, as a checkpoint carries them
    CAROUSEL_STATE = ("pool", "pool_has", "seen", "turn", "starts")

    def _carousel_step(self, done):
        """The carousel call after an env step with auto-reset: restarts where done, records elsewhere."""
        env = self.env
        check(self.net._lib.r48_ntuple_carousel(ptr(env.boards), env.n, ptr(done), self._carousel, len(self.carousel),
                                                ptr(self.pool), ptr(self.pool_has), ptr(self.seen), ptr(self.turn),
                                                ptr(self.starts), env.seed, env.board_offset,
                                                self.updates & 0xFFFFFFFF, _stream(env.boards)))

    def carousel_stats(self):
        """{"starts": episode starts per stage since the trainer was built (or since the checkpoint's
        trainer was), "filled": per stage the share of board slots whose pool slot holds an entry
        board -- 1.0 for stage 0, which starts from the env's fresh board}."""
        if not self.carousel:
            raise ValueError("carousel_stats needs a trainer built with cfg.carousel")
        return {"starts": [int(x) for x in self.starts.tolist()],
                "filled": [1.0] + [float(x) for x in self.pool_has.float().mean(dim=1).tolist()]}

    @torch.no_grad()
    def train_step(self):
        net, env = self.net, self.env
        if self.cfg.fused:
            net.td_act(env.boards, self.prev_after, self.prev_value, self.prev_done, self.prev_valid, self.actions,
                       self.after, self.value, self.reward, self.legal, self.valid, self.delta)
            net.apply(self.prev_after, self.cfg.alpha / (8.0 * net.m), self.prev_valid)
            env.step(self.actions, auto_reset=True, done_out=self.prev_done)
            self.valid, self.prev_valid = self.prev_valid, self.valid
        else:
            net.act(env.boards, self.actions, self.after, self.value, self.reward, self.legal)
            target = torch.where(self.prev_done != 0, torch.zeros_like(self.value), self.reward.float() + self.value)
            torch.sub(target, self.prev_value, out=self.delta)
            net.td_update(self.prev_after, self.delta, self.cfg.alpha, self.prev_valid)
            _, _, done = env.step(self.actions, auto_reset=True)
            self.prev_done.copy_(done)
            self.prev_valid.copy_(self.legal != 0)   # an afterstate exists where a move did
        if self.carousel:
            self._carousel_step(self.prev_done)
        # this step's afterstates and values become the previous ones
        self.after, self.prev_after = self.prev_after, self.after
        self.value, self.prev_value = self.prev_value, self.value
        self.updates += 1

    def train_steps(self, k):
        """k train_step()s in one Python call."""
        for _ in range(int(k)):
            self.train_step()

    def policy(self, depth=1, rule=None):
        return self.net.policy(depth, rule)


MAX_REPLICAS = 64


def replica_steps(replicas, alphas, alpha, m):
    """The per-replica steps of NTupleReplicaTrainer as a list of `replicas` Python floats, each a
    float32 value: alpha_r / (8m) rounded as c_float(alpha / (8.0 * m)) rounds the solo trainer's
    step. `replicas` is 1..64; `alphas` is None (`alpha` everywhere) or `replicas` finite numbers.
    Needs no GPU."""
    if isinstance(replicas, bool) or int(replicas) != replicas:
        raise ValueError("replicas is a whole number, got %r" % (replicas,))
    replicas = int(replicas)
    if not 1 <= replicas <= MAX_REPLICAS:
        raise ValueError("replicas is 1..%d, got %d" % (MAX_REPLICAS, replicas))
    m = int(m)
    if not 1 <= m <= 8:
        raise ValueError("a layout has 1..8 tuples, got %d" % m)
    if alphas is None:
        alphas = (alpha,) * replicas
    alphas = tuple(float(a) for a in alphas)
    if len(alphas) != replicas:
        raise ValueError("alphas holds one alpha per replica (%d), got %d" % (replicas, len(alphas)))
    if any(a != a or a in (float("inf"), float("-inf")) for a in alphas):
        raise ValueError("alphas are finite numbers, got %r" % (alphas,))
    return [C.c_float(a / (8.0 * m)).value for a in alphas]


class NTupleReplicaTrainer:
    """`replicas` independent unstaged n-tuple nets trained in the same three launches per step
    (the contract is in rein48_amd/csrc/r48_ntuple.h, "Replicas"): cfg.n_boards boards PER REPLICA
    in one VecGame of replicas * cfg.n_boards boards with seed cfg.seed, replica r playing the
    global board ids r * n_boards .. -- its own games, which is its independent "seed" -- on its own
    tables [replicas, m, 16^L] and, with `alphas`, its own alpha (None: cfg.alpha everywhere).
    train_step() is NTupleTrainer's fused step: td_act_replicas, apply_replicas (cfg.tc:
    apply_tc_replicas), env.step with auto-reset, the "previous" buffers swapped by reference. Replica
    r's slices hold the bits a solo NTupleTrainer(fused=True) with alpha_r on VecGame(n_boards,
    seed, board_offset=r * n_boards) holds after the same number of steps. cfg.fused is not
    consulted; cfg.stages and cfg.carousel are refused (replicas of staged nets are not built, and
    the carousel's donor draw ranges over the whole batch and would mix replicas). net(r) is replica
    r as an NTupleNet over views. Single GPU."""

    def __init__(self, cfg: NTupleConfig, replicas, alphas=None, device="cuda:0"):
        if tuple(cfg.stages):
            raise ValueError("NTupleReplicaTrainer: replicas of staged nets are not built (cfg.stages = %r)" % (cfg.stages,))
        if tuple(cfg.carousel):
            raise ValueError("NTupleReplicaTrainer: the carousel is not built for replicas (cfg.carousel = %r)"
                             % (cfg.carousel,))
        self.cfg = cfg
        self.cells = layout_cells(cfg.layout)
        self.m, self.L = len(self.cells), len(self.cells[0])
        self.step_values = replica_steps(replicas, alphas, cfg.alpha, self.m)
        self.replicas = R = len(self.step_values)
        if R * self.m * 16 ** self.L > 1 << 32:
            raise ValueError("%d replicas of %d tables of 16^%d entries exceed 2^32 entries" % (R, self.m, self.L))
        self.per = int(cfg.n_boards)
        if self.per < 1:
            raise ValueError("n_boards is at least 1 board per replica, got %d" % self.per)
        n = R * self.per
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("NTupleReplicaTrainer device must be a GPU, got %s" % self.device)
        self.rank = 0
        self.tc = bool(cfg.tc)
        self.env = VecGame(n, device=self.device, seed=cfg.seed)
        self.device = d = self.env.device
        self.env.reset()
        flat = [c for t in self.cells for c in t]
        self._cells = (C.c_uint8 * len(flat))(*flat)
        shape = (R, self.m, 16 ** self.L)
        self.tables = torch.zeros(shape, dtype=torch.float32, device=d)
        self.acc = torch.zeros(shape, dtype=torch.int64, device=d)
        self.cnt = torch.zeros(shape, dtype=torch.int32, device=d)
        self.tc_e = torch.zeros(shape, dtype=torch.float32, device=d) if self.tc else None
        self.tc_a = torch.zeros(shape, dtype=torch.float32, device=d) if self.tc else None
        self.steps = torch.tensor(self.step_values, dtype=torch.float32, device=d)   # exact: the values are float32's
        self.actions = torch.zeros(n, dtype=torch.int8, device=d)
        self.reward = torch.zeros(n, dtype=torch.int32, device=d)
        self.legal = torch.zeros(n, dtype=torch.uint8, device=d)
        self.after, self.prev_after = (torch.zeros((n, 16), dtype=torch.int8, device=d) for _ in range(2))
        self.value, self.prev_value = (torch.zeros(n, dtype=torch.float32, device=d) for _ in range(2))
        self.prev_done = torch.zeros(n, dtype=torch.uint8, device=d)
        self.valid, self.prev_valid = (torch.zeros(n, dtype=torch.uint8, device=d) for _ in range(2))
        self.delta = torch.zeros(n, dtype=torch.float32, device=d)
        self.updates = 0
        self._lib = _lib.load()

    def net(self, r):
        """Replica r as an NTupleNet whose tables, acc, cnt, tc_e and tc_a are views of the trainer's:
        nothing is allocated. value, act, the searches, play_episodes, save and state_dict work on it
        as on any unstaged net, and a solo NTupleNet.load reads what it saved."""
        r = int(r)
        if not 0 <= r < self.replicas:
            raise ValueError("replica %d of %d" % (r, self.replicas))
        return NTupleNet._over(self.cells, self.tables[r], self.acc[r], self.cnt[r],
                               self.tc_e[r] if self.tc else None, self.tc_a[r] if self.tc else None)

    def replica(self, t, r):
        """Replica r's rows of a per-board tensor of the trainer (env.boards, prev_after, ...)."""
        return t[r * self.per:(r + 1) * self.per]

    @torch.no_grad()
    def train_step(self):
        env, lib = self.env, self._lib
        n, s = env.n, _stream(env.boards)
        lay = (self._cells, self.m, self.L)
        check(lib.r48_ntuple_td_act_replicas(
            ptr(env.boards), n, self.replicas, *lay, ptr(self.tables), ptr(self.prev_after), ptr(self.prev_value),
            ptr(self.prev_done), ptr(self.prev_valid), ptr(self.actions), ptr(self.after), ptr(self.value),
            ptr(self.reward), ptr(self.legal), ptr(self.valid), ptr(self.delta), ptr(self.acc), ptr(self.cnt), s))
        if self.tc:
            check(lib.r48_ntuple_apply_tc_replicas(ptr(self.prev_after), n, self.replicas, ptr(self.prev_valid), *lay,
                                                   ptr(self.steps), ptr(self.tables), ptr(self.tc_e), ptr(self.tc_a),
                                                   ptr(self.acc), ptr(self.cnt), s))
        else:
            check(lib.r48_ntuple_apply_replicas(ptr(self.prev_after), n, self.replicas, ptr(self.prev_valid), *lay,
                                                ptr(self.steps), ptr(self.tables), ptr(self.acc), ptr(self.cnt), s))
        env.step(self.actions, auto_reset=True, done_out=self.prev_done)
        self.valid, self.prev_valid = self.prev_valid, self.valid
        self.after, self.prev_after = self.prev_after, self.after
        self.value, self.prev_value = self.prev_value, self.value
        self.updates += 1

    def train_steps(self, k):
        """k train_step()s in one Python call."""
        for _ in range(int(k)):
            self.train_step()

    def policy(self, r, depth=1, rule=None):
        return self.net(r).policy(depth, rule)
