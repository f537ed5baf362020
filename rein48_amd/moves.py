"""Legal-move masks and afterstates of int8 boards (rein48_amd/csrc/r48_moves.hip).

Game.step (nevertiree/Rein48 game/GameClient.py:40-51) spawns only when the move changed the
board, so an illegal move is a silent no-op; these two calls say which moves are legal and what
each would produce, for any boards array on the GPU (env boards, replay samples, one plane of an
earlier afterstates call). Action codes 0 UP, 1 DOWN, 2 LEFT, 3 RIGHT. An empty board has no
legal move.
"""
import torch

from . import _lib
from ._lib import check, ptr
from .a3c.kernels import _dev, _stream


def _boards(boards):
    _dev(boards, "boards", torch.int8)
    if boards.dim() < 1 or boards.shape[-1] != 16:
        raise ValueError("boards must be int8 [..., 16], got %s" % (tuple(boards.shape),))
    return boards.numel() // 16


def _out(t, name, dtype, shape, like):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    _dev(t, name, dtype)
    if t.device != like.device:
        raise ValueError("%s must be on %s, got %s" % (name, like.device, t.device))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def legal_actions(boards, out=None):
    """uint8 [n]: bit a is set iff action a changes board i (update_matrix's has_changed)."""
    n = _boards(boards)
    out = _out(out, "out", torch.uint8, (n,), boards)
    check(_lib.load().r48_boards_legal(ptr(boards), n, ptr(out), _stream(boards)))
    return out


def afterstates(boards, after=None, reward=None, legal=None, want_reward=True, want_legal=True):
    """All four moves of every board in one launch -> (after int8 [4, n, 16], reward int32 [4, n]
    or None, legal uint8 [n] or None). Action-major: after[a] is itself a boards array; an illegal
    move's plane holds the unchanged board and its reward is 0 (reward = merged tile values)."""
    n = _boards(boards)
    after = _out(after, "after", torch.int8, (4, n, 16), boards)
    if reward is not None or want_reward:
        reward = _out(reward, "reward", torch.int32, (4, n), boards)
    if legal is not None or want_legal:
        legal = _out(legal, "legal", torch.uint8, (n,), boards)
    check(_lib.load().r48_boards_afterstates(ptr(boards), n, ptr(after), ptr(reward), ptr(legal), _stream(boards)))
    return after, reward, legal
