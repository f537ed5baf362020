"""The exact argument-error text of one entry point per translation unit of librein48.so, without a
GPU: each call below is refused by the checks at the top of its entry point, so it returns R48_EINVAL
with r48_last_error set before any HIP call, and no stand-in pointer is dereferenced.

The expected strings were recorded from a build of the commit before the host-side helpers (fail,
launched, grid_for, the alignment checks, DeviceGuard) moved into r48_host.h, not from the code they
now test: the move must leave every message byte for byte as it was."""
import ctypes as C

import pytest

from rein48_amd import _lib

P = C.c_void_p(0x1000)     # a non-NULL, 16-byte aligned stand-in: never dereferenced on these paths
ODD = C.c_void_p(0x1008)   # 8-byte but not 16-byte aligned
ODD4 = C.c_void_p(0x1004)  # not 8-byte aligned
HANDLE = C.c_void_p()      # a real out-parameter for the _create calls (they clear it first)

# translation unit -> (entry point, arguments, the message of the parent commit)
CASES = {
    "r48_env": ("r48_env_create", (C.byref(HANDLE), 0, 0, 1, 0), b"n_boards out of range"),
    "r48_a3c": ("r48_sample_actions", (ODD, 4, 1, 0, 0, P, None, None, None), b"logits must be 16-byte aligned"),
    "r48_policy": ("r48_cnn_rollout", (None, 4, 2, P, P, 0, P, P, P, None, None, None, 1, 0, 0, 1, 0, 0, None),
                   b"r48_cnn_rollout: NULL argument, n/gid0 < 0, n_steps < 1, bad mode or flags"),
    "r48_replay": ("r48_replay_create", (None, 0, 16, 0, 1), b"out NULL, capacity < 1 or unknown mode"),
    "r48_dqn": ("r48_adam", (P, P, P, ODD, 8, 1e-3, 0.9, 0.999, 1e-8, 1, None),
                b"r48_adam: NULL argument, n < 1, n not a multiple of 4, step < 1 or a buffer not 16-byte aligned"),
    "r48_resnet": ("r48_resnet_pack", (None, 1e-5, P, None), b"r48_resnet_pack: NULL or misaligned argument"),
    "r48_a3c_train": ("r48_cnn_train_grad", (None, 4, 2, P, P, P, None, None, 0.01, 0, P, P, P, P, None),
                      b"NULL argument, rows/n_boards < 1, bad mode, or cm without counts"),
    "r48_bn": ("r48_bn_apply", (ODD, None, 4, 64, P, 0, P, None, None), b"r48_bn: activations must be 16-byte aligned"),
    "r48_conv": ("r48_q_head_backward", (P, P, 4, P, P, P, ODD, None),
                 b"r48_q_head_backward: all pointers must be 16-byte aligned"),
    "r48_game": ("r48_game_step1", (P, 5, P, None), b"board/out NULL or action outside 0..3"),
    "r48_mlp": ("r48_mlp_policy_forward", (P, 4, P, 0, ODD, None, None, 1, 0, 0, None),
                b"r48_mlp_policy_forward: boards, w and logits must be 16-byte aligned"),
    "r48_mlp_train": ("r48_mlp_train_grad_seg", (P, 4, 2, P, P, P, None, 0.01, 0, P, P, ODD, None),
                      b"r48_mlp_train_grad_seg: boards, w, seg, counts, workspace and grad must be 16-byte aligned"),
    "r48_moves": ("r48_boards_legal", (ODD, 4, P, None),
                  b"r48_boards_legal: boards/legal NULL, boards not 16-byte aligned or n < 0"),
    "r48_ntuple": ("r48_ntuple_carousel", (P, 4, P, P, 1, P, P, P, P, ODD4, 1, 0, 0, None),
                   b"r48_ntuple_carousel: starts is not 8-byte aligned"),
}


@pytest.mark.parametrize("unit", sorted(CASES))
def test_argument_error_message_is_unchanged(unit):
    lib = _lib.load()
    name, args, want = CASES[unit]
    assert getattr(lib, name)(*args) == _lib.R48_EINVAL, (name, args)
    assert lib.r48_last_error() == want
