// r48_moves.hip -- legal-move masks, afterstates and the legal-move masked forms of the action
// selection / TD target kernels, behind include/rein48.h. Stateless: plain device pointers, so
// they serve env boards and replay samples alike.
//
//   k_legal        board -> 4-bit set of the moves that change it (r48::legal_mask, a closed form)
//   k_afterstates  board -> the four moved boards, action-major [4][n][16] (each plane a boards
//                  array; every store instruction writes consecutive 16 B across the wave), and
//                  optionally the merge rewards [4][n] and the legal set
//   k_sample_m / k_egreedy_m / k_td_target_m
//                  k_sample / k_egreedy / k_td_target (r48_select.h: the same device code) with
//                  the legal set of the row's board computed in registers -- no mask plane is
//                  written to HBM and read back on the training path
// One board per lane, one 16-byte board load; all memory-bound.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rein48.h"
#include "r48_board.h"
#include "r48_host.h"
#include "r48_select.h"

using r48::aligned16;
using r48::fail;
using r48::grid_for;
using r48::launched;

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_legal(const int8_t *__restrict__ boards, int64_t n,
                                                  uint8_t *__restrict__ legal)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    legal[i] = (uint8_t)r48::legal_mask(r48::load_board(boards, i));
}

__device__ __forceinline__ void store_board(int8_t *__restrict__ plane, int64_t i, const r48::Board &b)
{
    *reinterpret_cast<uint4 *>(plane + 16 * i) = make_uint4(b.w0, b.w1, b.w2, b.w3);
}

// The legal set falls out of the moved boards (moved != input), which keeps it consistent with
// the planes by construction; r48::legal_mask is the closed form of the same predicate.
template <bool REWARD>
__global__ __launch_bounds__(kBlock) void k_afterstates(const int8_t *__restrict__ boards, int64_t n,
                                                        int8_t *__restrict__ after, int32_t *__restrict__ reward,
                                                        uint8_t *__restrict__ legal)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::Board b = r48::load_board(boards, i);
    const r48::Moves4 m = r48::move_rows4<REWARD>(b);
    const int64_t plane = 16 * n;
    store_board(after, i, m.up);
    store_board(after + plane, i, m.down);
    store_board(after + 2 * plane, i, m.left);
    store_board(after + 3 * plane, i, m.right);
    if (REWARD) {
        reward[i] = (int32_t)m.r_up;
        reward[n + i] = (int32_t)m.r_down;
        reward[2 * n + i] = (int32_t)m.r_left;
        reward[3 * n + i] = (int32_t)m.r_right;
    }
    if (legal)
        legal[i] = (uint8_t)((r48::differs(m.up, b) ? 1u : 0u) | (r48::differs(m.down, b) ? 2u : 0u) |
                             (r48::differs(m.left, b) ? 4u : 0u) | (r48::differs(m.right, b) ? 8u : 0u));
}

__global__ __launch_bounds__(kBlock) void k_sample_m(const float *__restrict__ logits,
                                                     const int8_t *__restrict__ boards, int64_t n, int64_t gid0,
                                                     uint32_t k0, uint32_t k1, uint32_t ctr,
                                                     int8_t *__restrict__ actions, float *__restrict__ logp,
                                                     float *__restrict__ entropy)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t legal = r48::legal_or_all(r48::load_board(boards, i));
    r48::sample_row<true>(logits, i, legal, gid0, k0, k1, ctr, actions, logp, entropy);
}

__global__ __launch_bounds__(kBlock) void k_egreedy_m(const float *__restrict__ q, const int8_t *__restrict__ boards,
                                                      int64_t n, float eps, uint32_t k0, uint32_t k1, int64_t gid0,
                                                      uint32_t ctr, int8_t *__restrict__ actions)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t legal = r48::legal_or_all(r48::load_board(boards, i));
    r48::egreedy_row<true>(q, i, legal, eps, k0, k1, gid0, ctr, actions);
}

template <bool DOUBLE, bool LOG2>
__global__ __launch_bounds__(kBlock) void k_td_target_m(const float *__restrict__ reward,
                                                        const uint8_t *__restrict__ done,
                                                        const float *__restrict__ q_next_target,
                                                        const float *__restrict__ q_next_online,
                                                        const int8_t *__restrict__ next_boards, int64_t n,
                                                        float gamma, float *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t legal = r48::legal_mask(r48::load_board(next_boards, i));
    r48::td_row<DOUBLE, LOG2, true>(reward, done, q_next_target, q_next_online, i, legal ? legal : 15u, legal == 0u,
                                    gamma, y);
}

}  // namespace

extern "C" {

int r48_boards_legal(const int8_t *boards, int64_t n, uint8_t *legal, void *stream)
{
    if (!boards || !legal || n < 0 || !aligned16(boards))
        return fail(R48_EINVAL, "r48_boards_legal: boards/legal NULL, boards not 16-byte aligned or n < 0");
    if (n == 0)
        return R48_OK;
    hipLaunchKernelGGL(k_legal, grid_for(n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, boards, n, legal);
    return launched("k_legal");
}

int r48_boards_afterstates(const int8_t *boards, int64_t n, int8_t *after, int32_t *reward, uint8_t *legal,
                           void *stream)
{
    if (!boards || !after || n < 0 || !aligned16(boards) || !aligned16(after))
        return fail(R48_EINVAL, "r48_boards_afterstates: boards/after NULL or not 16-byte aligned, or n < 0");
    if (n == 0)
        return R48_OK;
    if (reward)
        hipLaunchKernelGGL(k_afterstates<true>, grid_for(n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, boards, n, after,
                           reward, legal);
    else
        hipLaunchKernelGGL(k_afterstates<false>, grid_for(n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, boards, n, after,
                           nullptr, legal);
    return launched("k_afterstates");
}

int r48_sample_actions_masked(const float *logits, const int8_t *boards, int64_t n, uint64_t seed, int64_t gid0,
                              uint32_t ctr, int8_t *actions, float *logp, float *entropy, void *stream)
{
    if (!logits || !boards || !actions || n < 0 || gid0 < 0 || !aligned16(logits) || !aligned16(boards))
        return fail(R48_EINVAL, "r48_sample_actions_masked: logits/boards/actions NULL or not 16-byte aligned, or "
                                "n/gid0 < 0");
    if (n == 0)
        return R48_OK;
    hipLaunchKernelGGL(k_sample_m, grid_for(n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, logits, boards, n, gid0,
                       (uint32_t)seed, (uint32_t)(seed >> 32), ctr, actions, logp, entropy);
    return launched("k_sample_m");
}

int r48_egreedy_actions_masked(const float *q, const int8_t *boards, int64_t n, float eps, uint64_t seed,
                               int64_t gid0, uint32_t ctr, int8_t *actions, void *stream)
{
    if (!q || !boards || !actions || n < 0 || gid0 < 0 || !aligned16(q) || !aligned16(boards))
        return fail(R48_EINVAL, "r48_egreedy_actions_masked: q/boards/actions NULL or not 16-byte aligned, or "
                                "n/gid0 < 0");
    if (n == 0)
        return R48_OK;
    hipLaunchKernelGGL(k_egreedy_m, grid_for(n, kBlock), dim3(kBlock), 0, (hipStream_t)stream, q, boards, n, eps,
                       (uint32_t)seed, (uint32_t)(seed >> 32), gid0, ctr, actions);
    return launched("k_egreedy_m");
}

int r48_td_target_masked(const float *reward, const uint8_t *done, const float *q_next_target,
                         const float *q_next_online, const int8_t *next_boards, int64_t n, float gamma,
                         int32_t log2_reward, float *y, void *stream)
{
    if (!reward || !q_next_target || !next_boards || !y || n < 0 || !aligned16(q_next_target) ||
        (q_next_online && !aligned16(q_next_online)) || !aligned16(next_boards))
        return fail(R48_EINVAL, "r48_td_target_masked: reward/q_next_target/next_boards/y NULL, n < 0, or Q / "
                                "next_boards not 16-byte aligned");
    if (n == 0)
        return R48_OK;
    hipStream_t s = (hipStream_t)stream;
    if (q_next_online && log2_reward)
        hipLaunchKernelGGL((k_td_target_m<true, true>), grid_for(n, kBlock), dim3(kBlock), 0, s, reward, done, q_next_target,
                           q_next_online, next_boards, n, gamma, y);
    else if (q_next_online)
        hipLaunchKernelGGL((k_td_target_m<true, false>), grid_for(n, kBlock), dim3(kBlock), 0, s, reward, done, q_next_target,
                           q_next_online, next_boards, n, gamma, y);
    else if (log2_reward)
        hipLaunchKernelGGL((k_td_target_m<false, true>), grid_for(n, kBlock), dim3(kBlock), 0, s, reward, done, q_next_target,
                           nullptr, next_boards, n, gamma, y);
    else
        hipLaunchKernelGGL((k_td_target_m<false, false>), grid_for(n, kBlock), dim3(kBlock), 0, s, reward, done,
                           q_next_target, nullptr, next_boards, n, gamma, y);
    return launched("k_td_target_m");
}

}  // extern "C"
