// r48_select.h -- per-row action selection and TD target, shared by the unmasked kernels
// (k_sample in r48_a3c.hip, k_egreedy / k_td_target in r48_dqn.hip) and their legal-move masked
// forms (r48_moves.hip). One statement of the softmax, the argmax and the target: MASKED only
// turns an illegal action's logit / Q into -inf in front of the same arithmetic and repairs the
// two places where that alone could still name an illegal action, so on an all-legal board the
// masked result is the unmasked one bit for bit. `legal` is r48::legal_mask's 4-bit set; 0 (game
// over, or an empty board) counts as all-legal.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "r48_board.h"

namespace r48 {

constexpr uint32_t kSampleTag = 0xA3Cu;    // r48_sample_actions' draw tag
constexpr uint32_t kEgreedyTag = 0xD0Eu;   // r48_egreedy_actions' draw tag

__device__ __forceinline__ Board load_board(const int8_t *__restrict__ boards, int64_t i)
{
    const uint4 v = *reinterpret_cast<const uint4 *>(boards + 16 * i);
    return Board{v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ uint32_t legal_or_all(const Board &b)
{
    const uint32_t l = legal_mask(b);
    return l ? l : 15u;
}

template <bool MASKED>
__device__ __forceinline__ float4 mask_rows(float4 v, uint32_t legal)
{
    if (MASKED) {
        v.x = (legal & 1u) ? v.x : -INFINITY;
        v.y = (legal & 2u) ? v.y : -INFINITY;
        v.z = (legal & 4u) ? v.z : -INFINITY;
        v.w = (legal & 8u) ? v.w : -INFINITY;
    }
    return v;
}

// highest / lowest legal action code, legal in 1..15
__device__ __forceinline__ uint32_t last_legal(uint32_t legal) { return 31u - (uint32_t)__clz((int)legal); }
__device__ __forceinline__ uint32_t first_legal(uint32_t legal) { return (uint32_t)__ffs((int)legal) - 1u; }

__device__ __forceinline__ float pick(float4 q, uint32_t a)
{
    return a == 0 ? q.x : a == 1 ? q.y : a == 2 ? q.z : q.w;
}

// first argmax (np.argmax's tie rule); MASKED: among the legal actions
template <bool MASKED>
__device__ __forceinline__ uint32_t argmax4(float4 q, uint32_t legal = 15u)
{
    q = mask_rows<MASKED>(q, legal);
    uint32_t a = 0;
    float m = q.x;
    if (q.y > m) { m = q.y; a = 1; }
    if (q.z > m) { m = q.z; a = 2; }
    if (q.w > m) { a = 3; }
    if (MASKED)   // no legal Q above -inf (or NaN): still a legal action
        a = ((legal >> a) & 1u) ? a : first_legal(legal);
    return a;
}

// softmax over 4 logits + inverse-CDF draw with a Philox uniform (24-bit, [0,1)); writes
// actions[i] and, where asked, log p[a] and the entropy term -sum p log(p + 1e-5)
template <bool MASKED>
__device__ __forceinline__ void sample_row(const float *__restrict__ logits, int64_t i, uint32_t legal, int64_t gid0,
                                           uint32_t k0, uint32_t k1, uint32_t ctr, int8_t *__restrict__ actions,
                                           float *__restrict__ logp, float *__restrict__ entropy)
{
    const float4 z = mask_rows<MASKED>(*reinterpret_cast<const float4 *>(logits + 4 * i), legal);
    const float m = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
    const float e0 = __expf(z.x - m), e1 = __expf(z.y - m), e2 = __expf(z.z - m), e3 = __expf(z.w - m);
    const float s = e0 + e1 + e2 + e3, inv = 1.0f / s;
    const float p0 = e0 * inv, p1 = e1 * inv, p2 = e2 * inv, p3 = e3 * inv;
    uint32_t w[4] = {(uint32_t)(gid0 + i), (uint32_t)((uint64_t)(gid0 + i) >> 32), ctr, kSampleTag};
    philox4x32_10(w, k0, k1);
    const float u = (float)(w[0] >> 8) * (1.0f / 16777216.0f);
    // first k with cdf(k) > u (np.random.choice's searchsorted(..., side='right'))
    const float c0 = p0, c1 = c0 + p1, c2 = c1 + p2;
    int a = (c0 > u) ? 0 : (c1 > u) ? 1 : (c2 > u) ? 2 : 3;
    // an illegal action has p = 0, so the cdf never passes u AT it; only the fall-through to 3
    // (rounding left the cumulative sum at or below u) can be illegal: the last legal action then
    if (MASKED)
        a = ((legal >> a) & 1u) ? a : (int)last_legal(legal);
    actions[i] = (int8_t)a;
    if (logp) {
        const float za = a == 0 ? z.x : a == 1 ? z.y : a == 2 ? z.z : z.w;
        logp[i] = za - m - __logf(s);
    }
    if (entropy)
        entropy[i] = -(p0 * __logf(p0 + 1e-5f) + p1 * __logf(p1 + 1e-5f) + p2 * __logf(p2 + 1e-5f) +
                       p3 * __logf(p3 + 1e-5f));
}

// epsilon-greedy: u < eps -> a uniform action (MASKED: the mulhi(w1, k)-th of the k legal ones
// in code order; k = 4 gives w1 >> 30, the unmasked rule), else the first argmax
template <bool MASKED>
__device__ __forceinline__ void egreedy_row(const float *__restrict__ q, int64_t i, uint32_t legal, float eps,
                                            uint32_t k0, uint32_t k1, int64_t gid0, uint32_t ctr,
                                            int8_t *__restrict__ actions)
{
    const uint64_t gid = (uint64_t)(gid0 + i);
    uint32_t w[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), ctr, kEgreedyTag};
    philox4x32_10(w, k0, k1);
    const float u = (float)(w[0] >> 8) * (1.0f / 16777216.0f);
    const float4 qv = reinterpret_cast<const float4 *>(q)[i];
    uint32_t explore = w[1] >> 30;
    if (MASKED) {
        const uint32_t j = mulhi(w[1], popc(legal));
        uint32_t seen = 0;
        explore = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t bit = (legal >> b) & 1u;
            explore = (bit && seen == j) ? b : explore;
            seen += bit;
        }
    }
    actions[i] = (int8_t)(u < eps ? explore : argmax4<MASKED>(qv, legal));
}

// y = r + gamma (1 - done) Q'(s', a*), a* = argmax of the online net's Q(s') when DOUBLE, else of
// Q'(s'); MASKED: a* among the legal moves of s', and `terminal` (s' has no legal move) counts as done
template <bool DOUBLE, bool LOG2, bool MASKED>
__device__ __forceinline__ void td_row(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                       const float *__restrict__ q_next_target,
                                       const float *__restrict__ q_next_online, int64_t i, uint32_t legal,
                                       bool terminal, float gamma, float *__restrict__ y)
{
    const float4 qt = reinterpret_cast<const float4 *>(q_next_target)[i];
    const uint32_t a = DOUBLE ? argmax4<MASKED>(reinterpret_cast<const float4 *>(q_next_online)[i], legal)
                              : argmax4<MASKED>(qt, legal);
    const float boot = ((done && done[i]) || (MASKED && terminal)) ? 0.0f : pick(qt, a);
    const float r = LOG2 ? log2f(1.0f + reward[i]) : reward[i];   // trainer.py _reward, torch.log2(1.0 + r)
    y[i] = r + gamma * boot;
}

}  // namespace r48
