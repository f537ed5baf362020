// r48_ntuple.hip -- the n-tuple network (r48_ntuple.h) behind include/rein48.h: value, the fused
// one-ply afterstate search, the expectimax searches and the per-entry-mean TD update. Stateless
// like r48_moves.hip: plain device pointers plus the layout's cells on the host.
//
// Every body is stated once, as a __forceinline__ device routine, and the kernels are those
// routines behind a board load and their stores:
//   nt_act_board     the one-ply search of a board in one lane   k_nt_act, k_nt_td_act, k_nt_td_act_rep
//   nt_add_hits      cnt[e] += 1, acc[e] += delta over 8m hits   k_nt_accumulate, k_nt_td_act, k_nt_td_act_rep
//   nt_owned_hits    the exchange walk that finds an entry's     k_nt_apply, k_nt_apply_rep (plain mean step),
//                    one owner lane                              k_nt_apply_tc, k_nt_apply_tc_rep (TC rule)
//   nt_wave_q2       the depth-2 search of a board by a wave     k_nt_search<L, 2>, k_nt_search3,
//                                                                k_nt_search_ruled, nt_wave_q3
//   nt_wave_q1       the depth-1 search in the same lane mapping k_nt_search<L, 1>, k_nt_search_ruled
//   nt_wave_q3       the depth-3 search of a board by a wave:    k_nt_search_ruled (depth 4)
//                    nt_wave_q2 on each child, one after another
//   nt_slot_term     a slot lane's cell term from the leaves     nt_wave_q2, nt_wave_q3
//   nt_root_moves,   one board per workgroup: wave 0's root      k_nt_search3, k_nt_search_ruled
//   nt_deal_and_     moves, then children dealt from an LDS
//   finish           counter and finished by the last wave
//   nt_child_best,   one dealt child searched by a wave; the     nt_deal_and_finish, k_nt_play_ruled
//   nt_finish_rows   finishing row step over the stored leaves
//   nt_row_q,        how a search ends: butterfly, Q, the four   nt_wave_q2, nt_wave_q3, k_nt_search,
//   nt_write_search  rows' scores, argmax, the writes            nt_finish_rows / nt_deal_and_finish
//   nt_play_store    what a played board leaves behind           k_nt_play1 (over nt_act_board),
//                                                                k_nt_play2 (over nt_wave_q2),
//                                                                k_nt_play_ruled (over the ruled search)
// and r48_ntuple.h's nt_value (k_nt_value and everything above) and nt_tc_rate_mean (k_nt_tc_rate).
// k_nt_carousel_restart and k_nt_carousel_record are the two phases of carousel shaping
// (r48_ntuple.h), over nt_stage, nt_carousel_turn and nt_carousel_donor.
// k_nt_td_act is act, the trainer's TD error and accumulate for the previous step's afterstates in
// one launch: the fused training step. k_nt_search runs one board per WAVE, k_nt_search3,
// k_nt_search_ruled and k_nt_play_ruled one per WORKGROUP; every other kernel one board per lane
// with one 16-byte board load. All are templated on the tuple length L so the cell loops unroll; the expanded
// layout travels by value in the kernel arguments (wave-uniform).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/rein48.h"
#include "r48_board.h"
#include "r48_host.h"
#include "r48_ntuple.h"
#include "r48_select.h"

using r48::aligned;
using r48::aligned16;
using r48::fail;
using r48::grid_for;
using r48::launched;

namespace {

constexpr int kBlock = 256;

// Staging (r48_ntuple.h) is a compile-time parameter of every kernel: a trailing parameter pack C
// that is empty for the unstaged kernel -- its arguments are then exactly what they were -- and one
// argument for the staged twin: the cuts (r48::NtCuts) for a kernel that only reads, the cuts and
// the own flags (NtCutsOwn) for one that updates. nt_stg(cuts...) is the policy the bodies take.
struct NtCutsOwn {
    r48::NtCuts cuts;
    uint8_t *own;
};

__device__ __forceinline__ r48::NtPlain nt_stg() { return r48::NtPlain{}; }
__device__ __forceinline__ r48::NtCuts nt_stg(const r48::NtCuts &c) { return c; }
__device__ __forceinline__ r48::NtCuts nt_stg(const NtCutsOwn &c) { return c.cuts; }
__device__ __forceinline__ uint8_t *nt_own() { return nullptr; }
__device__ __forceinline__ uint8_t *nt_own(const NtCutsOwn &c) { return c.own; }

template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_value(const int8_t *__restrict__ boards, int64_t n,
                                                     const r48::NtLayout lay, const float *__restrict__ tables,
                                                     float *__restrict__ value, const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::Board b = r48::load_board(boards, i);
    value[i] = r48::nt_value<L>(r48::nt_pack(b), lay, tables, r48::nt_base<L>(nt_stg(cuts...), lay.m, b));
}

// the move the one-ply search chooses
struct NtMove {
    r48::Board after;
    float value;
    uint32_t reward, action, legal;
};

// The one-ply search of one board in one lane: the four moves in registers (move_rows4), V of the
// legal ones only, the first maximiser of reward + V. No legal move: action 0, the board itself,
// value 0, reward 0.
template <int L, class Stg>
__device__ __forceinline__ NtMove nt_act_board(const r48::Board &b, const r48::NtLayout &lay,
                                               const float *__restrict__ tables, const Stg &stg)
{
    const r48::Moves4 m = r48::move_rows4<true>(b);
    const uint32_t lg = r48::nt_legal4(m, b);
    r48::Board best_b = b;
    float best_s = 0.0f, best_v = 0.0f;
    uint32_t best_r = 0u, best_a = 0u;
    bool have = false;
#pragma unroll 1
    for (uint32_t a = 0; a < 4u; a++) {
        if (!((lg >> a) & 1u))
            continue;
        // a is uniform: scalar-conditioned selects, no indexed private array
        const r48::Board c = a == 0u ? m.up : a == 1u ? m.down : a == 2u ? m.left : m.right;
        const uint32_t r = a == 0u ? m.r_up : a == 1u ? m.r_down : a == 2u ? m.r_left : m.r_right;
        const float v = r48::nt_value<L>(r48::nt_pack(c), lay, tables, r48::nt_base<L>(stg, lay.m, c));
        const float s = (float)(int32_t)r + v;
        if (!have || s > best_s) {
            have = true;
            best_s = s;
            best_v = v;
            best_r = r;
            best_a = a;
            best_b = c;
        }
    }
    return NtMove{best_b, best_v, best_r, best_a, lg};
}

template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_act(const int8_t *__restrict__ boards, int64_t n,
                                                   const r48::NtLayout lay, const float *__restrict__ tables,
                                                   int8_t *__restrict__ actions, int8_t *__restrict__ after,
                                                   float *__restrict__ value, int32_t *__restrict__ reward,
                                                   uint8_t *__restrict__ legal, const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const NtMove mv = nt_act_board<L>(r48::load_board(boards, i), lay, tables, nt_stg(cuts...));
    actions[i] = (int8_t)mv.action;
    if (after)
        *reinterpret_cast<uint4 *>(after + 16 * i) = make_uint4(mv.after.w0, mv.after.w1, mv.after.w2, mv.after.w3);
    if (value)
        value[i] = mv.value;
    if (reward)
        reward[i] = (int32_t)mv.reward;
    if (legal)
        legal[i] = (uint8_t)mv.legal;
}

// The accumulate half of the update for one board: every hit (t, g) adds 1 to cnt[e] and delta in
// fixed point to acc[e]. Integer atomics, so the sums do not depend on the order of the lanes.
// MARK (a staged update; base = nt_base of the board): a board above stage 0 also sets own[e] = 1
// for each of its hits -- the update's mark, a plain byte store of the one value every marker
// writes, finished with this launch and so before apply's begins.
template <int L, bool MARK = false>
__device__ __forceinline__ void nt_add_hits(const r48::NtBoard &b, const r48::NtLayout &lay, float delta,
                                            unsigned long long *__restrict__ acc, uint32_t *__restrict__ cnt,
                                            uint32_t base = 0u, uint8_t *__restrict__ own = nullptr)
{
    const unsigned long long q = (unsigned long long)r48::nt_fixed_delta(delta);   // two's complement: wraps as int64 adds
    for (int t = 0; t < lay.m; t++) {
#pragma unroll
        for (int g = 0; g < r48::kNtSyms; g++) {
            const uint32_t e = r48::nt_entry<L>(b, lay, r48::kNtSyms * t + g, base);
            atomicAdd(&cnt[e], 1u);
            atomicAdd(&acc[e], q);
            if constexpr (MARK) {
                if (base != 0u)
                    own[e] = 1;
            }
        }
    }
}

// One env step's act and the accumulate half of the TD update for the PREVIOUS afterstates, in one
// launch (the trainer's fused step; apply and the env step follow as their own launches, apply
// needs every sum finished). Lane i:
//   - loads its env board, and issues the loads of its previous afterstate, value, done and valid
//     flags right behind it: nothing needs them before the search is over, so they are in flight
//     under it
//   - runs act's search (nt_act_board) and writes the chosen move's outputs; valid_out = the board
//     had a move, i.e. this afterstate can be learned from at the next step
//   - forms delta = nt_td_delta(...) from this step's reward and value, in registers
//   - where prev_valid: accumulate's walk (nt_add_hits) over the previous afterstate
// tables is only read: acc and cnt are the only words two lanes share, and integer sums do not
// depend on their order, so the launch computes what act, the torch expression for delta and
// accumulate compute one after another, bit for bit. after / value / valid_out must not be the
// prev_ buffers (the entry point refuses it): apply reads the old ones after this kernel.
template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_td_act(
    const int8_t *__restrict__ boards, int64_t n, const r48::NtLayout lay, const float *__restrict__ tables,
    const int8_t *__restrict__ prev_after, const float *__restrict__ prev_value, const uint8_t *__restrict__ prev_done,
    const uint8_t *__restrict__ prev_valid, int8_t *__restrict__ actions, int8_t *__restrict__ after,
    float *__restrict__ value, int32_t *__restrict__ reward, uint8_t *__restrict__ legal, uint8_t *__restrict__ valid_out,
    float *__restrict__ delta_out, unsigned long long *__restrict__ acc, uint32_t *__restrict__ cnt, const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::Board b = r48::load_board(boards, i);
    const r48::Board pb = r48::load_board(prev_after, i);
    const float pv = prev_value[i];
    const uint32_t pd = prev_done[i], pok = prev_valid[i];
    const NtMove mv = nt_act_board<L>(b, lay, tables, nt_stg(cuts...));
    actions[i] = (int8_t)mv.action;
    *reinterpret_cast<uint4 *>(after + 16 * i) = make_uint4(mv.after.w0, mv.after.w1, mv.after.w2, mv.after.w3);
    value[i] = mv.value;
    if (reward)
        reward[i] = (int32_t)mv.reward;
    legal[i] = (uint8_t)mv.legal;
    valid_out[i] = mv.legal != 0u ? 1 : 0;
    const float delta = r48::nt_td_delta(pd, mv.reward, mv.value, pv);
    if (delta_out)
        delta_out[i] = delta;
    if (pok)
        nt_add_hits<L, sizeof...(C) != 0>(r48::nt_pack(pb), lay, delta, acc, cnt,
                                          r48::nt_base<L>(nt_stg(cuts...), lay.m, pb), nt_own(cuts...));
}

template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_accumulate(const int8_t *__restrict__ boards, int64_t n,
                                                          const float *__restrict__ delta,
                                                          const uint8_t *__restrict__ valid, const r48::NtLayout lay,
                                                          unsigned long long *__restrict__ acc,
                                                          uint32_t *__restrict__ cnt, const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const r48::Board b = r48::load_board(boards, i);
    nt_add_hits<L, sizeof...(C) != 0>(r48::nt_pack(b), lay, delta[i], acc, cnt,
                                      r48::nt_base<L>(nt_stg(cuts...), lay.m, b), nt_own(cuts...));
}

// The apply half: every hit again. The one lane of the launch whose exchange takes an entry's
// count owns the entry: update(e, count) runs once per entry hit, in that lane, and takes the
// entry's sum with nt_take_sum. Both scratch words are zero afterwards.
template <int L, class Update>
__device__ __forceinline__ void nt_owned_hits(const r48::NtBoard &b, const r48::NtLayout &lay,
                                              uint32_t *__restrict__ cnt, Update update, uint32_t base = 0u)
{
    for (int t = 0; t < lay.m; t++) {
#pragma unroll
        for (int g = 0; g < r48::kNtSyms; g++) {
            const uint32_t e = r48::nt_entry<L>(b, lay, r48::kNtSyms * t + g, base);
            const uint32_t c = atomicExch(&cnt[e], 0u);
            if (c != 0u)
                update(e, c);
        }
    }
}

__device__ __forceinline__ long long nt_take_sum(unsigned long long *__restrict__ acc, uint32_t e)
{
    return (long long)atomicExch(&acc[e], 0ull);
}

// The staged update's push (r48_ntuple.h): the owner of entry e, whose new value is w, writes w to
// the same entry of every stage above it up to the first owned one. Every mark of this update was
// set by the launch before, so a stage that the update touches is owned and is never written here;
// an unowned one has exactly one writer, the owner of the nearest owned stage below it. A board of
// the top stage pushes nothing. Only the staged kernels hold this code.
template <int L>
__device__ __forceinline__ void nt_push(float *tables, const uint8_t *own, uint32_t e, const r48::NtLayout &lay,
                                        const r48::NtCuts &cuts, float w)
{
    const uint32_t size = (uint32_t)lay.m << (4 * L), end = (uint32_t)(cuts.n + 1) * size;   // <= 2^29
    for (uint32_t k = e + size; k < end && own[k] == 0; k += size)
        tables[k] = w;
}

// The owner moves tables[e] by step * the mean delta of the entry's hits, once. No float atomics:
// bitwise reproducible.
template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_apply(const int8_t *__restrict__ boards, int64_t n,
                                                     const uint8_t *__restrict__ valid, const r48::NtLayout lay,
                                                     float step, float *__restrict__ tables,
                                                     unsigned long long *__restrict__ acc, uint32_t *__restrict__ cnt,
                                                     const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const r48::Board b = r48::load_board(boards, i);
    nt_owned_hits<L>(
        r48::nt_pack(b), lay, cnt,
        [&](uint32_t e, uint32_t c) {
            if constexpr (sizeof...(C) == 0) {
                tables[e] += step * r48::nt_mean(nt_take_sum(acc, e), c);
            } else {
                float w = tables[e];
                w += step * r48::nt_mean(nt_take_sum(acc, e), c);
                tables[e] = w;
                nt_push<L>(tables, nt_own(cuts...), e, lay, nt_stg(cuts...), w);
            }
        },
        r48::nt_base<L>(nt_stg(cuts...), lay.m, b));
}

// apply with temporal-coherence learning rates (r48_ntuple.h): the owner of an entry also owns
// E[e] and A[e] for this launch. Its three loads are issued together, the rule runs in registers,
// three plain stores follow. The sums are order-free integers and the owner's arithmetic does not
// depend on which lane it is, so all three tables are bitwise reproducible and independent of the
// boards' order in the batch.
template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_apply_tc(const int8_t *__restrict__ boards, int64_t n,
                                                        const uint8_t *__restrict__ valid, const r48::NtLayout lay,
                                                        float step, float *__restrict__ tables,
                                                        float *__restrict__ tc_e, float *__restrict__ tc_a,
                                                        unsigned long long *__restrict__ acc,
                                                        uint32_t *__restrict__ cnt, const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const r48::Board b = r48::load_board(boards, i);
    nt_owned_hits<L>(
        r48::nt_pack(b), lay, cnt,
        [&](uint32_t e, uint32_t c) {
            float w = tables[e], se = tc_e[e], sa = tc_a[e];
            r48::nt_tc_update(w, se, sa, r48::nt_mean(nt_take_sum(acc, e), c), step);
            tables[e] = w;
            tc_e[e] = se;
            tc_a[e] = sa;
            if constexpr (sizeof...(C) != 0)   // the value alone: a promoted entry's first update runs at rate 1
                nt_push<L>(tables, nt_own(cuts...), e, lay, nt_stg(cuts...), w);
        },
        r48::nt_base<L>(nt_stg(cuts...), lay.m, b));
}

// How settled the network is on a set of boards: the mean learning rate over each board's hits.
template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_tc_rate(const int8_t *__restrict__ boards, int64_t n,
                                                       const r48::NtLayout lay, const float *__restrict__ tc_e,
                                                       const float *__restrict__ tc_a, float *__restrict__ rate_out,
                                                       const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::Board b = r48::load_board(boards, i);
    rate_out[i] = r48::nt_tc_rate_mean<L>(r48::nt_pack(b), lay, tc_e, tc_a, r48::nt_base<L>(nt_stg(cuts...), lay.m, b));
}

// ---- replicas: R independent unstaged nets in the same launches (r48_ntuple.h) -------------------
// One board per lane like the parents, whose bodies run unchanged under the policy NtOffset: lane i
// belongs to replica r = i / per and reads and updates entries at the offset r * size, size =
// m << 4L. per need not be a multiple of 64, so r is a per-lane value; the division is 32-bit
// wherever the batch allows it (the branch is uniform) and hides behind the table gathers.
__device__ __forceinline__ uint32_t nt_replica(int64_t i, int64_t n, int64_t per)
{
    return n <= 0xFFFFFFFFll ? (uint32_t)i / (uint32_t)per : (uint32_t)(i / per);
}

// k_nt_td_act with the lane's replica offset: search and accumulate both stay inside replica r.
template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_td_act_rep(
    const int8_t *__restrict__ boards, int64_t n, int64_t per, uint32_t size, const r48::NtLayout lay,
    const float *__restrict__ tables, const int8_t *__restrict__ prev_after, const float *__restrict__ prev_value,
    const uint8_t *__restrict__ prev_done, const uint8_t *__restrict__ prev_valid, int8_t *__restrict__ actions,
    int8_t *__restrict__ after, float *__restrict__ value, int32_t *__restrict__ reward, uint8_t *__restrict__ legal,
    uint8_t *__restrict__ valid_out, float *__restrict__ delta_out, unsigned long long *__restrict__ acc,
    uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::NtOffset off{nt_replica(i, n, per) * size};
    const r48::Board b = r48::load_board(boards, i);
    const r48::Board pb = r48::load_board(prev_after, i);
    const float pv = prev_value[i];
    const uint32_t pd = prev_done[i], pok = prev_valid[i];
    const NtMove mv = nt_act_board<L>(b, lay, tables, off);
    actions[i] = (int8_t)mv.action;
    *reinterpret_cast<uint4 *>(after + 16 * i) = make_uint4(mv.after.w0, mv.after.w1, mv.after.w2, mv.after.w3);
    value[i] = mv.value;
    if (reward)
        reward[i] = (int32_t)mv.reward;
    legal[i] = (uint8_t)mv.legal;
    valid_out[i] = mv.legal != 0u ? 1 : 0;
    const float delta = r48::nt_td_delta(pd, mv.reward, mv.value, pv);
    if (delta_out)
        delta_out[i] = delta;
    if (pok)
        nt_add_hits<L>(r48::nt_pack(pb), lay, delta, acc, cnt, r48::nt_base<L>(off, lay.m, pb));
}

// k_nt_apply per replica: the lane loads its replica's step (steps is float[replicas] in device
// memory, L2-resident) and owns entries of its own replica only.
template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_apply_rep(const int8_t *__restrict__ boards, int64_t n, int64_t per,
                                                         uint32_t size, const uint8_t *__restrict__ valid,
                                                         const r48::NtLayout lay, const float *__restrict__ steps,
                                                         float *__restrict__ tables, unsigned long long *__restrict__ acc,
                                                         uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const uint32_t r = nt_replica(i, n, per);
    const float step = steps[r];
    const r48::Board b = r48::load_board(boards, i);
    nt_owned_hits<L>(
        r48::nt_pack(b), lay, cnt,
        [&](uint32_t e, uint32_t c) { tables[e] += step * r48::nt_mean(nt_take_sum(acc, e), c); },
        r48::nt_base<L>(r48::NtOffset{r * size}, lay.m, b));
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_apply_tc_rep(const int8_t *__restrict__ boards, int64_t n, int64_t per,
                                                            uint32_t size, const uint8_t *__restrict__ valid,
                                                            const r48::NtLayout lay, const float *__restrict__ steps,
                                                            float *__restrict__ tables, float *__restrict__ tc_e,
                                                            float *__restrict__ tc_a,
                                                            unsigned long long *__restrict__ acc,
                                                            uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const uint32_t r = nt_replica(i, n, per);
    const float step = steps[r];
    const r48::Board b = r48::load_board(boards, i);
    nt_owned_hits<L>(
        r48::nt_pack(b), lay, cnt,
        [&](uint32_t e, uint32_t c) {
            float w = tables[e], se = tc_e[e], sa = tc_a[e];
            r48::nt_tc_update(w, se, sa, r48::nt_mean(nt_take_sum(acc, e), c), step);
            tables[e] = w;
            tc_e[e] = se;
            tc_a[e] = sa;
        },
        r48::nt_base<L>(r48::NtOffset{r * size}, lay.m, b));
}

// The expectimax search of r48_ntuple.h, one board per wave: lane = 16 a + c is (move a, cell c).
// Every lane makes the board's four moves (the same registers in all 64 lanes) and keeps its
// row's afterstate s_a. Depth 2: lane (a, c) is a SLOT when a is legal and cell c of s_a is empty;
// a slot has two children, s_a[c <- 1] and s_a[c <- 2]. The children of the wave (2 to 120,
// ~35 on boards of running games) are packed densely over the lanes instead of being evaluated
// by their own slot's lane: with the slots' ballot in M, child j is spawn e = 1 + (j & 1) in the
// slot of rank j >> 1 (nt_select_bit finds it; any lane can build any child, it holds all four
// afterstates), lane l evaluates child l and, where there are more than 64, child l + 64
// (nt_leaf: move_rows4 + nt_value per legal reply). The slot's lane then reads its two leaves
// back (ds_bpermute) and forms the header's x_c = fmaf(9, leaf1, leaf2); every other lane holds
// +0, and S_a is the xor butterfly over the 16 lanes of the row -- the header's fixed order,
// whichever lane evaluated a leaf, no LDS. Against one slot per lane evaluating both of its
// children (27 % of the lanes busy, two leaves deep) the packing measured 1.58x / 1.33x faster
// at 2^16 boards (lines-squares / 4x6) and 1.10x / 1.07x at 4,096, the same bits (DESIGN.md
// section 16). At depth 1 the first lane of a row evaluates s_a itself. The four row scores are
// read from lanes 0, 16, 32, 48; those lanes write q, lane 0 the action and the legal set.
constexpr int kSearchBoards = kBlock / 64;   // boards (waves) per workgroup

__device__ __forceinline__ uint32_t uniform_word(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// How a search at depth 2 or 3 ends in lane 16 a + c: S_a by the xor butterfly over the row's
// cell terms x, then the header's Q(a); -inf where move a is illegal.
__device__ __forceinline__ float nt_row_q(float x, bool ok, uint32_t reward, const r48::Board &afterstate)
{
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 8);
    return ok ? r48::nt_q2(reward, x, r48::blanks(afterstate).n) : -__builtin_inff();
}

// What every search writes for board i from the rows' scores qa: the first lane of each row its
// q, lane 0 the first maximiser and the legal set.
__device__ __forceinline__ void nt_write_search(float qa, uint32_t lane, uint32_t lg, int64_t i,
                                                int8_t *__restrict__ actions, float *__restrict__ q,
                                                uint8_t *__restrict__ legal)
{
    const float q0 = __shfl(qa, 0), q1 = __shfl(qa, 16), q2 = __shfl(qa, 32), q3 = __shfl(qa, 48);
    if (q && (lane & 15u) == 0u)
        q[4 * i + (lane >> 4)] = qa;
    if (lane == 0u) {
        actions[i] = (int8_t)r48::nt_argmax4(q0, q1, q2, q3);
        if (legal)
            legal[i] = (uint8_t)lg;
    }
}

// The header's x_c in a slot lane from the wave's leaves, +0 in every other lane: the leaf of child
// j is in lane j & 63, in leaf0 for j < 64 and in leaf1 beyond, and the slot of rank rho (rank2 =
// 2 rho) owns children 2 rho and 2 rho + 1. rank2 is even, so rank2 + 1 stays in the wave.
__device__ __forceinline__ float nt_slot_term(float leaf0, float leaf1, uint32_t rank2, bool slot)
{
    const int src = (int)(rank2 & 63u);
    const float two0 = __shfl(leaf0, src), four0 = __shfl(leaf0, src + 1);
    const float two1 = __shfl(leaf1, src), four1 = __shfl(leaf1, src + 1);
    const bool late = rank2 >= 64u;
    return slot ? r48::nt_fma(9.0f, late ? two1 : two0, late ? four1 : four0) : 0.0f;
}

// The depth-2 search of a board that every lane of the wave holds (the lane mapping above): the
// lane's Q_2 of its row's move (-inf where the move is illegal) and the board's legal set. Shared
// by k_nt_search<L, 2>, whose board is the batch's, and k_nt_search3, whose boards are the root's
// children.
template <int L, class Stg>
__device__ __forceinline__ float nt_wave_q2(const r48::Board &b, uint32_t lane, const r48::NtLayout &lay,
                                            const float *__restrict__ tables, uint32_t &lg, const Stg &stg)
{
    const uint32_t a = lane >> 4, c = lane & 15u;
    const r48::Moves4 m = r48::move_rows4<true>(b);
    lg = r48::nt_legal4(m, b);
    const r48::Board s = r48::nt_pick(m, a);
    const uint32_t r = r48::nt_pick_reward(m, a);
    const bool ok = ((lg >> a) & 1u) != 0u;
    const bool slot = ok && r48::nt_cell(s, c) == 0u;
    const uint64_t M = __ballot(slot);
    const uint32_t kids = 2u * (uint32_t)__popcll(M);
    const uint32_t rank2 = 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
    float leaf0 = 0.0f, leaf1 = 0.0f;
#pragma unroll 1
    for (uint32_t base = 0u; base < kids; base += 64u) {   // uniform: at most two rounds
        float leaf = 0.0f;
        if (base + lane < kids) {
            const uint32_t p = r48::nt_select_bit(M, (base + lane) >> 1);
            r48::Board child = r48::nt_pick(m, p >> 4);
            r48::place(child, p & 15u, 1u + (lane & 1u), true);
            leaf = r48::nt_leaf<L>(child, lay, tables, stg);
        }
        leaf0 = base == 0u ? leaf : leaf0;
        leaf1 = base == 0u ? leaf1 : leaf;
    }
    return nt_row_q(nt_slot_term(leaf0, leaf1, rank2, slot), ok, r, s);
}

// The depth-1 search in the same lane mapping: the first lane of a row scores s_a itself, the row
// reads it. Shared by k_nt_search<L, 1> and k_nt_search_ruled.
template <int L, class Stg>
__device__ __forceinline__ float nt_wave_q1(const r48::Board &b, uint32_t lane, const r48::NtLayout &lay,
                                            const float *__restrict__ tables, uint32_t &lg, const Stg &stg)
{
    const uint32_t a = lane >> 4, c = lane & 15u;
    const r48::Moves4 m = r48::move_rows4<true>(b);
    lg = r48::nt_legal4(m, b);
    const bool ok = ((lg >> a) & 1u) != 0u;
    float x = 0.0f;
    if (ok && c == 0u)
        x = r48::nt_score<L>(r48::nt_pick(m, a), r48::nt_pick_reward(m, a), lay, tables, stg);
    return ok ? __shfl(x, (int)(lane & 48u)) : -__builtin_inff();
}

// The largest of a wave's four row scores, 0 where the board has no legal move: best_k of the
// board the wave searched at depth k. An illegal move holds -inf, so the plain max is the max over
// the legal ones.
__device__ __forceinline__ float nt_wave_best(float qa, uint32_t lg)
{
    const float b0 = __shfl(qa, 0), b1 = __shfl(qa, 16), b2 = __shfl(qa, 32), b3 = __shfl(qa, 48);
    return lg ? fmaxf(fmaxf(b0, b1), fmaxf(b2, b3)) : 0.0f;
}

// what nt_wave_q3 keeps of its board across the searches of the board's children, one per wave
struct WaveRoot {
    uint32_t after[4][4];   // the afterstate of move a, words w0 .. w3
    uint32_t reward[4];
};

// The depth-3 search of a board that every lane of the wave holds: nt_wave_q2 with the leaf one
// level deeper. The board's children (2 to 120, numbered as nt_wave_q2 numbers them: child j is
// spawn 1 + (j & 1) in the slot of rank j >> 1 of the ballot M) are searched one after another by
// the whole wave, nt_wave_q2 on each, and best_2(child j) is kept in lane j & 63 -- in its first
// leaf register for j < 64, its second beyond, by selects -- which is where nt_wave_q2's tail
// reads its leaves: by rank2 with __shfl, then nt_fma, then nt_row_q. The four afterstates do not
// stay in registers across the inner searches (held there, the 3-ply kernel's first form took
// 100 to 168 VGPRs): the first lane of each row leaves its afterstate in the wave's own LDS slot
// `keep`, the loop reads a child's parent from there with a uniform address and the tail its
// row's. Only this wave touches `keep`, and a wave's LDS operations complete in order.
template <int L, class Stg>
__device__ __forceinline__ float nt_wave_q3(const r48::Board &b, uint32_t lane, const r48::NtLayout &lay,
                                            const float *__restrict__ tables, WaveRoot &keep, uint32_t &lg,
                                            const Stg &stg)
{
    const uint32_t a = lane >> 4, c = lane & 15u;
    uint64_t M;
    {
        const r48::Moves4 m = r48::move_rows4<true>(b);
        lg = uniform_word(r48::nt_legal4(m, b));   // the same in every lane: a scalar across the loop
        const r48::Board s = r48::nt_pick(m, a);
        M = __ballot(((lg >> a) & 1u) != 0u && r48::nt_cell(s, c) == 0u);
        if (c == 0u) {
            keep.after[a][0] = s.w0;
            keep.after[a][1] = s.w1;
            keep.after[a][2] = s.w2;
            keep.after[a][3] = s.w3;
            keep.reward[a] = r48::nt_pick_reward(m, a);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t kids = 2u * (uint32_t)__popcll(M);
    float leaf0 = 0.0f, leaf1 = 0.0f;
#pragma unroll 1
    for (uint32_t j = 0u; j < kids; j++) {   // uniform
        const uint32_t p = r48::nt_select_bit(M, j >> 1);   // < 64
        const uint32_t *sa = keep.after[p >> 4];
        r48::Board child{sa[0], sa[1], sa[2], sa[3]};
        r48::place(child, p & 15u, 1u + (j & 1u), true);
        uint32_t lg2;
        const float q2a = nt_wave_q2<L>(child, lane, lay, tables, lg2, stg);
        const float best = nt_wave_best(q2a, uniform_word(lg2));
        const bool mine = lane == (j & 63u);
        leaf0 = (mine && j < 64u) ? best : leaf0;
        leaf1 = (mine && j >= 64u) ? best : leaf1;
    }
    const bool ok = ((lg >> a) & 1u) != 0u;
    const bool slot = ((M >> lane) & 1ull) != 0ull;
    const uint32_t rank2 = 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
    const r48::Board s{keep.after[a][0], keep.after[a][1], keep.after[a][2], keep.after[a][3]};
    return nt_row_q(nt_slot_term(leaf0, leaf1, rank2, slot), ok, keep.reward[a], s);
}

template <int L, int DEPTH, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_search(const int8_t *__restrict__ boards, int64_t n,
                                                      const r48::NtLayout lay, const float *__restrict__ tables,
                                                      int8_t *__restrict__ actions, float *__restrict__ q,
                                                      uint8_t *__restrict__ legal, const C... cuts)
{
    static_assert(DEPTH == 1 || DEPTH == 2, "depth 1 or 2");
    const int64_t i = (int64_t)blockIdx.x * kSearchBoards + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= n)
        return;   // the whole wave
    const uint32_t lane = threadIdx.x & 63u;
    const r48::Board b = r48::load_board(boards, i);
    uint32_t lg;
    float qa;
    if (DEPTH == 1)
        qa = nt_wave_q1<L>(b, lane, lay, tables, lg, nt_stg(cuts...));
    else
        qa = nt_wave_q2<L>(b, lane, lay, tables, lg, nt_stg(cuts...));
    nt_write_search(qa, lane, lg, i, actions, q, legal);
}

// The 3-ply search of r48_ntuple.h: a depth-2 search (nt_wave_q2) of each of the root's 2 to 120
// children, then the averaging step depth 2 ends with. One board per workgroup of WAVES waves.
// Wave 0 loads the board, makes the four moves and forms the root's slot ballot M with
// lane = 16 a + c as depth 2 does, and leaves the four afterstates, their rewards, the legal set
// and M in LDS; after the one barrier every wave reads what it needs from there (the other waves
// make no root move at all). The root's child j is spawn 1 + (j & 1) in the slot
// nt_select_bit(M, j >> 1), wave-uniform. The children are dealt through an LDS counter: wave w
// starts with child w and takes the next undealt one after each. A wave searches its child and
// its lane 0 stores best_2(child) = the largest of the child's four Q_2, 0 where it has no move,
// to leaf[j]. A wave that finds no child left adds the number it did to a second counter and
// leaves; the wave whose addition completes the count -- the last to arrive, whichever it is --
// finishes as depth 2 does: the slot lane of rank rho reads leaf[2 rho] and leaf[2 rho + 1],
// forms x_c by nt_fma, the butterfly and nt_q2 follow. Nobody waits for the slowest child. A leaf
// is the same wave-level routine on the same child and the last step reads leaves by child
// number, so where a board is in the grid, how the children were dealt and which wave did what
// do not reach the bits. A board with no legal move has no child: the workgroup leaves right
// after the barrier.
// How many waves share a board trades latency against throughput (DESIGN.md has the A/B): with 16
// a board's ~35 children are done in 2 to 3 rounds, which is the time of a small batch; in a
// large batch the machine is full either way, what counts is how many waves are resident, and a
// workgroup of 4 waves fills the wave slots that one of 16 leaves empty while its last children
// finish. The bits do not depend on it. R48_NT_SEARCH3_WAVES (an experiment's build) fixes one
// number for every n.
#ifdef R48_NT_SEARCH3_WAVES
constexpr int kSearch3WavesSmall = R48_NT_SEARCH3_WAVES, kSearch3WavesLarge = R48_NT_SEARCH3_WAVES;
#else
constexpr int kSearch3WavesSmall = 16, kSearch3WavesLarge = 4;
#endif
constexpr int64_t kSearch3SmallBatch = 8192;   // boards up to which the small batch's mapping runs
constexpr int kSearch3MaxKids = 120;           // 2 spawns in at most 4 * 15 slots

// what wave 0 leaves for the others
struct Search3Root {
    uint32_t after[4][4];   // the afterstate of move a, words w0 .. w3
    uint32_t reward[4];
    uint32_t legal, slots_lo, slots_hi;
    uint32_t dealt, done;   // children handed out; children whose leaf is stored
};

// Wave 0's part before the barrier: the root's four moves, the slot ballot and the counters, left
// in LDS for every wave (lane = 16 a + c as depth 2 has it).
template <int WAVES>
__device__ __forceinline__ void nt_root_moves(const r48::Board &b, uint32_t lane, Search3Root &root)
{
    const uint32_t a = lane >> 4, c = lane & 15u;
    const r48::Moves4 m = r48::move_rows4<true>(b);
    const uint32_t lg = r48::nt_legal4(m, b);
    const r48::Board s = r48::nt_pick(m, a);
    const uint64_t M = __ballot(((lg >> a) & 1u) != 0u && r48::nt_cell(s, c) == 0u);
    if (c == 0u) {
        root.after[a][0] = s.w0;
        root.after[a][1] = s.w1;
        root.after[a][2] = s.w2;
        root.after[a][3] = s.w3;
        root.reward[a] = r48::nt_pick_reward(m, a);
    }
    if (lane == 0u) {
        root.legal = lg;
        root.slots_lo = (uint32_t)M;
        root.slots_hi = (uint32_t)(M >> 32);
        root.dealt = (uint32_t)WAVES;   // children 0 .. waves - 1 are dealt by wave number
        root.done = 0u;
    }
}

// One dealt child, by a whole wave: the root's child j (spawn 1 + (j & 1) in the slot
// nt_select_bit(M, j >> 1), its parent afterstate read from `root` with a uniform address) searched
// INNER plies deep -- 2: nt_wave_q2, 3: nt_wave_q3 with the wave's own LDS slot -- and best_INNER of
// it in every lane. The per-child body of nt_deal_and_finish and of k_nt_play_ruled.
template <int L, int INNER, class Stg>
__device__ __forceinline__ float nt_child_best(const Search3Root &root, uint64_t M, uint32_t j, uint32_t lane,
                                               const r48::NtLayout &lay, const float *__restrict__ tables,
                                               WaveRoot *keep_w, const Stg &stg)
{
    static_assert(INNER == 2 || INNER == 3, "a child is searched 2 or 3 plies deep");
    const uint32_t p = r48::nt_select_bit(M, j >> 1);   // < 64
    const uint32_t *sa = root.after[p >> 4];
    r48::Board child{sa[0], sa[1], sa[2], sa[3]};
    r48::place(child, p & 15u, 1u + (j & 1u), true);
    uint32_t lgc;
    float qc;
    if constexpr (INNER == 2)
        qc = nt_wave_q2<L>(child, lane, lay, tables, lgc, stg);
    else
        qc = nt_wave_q3<L>(child, lane, lay, tables, *keep_w, lgc, stg);
    return nt_wave_best(qc, lgc);
}

// The finishing row step, by one wave once every leaf is stored: the slot lane of rank rho reads
// leaf[2 rho] and leaf[2 rho + 1] -- by child number, so the deal does not reach the bits -- forms
// x_c by nt_fma, and nt_row_q gives the lane its row's Q. Shared like nt_child_best.
__device__ __forceinline__ float nt_finish_rows(const Search3Root &root, const float *leaf, uint64_t M, uint32_t lg,
                                                uint32_t lane)
{
    const uint32_t a = lane >> 4;
    const r48::Board s{root.after[a][0], root.after[a][1], root.after[a][2], root.after[a][3]};
    const uint32_t r = root.reward[a];
    const bool ok = ((lg >> a) & 1u) != 0u;
    const bool slot = ((M >> lane) & 1ull) != 0ull;
    const uint32_t rank2 = 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
    float x = 0.0f;
    if (slot)   // rank2 + 1 < kids <= 120
        x = r48::nt_fma(9.0f, leaf[rank2], leaf[rank2 + 1u]);
    return nt_row_q(x, ok, r, s);
}

// Every wave's part after the barrier, the deal and the finish of the comment above, stated once
// for both kernels that run it. INNER is the depth a child is searched at: 2 (nt_wave_q2; the
// board's Q_3, k_nt_search3 and the ruled kernel at depth 3) or 3 (nt_wave_q3 with the wave's LDS
// slot `keep`; the board's Q_4). Nothing follows it in a kernel: a wave returns from it when it
// has no more to do.
template <int L, int WAVES, int INNER, class Stg>
__device__ __forceinline__ void nt_deal_and_finish(Search3Root &root, float *leaf, WaveRoot *keep, int64_t i, uint32_t w,
                                                   uint32_t lane, const r48::NtLayout &lay,
                                                   const float *__restrict__ tables, int8_t *__restrict__ actions,
                                                   float *__restrict__ q, uint8_t *__restrict__ legal, const Stg &stg)
{
    static_assert(INNER == 2 || INNER == 3, "a child is searched 2 or 3 plies deep");
    const uint32_t a = lane >> 4, c = lane & 15u;
    const uint32_t lg = uniform_word(root.legal);
    if (lg == 0u) {   // uniform over the workgroup
        if (w == 0u && lane == 0u) {
            actions[i] = 0;
            if (legal)
                legal[i] = 0;
        }
        if (q && w == 0u && c == 0u)
            q[4 * i + a] = -__builtin_inff();
        return;
    }
    const uint64_t M = (uint64_t)uniform_word(root.slots_lo) | ((uint64_t)uniform_word(root.slots_hi) << 32);
    const uint32_t kids = 2u * (uint32_t)__popcll(M);   // 4 .. 120
    uint32_t mine = 0u;
#pragma unroll 1
    for (uint32_t j = w; j < kids; mine++) {
        const float best = nt_child_best<L, INNER>(root, M, j, lane, lay, tables, keep + w, stg);
        uint32_t next = 0u;
        if (lane == 0u) {
            leaf[j] = best;
            next = __hip_atomic_fetch_add(&root.dealt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        j = uniform_word(next);
    }
    if (mine == 0u)
        return;   // more waves than children
    uint32_t before = 0u;
    if (lane == 0u)   // releases this wave's leaves, acquires the others' where it completes the count
        before = __hip_atomic_fetch_add(&root.done, mine, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (uniform_word(before) + mine != kids)
        return;
    nt_write_search(nt_finish_rows(root, leaf, M, lg, lane), lane, lg, i, actions, q, legal);
}

template <int L, int WAVES, class... C>
__global__ __launch_bounds__(64 * WAVES) void k_nt_search3(const int8_t *__restrict__ boards, int64_t n,
                                                           const r48::NtLayout lay, const float *__restrict__ tables,
                                                           int8_t *__restrict__ actions, float *__restrict__ q,
                                                           uint8_t *__restrict__ legal, const C... cuts)
{
    static_assert(WAVES >= 1 && WAVES <= 16, "a workgroup has at most 1024 lanes");
    __shared__ float leaf[kSearch3MaxKids];
    __shared__ Search3Root root;
    const int64_t i = blockIdx.x;   // the grid has one workgroup per board
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (w == 0u)
        nt_root_moves<WAVES>(r48::load_board(boards, i), lane, root);
    __syncthreads();
    nt_deal_and_finish<L, WAVES, 2>(root, leaf, nullptr, i, w, lane, lay, tables, actions, q, legal, nt_stg(cuts...));
}

// The ruled search of r48_ntuple.h: board i at depth d = rule[blanks(board i)], 1..4, one board per
// workgroup with k_nt_search3's scheme -- wave 0 makes the root's moves, one barrier, the children
// dealt from the LDS counter, the last wave to arrive finishes; no waiting loop, nothing shared
// between workgroups. The depth is uniform over the workgroup (wave 0 leaves it in LDS with the
// root):
//   d = 4   a child's leaf is best_3(child), from nt_wave_q3 (each wave with its own LDS slot)
//   d = 3   best_2(child), from nt_wave_q2: k_nt_search3's body and bits
//   d <= 2  wave 0 alone runs k_nt_search's depth-2 or depth-1 body on the board it still holds;
//           the other waves leave after the barrier
// The rule travels as one word (nt_rule_pack). depth_out[i] = d whether the board has a move or not.
template <int L, int WAVES, class... C>
__global__ __launch_bounds__(64 * WAVES) void k_nt_search_ruled(const int8_t *__restrict__ boards, int64_t n,
                                                                const r48::NtLayout lay, const float *__restrict__ tables,
                                                                const uint64_t rule, int8_t *__restrict__ actions,
                                                                float *__restrict__ q, uint8_t *__restrict__ legal,
                                                                uint8_t *__restrict__ depth_out, const C... cuts)
{
    static_assert(WAVES >= 1 && WAVES <= 16, "a workgroup has at most 1024 lanes");
    __shared__ float leaf[kSearch3MaxKids];
    __shared__ Search3Root root;
    __shared__ WaveRoot keep[WAVES];
    __shared__ uint32_t depth;
    const int64_t i = blockIdx.x;   // the grid has one workgroup per board
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    r48::Board b{0u, 0u, 0u, 0u};
    if (w == 0u) {
        b = r48::load_board(boards, i);
        const uint32_t d0 = uniform_word(r48::nt_packed_rule_depth(rule, b));
        if (d0 >= 3u)
            nt_root_moves<WAVES>(b, lane, root);
        if (lane == 0u) {
            depth = d0;
            if (depth_out)
                depth_out[i] = (uint8_t)d0;
        }
    }
    __syncthreads();
    const uint32_t d = uniform_word(depth);
    if (d == 4u) {
        nt_deal_and_finish<L, WAVES, 3>(root, leaf, keep, i, w, lane, lay, tables, actions, q, legal, nt_stg(cuts...));
    } else if (d == 3u) {
        nt_deal_and_finish<L, WAVES, 2>(root, leaf, keep, i, w, lane, lay, tables, actions, q, legal, nt_stg(cuts...));
    } else if (w == 0u) {
        uint32_t lg;
        const float qa = d == 2u ? nt_wave_q2<L>(b, lane, lay, tables, lg, nt_stg(cuts...))
                                 : nt_wave_q1<L>(b, lane, lay, tables, lg, nt_stg(cuts...));
        nt_write_search(qa, lane, lg, i, actions, q, legal);
    }
}

// ---- playing whole games: search and env step for n_steps steps in one launch -------------------
// The play contract of r48_ntuple.h. A board stays in registers from its one load to its one store;
// length and gain are summed in registers and added to the caller's words at the end. A board
// without a legal move is finished: the contract's remaining steps are the identity on it, so its
// lane stops searching (no gather is issued for it again) and a wave leaves the step loop once
// none of its boards is alive -- a batch played to the end costs each wave the moves of its longest
// game, not n_steps. Nothing is shared between boards: no barrier, no LDS, no atomics.

// what a board's play leaves behind, written by one lane
__device__ __forceinline__ void nt_play_store(int8_t *__restrict__ boards, int64_t i, const r48::Board &b, uint32_t len,
                                              uint32_t gn, int32_t *__restrict__ length, int32_t *__restrict__ gain,
                                              uint8_t *__restrict__ done)
{
    *reinterpret_cast<uint4 *>(boards + 16 * i) = make_uint4(b.w0, b.w1, b.w2, b.w3);
    if (length)
        length[i] += (int32_t)len;
    if (gain)
        gain[i] += (int32_t)gn;
    if (done)
        done[i] = (uint8_t)r48::nt_play_done(b);
}

// Depth 1, LANES lanes per board.
//   LANES == 4 (what runs): lane 4 j + a of a wave holds board j like its three neighbours and
//     scores move a alone (nt_score: nt_value's order); the four scores come back by __shfl and
//     every lane takes act's first maximiser over the legal moves, then makes the same step. A
//     board's dependent chain of gathers is a quarter as long and a batch is four times as many
//     waves: 4,096 boards are 256 waves instead of 64 on 1,024 SIMDs.
//   LANES == 1 (-DR48_NT_PLAY_LANES=1, an experiment's build): nt_act_board, act's search as it is.
// Either way the bits are act's: the value sum is nt_value's, the winner the first legal move whose
// score is strictly above every earlier legal one. Measured (DESIGN.md section 16,
// profiles/ntuple/play_mapping_ab.log): four lanes take a third of the time per step at 4,096
// boards and the same time at 2^16.
#ifndef R48_NT_PLAY_LANES
#define R48_NT_PLAY_LANES 4
#endif
constexpr int kPlayLanes = R48_NT_PLAY_LANES;

template <int L, int LANES, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_play1(int8_t *__restrict__ boards, int64_t n, const r48::NtLayout lay,
                                                     const float *__restrict__ tables, int32_t n_steps, uint32_t k0,
                                                     uint32_t k1, int64_t gid0, uint32_t step0,
                                                     int32_t *__restrict__ length, int32_t *__restrict__ gain,
                                                     uint8_t *__restrict__ done, const C... cuts)
{
    static_assert(LANES == 1 || LANES == 4, "one lane per board, or one per move");
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (i >= n)
        return;   // with LANES == 4, all four lanes of the board
    const uint32_t sub = threadIdx.x & (uint32_t)(LANES - 1);
    const uint64_t gid = (uint64_t)(gid0 + i);
    r48::Board b = r48::load_board(boards, i);
    uint32_t len = 0u, gn = 0u;
    bool alive = true;
#pragma unroll 1
    for (int32_t t = 0; t < n_steps; t++) {
        if (__ballot(alive) == 0ull)
            break;   // the whole wave is finished
        if (alive) {
            uint32_t action, lg;
            if (LANES == 1) {
                const NtMove mv = nt_act_board<L>(b, lay, tables, nt_stg(cuts...));
                action = mv.action;
                lg = mv.legal;
            } else {
                const r48::Moves4 m = r48::move_rows4<true>(b);
                lg = r48::nt_legal4(m, b);
                float s = 0.0f;
                if ((lg >> sub) & 1u)
                    s = r48::nt_score<L>(r48::nt_pick(m, sub), r48::nt_pick_reward(m, sub), lay, tables, nt_stg(cuts...));
                const int first = (int)(threadIdx.x & 63u & ~3u);
                action = 0u;
                float best = 0.0f;
                bool have = false;
#pragma unroll
                for (uint32_t a = 0; a < 4u; a++) {
                    const float sa = __shfl(s, first + (int)a);
                    if (((lg >> a) & 1u) && (!have || sa > best)) {
                        have = true;
                        best = sa;
                        action = a;
                    }
                }
            }
            if (lg == 0u) {
                alive = false;
            } else {
                const r48::StepOut o = r48::nt_play_step(b, action, gid, step0 + (uint32_t)t, k0, k1);
                len += o.changed;
                gn += o.reward;
                alive = o.done == 0u;
            }
        }
    }
    if (sub == 0u)
        nt_play_store(boards, i, b, len, gn, length, gain, done);
}

// Depth 2, one board per wave as k_nt_search<L, 2>: every lane holds the board, nt_wave_q2 searches
// it, the rows' scores are read as nt_write_search reads them and every lane takes their first
// maximiser and makes the same step, so the board stays wave-uniform; lane 0 stores it once at the
// end.
template <int L, class... C>
__global__ __launch_bounds__(kBlock) void k_nt_play2(int8_t *__restrict__ boards, int64_t n, const r48::NtLayout lay,
                                                     const float *__restrict__ tables, int32_t n_steps, uint32_t k0,
                                                     uint32_t k1, int64_t gid0, uint32_t step0,
                                                     int32_t *__restrict__ length, int32_t *__restrict__ gain,
                                                     uint8_t *__restrict__ done, const C... cuts)
{
    const int64_t i = (int64_t)blockIdx.x * kSearchBoards + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= n)
        return;   // the whole wave
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gid = (uint64_t)(gid0 + i);
    r48::Board b = r48::load_board(boards, i);
    uint32_t len = 0u, gn = 0u;
#pragma unroll 1
    for (int32_t t = 0; t < n_steps; t++) {
        uint32_t lg;
        const float qa = nt_wave_q2<L>(b, lane, lay, tables, lg, nt_stg(cuts...));
        if (uniform_word(lg) == 0u)
            break;   // finished: the wave leaves
        const float q0 = __shfl(qa, 0), q1 = __shfl(qa, 16), q2 = __shfl(qa, 32), q3 = __shfl(qa, 48);
        const r48::StepOut o = r48::nt_play_step(b, r48::nt_argmax4(q0, q1, q2, q3), gid, step0 + (uint32_t)t, k0, k1);
        len += o.changed;
        gn += o.reward;
    }
    if (lane == 0u)
        nt_play_store(boards, i, b, len, gn, length, gain, done);
}

// The ruled play contract of r48_ntuple.h: every step searches the board at rule[its blanks] plies.
// One board per workgroup of WAVES waves, as k_nt_search_ruled, and the workgroup stays on its board
// for all n_steps. EVERY wave holds the board and the step number t in registers, the same bits in
// all of them, and the loop below keeps it so; a step is one of two PHASES, chosen by the depth d of
// the board -- a function of those registers, hence the same in every wave:
//   d >= 3  a DEEP step. Wave 0 makes the root's moves into root[par] (nt_root_moves); barrier B1;
//           every wave reads the legal set and the slot ballot from there and the children are dealt
//           from the LDS counter, best_(d-1)(child j) to leaf[par][j] (nt_child_best); barrier B2 is
//           the hand-over that nt_deal_and_finish does by counting arrivals, since here the waves go
//           on; then EVERY wave runs the finishing row step (nt_finish_rows: the same LDS words, the
//           same arithmetic, so the same four scores), takes the first maximiser and makes the env's
//           step on its own copy of the board. Nothing is handed back: the copies stay equal.
//   d <= 2  a SHALLOW run. Wave 0 alone plays on -- nt_wave_q2 / nt_wave_q1 and the step, as
//           k_nt_play2 does -- for as long as the board stays at depth <= 2, has a move and steps
//           are left, then leaves the board, t and whether it still has a move in hand[hpar];
//           barrier B0; the other waves, which came straight to B0, take them from there.
// The barriers. A wave's path through the loop is decided by t < n_steps, d and, after a barrier,
// by two LDS words: root[par].legal (game over at a deep step) and hand[hpar].alive (at a shallow
// run). t and the board are equal registers in every wave (by induction: both phases leave them
// equal), and each of the two words is written by wave 0 BEFORE the barrier it is read after and not
// again until wave 0 has passed two more barriers (below), so no wave can read another value of it:
// every condition that guards a barrier is workgroup-uniform by construction, and all waves make
// the same sequence of B0 / B1 / B2 and leave the loop together.
// The buffers. root / leaf and hand are double-buffered by the parity of the deep steps (par) and of
// the shallow runs (hpar), which every wave counts alike. A deep step's buffers are last read in its
// finishing step, i.e. before the reader arrives at its next barrier; wave 0 writes the same parity
// again two deep steps later, after it has passed B1 and B2 of the step in between, which no wave
// passes before every wave has arrived there. The same holds for hand with the B0 of the run in
// between (and a shallow run is in fact always followed by a deep step or the end). So no second
// barrier per phase is needed to protect leaf[], the counters or the hand-over words.
// length and gain are wave 0's sums (it makes every step); lane 0 of wave 0 stores once.
// Waves per board: 16 up to 8,192 boards and 4 beyond, as k_nt_search_ruled. Measured (DESIGN.md,
// profiles/ntuple/exp_ntuple_play_ruled_waves.json): 8 waves take 4 to 6 % less than 16 for 4,096
// depth-3 evaluations but 14 to 17 % more under depth_rule(16, 1) and 1.4x at 64 boards, where a
// board's own latency is what counts; 4 waves lose everywhere up to 8,192 boards and win beyond.
// R48_NT_PLAY_RULED_WAVES (an experiment's build) fixes one number of waves for every n; the bits do
// not depend on it.
#ifdef R48_NT_PLAY_RULED_WAVES
constexpr int kPlayRuledWavesSmall = R48_NT_PLAY_RULED_WAVES, kPlayRuledWavesLarge = R48_NT_PLAY_RULED_WAVES;
#else
constexpr int kPlayRuledWavesSmall = 16, kPlayRuledWavesLarge = 4;
#endif

// A board whose words are the same in every lane, as scalars: what is carried from step to step
// lives in SGPRs and takes no vector register across a search.
__device__ __forceinline__ r48::Board uniform_board(const r48::Board &b)
{
    return r48::Board{uniform_word(b.w0), uniform_word(b.w1), uniform_word(b.w2), uniform_word(b.w3)};
}

// what wave 0 leaves for the others after a shallow run
struct PlayHand {
    uint32_t board[4];
    uint32_t t, alive;
};

template <int L, int WAVES, class... C>
__global__ __launch_bounds__(64 * WAVES) void k_nt_play_ruled(int8_t *__restrict__ boards, int64_t n,
                                                              const r48::NtLayout lay, const float *__restrict__ tables,
                                                              const uint64_t rule, int32_t n_steps, uint32_t k0,
                                                              uint32_t k1, int64_t gid0, uint32_t step0,
                                                              int32_t *__restrict__ length, int32_t *__restrict__ gain,
                                                              uint8_t *__restrict__ done, const C... cuts)
{
    static_assert(WAVES >= 1 && WAVES <= 16, "a workgroup has at most 1024 lanes");
    __shared__ float leaf[2][kSearch3MaxKids];
    __shared__ Search3Root root[2];
    __shared__ WaveRoot keep[WAVES];
    __shared__ PlayHand hand[2];
    const int64_t i = blockIdx.x;   // the grid has one workgroup per board
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gid = (uint64_t)(gid0 + i);
    r48::Board b = uniform_board(r48::load_board(boards, i));   // every wave, the same address
    uint32_t len = 0u, gn = 0u, par = 0u, hpar = 0u;
    uint32_t t = 0u;
    const uint32_t steps = (uint32_t)n_steps;    // > 0, the entry point returns before the launch otherwise
#pragma unroll 1
    while (t < steps) {   // uniform over the workgroup: t is
        uint32_t d = uniform_word(r48::nt_packed_rule_depth(rule, b));
        if (d <= 2u) {    // uniform over the workgroup: the board is
            PlayHand &h = hand[hpar];
            hpar ^= 1u;
            if (w == 0u) {
                uint32_t alive = 1u;
#pragma unroll 1
                do {
                    uint32_t lg;
                    const float qa = d == 2u ? nt_wave_q2<L>(b, lane, lay, tables, lg, nt_stg(cuts...))
                                             : nt_wave_q1<L>(b, lane, lay, tables, lg, nt_stg(cuts...));
                    if (uniform_word(lg) == 0u) {
                        alive = 0u;   // finished
                        break;
                    }
                    const float q0 = __shfl(qa, 0), q1 = __shfl(qa, 16), q2 = __shfl(qa, 32), q3 = __shfl(qa, 48);
                    const r48::StepOut o = r48::nt_play_step(b, r48::nt_argmax4(q0, q1, q2, q3), gid, step0 + t, k0, k1);
                    b = uniform_board(b);
                    len += uniform_word(o.changed);
                    gn += uniform_word(o.reward);
                    t++;
                    d = uniform_word(r48::nt_packed_rule_depth(rule, b));
                } while (t < steps && d <= 2u);
                if (lane == 0u) {
                    h.board[0] = b.w0;
                    h.board[1] = b.w1;
                    h.board[2] = b.w2;
                    h.board[3] = b.w3;
                    h.t = t;
                    h.alive = alive;
                }
            }
            // B0. Reached by every wave: the branch above is taken on d and t, equal in all of them, and
            // the only code that skips ahead inside it is wave 0's own loop, which ends here too.
            __syncthreads();
            b = uniform_board(r48::Board{h.board[0], h.board[1], h.board[2], h.board[3]});
            t = uniform_word(h.t);
            // h was written before B0 and is not written again before two more barriers: every wave
            // reads the same alive, and all leave or none
            if (uniform_word(h.alive) == 0u)
                break;
            continue;
        }
        Search3Root &rt = root[par];
        float *lf = leaf[par];
        par ^= 1u;
        if (w == 0u)
            nt_root_moves<WAVES>(b, lane, rt);
        // B1. Reached by every wave: nothing between the loop's head and here depends on anything but
        // t and d.
        __syncthreads();
        // rt.legal was written before B1 and is not written again before wave 0 has passed B2 and the
        // barriers of the next deep step: every wave reads the same set, and all leave or none
        const uint32_t lg = uniform_word(rt.legal);
        if (lg == 0u)
            break;   // finished
        const uint64_t M = (uint64_t)uniform_word(rt.slots_lo) | ((uint64_t)uniform_word(rt.slots_hi) << 32);
        const uint32_t kids = 2u * (uint32_t)__popcll(M);   // 4 .. 120
#pragma unroll 1
        for (uint32_t j = w; j < kids;) {   // a wave's own loop: it ends at B2 however many children it took, none included
            const float best = d == 4u ? nt_child_best<L, 3>(rt, M, j, lane, lay, tables, keep + w, nt_stg(cuts...))
                                       : nt_child_best<L, 2>(rt, M, j, lane, lay, tables, keep + w, nt_stg(cuts...));
            uint32_t next = 0u;
            if (lane == 0u) {
                lf[j] = best;   // j < kids <= kSearch3MaxKids
                next = __hip_atomic_fetch_add(&rt.dealt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            j = uniform_word(next);
        }
        // B2, the hand-over: every leaf is stored before it, every wave reads them after it. Reached by
        // every wave: the break above is uniform (lg), the deal loop is left by every wave in the end,
        // and there is no other way out of this step.
        __syncthreads();
        const float qa = nt_finish_rows(rt, lf, M, lg, lane);
        const float q0 = __shfl(qa, 0), q1 = __shfl(qa, 16), q2 = __shfl(qa, 32), q3 = __shfl(qa, 48);
        const r48::StepOut o = r48::nt_play_step(b, r48::nt_argmax4(q0, q1, q2, q3), gid, step0 + t, k0, k1);
        b = uniform_board(b);
        len += uniform_word(o.changed);
        gn += uniform_word(o.reward);
        t++;
    }
    if (w == 0u && lane == 0u)
        nt_play_store(boards, i, b, len, gn, length, gain, done);
}

// ---- carousel shaping: where the next episode of a finished board starts --------------------------
// The carousel contract of r48_ntuple.h, one board per lane: the board and a pool slot are one
// 16-byte load or store each, the flags bytes, the cuts wave-uniform arguments; no LDS. Two kernels,
// launched one after the other on the stream: a restarting board may draw a donor slot whose own
// board records in the same call, and it must read what that slot held before the call.

__device__ __forceinline__ void store_board(int8_t *__restrict__ boards, int64_t i, const r48::Board &b)
{
    *reinterpret_cast<uint4 *>(boards + 16 * i) = make_uint4(b.w0, b.w1, b.w2, b.w3);
}

// Restart phase: the lanes of finished boards only (the others leave at once, and only these make
// the Philox draw). Reads the pool, writes boards[i], turn[i], seen[i] and counts the start.
__global__ __launch_bounds__(kBlock) void k_nt_carousel_restart(int8_t *__restrict__ boards, int64_t n,
                                                                const uint8_t *__restrict__ done, const r48::NtCuts cuts,
                                                                const int8_t *__restrict__ pool,
                                                                const uint8_t *__restrict__ pool_has,
                                                                uint8_t *__restrict__ seen, uint8_t *__restrict__ turn,
                                                                unsigned long long *__restrict__ starts, uint32_t k0,
                                                                uint32_t k1, int64_t gid0, uint32_t ctr)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || done[i] == 0)
        return;
    uint32_t t = r48::nt_carousel_turn(turn[i], cuts);   // 0 .. cuts.n
    r48::Board b;
    if (t > 0u) {
        // j < n: mulhi of a 32-bit word with n <= 2^31 - 1, so at < cuts.n * n, the pool's slots
        const int64_t at = (int64_t)(t - 1u) * n + r48::nt_carousel_donor((uint64_t)(gid0 + i), ctr, k0, k1, (uint32_t)n);
        if (pool_has[at] != 0) {
            b = r48::load_board(pool, at);
            store_board(boards, i, b);
        } else {
            t = 0u;
        }
    }
    if (t == 0u)
        b = r48::load_board(boards, i);   // the env's fresh board stays
    turn[i] = (uint8_t)t;
    seen[i] = (uint8_t)r48::nt_stage(cuts, b);
    if (starts)
        atomicAdd(starts + t, 1ull);
}

// Record phase: a running board that has crossed a cut since its episode was last recorded or started
// goes into its own pool slot of the stage it entered.
__global__ __launch_bounds__(kBlock) void k_nt_carousel_record(const int8_t *__restrict__ boards, int64_t n,
                                                               const uint8_t *__restrict__ done, const r48::NtCuts cuts,
                                                               int8_t *__restrict__ pool, uint8_t *__restrict__ pool_has,
                                                               uint8_t *__restrict__ seen)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || done[i] != 0)
        return;
    const r48::Board b = r48::load_board(boards, i);
    const uint32_t s = r48::nt_stage(cuts, b);   // 0 .. cuts.n
    if (s > seen[i]) {
        const int64_t at = (int64_t)(s - 1u) * n + i;
        store_board(pool, at, b);
        pool_has[at] = 1;
        seen[i] = (uint8_t)s;
    }
}

// ---- the entry points ---------------------------------------------------------------------------

// one pointer argument of an entry point: its name in the message, the alignment it needs, and
// whether it may be NULL
struct PtrArg {
    const char *name;
    const void *p;
    uintptr_t align;
    bool required;
};

// The pointers in the order listed: R48_OK, or R48_EINVAL for the first that is NULL though required
// or misaligned, named in the message.
int check_ptrs(const char *fn, std::initializer_list<PtrArg> ptrs)
{
    for (const PtrArg &a : ptrs) {
        if (!a.p && a.required)
            return fail(R48_EINVAL, std::string(fn) + ": " + a.name + " is NULL");
        if (!aligned(a.p, a.align))
            return fail(R48_EINVAL, std::string(fn) + ": " + a.name + " is not " + std::to_string(a.align) + "-byte aligned");
    }
    return R48_OK;
}

// What every entry point checks first, in this order: boards and n, the layout (expanded into
// lay), then the pointers as listed. R48_OK, or R48_EINVAL with the message set.
int check_args(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
               r48::NtLayout &lay, std::initializer_list<PtrArg> ptrs)
{
    if (!boards || !aligned16(boards) || n < 0)
        return fail(R48_EINVAL, std::string(fn) + ": boards NULL or not 16-byte aligned, or n < 0");
    if (const char *why = r48::nt_expand(cells, m, L, lay))
        return fail(R48_EINVAL, std::string(fn) + ": bad layout: " + why);
    return check_ptrs(fn, ptrs);
}

// What follows the checks: nothing for n == 0, else f(std::integral_constant<int, L>()) launches
// the instantiation for the layout's tuple length.
template <class F>
int run(const char *what, int64_t n, int L, F f)
{
    if (n == 0)
        return R48_OK;
    switch (L) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    default: f(std::integral_constant<int, 6>()); break;
    }
    return launched(what);
}

template <class Kernel, class... A>
void launch(Kernel kernel, dim3 grid, dim3 block, void *stream, const A &...args)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, args...);
}

unsigned long long *words(int64_t *acc) { return reinterpret_cast<unsigned long long *>(acc); }

// The staging of one call: off for the plain entry points and for n_cuts == 0, which run the
// unstaged kernels; else the checked cuts as the staged kernels take them.
struct Staging {
    bool on = false;
    r48::NtCuts cuts{0u, 0};
    NtCutsOwn upd{{0u, 0}, nullptr};
};

// What every staged entry point checks after check_args: the cuts, and own where it updates.
int check_cuts(const char *fn, const uint8_t *cuts, int32_t n_cuts, bool updates, uint8_t *own, Staging &st)
{
    if (const char *why = r48::nt_cuts_check(cuts, n_cuts))
        return fail(R48_EINVAL, std::string(fn) + ": bad cuts: " + why);
    if (updates && n_cuts > 0 && !own)
        return fail(R48_EINVAL, std::string(fn) + ": own is NULL");
    st.on = n_cuts > 0;
    st.cuts = r48::nt_cuts_pack(cuts, n_cuts);
    st.upd = NtCutsOwn{st.cuts, own};
    return R48_OK;
}

// the unstaged kernel with its arguments, or its staged twin with x (the cuts) behind them
template <class Plain, class Staged, class X, class... A>
void launch2(bool staged, Plain plain, Staged twin, dim3 grid, dim3 block, void *stream, const X &x, const A &...args)
{
    if (staged)
        launch(twin, grid, block, stream, args..., x);
    else
        launch(plain, grid, block, stream, args...);
}

// ---- one body per pair of entry points: fn is the name in the messages, cuts / n_cuts / own are
// NULL / 0 / NULL from the plain one --------------------------------------------------------------

int nt_value(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
             const uint8_t *cuts, int32_t n_cuts, const float *tables, float *value, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay, {{"tables", tables, 4, true}, {"value", value, 4, true}}))
        return rc;
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    return run("k_nt_value", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_value<len()>, k_nt_value<len(), r48::NtCuts>, grid_for(n, kBlock), kBlock, stream, st.cuts,
                boards, n, lay, tables, value);
    });
}

int nt_act(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
           const uint8_t *cuts, int32_t n_cuts, const float *tables, int8_t *actions, int8_t *after, float *value,
           int32_t *reward, uint8_t *legal, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"actions", actions, 1, true}, {"after", after, 16, false},
                                   {"value", value, 4, false}, {"reward", reward, 4, false}}))
        return rc;
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    return run("k_nt_act", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_act<len()>, k_nt_act<len(), r48::NtCuts>, grid_for(n, kBlock), kBlock, stream, st.cuts, boards,
                n, lay, tables, actions, after, value, reward, legal);
    });
}

int nt_td_act(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
              const uint8_t *cuts, int32_t n_cuts, const float *tables, const int8_t *prev_after, const float *prev_value,
              const uint8_t *prev_done, const uint8_t *prev_valid, int8_t *actions, int8_t *after, float *value,
              int32_t *reward, uint8_t *legal, uint8_t *valid_out, float *delta_out, int64_t *acc, uint32_t *cnt,
              uint8_t *own, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"prev_after", prev_after, 16, true},
                                   {"prev_value", prev_value, 4, true}, {"prev_done", prev_done, 1, true},
                                   {"prev_valid", prev_valid, 1, true}, {"actions", actions, 1, true},
                                   {"after", after, 16, true}, {"value", value, 4, true}, {"reward", reward, 4, false},
                                   {"legal", legal, 1, true}, {"valid_out", valid_out, 1, true},
                                   {"delta_out", delta_out, 4, false}, {"acc", acc, 8, true}, {"cnt", cnt, 4, true}}))
        return rc;
    if (after == prev_after || value == prev_value || valid_out == prev_valid)
        return fail(R48_EINVAL, std::string(fn) + ": after, value and valid_out must not be the prev_ buffers (apply "
                                                  "reads the previous afterstates and flags after this call; swap the buffers then)");
    if (const int rc = check_cuts(fn, cuts, n_cuts, true, own, st))
        return rc;
    return run("k_nt_td_act", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_td_act<len()>, k_nt_td_act<len(), NtCutsOwn>, grid_for(n, kBlock), kBlock, stream, st.upd,
                boards, n, lay, tables, prev_after, prev_value, prev_done, prev_valid, actions, after, value, reward, legal,
                valid_out, delta_out, words(acc), cnt);
    });
}

int nt_search(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
              const uint8_t *cuts, int32_t n_cuts, const float *tables, int32_t depth, int8_t *actions, float *q,
              uint8_t *legal, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"actions", actions, 1, true}, {"q", q, 4, false}}))
        return rc;
    if (depth != 1 && depth != 2)
        return fail(R48_EINVAL, std::string(fn) + ": depth must be 1 or 2, got " + std::to_string(depth));
    const int64_t blocks = n / kSearchBoards + (n % kSearchBoards ? 1 : 0);   // one board per wave
    if (blocks > 0x7FFFFFFFll)
        return fail(R48_EINVAL, std::string(fn) + ": n = " + std::to_string(n) + " boards exceed the grid (" +
                                    std::to_string(kSearchBoards) + " boards per workgroup, 2^31 - 1 workgroups)");
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    const dim3 grid((unsigned)blocks);
    return run("k_nt_search", n, lay.L, [&](auto len) {
        if (depth == 1)
            launch2(st.on, k_nt_search<len(), 1>, k_nt_search<len(), 1, r48::NtCuts>, grid, kBlock, stream, st.cuts, boards,
                    n, lay, tables, actions, q, legal);
        else
            launch2(st.on, k_nt_search<len(), 2>, k_nt_search<len(), 2, r48::NtCuts>, grid, kBlock, stream, st.cuts, boards,
                    n, lay, tables, actions, q, legal);
    });
}

int nt_search3(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
               const uint8_t *cuts, int32_t n_cuts, const float *tables, int8_t *actions, float *q, uint8_t *legal,
               void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"actions", actions, 1, true}, {"q", q, 4, false}}))
        return rc;
    if (n > 0x7FFFFFFFll)   // one board per workgroup
        return fail(R48_EINVAL, std::string(fn) + ": n = " + std::to_string(n) +
                                    " boards exceed the grid (one per workgroup, 2^31 - 1 workgroups)");
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    const dim3 grid((unsigned)n);
    return run("k_nt_search3", n, lay.L, [&](auto len) {
        if (n <= kSearch3SmallBatch)
            launch2(st.on, k_nt_search3<len(), kSearch3WavesSmall>, k_nt_search3<len(), kSearch3WavesSmall, r48::NtCuts>,
                    grid, 64 * kSearch3WavesSmall, stream, st.cuts, boards, n, lay, tables, actions, q, legal);
        else
            launch2(st.on, k_nt_search3<len(), kSearch3WavesLarge>, k_nt_search3<len(), kSearch3WavesLarge, r48::NtCuts>,
                    grid, 64 * kSearch3WavesLarge, stream, st.cuts, boards, n, lay, tables, actions, q, legal);
    });
}

int nt_search_ruled(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                    const uint8_t *cuts, int32_t n_cuts, const float *tables, const uint8_t *rule, int8_t *actions,
                    float *q, uint8_t *legal, uint8_t *depth_out, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"actions", actions, 1, true}, {"q", q, 4, false}}))
        return rc;
    if (const char *why = r48::nt_rule_check(rule))
        return fail(R48_EINVAL, std::string(fn) + ": bad rule: " + why);
    if (n > 0x7FFFFFFFll)   // one board per workgroup
        return fail(R48_EINVAL, std::string(fn) + ": n = " + std::to_string(n) +
                                    " boards exceed the grid (one per workgroup, 2^31 - 1 workgroups)");
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    const uint64_t packed = r48::nt_rule_pack(rule);
    const dim3 grid((unsigned)n);
    return run("k_nt_search_ruled", n, lay.L, [&](auto len) {
        if (n <= kSearch3SmallBatch)
            launch2(st.on, k_nt_search_ruled<len(), kSearch3WavesSmall>,
                    k_nt_search_ruled<len(), kSearch3WavesSmall, r48::NtCuts>, grid, 64 * kSearch3WavesSmall, stream, st.cuts,
                    boards, n, lay, tables, packed, actions, q, legal, depth_out);
        else
            launch2(st.on, k_nt_search_ruled<len(), kSearch3WavesLarge>,
                    k_nt_search_ruled<len(), kSearch3WavesLarge, r48::NtCuts>, grid, 64 * kSearch3WavesLarge, stream, st.cuts,
                    boards, n, lay, tables, packed, actions, q, legal, depth_out);
    });
}

int nt_play(const char *fn, int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const uint8_t *cuts,
            int32_t n_cuts, const float *tables, int32_t depth, int32_t n_steps, uint64_t env_seed, int64_t gid0,
            uint32_t env_step, int32_t *length, int32_t *gain, uint8_t *done, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"length", length, 4, false}, {"gain", gain, 4, false}}))
        return rc;
    if (depth != 1 && depth != 2)
        return fail(R48_EINVAL, std::string(fn) + ": depth must be 1 or 2, got " + std::to_string(depth));
    if (n_steps < 0)
        return fail(R48_EINVAL, std::string(fn) + ": n_steps must not be negative, got " + std::to_string(n_steps));
    const int64_t per = depth == 2 ? kSearchBoards : kBlock / kPlayLanes;   // boards per workgroup
    const int64_t blocks = n / per + (n % per ? 1 : 0);
    if (blocks > 0x7FFFFFFFll)
        return fail(R48_EINVAL, std::string(fn) + ": n = " + std::to_string(n) + " boards exceed the grid (" +
                                    std::to_string(per) + " boards per workgroup, 2^31 - 1 workgroups)");
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    if (n_steps == 0)
        return R48_OK;
    const dim3 grid((unsigned)blocks);
    const uint32_t k0 = (uint32_t)env_seed, k1 = (uint32_t)(env_seed >> 32);
    return run("k_nt_play", n, lay.L, [&](auto len) {
        if (depth == 1)
            launch2(st.on, k_nt_play1<len(), kPlayLanes>, k_nt_play1<len(), kPlayLanes, r48::NtCuts>, grid, kBlock, stream,
                    st.cuts, boards, n, lay, tables, n_steps, k0, k1, gid0, env_step, length, gain, done);
        else
            launch2(st.on, k_nt_play2<len()>, k_nt_play2<len(), r48::NtCuts>, grid, kBlock, stream, st.cuts, boards, n, lay,
                    tables, n_steps, k0, k1, gid0, env_step, length, gain, done);
    });
}

int nt_play_ruled(const char *fn, int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                  const uint8_t *cuts, int32_t n_cuts, const float *tables, const uint8_t *rule, int32_t n_steps,
                  uint64_t env_seed, int64_t gid0, uint32_t env_step, int32_t *length, int32_t *gain, uint8_t *done,
                  void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"length", length, 4, false}, {"gain", gain, 4, false}}))
        return rc;
    if (const char *why = r48::nt_rule_check(rule))
        return fail(R48_EINVAL, std::string(fn) + ": bad rule: " + why);
    if (n_steps < 0)
        return fail(R48_EINVAL, std::string(fn) + ": n_steps must not be negative, got " + std::to_string(n_steps));
    if (n > 0x7FFFFFFFll)   // one board per workgroup
        return fail(R48_EINVAL, std::string(fn) + ": n = " + std::to_string(n) +
                                    " boards exceed the grid (one per workgroup, 2^31 - 1 workgroups)");
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    if (n_steps == 0)
        return R48_OK;
    const uint64_t packed = r48::nt_rule_pack(rule);
    const dim3 grid((unsigned)n);
    const uint32_t k0 = (uint32_t)env_seed, k1 = (uint32_t)(env_seed >> 32);
    return run("k_nt_play_ruled", n, lay.L, [&](auto len) {
        if (n <= kSearch3SmallBatch)
            launch2(st.on, k_nt_play_ruled<len(), kPlayRuledWavesSmall>,
                    k_nt_play_ruled<len(), kPlayRuledWavesSmall, r48::NtCuts>, grid, 64 * kPlayRuledWavesSmall, stream,
                    st.cuts, boards, n, lay, tables, packed, n_steps, k0, k1, gid0, env_step, length, gain, done);
        else
            launch2(st.on, k_nt_play_ruled<len(), kPlayRuledWavesLarge>,
                    k_nt_play_ruled<len(), kPlayRuledWavesLarge, r48::NtCuts>, grid, 64 * kPlayRuledWavesLarge, stream,
                    st.cuts, boards, n, lay, tables, packed, n_steps, k0, k1, gid0, env_step, length, gain, done);
    });
}

int nt_accumulate(const char *fn, const int8_t *boards, int64_t n, const float *delta, const uint8_t *valid,
                  const uint8_t *cells, int32_t m, int32_t L, const uint8_t *cuts, int32_t n_cuts, int64_t *acc,
                  uint32_t *cnt, uint8_t *own, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"delta", delta, 4, true}, {"acc", acc, 8, true}, {"cnt", cnt, 4, true}}))
        return rc;
    if (const int rc = check_cuts(fn, cuts, n_cuts, true, own, st))
        return rc;
    return run("k_nt_accumulate", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_accumulate<len()>, k_nt_accumulate<len(), NtCutsOwn>, grid_for(n, kBlock), kBlock, stream,
                st.upd, boards, n, delta, valid, lay, words(acc), cnt);
    });
}

int nt_apply(const char *fn, const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m,
             int32_t L, const uint8_t *cuts, int32_t n_cuts, float step, float *tables, int64_t *acc, uint32_t *cnt,
             uint8_t *own, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"acc", acc, 8, true}, {"cnt", cnt, 4, true}}))
        return rc;
    if (const int rc = check_cuts(fn, cuts, n_cuts, true, own, st))
        return rc;
    return run("k_nt_apply", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_apply<len()>, k_nt_apply<len(), NtCutsOwn>, grid_for(n, kBlock), kBlock, stream, st.upd, boards,
                n, valid, lay, step, tables, words(acc), cnt);
    });
}

int nt_apply_tc(const char *fn, const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m,
                int32_t L, const uint8_t *cuts, int32_t n_cuts, float step, float *tables, float *tc_e, float *tc_a,
                int64_t *acc, uint32_t *cnt, uint8_t *own, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"tc_e", tc_e, 4, true}, {"tc_a", tc_a, 4, true},
                                   {"acc", acc, 8, true}, {"cnt", cnt, 4, true}}))
        return rc;
    if (const int rc = check_cuts(fn, cuts, n_cuts, true, own, st))
        return rc;
    return run("k_nt_apply_tc", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_apply_tc<len()>, k_nt_apply_tc<len(), NtCutsOwn>, grid_for(n, kBlock), kBlock, stream, st.upd,
                boards, n, valid, lay, step, tables, tc_e, tc_a, words(acc), cnt);
    });
}

// ---- the replica entry points: what the parents check, then the replicas (r48_ntuple.h) ---------

// What every replica entry point checks after check_args: replicas, n and the entry count.
int check_replicas(const char *fn, int64_t n, int32_t replicas, const r48::NtLayout &lay)
{
    if (const char *why = r48::nt_replicas_check(n, replicas, lay.m, lay.L))
        return fail(R48_EINVAL, std::string(fn) + ": bad replicas (" + std::to_string(replicas) + " for n = " +
                                    std::to_string(n) + "): " + why);
    return R48_OK;
}

// entries of one replica, m << 4L (at most 2^27)
uint32_t replica_size(const r48::NtLayout &lay) { return (uint32_t)lay.m << (4 * lay.L); }

int nt_td_act_replicas(const char *fn, const int8_t *boards, int64_t n, int32_t replicas, const uint8_t *cells, int32_t m,
                       int32_t L, const float *tables, const int8_t *prev_after, const float *prev_value,
                       const uint8_t *prev_done, const uint8_t *prev_valid, int8_t *actions, int8_t *after, float *value,
                       int32_t *reward, uint8_t *legal, uint8_t *valid_out, float *delta_out, int64_t *acc, uint32_t *cnt,
                       void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tables", tables, 4, true}, {"prev_after", prev_after, 16, true},
                                   {"prev_value", prev_value, 4, true}, {"prev_done", prev_done, 1, true},
                                   {"prev_valid", prev_valid, 1, true}, {"actions", actions, 1, true},
                                   {"after", after, 16, true}, {"value", value, 4, true}, {"reward", reward, 4, false},
                                   {"legal", legal, 1, true}, {"valid_out", valid_out, 1, true},
                                   {"delta_out", delta_out, 4, false}, {"acc", acc, 8, true}, {"cnt", cnt, 4, true}}))
        return rc;
    if (after == prev_after || value == prev_value || valid_out == prev_valid)
        return fail(R48_EINVAL, std::string(fn) + ": after, value and valid_out must not be the prev_ buffers (apply "
                                                  "reads the previous afterstates and flags after this call; swap the buffers then)");
    if (const int rc = check_replicas(fn, n, replicas, lay))
        return rc;
    return run("k_nt_td_act_rep", n, lay.L, [&](auto len) {
        launch(k_nt_td_act_rep<len()>, grid_for(n, kBlock), kBlock, stream, boards, n, n / replicas, replica_size(lay), lay,
               tables, prev_after, prev_value, prev_done, prev_valid, actions, after, value, reward, legal, valid_out,
               delta_out, words(acc), cnt);
    });
}

int nt_apply_replicas(const char *fn, const int8_t *boards, int64_t n, int32_t replicas, const uint8_t *valid,
                      const uint8_t *cells, int32_t m, int32_t L, const float *steps, float *tables, float *tc_e,
                      float *tc_a, bool tc, int64_t *acc, uint32_t *cnt, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay, {{"steps", steps, 4, true}, {"tables", tables, 4, true}}))
        return rc;
    if (tc)
        if (const int rc = check_ptrs(fn, {{"tc_e", tc_e, 4, true}, {"tc_a", tc_a, 4, true}}))
            return rc;
    if (const int rc = check_ptrs(fn, {{"acc", acc, 8, true}, {"cnt", cnt, 4, true}}))
        return rc;
    if (const int rc = check_replicas(fn, n, replicas, lay))
        return rc;
    return run(tc ? "k_nt_apply_tc_rep" : "k_nt_apply_rep", n, lay.L, [&](auto len) {
        if (tc)
            launch(k_nt_apply_tc_rep<len()>, grid_for(n, kBlock), kBlock, stream, boards, n, n / replicas, replica_size(lay),
                   valid, lay, steps, tables, tc_e, tc_a, words(acc), cnt);
        else
            launch(k_nt_apply_rep<len()>, grid_for(n, kBlock), kBlock, stream, boards, n, n / replicas, replica_size(lay),
                   valid, lay, steps, tables, words(acc), cnt);
    });
}

int nt_tc_rate(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
               const uint8_t *cuts, int32_t n_cuts, const float *tc_e, const float *tc_a, float *rate_out, void *stream)
{
    r48::NtLayout lay;
    Staging st;
    if (const int rc = check_args(fn, boards, n, cells, m, L, lay,
                                  {{"tc_e", tc_e, 4, true}, {"tc_a", tc_a, 4, true}, {"rate_out", rate_out, 4, true}}))
        return rc;
    if (const int rc = check_cuts(fn, cuts, n_cuts, false, nullptr, st))
        return rc;
    return run("k_nt_tc_rate", n, lay.L, [&](auto len) {
        launch2(st.on, k_nt_tc_rate<len()>, k_nt_tc_rate<len(), r48::NtCuts>, grid_for(n, kBlock), kBlock, stream, st.cuts,
                boards, n, lay, tc_e, tc_a, rate_out);
    });
}

int nt_carousel(const char *fn, int8_t *boards, int64_t n, const uint8_t *done, const uint8_t *cuts, int32_t n_cuts,
                int8_t *pool, uint8_t *pool_has, uint8_t *seen, uint8_t *turn, uint64_t *starts, uint64_t seed, int64_t gid0,
                uint32_t ctr, void *stream)
{
    if (const int rc = check_ptrs(fn, {{"boards", boards, 16, true}, {"done", done, 1, true}, {"cuts", cuts, 1, true},
                                       {"pool", pool, 16, true}, {"pool_has", pool_has, 1, true}, {"seen", seen, 1, true},
                                       {"turn", turn, 1, true}, {"starts", starts, 8, false}}))
        return rc;
    if (n < 0 || n > 0x7FFFFFFFll)
        return fail(R48_EINVAL, std::string(fn) + ": n = " + std::to_string(n) + " boards, must be 0 .. 2^31 - 1 (the donor is a 32-bit draw)");
    if (const char *why = r48::nt_carousel_cuts_check(cuts, n_cuts))
        return fail(R48_EINVAL, std::string(fn) + ": bad cuts: " + why);
    if (n == 0)
        return R48_OK;
    const r48::NtCuts c = r48::nt_cuts_pack(cuts, n_cuts);
    launch(k_nt_carousel_restart, grid_for(n, kBlock), kBlock, stream, boards, n, done, c, (const int8_t *)pool,
           (const uint8_t *)pool_has, seen, turn, reinterpret_cast<unsigned long long *>(starts), (uint32_t)seed,
           (uint32_t)(seed >> 32), gid0, ctr);
    if (const int rc = launched("k_nt_carousel_restart"))
        return rc;
    launch(k_nt_carousel_record, grid_for(n, kBlock), kBlock, stream, (const int8_t *)boards, n, done, c, pool, pool_has,
           seen);
    return launched("k_nt_carousel_record");
}

}  // namespace

extern "C" {

int r48_ntuple_value(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                     float *value, void *stream)
{
    return nt_value("r48_ntuple_value", boards, n, cells, m, L, nullptr, 0, tables, value, stream);
}

int r48_ntuple_value_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                            const uint8_t *cuts, int32_t n_cuts, const float *tables, float *value, void *stream)
{
    return nt_value("r48_ntuple_value_staged", boards, n, cells, m, L, cuts, n_cuts, tables, value, stream);
}

int r48_ntuple_act(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                   int8_t *actions, int8_t *after, float *value, int32_t *reward, uint8_t *legal, void *stream)
{
    return nt_act("r48_ntuple_act", boards, n, cells, m, L, nullptr, 0, tables, actions, after, value, reward, legal, stream);
}

int r48_ntuple_act_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                          const uint8_t *cuts, int32_t n_cuts, const float *tables, int8_t *actions, int8_t *after,
                          float *value, int32_t *reward, uint8_t *legal, void *stream)
{
    return nt_act("r48_ntuple_act_staged", boards, n, cells, m, L, cuts, n_cuts, tables, actions, after, value, reward, legal,
                  stream);
}

int r48_ntuple_td_act(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                      const int8_t *prev_after, const float *prev_value, const uint8_t *prev_done,
                      const uint8_t *prev_valid, int8_t *actions, int8_t *after, float *value, int32_t *reward,
                      uint8_t *legal, uint8_t *valid_out, float *delta_out, int64_t *acc, uint32_t *cnt, void *stream)
{
    return nt_td_act("r48_ntuple_td_act", boards, n, cells, m, L, nullptr, 0, tables, prev_after, prev_value, prev_done,
                     prev_valid, actions, after, value, reward, legal, valid_out, delta_out, acc, cnt, nullptr, stream);
}

int r48_ntuple_td_act_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                             const uint8_t *cuts, int32_t n_cuts, const float *tables, const int8_t *prev_after,
                             const float *prev_value, const uint8_t *prev_done, const uint8_t *prev_valid,
                             int8_t *actions, int8_t *after, float *value, int32_t *reward, uint8_t *legal,
                             uint8_t *valid_out, float *delta_out, int64_t *acc, uint32_t *cnt, uint8_t *own, void *stream)
{
    return nt_td_act("r48_ntuple_td_act_staged", boards, n, cells, m, L, cuts, n_cuts, tables, prev_after, prev_value,
                     prev_done, prev_valid, actions, after, value, reward, legal, valid_out, delta_out, acc, cnt, own, stream);
}

int r48_ntuple_search(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                      int32_t depth, int8_t *actions, float *q, uint8_t *legal, void *stream)
{
    return nt_search("r48_ntuple_search", boards, n, cells, m, L, nullptr, 0, tables, depth, actions, q, legal, stream);
}

int r48_ntuple_search_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                             const uint8_t *cuts, int32_t n_cuts, const float *tables, int32_t depth, int8_t *actions,
                             float *q, uint8_t *legal, void *stream)
{
    return nt_search("r48_ntuple_search_staged", boards, n, cells, m, L, cuts, n_cuts, tables, depth, actions, q, legal,
                     stream);
}

int r48_ntuple_search3(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                       const float *tables, int8_t *actions, float *q, uint8_t *legal, void *stream)
{
    return nt_search3("r48_ntuple_search3", boards, n, cells, m, L, nullptr, 0, tables, actions, q, legal, stream);
}

int r48_ntuple_search3_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                              const uint8_t *cuts, int32_t n_cuts, const float *tables, int8_t *actions, float *q,
                              uint8_t *legal, void *stream)
{
    return nt_search3("r48_ntuple_search3_staged", boards, n, cells, m, L, cuts, n_cuts, tables, actions, q, legal, stream);
}

int r48_ntuple_search_ruled(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                            const float *tables, const uint8_t *rule, int8_t *actions, float *q, uint8_t *legal,
                            uint8_t *depth_out, void *stream)
{
    return nt_search_ruled("r48_ntuple_search_ruled", boards, n, cells, m, L, nullptr, 0, tables, rule, actions, q, legal,
                           depth_out, stream);
}

int r48_ntuple_search_ruled_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                                   const uint8_t *cuts, int32_t n_cuts, const float *tables, const uint8_t *rule,
                                   int8_t *actions, float *q, uint8_t *legal, uint8_t *depth_out, void *stream)
{
    return nt_search_ruled("r48_ntuple_search_ruled_staged", boards, n, cells, m, L, cuts, n_cuts, tables, rule, actions, q,
                           legal, depth_out, stream);
}

int r48_ntuple_play(int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                    int32_t depth, int32_t n_steps, uint64_t env_seed, int64_t gid0, uint32_t env_step, int32_t *length,
                    int32_t *gain, uint8_t *done, void *stream)
{
    return nt_play("r48_ntuple_play", boards, n, cells, m, L, nullptr, 0, tables, depth, n_steps, env_seed, gid0, env_step,
                   length, gain, done, stream);
}

int r48_ntuple_play_staged(int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const uint8_t *cuts,
                           int32_t n_cuts, const float *tables, int32_t depth, int32_t n_steps, uint64_t env_seed,
                           int64_t gid0, uint32_t env_step, int32_t *length, int32_t *gain, uint8_t *done, void *stream)
{
    return nt_play("r48_ntuple_play_staged", boards, n, cells, m, L, cuts, n_cuts, tables, depth, n_steps, env_seed, gid0,
                   env_step, length, gain, done, stream);
}

int r48_ntuple_play_ruled(int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                          const uint8_t *rule, int32_t n_steps, uint64_t env_seed, int64_t gid0, uint32_t env_step,
                          int32_t *length, int32_t *gain, uint8_t *done, void *stream)
{
    return nt_play_ruled("r48_ntuple_play_ruled", boards, n, cells, m, L, nullptr, 0, tables, rule, n_steps, env_seed, gid0,
                         env_step, length, gain, done, stream);
}

int r48_ntuple_play_ruled_staged(int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                                 const uint8_t *cuts, int32_t n_cuts, const float *tables, const uint8_t *rule,
                                 int32_t n_steps, uint64_t env_seed, int64_t gid0, uint32_t env_step, int32_t *length,
                                 int32_t *gain, uint8_t *done, void *stream)
{
    return nt_play_ruled("r48_ntuple_play_ruled_staged", boards, n, cells, m, L, cuts, n_cuts, tables, rule, n_steps, env_seed,
                         gid0, env_step, length, gain, done, stream);
}

int r48_ntuple_accumulate(const int8_t *boards, int64_t n, const float *delta, const uint8_t *valid,
                          const uint8_t *cells, int32_t m, int32_t L, int64_t *acc, uint32_t *cnt, void *stream)
{
    return nt_accumulate("r48_ntuple_accumulate", boards, n, delta, valid, cells, m, L, nullptr, 0, acc, cnt, nullptr, stream);
}

int r48_ntuple_accumulate_staged(const int8_t *boards, int64_t n, const float *delta, const uint8_t *valid,
                                 const uint8_t *cells, int32_t m, int32_t L, const uint8_t *cuts, int32_t n_cuts,
                                 int64_t *acc, uint32_t *cnt, uint8_t *own, void *stream)
{
    return nt_accumulate("r48_ntuple_accumulate_staged", boards, n, delta, valid, cells, m, L, cuts, n_cuts, acc, cnt, own,
                         stream);
}

int r48_ntuple_apply(const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m, int32_t L,
                     float step, float *tables, int64_t *acc, uint32_t *cnt, void *stream)
{
    return nt_apply("r48_ntuple_apply", boards, n, valid, cells, m, L, nullptr, 0, step, tables, acc, cnt, nullptr, stream);
}

int r48_ntuple_apply_staged(const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m,
                            int32_t L, const uint8_t *cuts, int32_t n_cuts, float step, float *tables, int64_t *acc,
                            uint32_t *cnt, uint8_t *own, void *stream)
{
    return nt_apply("r48_ntuple_apply_staged", boards, n, valid, cells, m, L, cuts, n_cuts, step, tables, acc, cnt, own,
                    stream);
}

int r48_ntuple_apply_tc(const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m,
                        int32_t L, float step, float *tables, float *tc_e, float *tc_a, int64_t *acc, uint32_t *cnt,
                        void *stream)
{
    return nt_apply_tc("r48_ntuple_apply_tc", boards, n, valid, cells, m, L, nullptr, 0, step, tables, tc_e, tc_a, acc, cnt,
                       nullptr, stream);
}

int r48_ntuple_apply_tc_staged(const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m,
                               int32_t L, const uint8_t *cuts, int32_t n_cuts, float step, float *tables, float *tc_e,
                               float *tc_a, int64_t *acc, uint32_t *cnt, uint8_t *own, void *stream)
{
    return nt_apply_tc("r48_ntuple_apply_tc_staged", boards, n, valid, cells, m, L, cuts, n_cuts, step, tables, tc_e, tc_a,
                       acc, cnt, own, stream);
}

int r48_ntuple_td_act_replicas(const int8_t *boards, int64_t n, int32_t replicas, const uint8_t *cells, int32_t m,
                               int32_t L, const float *tables, const int8_t *prev_after, const float *prev_value,
                               const uint8_t *prev_done, const uint8_t *prev_valid, int8_t *actions, int8_t *after,
                               float *value, int32_t *reward, uint8_t *legal, uint8_t *valid_out, float *delta_out,
                               int64_t *acc, uint32_t *cnt, void *stream)
{
    return nt_td_act_replicas("r48_ntuple_td_act_replicas", boards, n, replicas, cells, m, L, tables, prev_after, prev_value,
                              prev_done, prev_valid, actions, after, value, reward, legal, valid_out, delta_out, acc, cnt,
                              stream);
}

int r48_ntuple_apply_replicas(const int8_t *boards, int64_t n, int32_t replicas, const uint8_t *valid, const uint8_t *cells,
                              int32_t m, int32_t L, const float *steps, float *tables, int64_t *acc, uint32_t *cnt,
                              void *stream)
{
    return nt_apply_replicas("r48_ntuple_apply_replicas", boards, n, replicas, valid, cells, m, L, steps, tables, nullptr,
                             nullptr, false, acc, cnt, stream);
}

int r48_ntuple_apply_tc_replicas(const int8_t *boards, int64_t n, int32_t replicas, const uint8_t *valid,
                                 const uint8_t *cells, int32_t m, int32_t L, const float *steps, float *tables, float *tc_e,
                                 float *tc_a, int64_t *acc, uint32_t *cnt, void *stream)
{
    return nt_apply_replicas("r48_ntuple_apply_tc_replicas", boards, n, replicas, valid, cells, m, L, steps, tables, tc_e,
                             tc_a, true, acc, cnt, stream);
}

int r48_ntuple_tc_rate(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tc_e,
                       const float *tc_a, float *rate_out, void *stream)
{
    return nt_tc_rate("r48_ntuple_tc_rate", boards, n, cells, m, L, nullptr, 0, tc_e, tc_a, rate_out, stream);
}

int r48_ntuple_tc_rate_staged(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                              const uint8_t *cuts, int32_t n_cuts, const float *tc_e, const float *tc_a, float *rate_out,
                              void *stream)
{
    return nt_tc_rate("r48_ntuple_tc_rate_staged", boards, n, cells, m, L, cuts, n_cuts, tc_e, tc_a, rate_out, stream);
}

int r48_ntuple_carousel(int8_t *boards, int64_t n, const uint8_t *done, const uint8_t *cuts, int32_t n_cuts, int8_t *pool,
                        uint8_t *pool_has, uint8_t *seen, uint8_t *turn, uint64_t *starts, uint64_t seed, int64_t gid0,
                        uint32_t ctr, void *stream)
{
    return nt_carousel("r48_ntuple_carousel", boards, n, done, cuts, n_cuts, pool, pool_has, seen, turn, starts, seed, gid0,
                       ctr, stream);
}

}  // extern "C"
