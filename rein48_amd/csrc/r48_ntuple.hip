// r48_ntuple.hip -- the n-tuple network (r48_ntuple.h) behind include/rein48.h: value, the fused
// one-ply afterstate search, and the two halves of the per-entry-mean TD update. Stateless like
// r48_moves.hip: plain device pointers plus the layout's cells on the host.
//
//   k_nt_value       board -> V(board): 8m table gathers, fp32 sum in the header's fixed order
//   k_nt_act         board -> the four moves in registers (move_rows4), V of the legal ones only,
//                    argmax of reward + V with ties to the lowest code; writes the chosen move's
//                    afterstate / V / reward and the legal set. No afterstate plane goes through
//                    HBM on the way to the values.
//   k_nt_accumulate  every hit (i, t, g) of a valid board: cnt[e] += 1, acc[e] += delta_i in
//                    fixed point (2^-16) -- integer atomics, so the sums do not depend on order
//   k_nt_td_act      k_nt_act on the env boards and, in the same launch, the trainer's TD error and
//                    k_nt_accumulate for the previous step's afterstates: the fused training step
//   k_nt_apply       every hit again: the one lane whose exchange takes the entry's count also
//                    takes its sum and moves tables[e] by step * mean delta, once; both scratch
//                    words are zero afterwards. No float atomics: bitwise reproducible.
//   k_nt_apply_tc    apply with temporal-coherence learning rates: the owner lane also owns the
//                    entry's error sums E[e], A[e] and scales its step by |E| / A
//   k_nt_tc_rate     board -> the mean learning rate |E| / A over its 8m hits (read-only)
//   k_nt_search      board -> the four action values Q and their first argmax at depth 1 (act's
//                    scores) or depth 2 (expectimax over the tile spawn); one board per WAVE
//   k_nt_search3     the same three plies deep: one board per WORKGROUP, whose waves search the
//                    board's children with depth 2's wave-level routine
// Otherwise one board per lane, one 16-byte board load; templated on the tuple length L so the cell loops
// unroll; the expanded layout travels by value in the kernel arguments (wave-uniform).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rein48.h"
#include "r48_board.h"
#include "r48_ntuple.h"
#include "r48_select.h"

namespace r48 {
void set_last_error(const std::string &msg);
}

namespace {

constexpr int kBlock = 256;
constexpr float kFixedOne = r48::kNtFixedOne;   // acc counts delta in units of 2^-16 (nt_fixed_delta)

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

int fail(int code, const std::string &msg)
{
    r48::set_last_error(msg);
    return code;
}

int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        r48::set_last_error(std::string(what) + ": " + hipGetErrorString(e));
        return R48_EHIP;
    }
    return R48_OK;
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_value(const int8_t *__restrict__ boards, int64_t n,
                                                     const r48::NtLayout lay, const float *__restrict__ tables,
                                                     float *__restrict__ value)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    value[i] = r48::nt_value<L>(r48::nt_pack(r48::load_board(boards, i)), lay, tables);
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_act(const int8_t *__restrict__ boards, int64_t n,
                                                   const r48::NtLayout lay, const float *__restrict__ tables,
                                                   int8_t *__restrict__ actions, int8_t *__restrict__ after,
                                                   float *__restrict__ value, int32_t *__restrict__ reward,
                                                   uint8_t *__restrict__ legal)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::Board b = r48::load_board(boards, i);
    const r48::Moves4 m = r48::move_rows4<true>(b);
    const uint32_t lg = (r48::differs(m.up, b) ? 1u : 0u) | (r48::differs(m.down, b) ? 2u : 0u) |
                        (r48::differs(m.left, b) ? 4u : 0u) | (r48::differs(m.right, b) ? 8u : 0u);
    // no legal move: action 0, the board itself, value 0, reward 0
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
        const float v = r48::nt_value<L>(r48::nt_pack(c), lay, tables);
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
    actions[i] = (int8_t)best_a;
    if (after)
        *reinterpret_cast<uint4 *>(after + 16 * i) = make_uint4(best_b.w0, best_b.w1, best_b.w2, best_b.w3);
    if (value)
        value[i] = best_v;
    if (reward)
        reward[i] = (int32_t)best_r;
    if (legal)
        legal[i] = (uint8_t)lg;
}

// One env step's act and the accumulate half of the TD update for the PREVIOUS afterstates, in one
// launch (the trainer's fused step; apply and the env step follow as their own launches, apply
// needs every sum finished). Lane i:
//   - loads its env board, and issues the loads of its previous afterstate, value, done and valid
//     flags right behind it: nothing needs them before the search is over, so they are in flight
//     under it
//   - runs k_nt_act's search, statement for statement (the same move_rows4, nt_value and
//     first-maximiser rule: the same bits; written out again so that k_nt_act and its code
//     objects stay what they are), and writes the chosen move's outputs; valid_out = the board
//     had a move, i.e. this afterstate can be learned from at the next step
//   - forms delta = nt_td_delta(...) from this step's reward and value, in registers
//   - where prev_valid: walks the 8m hits of the previous afterstate with k_nt_accumulate's two
//     integer atomics per hit
// tables is only read: acc and cnt are the only words two lanes share, and integer sums do not
// depend on their order, so the launch computes what act, the torch expression for delta and
// accumulate compute one after another, bit for bit. after / value / valid_out must not be the
// prev_ buffers (the entry point refuses it): apply reads the old ones after this kernel.
template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_td_act(
    const int8_t *__restrict__ boards, int64_t n, const r48::NtLayout lay, const float *__restrict__ tables,
    const int8_t *__restrict__ prev_after, const float *__restrict__ prev_value, const uint8_t *__restrict__ prev_done,
    const uint8_t *__restrict__ prev_valid, int8_t *__restrict__ actions, int8_t *__restrict__ after,
    float *__restrict__ value, int32_t *__restrict__ reward, uint8_t *__restrict__ legal, uint8_t *__restrict__ valid_out,
    float *__restrict__ delta_out, unsigned long long *__restrict__ acc, uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    const r48::Board b = r48::load_board(boards, i);
    const r48::Board pb = r48::load_board(prev_after, i);
    const float pv = prev_value[i];
    const uint32_t pd = prev_done[i], pok = prev_valid[i];
    const r48::Moves4 m = r48::move_rows4<true>(b);
    const uint32_t lg = r48::nt_legal4(m, b);
    // no legal move: action 0, the board itself, value 0, reward 0
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
        const float v = r48::nt_value<L>(r48::nt_pack(c), lay, tables);
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
    actions[i] = (int8_t)best_a;
    *reinterpret_cast<uint4 *>(after + 16 * i) = make_uint4(best_b.w0, best_b.w1, best_b.w2, best_b.w3);
    value[i] = best_v;
    if (reward)
        reward[i] = (int32_t)best_r;
    legal[i] = (uint8_t)lg;
    valid_out[i] = lg != 0u ? 1 : 0;
    const float delta = r48::nt_td_delta(pd, best_r, best_v, pv);
    if (delta_out)
        delta_out[i] = delta;
    if (!pok)
        return;
    const r48::NtBoard p = r48::nt_pack(pb);
    const unsigned long long q = (unsigned long long)r48::nt_fixed_delta(delta);   // two's complement: wraps as int64 adds
    for (int t = 0; t < lay.m; t++) {
#pragma unroll
        for (int g = 0; g < r48::kNtSyms; g++) {
            const uint32_t e = r48::nt_entry<L>(p, lay, r48::kNtSyms * t + g);
            atomicAdd(&cnt[e], 1u);
            atomicAdd(&acc[e], q);
        }
    }
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_accumulate(const int8_t *__restrict__ boards, int64_t n,
                                                          const float *__restrict__ delta,
                                                          const uint8_t *__restrict__ valid, const r48::NtLayout lay,
                                                          unsigned long long *__restrict__ acc,
                                                          uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const r48::NtBoard b = r48::nt_pack(r48::load_board(boards, i));
    const unsigned long long q = (unsigned long long)r48::nt_fixed_delta(delta[i]);   // two's complement: wraps as int64 adds
    for (int t = 0; t < lay.m; t++) {
#pragma unroll
        for (int g = 0; g < r48::kNtSyms; g++) {
            const uint32_t e = r48::nt_entry<L>(b, lay, r48::kNtSyms * t + g);
            atomicAdd(&cnt[e], 1u);
            atomicAdd(&acc[e], q);
        }
    }
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_apply(const int8_t *__restrict__ boards, int64_t n,
                                                     const uint8_t *__restrict__ valid, const r48::NtLayout lay,
                                                     float step, float *__restrict__ tables,
                                                     unsigned long long *__restrict__ acc, uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const r48::NtBoard b = r48::nt_pack(r48::load_board(boards, i));
    for (int t = 0; t < lay.m; t++) {
#pragma unroll
        for (int g = 0; g < r48::kNtSyms; g++) {
            const uint32_t e = r48::nt_entry<L>(b, lay, r48::kNtSyms * t + g);
            const uint32_t c = atomicExch(&cnt[e], 0u);
            if (c != 0u) {
                // the only lane of this launch that sees a count for e: it owns tables[e]
                const long long a = (long long)atomicExch(&acc[e], 0ull);
                tables[e] += step * (((float)a * (1.0f / kFixedOne)) / (float)c);
            }
        }
    }
}

// apply with temporal-coherence learning rates (r48_ntuple.h): the lane that takes an entry's
// count owns tables[e], E[e] and A[e] for this launch. Its three loads are issued together, the
// rule runs in registers, three plain stores follow. The sums are order-free integers and the
// owner's arithmetic does not depend on which lane it is, so all three tables are bitwise
// reproducible and independent of the boards' order in the batch.
template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_apply_tc(const int8_t *__restrict__ boards, int64_t n,
                                                        const uint8_t *__restrict__ valid, const r48::NtLayout lay,
                                                        float step, float *__restrict__ tables,
                                                        float *__restrict__ tc_e, float *__restrict__ tc_a,
                                                        unsigned long long *__restrict__ acc,
                                                        uint32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || (valid && !valid[i]))
        return;
    const r48::NtBoard b = r48::nt_pack(r48::load_board(boards, i));
    for (int t = 0; t < lay.m; t++) {
#pragma unroll
        for (int g = 0; g < r48::kNtSyms; g++) {
            const uint32_t e = r48::nt_entry<L>(b, lay, r48::kNtSyms * t + g);
            const uint32_t c = atomicExch(&cnt[e], 0u);
            if (c != 0u) {
                float w = tables[e], se = tc_e[e], sa = tc_a[e];
                const long long a = (long long)atomicExch(&acc[e], 0ull);
                r48::nt_tc_update(w, se, sa, r48::nt_mean(a, c), step);
                tables[e] = w;
                tc_e[e] = se;
                tc_a[e] = sa;
            }
        }
    }
}

// How settled the network is on a set of boards: the mean learning rate over each board's hits.
template <int L>
__global__ __launch_bounds__(kBlock) void k_nt_tc_rate(const int8_t *__restrict__ boards, int64_t n,
                                                       const r48::NtLayout lay, const float *__restrict__ tc_e,
                                                       const float *__restrict__ tc_a, float *__restrict__ rate_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n)
        return;
    rate_out[i] = r48::nt_tc_rate_mean<L>(r48::nt_pack(r48::load_board(boards, i)), lay, tc_e, tc_a);
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

// The depth-2 search of a board that every lane of the wave holds (the comment above): the
// lane's Q_2 of its row's move (-inf where the move is illegal) and the board's legal set. Shared
// by k_nt_search<L, 2>, whose board is the batch's, and k_nt_search3, whose boards are the root's
// children.
template <int L>
__device__ __forceinline__ float nt_wave_q2(const r48::Board &b, uint32_t lane, const r48::NtLayout &lay,
                                            const float *__restrict__ tables, uint32_t &lg)
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
            leaf = r48::nt_leaf<L>(child, lay, tables);
        }
        leaf0 = base == 0u ? leaf : leaf0;
        leaf1 = base == 0u ? leaf1 : leaf;
    }
    const int src = (int)(rank2 & 63u);
    const float two0 = __shfl(leaf0, src), four0 = __shfl(leaf0, src + 1);
    const float two1 = __shfl(leaf1, src), four1 = __shfl(leaf1, src + 1);
    const bool late = rank2 >= 64u;
    float x = slot ? r48::nt_fma(9.0f, late ? two1 : two0, late ? four1 : four0) : 0.0f;
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 8);
    return ok ? r48::nt_q2(r, x, r48::blanks(s).n) : -__builtin_inff();
}

template <int L, int DEPTH>
__global__ __launch_bounds__(kBlock) void k_nt_search(const int8_t *__restrict__ boards, int64_t n,
                                                      const r48::NtLayout lay, const float *__restrict__ tables,
                                                      int8_t *__restrict__ actions, float *__restrict__ q,
                                                      uint8_t *__restrict__ legal)
{
    static_assert(DEPTH == 1 || DEPTH == 2, "depth 1 or 2");
    const int64_t i = (int64_t)blockIdx.x * kSearchBoards + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= n)
        return;   // the whole wave
    const uint32_t lane = threadIdx.x & 63u, a = lane >> 4, c = lane & 15u;
    const r48::Board b = r48::load_board(boards, i);
    uint32_t lg;
    float qa;
    if (DEPTH == 1) {
        const r48::Moves4 m = r48::move_rows4<true>(b);
        lg = r48::nt_legal4(m, b);
        const bool ok = ((lg >> a) & 1u) != 0u;
        float x = 0.0f;
        if (ok && c == 0u)
            x = r48::nt_score<L>(r48::nt_pick(m, a), r48::nt_pick_reward(m, a), lay, tables);
        qa = ok ? __shfl(x, (int)(lane & 48u)) : -__builtin_inff();
    } else {
        qa = nt_wave_q2<L>(b, lane, lay, tables, lg);
    }
    const float q0 = __shfl(qa, 0), q1 = __shfl(qa, 16), q2 = __shfl(qa, 32), q3 = __shfl(qa, 48);
    if (q && c == 0u)
        q[4 * i + a] = qa;
    if (lane == 0u) {
        actions[i] = (int8_t)r48::nt_argmax4(q0, q1, q2, q3);
        if (legal)
            legal[i] = (uint8_t)lg;
    }
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

__device__ __forceinline__ uint32_t uniform_word(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// what wave 0 leaves for the others
struct Search3Root {
    uint32_t after[4][4];   // the afterstate of move a, words w0 .. w3
    uint32_t reward[4];
    uint32_t legal, slots_lo, slots_hi;
    uint32_t dealt, done;   // children handed out; children whose leaf is stored
};

template <int L, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_nt_search3(const int8_t *__restrict__ boards, int64_t n,
                                                           const r48::NtLayout lay, const float *__restrict__ tables,
                                                           int8_t *__restrict__ actions, float *__restrict__ q,
                                                           uint8_t *__restrict__ legal)
{
    static_assert(WAVES >= 1 && WAVES <= 16, "a workgroup has at most 1024 lanes");
    __shared__ float leaf[kSearch3MaxKids];
    __shared__ Search3Root root;
    const int64_t i = blockIdx.x;   // the grid has one workgroup per board
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u, a = lane >> 4, c = lane & 15u;
    if (w == 0u) {
        const r48::Board b = r48::load_board(boards, i);
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
    __syncthreads();
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
        const uint32_t p = r48::nt_select_bit(M, j >> 1);   // < 64
        const uint32_t *sa = root.after[p >> 4];
        r48::Board child{sa[0], sa[1], sa[2], sa[3]};
        r48::place(child, p & 15u, 1u + (j & 1u), true);
        uint32_t lg2;
        const float q2a = nt_wave_q2<L>(child, lane, lay, tables, lg2);
        // the rows' scores; an illegal reply holds -inf, so the plain max is the max over the legal ones
        const float b0 = __shfl(q2a, 0), b1 = __shfl(q2a, 16), b2 = __shfl(q2a, 32), b3 = __shfl(q2a, 48);
        uint32_t next = 0u;
        if (lane == 0u) {
            leaf[j] = lg2 ? fmaxf(fmaxf(b0, b1), fmaxf(b2, b3)) : 0.0f;
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
    const r48::Board s{root.after[a][0], root.after[a][1], root.after[a][2], root.after[a][3]};
    const uint32_t r = root.reward[a];
    const bool ok = ((lg >> a) & 1u) != 0u;
    const bool slot = ((M >> lane) & 1ull) != 0ull;
    const uint32_t rank2 = 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
    float x = 0.0f;
    if (slot)   // rank2 + 1 < kids <= 120
        x = r48::nt_fma(9.0f, leaf[rank2], leaf[rank2 + 1u]);
    x += __shfl_xor(x, 1);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 8);
    const float qa = ok ? r48::nt_q2(r, x, r48::blanks(s).n) : -__builtin_inff();
    const float q0 = __shfl(qa, 0), q1 = __shfl(qa, 16), q2 = __shfl(qa, 32), q3 = __shfl(qa, 48);
    if (q && c == 0u)
        q[4 * i + a] = qa;
    if (lane == 0u) {
        actions[i] = (int8_t)r48::nt_argmax4(q0, q1, q2, q3);
        if (legal)
            legal[i] = (uint8_t)lg;
    }
}

// the arguments every entry point shares: boards, n, the layout
int check_common(const char *fn, const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                 r48::NtLayout &lay)
{
    if (!boards || !aligned(boards, 16) || n < 0)
        return fail(R48_EINVAL, std::string(fn) + ": boards NULL or not 16-byte aligned, or n < 0");
    if (const char *why = r48::nt_expand(cells, m, L, lay))
        return fail(R48_EINVAL, std::string(fn) + ": bad layout: " + why);
    return R48_OK;
}

#define R48_NT_DISPATCH(KERNEL, ...)                                                                       \
    switch (lay.L) {                                                                                       \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    case 5: hipLaunchKernelGGL(KERNEL<5>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(KERNEL<6>, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); break; \
    }

}  // namespace

extern "C" {

int r48_ntuple_value(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                     float *value, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_value", boards, n, cells, m, L, lay))
        return rc;
    if (!tables || !value || !aligned(tables, 4) || !aligned(value, 4))
        return fail(R48_EINVAL, "r48_ntuple_value: tables/value NULL or not 4-byte aligned");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_value, boards, n, lay, tables, value)
    return launched("k_nt_value");
}

int r48_ntuple_act(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                   int8_t *actions, int8_t *after, float *value, int32_t *reward, uint8_t *legal, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_act", boards, n, cells, m, L, lay))
        return rc;
    if (!tables || !actions || !aligned(tables, 4) || !aligned(after, 16) || !aligned(value, 4) || !aligned(reward, 4))
        return fail(R48_EINVAL, "r48_ntuple_act: tables/actions NULL, after not 16-byte aligned, or tables / value / "
                                "reward not 4-byte aligned");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_act, boards, n, lay, tables, actions, after, value, reward, legal)
    return launched("k_nt_act");
}

int r48_ntuple_td_act(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                      const int8_t *prev_after, const float *prev_value, const uint8_t *prev_done,
                      const uint8_t *prev_valid, int8_t *actions, int8_t *after, float *value, int32_t *reward,
                      uint8_t *legal, uint8_t *valid_out, float *delta_out, int64_t *acc, uint32_t *cnt, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_td_act", boards, n, cells, m, L, lay))
        return rc;
    if (!tables || !prev_after || !prev_value || !prev_done || !prev_valid || !actions || !after || !value || !legal ||
        !valid_out || !acc || !cnt)
        return fail(R48_EINVAL, "r48_ntuple_td_act: tables, prev_after / prev_value / prev_done / prev_valid, actions, "
                                "after, value, legal, valid_out, acc or cnt NULL (only reward and delta_out may be)");
    if (!aligned(prev_after, 16) || !aligned(after, 16) || !aligned(acc, 8) || !aligned(tables, 4) ||
        !aligned(prev_value, 4) || !aligned(value, 4) || !aligned(reward, 4) || !aligned(delta_out, 4) || !aligned(cnt, 4))
        return fail(R48_EINVAL, "r48_ntuple_td_act: prev_after / after not 16-byte aligned, acc not 8-byte aligned, or "
                                "tables / prev_value / value / reward / delta_out / cnt not 4-byte aligned");
    if (after == prev_after || value == prev_value || valid_out == prev_valid)
        return fail(R48_EINVAL, "r48_ntuple_td_act: after, value and valid_out must not be the prev_ buffers (apply "
                                "reads the previous afterstates and flags after this call; swap the buffers then)");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_td_act, boards, n, lay, tables, prev_after, prev_value, prev_done, prev_valid, actions, after,
                    value, reward, legal, valid_out, delta_out, reinterpret_cast<unsigned long long *>(acc), cnt)
    return launched("k_nt_td_act");
}

int r48_ntuple_search(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tables,
                      int32_t depth, int8_t *actions, float *q, uint8_t *legal, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_search", boards, n, cells, m, L, lay))
        return rc;
    if (depth != 1 && depth != 2)
        return fail(R48_EINVAL, "r48_ntuple_search: depth must be 1 or 2, got " + std::to_string(depth));
    if (!tables || !actions || !aligned(tables, 4) || !aligned(q, 4))
        return fail(R48_EINVAL, "r48_ntuple_search: tables/actions NULL, or tables / q not 4-byte aligned");
    const int64_t blocks = n / kSearchBoards + (n % kSearchBoards ? 1 : 0);   // one board per wave
    if (blocks > 0x7FFFFFFFll)
        return fail(R48_EINVAL, "r48_ntuple_search: n = " + std::to_string(n) + " boards exceed the grid (" +
                                    std::to_string(kSearchBoards) + " boards per workgroup, 2^31 - 1 workgroups)");
    if (n == 0)
        return R48_OK;
    const dim3 grid((unsigned)blocks), block(kBlock);
    const hipStream_t st = (hipStream_t)stream;
#define R48_NT_SEARCH(LEN)                                                                                         \
    case LEN:                                                                                                      \
        if (depth == 1)                                                                                            \
            hipLaunchKernelGGL((k_nt_search<LEN, 1>), grid, block, 0, st, boards, n, lay, tables, actions, q, legal); \
        else                                                                                                       \
            hipLaunchKernelGGL((k_nt_search<LEN, 2>), grid, block, 0, st, boards, n, lay, tables, actions, q, legal); \
        break;
    switch (lay.L) {
        R48_NT_SEARCH(2)
        R48_NT_SEARCH(3)
        R48_NT_SEARCH(4)
        R48_NT_SEARCH(5)
        R48_NT_SEARCH(6)
    }
#undef R48_NT_SEARCH
    return launched("k_nt_search");
}

int r48_ntuple_search3(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L,
                       const float *tables, int8_t *actions, float *q, uint8_t *legal, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_search3", boards, n, cells, m, L, lay))
        return rc;
    if (!tables || !actions || !aligned(tables, 4) || !aligned(q, 4))
        return fail(R48_EINVAL, "r48_ntuple_search3: tables/actions NULL, or tables / q not 4-byte aligned");
    if (n > 0x7FFFFFFFll)   // one board per workgroup
        return fail(R48_EINVAL, "r48_ntuple_search3: n = " + std::to_string(n) +
                                    " boards exceed the grid (one per workgroup, 2^31 - 1 workgroups)");
    if (n == 0)
        return R48_OK;
    const dim3 grid((unsigned)n);
    const hipStream_t st = (hipStream_t)stream;
    const bool small = n <= kSearch3SmallBatch;
#define R48_NT_SEARCH3(LEN)                                                                                          \
    case LEN:                                                                                                        \
        if (small)                                                                                                   \
            hipLaunchKernelGGL((k_nt_search3<LEN, kSearch3WavesSmall>), grid, dim3(64 * kSearch3WavesSmall), 0, st,  \
                               boards, n, lay, tables, actions, q, legal);                                           \
        else                                                                                                         \
            hipLaunchKernelGGL((k_nt_search3<LEN, kSearch3WavesLarge>), grid, dim3(64 * kSearch3WavesLarge), 0, st,  \
                               boards, n, lay, tables, actions, q, legal);                                           \
        break;
    switch (lay.L) {
        R48_NT_SEARCH3(2)
        R48_NT_SEARCH3(3)
        R48_NT_SEARCH3(4)
        R48_NT_SEARCH3(5)
        R48_NT_SEARCH3(6)
    }
#undef R48_NT_SEARCH3
    return launched("k_nt_search3");
}

int r48_ntuple_accumulate(const int8_t *boards, int64_t n, const float *delta, const uint8_t *valid,
                          const uint8_t *cells, int32_t m, int32_t L, int64_t *acc, uint32_t *cnt, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_accumulate", boards, n, cells, m, L, lay))
        return rc;
    if (!delta || !acc || !cnt || !aligned(delta, 4) || !aligned(acc, 8) || !aligned(cnt, 4))
        return fail(R48_EINVAL, "r48_ntuple_accumulate: delta/acc/cnt NULL, acc not 8-byte aligned, or delta / cnt "
                                "not 4-byte aligned");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_accumulate, boards, n, delta, valid, lay, reinterpret_cast<unsigned long long *>(acc), cnt)
    return launched("k_nt_accumulate");
}

int r48_ntuple_apply(const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m, int32_t L,
                     float step, float *tables, int64_t *acc, uint32_t *cnt, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_apply", boards, n, cells, m, L, lay))
        return rc;
    if (!tables || !acc || !cnt || !aligned(tables, 4) || !aligned(acc, 8) || !aligned(cnt, 4))
        return fail(R48_EINVAL, "r48_ntuple_apply: tables/acc/cnt NULL, acc not 8-byte aligned, or tables / cnt not "
                                "4-byte aligned");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_apply, boards, n, valid, lay, step, tables, reinterpret_cast<unsigned long long *>(acc), cnt)
    return launched("k_nt_apply");
}

int r48_ntuple_apply_tc(const int8_t *boards, int64_t n, const uint8_t *valid, const uint8_t *cells, int32_t m,
                        int32_t L, float step, float *tables, float *tc_e, float *tc_a, int64_t *acc, uint32_t *cnt,
                        void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_apply_tc", boards, n, cells, m, L, lay))
        return rc;
    if (!tables || !tc_e || !tc_a || !acc || !cnt || !aligned(tables, 4) || !aligned(tc_e, 4) || !aligned(tc_a, 4) ||
        !aligned(acc, 8) || !aligned(cnt, 4))
        return fail(R48_EINVAL, "r48_ntuple_apply_tc: tables/tc_e/tc_a/acc/cnt NULL, acc not 8-byte aligned, or "
                                "tables / tc_e / tc_a / cnt not 4-byte aligned");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_apply_tc, boards, n, valid, lay, step, tables, tc_e, tc_a,
                    reinterpret_cast<unsigned long long *>(acc), cnt)
    return launched("k_nt_apply_tc");
}

int r48_ntuple_tc_rate(const int8_t *boards, int64_t n, const uint8_t *cells, int32_t m, int32_t L, const float *tc_e,
                       const float *tc_a, float *rate_out, void *stream)
{
    r48::NtLayout lay;
    if (const int rc = check_common("r48_ntuple_tc_rate", boards, n, cells, m, L, lay))
        return rc;
    if (!tc_e || !tc_a || !rate_out || !aligned(tc_e, 4) || !aligned(tc_a, 4) || !aligned(rate_out, 4))
        return fail(R48_EINVAL, "r48_ntuple_tc_rate: tc_e/tc_a/rate_out NULL or not 4-byte aligned");
    if (n == 0)
        return R48_OK;
    R48_NT_DISPATCH(k_nt_tc_rate, boards, n, lay, tc_e, tc_a, rate_out)
    return launched("k_nt_tc_rate");
}

}  // extern "C"
