// r48_ntuple.h -- the n-tuple network's layout, entry index and value sum, for the gfx950 kernels
// (r48_ntuple.hip) and, like r48_board.h, for the host (tests/native/ntuple_logic_test.cpp).
//
// A layout is m tuples (1..8) of L distinct cells each (2..6), cells numbered 0..15 row-major as
// the board bytes are. The network's value is a sum of table entries,
//     V(b) = sum over t < m, g in D4 of tables[t][index(g . b, t)],
//     index(b, t) = sum over k < L of min(b[cell_k], 15) << 4k,
// every (t, g) counted, duplicates included. Exponents above 15 share entry 15 (a board can hold
// 18 = 17 + 17), so a table has 16^L entries.
//
// Nothing transforms a board at run time: g . b read at cell c is b read at cell sym(g, c), so the
// host expands the layout once into 8m PLACED tuples -- for each (t, g) the L cells sym(g, cell_k)
// as shift amounts (4 * cell) into the board packed to 16 nibbles in 64 bits. The expansion goes
// to the kernels by value in their arguments, so it is wave-uniform: a placed tuple is one 8-byte
// scalar load, a cell one bit-field extract with a scalar shift.
//
// Summation order (the contract every kernel here shares, so value and act agree bit for bit):
// fp32, starting from 0, hits in the order p = 8t + g = 0, 1, ..., 8m - 1.
//
// The search (k_nt_search, k_nt_search3, k_nt_search_ruled, and nt_search_board for one board on
// the host). For a move a that changes the board: afterstate s_a, merge reward r_a, and
//     depth 1   Q(a) = (float)r_a + V(s_a)                                  (act's score)
//     depth 2   Q(a) = (float)r_a + S_a / (float)(10 |E|),  E = the empty cells of s_a,
//               S_a = sum over c in E of (9 leaf(s_a[c <- 1]) + leaf(s_a[c <- 2])),
//               leaf(child) = max over the child's legal moves a' of (float)r_a' + V(after_a'), and
//               0 where the child has no legal move (the game-over value of the trainer's target)
// -- the spawn rule of r48_board.h: uniform over the blanks, P(4) = 0.1. Illegal moves have
// Q = -inf; the action is the first maximiser of Q (lowest code), 0 where no move is legal.
// Arithmetic (the contract the kernel and the host share, so they agree bit for bit):
//   - fp32 throughout, V is nt_value
//   - a cell's term is fmaf(9, leaf(c, 1), leaf(c, 2)): one rounding, none with integer tables,
//     where S_a is then exact (below 2^24) and symmetric boards tie bit for bit; one division
//     by 10 |E| afterwards
//   - S_a adds the 16 terms x_0 .. x_15 of the cells in row-major order, x_c = +0 where cell c
//     of s_a holds a tile, as the xor butterfly does: x_c += x_(c ^ 1), then ^ 2, ^ 4, ^ 8, i.e.
//     (((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7))) + (the same of x8 .. x15). fp32 addition
//     commutes, so every lane of the butterfly holds these bits. The order depends on nothing
//     but the cell numbers: not on the batch, on n, or on which cells are empty.
//
// The same, recursively, for any number of plies k (k_nt_search3 runs k = 3, k_nt_search_ruled and
// nt_search_board 1..4):
//     best_k(board) = max over the board's legal moves a of Q_k(a), 0 where it has none
//     Q_1(a)        = (float)r_a + V(s_a)
//     Q_k(a), k > 1 = (float)r_a + S_a / (float)(10 |E|),  S_a = nt_sum16 of the sixteen cell terms
//                     x_c = fmaf(9, best_(k-1)(s_a[c <- 1]), best_(k-1)(s_a[c <- 2])), x_c = +0 where
//                     cell c of s_a holds a tile
// Depth 2 is the above with leaf = best_1; depth 3's leaf is best_2, depth 4's best_3:
//     Q_4(a) = (float)r_a + nt_sum16(x) / (float)(10 |E|),
//     x_c = nt_fma(9, best_3(s_a[c <- 1]), best_3(s_a[c <- 2])).
// The arithmetic is the same at every level: fp32, nt_fma for a cell term, the butterfly's order,
// one division by 10 |E| per level (nt_q2). The max over the legal moves of fp32 scores does not
// depend on their order.
//
// The ruled search (k_nt_search_ruled, nt_search_board_ruled) chooses the depth per board. A RULE
// is uint8 depth_of_blanks[17], every entry in 1..4; board i is searched at depth
//     d_i = rule[blanks(board_i)],  blanks = the zero cells of the root board, 0..16,
// and its actions / q / legal are exactly those of the search at depth d_i above: the bits of
// k_nt_search at d_i = 1 or 2 and of k_nt_search3 at d_i = 3. depth_out[i] (nullable) = d_i for
// every board, one without a legal move included (its q is -inf, its action 0, and depth_out is
// still rule[blanks]). As everywhere here, q does not depend on where the board is in the batch,
// on n, on how the children were dealt or on which wave did what -- nor on the rule's other
// entries. A roomy board at depth 4 costs about a hundred times depth 3: the rule is the cost
// guard.
//
// Stages (multi-stage tables with lazy weight promotion; Jaskowski 2016). A staged net has n_cuts in
// 1..3 CUTS, strictly ascending exponents in 1..15, and S = n_cuts + 1 stages:
//     stage(b) = #{ j : max over the 16 cells of min(b[c], 15) >= cuts[j] }
// of the board being EVALUATED -- the afterstate, never the root of a search or the env board.
// tables, acc, cnt and with TC tc_e / tc_a are [S][m][16^L]; own is uint8 [S][m][16^L] with own[0]
// all 1 and every other entry 0 at the start; everything else starts at zero. Hit p = 8t + g of
// board b reads entry
//     ((stage(b) * m + t) << 4L) + index(b, placed[p]).
// Everything read-only (V, act, every search depth, the ruled search, both play kernels, tc_rate) is
// the contract above word for word with that entry: the same summation order, the same nt_fma /
// butterfly / nt_q2 arithmetic, the same first maximiser, and still nothing depends on the batch
// position, on n or on which wave did what. A reader never follows a fallback chain.
// The update (accumulate then apply, or td_act then apply):
//   1. MARK, in the accumulate walk (nt_add_hits, so in k_nt_td_act too): every hit (s, e) of a
//      valid board with s >= 1 sets own[s][e] = 1, a plain byte store of one value, complete before
//      apply's launch begins.
//   2. APPLY: the lane that owns touched entry (s, e) (it got the count from the exchange) computes
//      the new value exactly as the unstaged update does, from tables[s][e] (TC: tc_e[s][e] and
//      tc_a[s][e] by nt_tc_update), stores it and then PUSHES it: for k = s + 1, s + 2, ... while
//      k < S and own[k][e] == 0, tables[k][e] = new; it stops at the first owned stage. tc_e and tc_a
//      are never pushed: an entry's first update in a new stage runs at rate 1.
// This is lazy weight promotion: the first update of (s, e) starts from the value the nearest lower
// owned stage had after the previous update call, and until then (s, e) reads as that stage's
// current value. A call's marks are all set before any of its exchanges, so the owner of (0, e)
// never writes into a stage that the same call takes ownership of: no race, no dependence on the
// order of the boards, bitwise reproducible as the unstaged update is.
// Invariant: after any sequence of updates, for every k >= 1 and e with own[k][e] == 0, tables[k][e]
// has the bits of tables[k - 1][e].
// Staging is a compile-time parameter of every body below: the policy NtPlain (no stages, the
// entry offset is the constant 0 and nothing is computed) or NtCuts (the cuts in one word).
// nt_staged_update_pull restates the update on the host in the PULL form: an unowned entry is not
// stored at all, a read resolves to the nearest lower owned stage and a first touch copies it.
//
// Replicas (R independent unstaged nets trained in the same launches: k_nt_td_act_rep,
// k_nt_apply_rep, k_nt_apply_tc_rep). A batch of n boards holds `replicas` replicas, 1..64; n is a
// multiple of replicas, per = n / replicas >= 1, and board i belongs to replica r = i / per -- by its
// position in the batch, not by its contents. tables, acc, cnt and with TC tc_e / tc_a are
// [replicas][m][16^L]. Hit p = 8t + g of board i uses entry
//     r * (m << 4L) + (t << 4L) + index(b, placed[p]),
// and replicas * m * 16^L must not exceed 2^32 (an entry is a uint32_t; the entry points refuse more).
// apply's step is per replica: steps is float[replicas] in device memory and board i moves its
// entries by steps[r]. Everything else is the unstaged contract word for word: the summation order,
// nt_td_delta, the fixed-point integer atomics, the owner lane that takes an entry's count by
// exchange, nt_mean, nt_tc_update. Two replicas share no entry, so a call on [replicas * per] boards
// leaves in replica r's slices of every array the bits that the unstaged entry point leaves when it
// is called on that replica's boards, tables and scratch alone, whatever `replicas` is and whatever
// the other replicas hold. No stages: a replica is an unstaged net. The policy is NtOffset, the
// lane's offset r * (m << 4L): a wave may straddle a replica boundary (per need not be a multiple of
// 64), so r, the offset and the step are per-lane values.
//
// Carousel shaping (Jaskowski 2016; k_nt_carousel_restart + k_nt_carousel_record, nt_carousel_host
// on the host). Episodes start in turn from stage 0, 1, ..., S - 1, from a board with which a recent
// episode ENTERED that stage, so every stage gets an equal share of the episode starts. The carousel
// has its own cuts (1..3, checked as the stage cuts are; they need not be the net's, and the net may
// be unstaged), S = n_cuts + 1, and the stage of a board is nt_stage(cuts, board) of the ENV board,
// after the spawn. Per board slot i of a batch of n, all caller-owned:
//     pool     int8  [S - 1][n][16]  pool[s - 1][i]: the board with which slot i last entered stage s
//     pool_has uint8 [S - 1][n]      1 where the pool slot holds a board            (0 at the start)
//     seen     uint8 [n]             highest stage the slot's current episode was recorded or
//                                    started in                                     (0 at the start)
//     turn     uint8 [n]             stage of the slot's last episode start         (0 at the start)
//     starts   uint64 [S], nullable  episode starts per stage                       (0 at the start)
// One call follows an env step with auto-reset and works on the boards in place, with that step's
// done flags, in two phases over the whole batch, in this order:
//   RESTART, boards with done[i] != 0 (the env has put a fresh board there):
//     t = (turn[i] + 1) % S
//     t > 0: the donor is j = mulhi(w0, (uint32)n), w0 = word 0 of Philox4x32-10(key = {seed lo,
//            seed hi}, counter = {gid lo, gid hi, ctr, kCarouselTag}), gid = gid0 + i. Where
//            pool_has[t - 1][j], boards[i] = pool[t - 1][j]; else t = 0 (the paper's fallback to the
//            first stage) -- the next restart of the slot tries stage 1 again
//     t == 0: the fresh board stays
//     then turn[i] = t, seen[i] = nt_stage(cuts, boards[i]), starts[t] += 1
//   RECORD, boards with done[i] == 0:
//     s = nt_stage(cuts, boards[i]); where s > seen[i]: pool[s - 1][i] = boards[i],
//     pool_has[s - 1][i] = 1, seen[i] = s
// The restart phase reads the pool as it was BEFORE the call: a donor slot may record in the same
// call, so on the GPU the phases are two launches on one stream, restart then record (one kernel
// would race; no grid-wide barrier). Every slot writes its own pool slot only, there is no shared
// ring: plain stores of integers, and integer atomics (order-free) for starts. The result is bitwise
// reproducible and independent of the launch geometry; it depends on the batch through n and gid0.
#pragma once
#include <stdint.h>

#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>

#include <map>
#include <vector>
#endif

#include "r48_board.h"

namespace r48 {

static constexpr int kNtMaxTuples = 8;
static constexpr int kNtMinLen = 2, kNtMaxLen = 6;
static constexpr int kNtSyms = 8;

// placed[8 * t + g]: byte k = 4 * sym(g, cells[t][k]), the shift of the tuple's k-th cell in the
// nibble-packed board (bytes L.. are 0)
struct NtLayout {
    uint64_t placed[kNtSyms * kNtMaxTuples];
    int32_t m, L;
};

// entries of one table: 16^L
R48_HD int64_t nt_table_size(int L) { return (int64_t)1 << (4 * L); }

// The cell of b that (g . b) holds at cell c, g = 0..7: bit 0 mirrors the rows, bit 1 the columns,
// bit 2 transposes -- the eight symmetries of the square, each once.
R48_HD int nt_sym_cell(int g, int c)
{
    int r = c >> 2, col = c & 3;
    if (g & 1)
        r = 3 - r;
    if (g & 2)
        col = 3 - col;
    return (g & 4) ? 4 * col + r : 4 * r + col;
}

// Validate a layout and expand it. Returns NULL, or what is wrong with it.
inline const char *nt_expand(const uint8_t *cells, int m, int L, NtLayout &out)
{
    if (!cells)
        return "cells is NULL";
    if (m < 1 || m > kNtMaxTuples)
        return "m must be 1..8 tuples";
    if (L < kNtMinLen || L > kNtMaxLen)
        return "L must be 2..6 cells per tuple";
    for (int t = 0; t < m; t++) {
        uint32_t seen = 0;
        for (int k = 0; k < L; k++) {
            const uint8_t c = cells[t * L + k];
            if (c >= 16)
                return "a cell is not in 0..15";
            if (seen & (1u << c))
                return "a tuple repeats a cell";
            seen |= 1u << c;
        }
    }
    for (int p = 0; p < kNtSyms * kNtMaxTuples; p++)
        out.placed[p] = 0;
    for (int t = 0; t < m; t++)
        for (int g = 0; g < kNtSyms; g++) {
            uint64_t w = 0;
            for (int k = 0; k < L; k++)
                w |= (uint64_t)(4 * nt_sym_cell(g, cells[t * L + k])) << (8 * k);
            out.placed[kNtSyms * t + g] = w;
        }
    out.m = m;
    out.L = L;
    return nullptr;
}

// A board as 16 nibbles min(cell, 15), cell c at bits 4c: lo = cells 0..7, hi = cells 8..15.
struct NtBoard {
    uint32_t lo, hi;
};

// bytes (<= 0x7F) of one row word -> 16 bits of clamped nibbles
R48_HD uint32_t nt_pack_row(uint32_t w)
{
    const uint32_t over = (w + 0x70707070u) & 0x80808080u;   // bit 7: the byte is >= 16
    const uint32_t x = bsel(m7f(over), 0x0F0F0F0Fu, w);
    const uint32_t y = x | (x >> 4);                          // byte 0 = cells 0, 1; byte 2 = cells 2, 3
    return (y & 0xFFu) | ((y >> 8) & 0xFF00u);
}

R48_HD NtBoard nt_pack(const Board &b)
{
    return NtBoard{nt_pack_row(b.w0) | (nt_pack_row(b.w1) << 16), nt_pack_row(b.w2) | (nt_pack_row(b.w3) << 16)};
}

#if defined(__HIPCC__)
#define R48_NO_UNROLL _Pragma("unroll 1")
#else
#define R48_NO_UNROLL
#endif

// ---- stages -----------------------------------------------------------------------------------
static constexpr int kNtMaxCuts = 3;

// the two staging policies: none, or the checked cuts in one word (cut j in byte j, n of them)
struct NtPlain {};
struct NtCuts {
    uint32_t w;
    int32_t n;
};

// NULL, or what is wrong with the cuts of a staged entry point (n_cuts == 0: unstaged, cuts unused)
inline const char *nt_cuts_check(const uint8_t *cuts, int n_cuts)
{
    if (n_cuts < 0 || n_cuts > kNtMaxCuts)
        return "n_cuts must be 0..3";
    if (n_cuts > 0 && !cuts)
        return "cuts is NULL";
    for (int j = 0; j < n_cuts; j++) {
        if (cuts[j] < 1 || cuts[j] > 15)
            return "a cut is not in 1..15";
        if (j > 0 && cuts[j] <= cuts[j - 1])
            return "cuts are not strictly ascending";
    }
    return nullptr;
}

inline NtCuts nt_cuts_pack(const uint8_t *cuts, int n_cuts)
{
    NtCuts c{0u, n_cuts};
    for (int j = 0; j < n_cuts; j++)
        c.w |= (uint32_t)cuts[j] << (8 * j);
    return c;
}

// stage(b) of the contract, from the row words (bytes <= 0x7F): byte + (0x80 - cut) has bit 7 set
// exactly where the byte is >= cut, and a byte of 16..18 is above every cut as its clamp 15 is. Per
// cut four adds, two ors, one and, a compare and an add; the addend is wave-uniform.
R48_HD uint32_t nt_stage(const NtCuts &c, const Board &b)
{
    uint32_t s = 0u;
    R48_NO_UNROLL
    for (int j = 0; j < c.n; j++) {
        const uint32_t k = (0x80u - ((c.w >> (8 * j)) & 0xFFu)) * 0x01010101u;
        const uint32_t hit = or3(b.w0 + k, b.w1 + k, b.w2 + k) | (b.w3 + k);
        s += (hit & 0x80808080u) != 0u ? 1u : 0u;
    }
    return s;
}

// the offset of the board's stage in the contiguous [S][m][16^L] arrays: (stage * m) << 4L, below
// 2^29. Without stages the constant 0.
template <int L>
R48_HD uint32_t nt_base(const NtPlain &, int32_t, const Board &)
{
    return 0u;
}

template <int L>
R48_HD uint32_t nt_base(const NtCuts &c, int32_t m, const Board &b)
{
    return (nt_stage(c, b) * (uint32_t)m) << (4 * L);
}

// ---- replicas ----------------------------------------------------------------------------------
static constexpr int kNtMaxReplicas = 64;

// the third policy: the offset of the lane's replica in the contiguous [replicas][m][16^L] arrays,
// r * (m << 4L), whatever the board holds
struct NtOffset {
    uint32_t base;
};

template <int L>
R48_HD uint32_t nt_base(const NtOffset &o, int32_t, const Board &)
{
    return o.base;
}

// NULL, or what is wrong with the replicas of a batch of n boards of an (m, L) layout
inline const char *nt_replicas_check(int64_t n, int32_t replicas, int m, int L)
{
    if (replicas < 1 || replicas > kNtMaxReplicas)
        return "replicas must be 1..64";
    if (n % replicas != 0)
        return "n is not a multiple of replicas";
    if ((int64_t)replicas * m * nt_table_size(L) > ((int64_t)1 << 32))
        return "replicas * m * 16^L exceeds 2^32 entries";
    return nullptr;
}

// ---- carousel shaping --------------------------------------------------------------------------
// NULL, or what is wrong with a carousel's cuts: the stage cuts' rules, and at least one cut
inline const char *nt_carousel_cuts_check(const uint8_t *cuts, int n_cuts)
{
    if (n_cuts < 1 || n_cuts > kNtMaxCuts)
        return "n_cuts must be 1..3";
    return nt_cuts_check(cuts, n_cuts);
}

// t of the contract before the pool is looked at: the stage after the slot's last start, S - 1 wraps to 0
R48_HD uint32_t nt_carousel_turn(uint32_t turn, const NtCuts &c) { return (turn + 1u) % (uint32_t)(c.n + 1); }

// the donor slot j of restarting board gid: one Philox4x32-10 block, word 0 scaled to 0..n - 1
R48_HD uint32_t nt_carousel_donor(uint64_t gid, uint32_t ctr, uint32_t k0, uint32_t k1, uint32_t n)
{
    uint32_t w[4] = {(uint32_t)gid, (uint32_t)(gid >> 32), ctr, kCarouselTag};
    philox4x32_10(w, k0, k1);
    return mulhi(w[0], n);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One call of the contract on the host, serially: the restart phase over the whole batch, then the
// record phase. The restart phase writes no pool slot, so it reads the pool as it was before the call.
inline void nt_carousel_host(int8_t *boards, int64_t n, const uint8_t *done, const NtCuts &cuts, int8_t *pool,
                             uint8_t *pool_has, uint8_t *seen, uint8_t *turn, uint64_t *starts, uint64_t seed,
                             int64_t gid0, uint32_t ctr)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int64_t i = 0; i < n; i++) {
        if (!done[i])
            continue;
        uint32_t t = nt_carousel_turn(turn[i], cuts);
        if (t > 0u) {
            const int64_t at = (int64_t)(t - 1u) * n + nt_carousel_donor((uint64_t)(gid0 + i), ctr, k0, k1, (uint32_t)n);
            if (pool_has[at])
                memcpy(boards + 16 * i, pool + 16 * at, 16);
            else
                t = 0u;
        }
        Board b;
        memcpy(&b, boards + 16 * i, 16);
        turn[i] = (uint8_t)t;
        seen[i] = (uint8_t)nt_stage(cuts, b);
        if (starts)
            starts[t] += 1u;
    }
    for (int64_t i = 0; i < n; i++) {
        if (done[i])
            continue;
        Board b;
        memcpy(&b, boards + 16 * i, 16);
        const uint32_t s = nt_stage(cuts, b);
        if (s > seen[i]) {
            const int64_t at = (int64_t)(s - 1u) * n + i;
            memcpy(pool + 16 * at, boards + 16 * i, 16);
            pool_has[at] = 1;
            seen[i] = (uint8_t)s;
        }
    }
}
#endif

// entry index of one placed tuple
template <int L>
R48_HD uint32_t nt_index(const NtBoard &b, uint64_t placed)
{
    uint32_t idx = 0;
    R48_UNROLL
    for (int k = 0; k < L; k++) {
        const uint32_t s = (uint32_t)(placed >> (8 * k)) & 0xFFu;
        const uint32_t w = (s & 32u) ? b.hi : b.lo;
        idx |= ((w >> (s & 31u)) & 15u) << (4 * k);
    }
    return idx;
}

// entry of hit p = 8t + g in the contiguous tables[m][16^L]; staged: in [S][m][16^L], base =
// nt_base of the board
template <int L>
R48_HD uint32_t nt_entry(const NtBoard &b, const NtLayout &lay, int p, uint32_t base = 0u)
{
    return base + ((uint32_t)(p >> 3) << (4 * L)) + nt_index<L>(b, lay.placed[p]);
}

// V(b) in the contract's order. The loads of two tuples (16 hits) are issued before their adds.
template <int L>
R48_HD float nt_value(const NtBoard &b, const NtLayout &lay, const float *__restrict__ tables, uint32_t base = 0u)
{
    const int np = kNtSyms * lay.m;
    float sum = 0.0f;
    int p = 0;
    for (; p + 16 <= np; p += 16) {
        float v[16];
        R48_UNROLL
        for (int j = 0; j < 16; j++)
            v[j] = tables[nt_entry<L>(b, lay, p + j, base)];
        R48_UNROLL
        for (int j = 0; j < 16; j++)
            sum += v[j];
    }
    if (p < np) {
        float v[8];
        R48_UNROLL
        for (int j = 0; j < 8; j++)
            v[j] = tables[nt_entry<L>(b, lay, p + j, base)];
        R48_UNROLL
        for (int j = 0; j < 8; j++)
            sum += v[j];
    }
    return sum;
}

// ---- temporal-coherence learning rates ---------------------------------------------------------
// Every table entry e keeps E[e], the running sum of the mean errors it was updated with, and
// A[e], the running sum of their absolute values (float[m][16^L] like the tables, zero at the
// start). It learns at rate |E| / A: 1 while its errors agree in sign, towards 0 once they turn
// to noise (Beal & Smith; Jaskowski 2016). For an entry hit in an update, with mean = the
// update's mean delta of its hits (nt_mean, the expression plain apply uses):
//     rate       = A[e] > 0 ? fminf(fabsf(E[e]) / A[e], 1) : 1
//     tables[e] += step * (rate * mean)
//     E[e]      += mean
//     A[e]      += fabsf(mean)
// fp32 throughout. rate * mean is formed first, so with rate == 1 the table moves by the bits
// plain apply moves it by: TC without history is TD.

// the mean delta of an entry's hits from the update's scratch: acc counts 2^-16, cnt the hits
R48_HD float nt_mean(long long acc, uint32_t cnt)
{
    return ((float)acc * (1.0f / 65536.0f)) / (float)cnt;
}

R48_HD float nt_tc_rate(float e, float a)
{
    return a > 0.0f ? __builtin_fminf(__builtin_fabsf(e) / a, 1.0f) : 1.0f;
}

// one entry's update, in place
R48_HD void nt_tc_update(float &table, float &e, float &a, float mean, float step)
{
    const float rate = nt_tc_rate(e, a);
    table += step * (rate * mean);
    e += mean;
    a += __builtin_fabsf(mean);
}

// ---- the TD step ------------------------------------------------------------------------------
// The trainer's error for a board whose previous afterstate had value prev_value, from this step's
// chosen move (merge reward, V of its afterstate): the target is 0 where the previous step ended
// the episode (the board is a fresh game's), else (float)reward + value -- act's score.
//     delta = target - prev_value
// fp32: one conversion (exact, a reward is below 2^24), one addition, one subtraction; there is no
// product, so nothing to contract.
R48_HD float nt_td_delta(uint32_t prev_done, uint32_t reward, float value, float prev_value)
{
    return (prev_done ? 0.0f : (float)(int32_t)reward + value) - prev_value;
}

// What one hit adds to acc for an error delta: clamped to +-2^20, in units of 2^-16, rounded to
// nearest with ties to even (the default rounding mode), so |word| <= 2^36 and 2^26 hits of one
// entry fit in acc. The value of llrintf(d * 65536), which is how HIP's llrintf is defined too.
static constexpr float kNtDeltaClamp = 1048576.0f;   // 2^20
static constexpr float kNtFixedOne = 65536.0f;       // acc counts delta in units of 2^-16

R48_HD long long nt_fixed_delta(float delta)
{
    const float d = __builtin_fminf(__builtin_fmaxf(delta, -kNtDeltaClamp), kNtDeltaClamp);
    return (long long)__builtin_rintf(d * kNtFixedOne);
}

// The mean of rate(e) over the board's 8m hits: fp32, summed from 0 in nt_value's order
// p = 0 .. 8m - 1, one division by (float)(8m) at the end. The loads of one tuple's hits (8 of E,
// 8 of A) are issued before their rates are formed.
template <int L>
R48_HD float nt_tc_rate_mean(const NtBoard &b, const NtLayout &lay, const float *__restrict__ tc_e,
                             const float *__restrict__ tc_a, uint32_t base = 0u)
{
    const int np = kNtSyms * lay.m;
    float sum = 0.0f;
    for (int p = 0; p < np; p += kNtSyms) {
        float e[kNtSyms], a[kNtSyms];
        R48_UNROLL
        for (int j = 0; j < kNtSyms; j++) {
            const uint32_t at = nt_entry<L>(b, lay, p + j, base);
            e[j] = tc_e[at];
            a[j] = tc_a[at];
        }
        R48_UNROLL
        for (int j = 0; j < kNtSyms; j++)
            sum += nt_tc_rate(e[j], a[j]);
    }
    return sum / (float)np;
}

// ---- the search -------------------------------------------------------------------------------

R48_HD float nt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// bit a: move a changes the board
R48_HD uint32_t nt_legal4(const Moves4 &m, const Board &b)
{
    return (differs(m.up, b) ? 1u : 0u) | (differs(m.down, b) ? 2u : 0u) | (differs(m.left, b) ? 4u : 0u) |
           (differs(m.right, b) ? 8u : 0u);
}

// move a of the four, by selects (no indexed private array)
R48_HD Board nt_pick(const Moves4 &m, uint32_t a)
{
    // word by word: a select between whole structs becomes a select of addresses, and with a
    // per-lane a the moves then live in private memory
    const bool v = a < 2u, o = (a & 1u) != 0u;
    return Board{sel(v, sel(o, m.down.w0, m.up.w0), sel(o, m.right.w0, m.left.w0)),
                 sel(v, sel(o, m.down.w1, m.up.w1), sel(o, m.right.w1, m.left.w1)),
                 sel(v, sel(o, m.down.w2, m.up.w2), sel(o, m.right.w2, m.left.w2)),
                 sel(v, sel(o, m.down.w3, m.up.w3), sel(o, m.right.w3, m.left.w3))};
}

R48_HD uint32_t nt_pick_reward(const Moves4 &m, uint32_t a)
{
    return sel(a < 2u, sel((a & 1u) != 0u, m.r_down, m.r_up), sel((a & 1u) != 0u, m.r_right, m.r_left));
}

// the exponent in cell c (0..15)
R48_HD uint32_t nt_cell(const Board &b, uint32_t c)
{
    const uint32_t w = sel((c & 8u) != 0u, sel((c & 4u) != 0u, b.w3, b.w2), sel((c & 4u) != 0u, b.w1, b.w0));
    return (w >> (8u * (c & 3u))) & 0xFFu;
}

// (float)reward + V(afterstate): the score of one move, at either depth. The stage is the
// afterstate's.
template <int L, class Stg = NtPlain>
R48_HD float nt_score(const Board &after, uint32_t reward, const NtLayout &lay, const float *__restrict__ tables,
                      const Stg &stg = Stg())
{
    return (float)(int32_t)reward + nt_value<L>(nt_pack(after), lay, tables, nt_base<L>(stg, lay.m, after));
}

// the best score over the legal moves of `child` (act's), 0 where it has none
template <int L, class Stg = NtPlain>
R48_HD float nt_leaf(const Board &child, const NtLayout &lay, const float *__restrict__ tables, const Stg &stg = Stg())
{
    const Moves4 m = move_rows4<true>(child);
    const uint32_t lg = nt_legal4(m, child);
    float best = 0.0f;
    bool have = false;
    R48_NO_UNROLL
    for (uint32_t a = 0; a < 4u; a++) {
        if (!((lg >> a) & 1u))
            continue;
        const float s = nt_score<L>(nt_pick(m, a), nt_pick_reward(m, a), lay, tables, stg);
        if (!have || s > best) {
            have = true;
            best = s;
        }
    }
    return best;
}

// x_c of the contract: 9 leaf(s[c <- 1]) + leaf(s[c <- 2]), +0 where cell c of s holds a tile
template <int L>
R48_HD float nt_cell_term(const Board &s, uint32_t c, const NtLayout &lay, const float *__restrict__ tables)
{
    if (nt_cell(s, c) != 0u)
        return 0.0f;
    float two = 0.0f, four = 0.0f;
    R48_NO_UNROLL
    for (uint32_t e = 1; e <= 2u; e++) {
        Board child = s;
        place(child, c, e, true);
        const float leaf = nt_leaf<L>(child, lay, tables);
        two = e == 1u ? leaf : two;
        four = leaf;
    }
    return nt_fma(9.0f, two, four);
}

// position of the k-th set bit of m (k counted from 0, k < popcount(m)): a binary search by popcounts
R48_HD uint32_t nt_select_bit(uint64_t m, uint32_t k)
{
    uint32_t w = (uint32_t)m, pos = 0u;
    const uint32_t c = popc(w);
    if (k >= c) {
        k -= c;
        w = (uint32_t)(m >> 32);
        pos = 32u;
    }
    R48_UNROLL
    for (uint32_t sh = 16u; sh >= 1u; sh >>= 1) {
        const uint32_t low = w & ((1u << sh) - 1u);
        const uint32_t cnt = popc(low);
        const bool up = k >= cnt;
        k -= up ? cnt : 0u;
        w = up ? (w >> sh) : low;
        pos += up ? sh : 0u;
    }
    return pos;
}

// Q(a) at depth 2 from the reward, S_a and |E| (>= 1 after a legal move)
R48_HD float nt_q2(uint32_t reward, float s_a, uint32_t n_empty)
{
    return (float)(int32_t)reward + s_a / (float)(10u * n_empty);
}

// first maximiser of four scores; 0 where all are -inf
R48_HD uint32_t nt_argmax4(float q0, float q1, float q2, float q3)
{
    uint32_t a = 0u;
    float best = q0;
    if (q1 > best) {
        best = q1;
        a = 1u;
    }
    if (q2 > best) {
        best = q2;
        a = 2u;
    }
    if (q3 > best)
        a = 3u;
    return a;
}

// the contract's sum of sixteen cell terms, on the host: the butterfly's levels one after another
inline float nt_sum16(const float *x)
{
    float v[16], w[16];
    for (int c = 0; c < 16; c++)
        v[c] = x[c];
    for (int d = 1; d < 16; d <<= 1) {
        for (int c = 0; c < 16; c++)
            w[c] = v[c] + v[c ^ d];
        for (int c = 0; c < 16; c++)
            v[c] = w[c];
    }
    return v[0];
}

template <int L, class Stg = NtPlain>
inline float nt_q_level(const Board &s, uint32_t r, const NtLayout &lay, const float *tables, int k,
                        const Stg &stg = Stg());

// best_k(board) of the contract, on the host: plain recursion. best_1 is nt_leaf.
template <int L, class Stg = NtPlain>
inline float nt_best(const Board &board, const NtLayout &lay, const float *tables, int k, const Stg &stg = Stg())
{
    if (k <= 1)
        return nt_leaf<L>(board, lay, tables, stg);
    const Moves4 m = move_rows4<true>(board);
    const uint32_t lg = nt_legal4(m, board);
    float best = 0.0f;
    bool have = false;
    for (uint32_t a = 0; a < 4u; a++) {
        if (!((lg >> a) & 1u))
            continue;
        const float s = nt_q_level<L>(nt_pick(m, a), nt_pick_reward(m, a), lay, tables, k, stg);
        if (!have || s > best) {
            have = true;
            best = s;
        }
    }
    return best;
}

// Q_k(a), k >= 2, from the move's afterstate s and reward r
template <int L, class Stg>
inline float nt_q_level(const Board &s, uint32_t r, const NtLayout &lay, const float *tables, int k, const Stg &stg)
{
    float x[16];
    for (uint32_t c = 0; c < 16u; c++) {
        x[c] = 0.0f;
        if (nt_cell(s, c) != 0u)
            continue;
        Board two = s, four = s;
        place(two, c, 1u, true);
        place(four, c, 2u, true);
        x[c] = nt_fma(9.0f, nt_best<L>(two, lay, tables, k - 1, stg), nt_best<L>(four, lay, tables, k - 1, stg));
    }
    return nt_q2(r, nt_sum16(x), blanks(s).n);
}

// The whole search of one board, serially, at depth 1..4: the host's restatement of k_nt_search,
// k_nt_search3 and k_nt_search_ruled, which run the same nt_leaf / nt_fma / nt_q2 / nt_argmax4 but
// spread the children over lanes and waves and sum with the butterfly. Returns the action; q[4]
// and legal as the kernels write them.
template <int L, class Stg = NtPlain>
inline uint32_t nt_search_board(const Board &b, const NtLayout &lay, const float *tables, int depth, float q[4],
                                uint32_t &legal, const Stg &stg = Stg())
{
    const Moves4 m = move_rows4<true>(b);
    legal = nt_legal4(m, b);
    for (uint32_t a = 0; a < 4u; a++) {
        q[a] = -__builtin_inff();
        if (!((legal >> a) & 1u))
            continue;
        const Board s = nt_pick(m, a);
        const uint32_t r = nt_pick_reward(m, a);
        if (depth == 1) {
            q[a] = nt_score<L>(s, r, lay, tables, stg);
            continue;
        }
        q[a] = nt_q_level<L>(s, r, lay, tables, depth, stg);
    }
    return nt_argmax4(q[0], q[1], q[2], q[3]);
}

// ---- the ruled search: the depth by the board's blanks -----------------------------------------
static constexpr int kNtRuleLen = 17;      // blanks 0..16
static constexpr int kNtMaxDepth = 4;

// NULL, or what is wrong with a rule
inline const char *nt_rule_check(const uint8_t *rule)
{
    if (!rule)
        return "rule is NULL";
    for (int k = 0; k < kNtRuleLen; k++)
        if (rule[k] < 1 || rule[k] > kNtMaxDepth)
            return "a rule entry is not in 1..4";
    return nullptr;
}

// A checked rule in one word, as it travels to the kernel: depth - 1 of k blanks at bits 2k, 2k + 1.
inline uint64_t nt_rule_pack(const uint8_t *rule)
{
    uint64_t w = 0;
    for (int k = 0; k < kNtRuleLen; k++)
        w |= (uint64_t)(rule[k] - 1u) << (2 * k);
    return w;
}

R48_HD uint32_t nt_packed_rule_depth(uint64_t packed, const Board &b)
{
    return 1u + ((uint32_t)(packed >> (2u * blanks(b).n)) & 3u);
}

// d_i of the contract: rule[blanks(board)]
inline uint32_t nt_rule_depth(const uint8_t *rule, const Board &b) { return rule[blanks(b).n]; }

// The ruled contract for one board: nt_search_board at rule[blanks]; depth_out (nullable) as the
// kernel writes it, whether or not the board has a legal move.
template <int L, class Stg = NtPlain>
inline uint32_t nt_search_board_ruled(const Board &b, const NtLayout &lay, const float *tables, const uint8_t *rule,
                                      float q[4], uint32_t &legal, uint8_t *depth_out, const Stg &stg = Stg())
{
    const uint32_t d = nt_rule_depth(rule, b);
    if (depth_out)
        *depth_out = (uint8_t)d;
    return nt_search_board<L>(b, lay, tables, (int)d, q, legal, stg);
}

// ---- playing whole games ----------------------------------------------------------------------
// The play contract (k_nt_play1, k_nt_play2, and nt_play_board for one board on the host): for
// t = 0 .. n_steps - 1 the board takes the search's action (depth 1: act's, depth 2: the search's)
// and then the env's Philox-mode step with it (r48_env_step, flags 0: no auto-reset) as board
// `gid` of an env with key (k0, k1) at step counter step0 + t (uint32, it wraps) -- draw contract
// 3: step_draw's pair sharing, the rank over the blanks in the line order of the move,
// kFourThresh30. A board without a legal move gets action 0, which leaves it as it is: it is
// finished, and every later step is the identity on it. length counts the steps that changed the
// board, gain sums their merge rewards, done is has_game_over after the last step -- a function of
// the final board alone (game over is invariant under the board's symmetries), so a kernel that
// stops stepping a finished board still writes the last step's done.

// The env's step of one board after the action is chosen: the draw and step_board, stated once for
// the kernels and the host.
R48_HD StepOut nt_play_step(Board &b, uint32_t action, uint64_t gid, uint32_t step, uint32_t k0, uint32_t k1)
{
    uint32_t x, y;
    step_draw(gid, step, k0, k1, x, y);
    return step_board<true, false, true>(b, action, y, (x & 0x3FFFFFFFu) < kFourThresh30);
}

// done as the last step writes it, from the board that step left
R48_HD uint32_t nt_play_done(const Board &b) { return game_over(b, blanks(b).n) ? 1u : 0u; }

// The contract for one board, serially: n_steps x (nt_search_board, nt_play_step), every step made
// whether the board is finished or not. length and gain are added to, done is written (each
// nullable); n_steps == 0 touches nothing.
template <int L, class Stg = NtPlain>
inline void nt_play_board(Board &board, const NtLayout &lay, const float *tables, int depth, int n_steps, uint32_t k0,
                          uint32_t k1, uint64_t gid, uint32_t step0, int32_t *length, int32_t *gain, uint8_t *done,
                          const Stg &stg = Stg())
{
    for (int t = 0; t < n_steps; t++) {
        float q[4];
        uint32_t legal;
        const uint32_t action = nt_search_board<L>(board, lay, tables, depth, q, legal, stg);
        const StepOut o = nt_play_step(board, action, gid, step0 + (uint32_t)t, k0, k1);
        if (length)
            *length += (int32_t)o.changed;
        if (gain)
            *gain += (int32_t)o.reward;
        if (done)
            *done = (uint8_t)o.done;
    }
}

// The ruled play contract (k_nt_play_ruled, and nt_play_board_ruled for one board on the host): the
// play contract above with the ruled search choosing the move. For t = 0 .. n_steps - 1 the board
//   1. takes the action of the ruled search of its CURRENT board: nt_search_board_ruled under
//      `rule`, i.e. the search at depth rule[blanks(board)], 1..4 -- the depth follows the game,
//   2. makes nt_play_step with it: draw contract 3 as board `gid` at step counter step0 + t (uint32,
//      it wraps), no auto-reset.
// length, gain and done mean what they mean above: length and gain are added to, so chunked calls
// add up, done is nt_play_done of the final board, and a board without a legal move is finished:
// every later step is the identity on it, whatever its depth. Everything equals n_steps x
// (r48_ntuple_search_ruled, r48_env_step) bit for bit, for every n, gid, step0 and rule; the bits
// depend neither on the number of waves that share a board nor on how its children were dealt.
template <int L, class Stg = NtPlain>
inline void nt_play_board_ruled(Board &board, const NtLayout &lay, const float *tables, const uint8_t *rule, int n_steps,
                                uint32_t k0, uint32_t k1, uint64_t gid, uint32_t step0, int32_t *length, int32_t *gain,
                                uint8_t *done, const Stg &stg = Stg())
{
    for (int t = 0; t < n_steps; t++) {
        float q[4];
        uint32_t legal;
        const uint32_t action = nt_search_board_ruled<L>(board, lay, tables, rule, q, legal, nullptr, stg);
        const StepOut o = nt_play_step(board, action, gid, step0 + (uint32_t)t, k0, k1);
        if (length)
            *length += (int32_t)o.changed;
        if (gain)
            *gain += (int32_t)o.reward;
        if (done)
            *done = (uint8_t)o.done;
    }
}

// ---- the staged update on the host, in the PULL form -------------------------------------------
// The kernels store an unowned entry's value eagerly (the owner of the nearest lower owned stage
// pushes it). Here nothing is pushed: tables[k][e] of an unowned (k, e) is never read or written, a
// read RESOLVES to the nearest lower owned stage (stage 0 owns everything), and the first touch of
// (s, e) copies the resolved value in before the call's updates run. The contract says the two
// agree bit for bit on every resolved entry.
#if !defined(__HIP_DEVICE_COMPILE__)

// the value entry e (an offset within one stage, t * 16^L + index) reads as in stage s
inline float nt_pull_read(const float *tables, const uint8_t *own, int64_t stage_size, int s, int64_t e)
{
    while (s > 0 && !own[s * stage_size + e])
        s--;
    return tables[s * stage_size + e];
}

// One update call, serially: boards[i] with valid[i] != 0 (valid nullable) add delta[i] over their 8m
// hits; every touched entry then moves by step * its mean delta, with tc_e / tc_a (both or neither)
// by nt_tc_update. All arrays [S][m][16^L], S = cuts.n + 1.
template <int L>
inline void nt_staged_update_pull(const Board *boards, const float *delta, const uint8_t *valid, int64_t n,
                                  const NtLayout &lay, const NtCuts &cuts, float step, float *tables, float *tc_e,
                                  float *tc_a, uint8_t *own)
{
    struct Sum {
        long long acc = 0;
        uint32_t cnt = 0;
    };
    const int64_t stage_size = (int64_t)lay.m << (4 * L);
    std::map<int64_t, Sum> sums;   // by s * stage_size + e: ascending stages for one e
    for (int64_t i = 0; i < n; i++) {
        if (valid && !valid[i])
            continue;
        const NtBoard nb = nt_pack(boards[i]);
        const int64_t s = nt_stage(cuts, boards[i]);
        for (int p = 0; p < kNtSyms * lay.m; p++) {
            Sum &x = sums[s * stage_size + nt_entry<L>(nb, lay, p)];
            x.acc += nt_fixed_delta(delta[i]);
            x.cnt += 1u;
        }
    }
    // first touches: the pre-call value of the nearest lower owned stage (ascending keys, so a lower
    // stage touched for the first time in this call is resolved before a higher one copies from it)
    for (const auto &kv : sums) {
        const int64_t s = kv.first / stage_size, e = kv.first % stage_size;
        if (!own[kv.first]) {
            tables[kv.first] = nt_pull_read(tables, own, stage_size, (int)s, e);
            own[kv.first] = 1;
        }
    }
    for (const auto &kv : sums) {
        const float mean = nt_mean(kv.second.acc, kv.second.cnt);
        if (tc_e)
            nt_tc_update(tables[kv.first], tc_e[kv.first], tc_a[kv.first], mean, step);
        else
            tables[kv.first] += step * mean;
    }
}
#endif

}  // namespace r48
