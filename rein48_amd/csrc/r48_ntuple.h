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
#pragma once
#include <stdint.h>

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

// entry of hit p = 8t + g in the contiguous tables[m][16^L]
template <int L>
R48_HD uint32_t nt_entry(const NtBoard &b, const NtLayout &lay, int p)
{
    return ((uint32_t)(p >> 3) << (4 * L)) + nt_index<L>(b, lay.placed[p]);
}

// V(b) in the contract's order. The loads of two tuples (16 hits) are issued before their adds.
template <int L>
R48_HD float nt_value(const NtBoard &b, const NtLayout &lay, const float *__restrict__ tables)
{
    const int np = kNtSyms * lay.m;
    float sum = 0.0f;
    int p = 0;
    for (; p + 16 <= np; p += 16) {
        float v[16];
        R48_UNROLL
        for (int j = 0; j < 16; j++)
            v[j] = tables[nt_entry<L>(b, lay, p + j)];
        R48_UNROLL
        for (int j = 0; j < 16; j++)
            sum += v[j];
    }
    if (p < np) {
        float v[8];
        R48_UNROLL
        for (int j = 0; j < 8; j++)
            v[j] = tables[nt_entry<L>(b, lay, p + j)];
        R48_UNROLL
        for (int j = 0; j < 8; j++)
            sum += v[j];
    }
    return sum;
}

}  // namespace r48
