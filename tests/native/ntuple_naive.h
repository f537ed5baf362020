// What the native n-tuple tests (ntuple_*_test.cpp) share: the CHECK scaffolding and the naive
// restatement of the game and the network that rein48_amd/csrc/r48_ntuple.h is held to -- explicit
// 4x4 arrays, a line-by-line move, eight explicit board transforms, the index cell by cell, float64.
// Nothing below the scaffolding uses r48_ntuple.h or r48_board.h. A CPU test harness, never shipped.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rein48_amd/csrc/r48_board.h"

// ---- scaffolding ------------------------------------------------------------------------------
inline int fails = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (fails < 20) {                             \
                fprintf(stderr, "FAIL %s:%d ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);             \
                fprintf(stderr, "\n");                    \
            }                                             \
            fails++;                                      \
        }                                                 \
    } while (0)

// board bytes -> the Board of the header under test
inline r48::Board load(const int8_t *b)
{
    r48::Board r;
    memcpy(&r, b, 16);
    return r;
}

inline uint32_t bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// ---- the naive restatement ------------------------------------------------------------------
struct Grid {
    int g[4][4];
};

inline Grid grid_of(const int8_t *b)
{
    Grid x;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++)
            x.g[r][c] = b[4 * r + c];
    return x;
}

// one line toward index 0: drop the blanks, merge equal neighbours once from the wall outwards
inline long move_line(int line[4])
{
    int t[4], k = 0;
    long reward = 0;
    for (int i = 0; i < 4; i++)
        if (line[i])
            t[k++] = line[i];
    int out[4] = {0, 0, 0, 0}, o = 0;
    for (int i = 0; i < k; i++) {
        if (i + 1 < k && t[i] == t[i + 1]) {
            out[o++] = t[i] + 1;
            reward += 1L << (t[i] + 1);
            i++;
        } else {
            out[o++] = t[i];
        }
    }
    for (int i = 0; i < 4; i++)
        line[i] = out[i];
    return reward;
}

// action 0 UP, 1 DOWN, 2 LEFT, 3 RIGHT; returns whether the grid changed
inline bool naive_move(const Grid &in, int a, Grid &out, long &reward)
{
    out = in;
    reward = 0;
    for (int l = 0; l < 4; l++) {
        int line[4];
        for (int k = 0; k < 4; k++) {
            const int j = (a & 1) ? 3 - k : k;   // DOWN / RIGHT: counted from the far wall
            line[k] = a < 2 ? in.g[j][l] : in.g[l][j];
        }
        reward += move_line(line);
        for (int k = 0; k < 4; k++) {
            const int j = (a & 1) ? 3 - k : k;
            (a < 2 ? out.g[j][l] : out.g[l][j]) = line[k];
        }
    }
    return memcmp(&in, &out, sizeof in) != 0;
}

struct Layout {
    const char *name;
    int m, L;
    uint8_t cells[48];
};

inline const Layout kLinesSquares = {"lines-squares", 5, 4, {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 4, 5, 1, 2, 5, 6, 5, 6, 9, 10}};
inline const Layout k4x6 = {"4x6", 4, 6, {0, 1, 2, 3, 4, 5, 4, 5, 6, 7, 8, 9, 0, 1, 2, 4, 5, 6, 4, 5, 6, 8, 9, 10}};
inline const Layout k3x3 = {"3x3", 3, 3, {0, 1, 2, 5, 9, 10, 15, 3, 12}};
inline const Layout k1x2 = {"1x2", 1, 2, {7, 8}};
inline const Layout k8x5 = {"8x5", 8, 5, {0, 1, 2, 3, 4,  5, 6, 7, 8, 9,  10, 11, 12, 13, 14,  15, 0, 5, 10, 3,
                                          12, 9, 6, 3, 0,  1, 4, 2, 8, 15,  14, 13, 11, 7, 2,  6, 10, 14, 12, 4}};

// the eight symmetries of the square as explicit transforms of a 4x4 grid: out[r][c] = ...
inline void transform(int which, const Grid &in, Grid &out)
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            int sr, sc;
            switch (which) {
            case 0: sr = r; sc = c; break;              // identity
            case 1: sr = 3 - c; sc = r; break;          // quarter turn
            case 2: sr = 3 - r; sc = 3 - c; break;      // half turn
            case 3: sr = c; sc = 3 - r; break;          // three quarter turn
            case 4: sr = r; sc = 3 - c; break;          // mirror left-right
            case 5: sr = 3 - r; sc = c; break;          // mirror top-bottom
            case 6: sr = c; sc = r; break;              // main diagonal
            default: sr = 3 - c; sc = 3 - r; break;     // anti-diagonal
            }
            out.g[r][c] = in.g[sr][sc];
        }
}

// the entry of one tuple on a grid: sum over k of min(cell_k, 15) * 16^k
inline size_t naive_index(const Grid &b, const uint8_t *tuple, int L)
{
    size_t idx = 0, scale = 1;
    for (int k = 0; k < L; k++) {
        const int e = b.g[tuple[k] >> 2][tuple[k] & 3];
        idx += (size_t)(e < 15 ? e : 15) * scale;
        scale *= 16;
    }
    return idx;
}

// V in float64 and, where asked for, the sum of its hits' magnitudes
inline double naive_value(const Layout &ly, const std::vector<float> &tables, const Grid &b, double *habs = nullptr)
{
    double v = 0.0, mag = 0.0;
    for (int g = 0; g < 8; g++) {
        Grid t;
        transform(g, b, t);
        for (int k = 0; k < ly.m; k++) {
            const double h = tables[((size_t)k << (4 * ly.L)) + naive_index(t, ly.cells + k * ly.L, ly.L)];
            v += h;
            mag += std::fabs(h);
        }
    }
    if (habs)
        *habs = mag;
    return v;
}
