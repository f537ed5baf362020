// The naive restatement of the multi-stage n-tuple network for the native stage test: the stage of
// a board cell by cell, V over explicit board transforms in float64, and the staged update in the
// PUSH form the kernels run (mark in the accumulate pass; apply pass: new value, then copied upwards
// to the first owned stage) -- written over ntuple_naive.h's grids and indices, not over
// r48_ntuple.h's placed tuples. Only the update's scalar arithmetic (nt_fixed_delta, nt_mean,
// nt_tc_update: tested on their own in ntuple_tc_test.cpp) is the header's. A CPU test harness,
// never shipped.
#pragma once
#include <map>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

// stage(b) = #{ j : max over the cells of min(b[c], 15) >= cuts[j] }
inline int naive_stage(const int8_t *b, const uint8_t *cuts, int n_cuts)
{
    int top = 0;
    for (int c = 0; c < 16; c++) {
        const int e = b[c] < 15 ? b[c] : 15;
        top = e > top ? e : top;
    }
    int s = 0;
    for (int j = 0; j < n_cuts; j++)
        s += top >= cuts[j] ? 1 : 0;
    return s;
}

// the 8m entries of a board within its stage's [m][16^L] block, one per (transform, tuple)
inline std::vector<size_t> naive_hits(const Layout &ly, const int8_t *b)
{
    std::vector<size_t> hits;
    const Grid g0 = grid_of(b);
    for (int g = 0; g < 8; g++) {
        Grid t;
        transform(g, g0, t);
        for (int k = 0; k < ly.m; k++)
            hits.push_back(((size_t)k << (4 * ly.L)) + naive_index(t, ly.cells + k * ly.L, ly.L));
    }
    return hits;
}

// V of a staged net in float64: the board's stage block, no fallback
inline double naive_value_staged(const Layout &ly, const std::vector<float> &tables, const int8_t *b, const uint8_t *cuts,
                                 int n_cuts)
{
    const size_t block = (size_t)ly.m << (4 * ly.L);
    double v = 0.0;
    for (size_t e : naive_hits(ly, b))
        v += tables[naive_stage(b, cuts, n_cuts) * block + e];
    return v;
}

// a staged net's arrays, [S][m][16^L] each (tc_e / tc_a empty without TC)
struct StagedNet {
    int S;
    size_t block;
    std::vector<float> tables, tc_e, tc_a;
    std::vector<uint8_t> own;
    StagedNet(const Layout &ly, int n_cuts, bool tc)
        : S(n_cuts + 1), block((size_t)ly.m << (4 * ly.L)), tables(S * block, 0.0f), tc_e(tc ? S * block : 0, 0.0f),
          tc_a(tc ? S * block : 0, 0.0f), own(S * block, 0)
    {
        for (size_t e = 0; e < block; e++)
            own[e] = 1;
    }
};

// One update call in the push form: boards[16 i ..] with valid[i] != 0 add delta[i] over their hits.
inline void naive_update_push(const Layout &ly, StagedNet &net, const int8_t *boards, const float *delta,
                              const uint8_t *valid, int n, const uint8_t *cuts, int n_cuts, float step)
{
    std::map<size_t, std::pair<long long, uint32_t>> sums;
    for (int i = 0; i < n; i++) {   // accumulate, and mark
        if (valid && !valid[i])
            continue;
        const int s = naive_stage(boards + 16 * i, cuts, n_cuts);
        for (size_t e : naive_hits(ly, boards + 16 * i)) {
            auto &x = sums[s * net.block + e];
            x.first += r48::nt_fixed_delta(delta[i]);
            x.second += 1u;
            if (s >= 1)
                net.own[s * net.block + e] = 1;
        }
    }
    // apply, highest entries first: the order must not matter, and it is not the pull form's
    for (auto it = sums.rbegin(); it != sums.rend(); ++it) {
        const size_t at = it->first;
        const float mean = r48::nt_mean(it->second.first, it->second.second);
        if (!net.tc_e.empty())
            r48::nt_tc_update(net.tables[at], net.tc_e[at], net.tc_a[at], mean, step);
        else
            net.tables[at] += step * mean;
        for (size_t k = at + net.block; k < net.S * net.block && !net.own[k]; k += net.block)
            net.tables[k] = net.tables[at];
    }
}
