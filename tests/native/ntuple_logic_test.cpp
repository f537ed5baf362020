// Host build of the n-tuple network's layout expansion, entry index and value sum
// (rein48_amd/csrc/r48_ntuple.h) checked against the naive restatement of ntuple_naive.h: eight
// explicit board transforms, the index cell by cell -- a CPU test harness, never shipped. Build+run:
// tests/test_ntuple_host.py (g++ -O2).
#include <algorithm>
#include <random>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

using r48::Board;

// the 8 indices of tuple t on board b, sorted (the enumeration order of the symmetries is free)
static void naive_hits(const int8_t *b, const uint8_t *tuple, int L, uint32_t out[8])
{
    for (int g = 0; g < 8; g++) {
        Grid tb;
        transform(g, grid_of(b), tb);
        out[g] = (uint32_t)naive_index(tb, tuple, L);
    }
    std::sort(out, out + 8);
}

// ---- the header under test ------------------------------------------------------------------
template <int L>
static void header_hits(const Board &b, const r48::NtLayout &lay, int t, uint32_t out[8])
{
    const r48::NtBoard nb = r48::nt_pack(b);
    for (int g = 0; g < 8; g++) {
        out[g] = r48::nt_index<L>(nb, lay.placed[8 * t + g]);
        CHECK(r48::nt_entry<L>(nb, lay, 8 * t + g) == ((uint32_t)t << (4 * L)) + out[g], "nt_entry t=%d g=%d", t, g);
    }
    std::sort(out, out + 8);
}

// integer tables in [-1024, 1024]: any summation order is exact in fp32
static std::vector<float> int_tables(int m, int L, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    std::vector<float> t((size_t)m << (4 * L));
    for (auto &x : t)
        x = (float)((int)(rng() % 2049) - 1024);
    return t;
}

template <int L>
static void check_board(const Layout &ly, const r48::NtLayout &lay, const std::vector<float> &tables, const int8_t *b,
                        const char *what, long it)
{
    // the nibble packing: min(cell, 15) at bits 4c
    const r48::NtBoard nb = r48::nt_pack(load(b));
    const uint64_t packed = ((uint64_t)nb.hi << 32) | nb.lo;
    for (int c = 0; c < 16; c++)
        CHECK(((packed >> (4 * c)) & 15u) == (uint32_t)(b[c] < 15 ? b[c] : 15), "%s %s it=%ld pack cell %d", ly.name,
              what, it, c);
    double want = 0.0;
    for (int t = 0; t < ly.m; t++) {
        uint32_t a[8], h[8];
        naive_hits(b, ly.cells + t * L, L, a);
        header_hits<L>(load(b), lay, t, h);
        CHECK(memcmp(a, h, sizeof a) == 0, "%s %s it=%ld tuple %d hits differ", ly.name, what, it, t);
        if (!tables.empty())
            for (int g = 0; g < 8; g++)
                want += tables[((size_t)t << (4 * L)) + a[g]];
    }
    if (!tables.empty()) {
        const float got = r48::nt_value<L>(nb, lay, tables.data());
        CHECK((double)got == want, "%s %s it=%ld value %f want %f", ly.name, what, it, got, want);
    }
}

template <int L>
static void run_layout(const Layout &ly)
{
    r48::NtLayout lay;
    const char *why = r48::nt_expand(ly.cells, ly.m, L, lay);
    CHECK(why == nullptr, "%s: nt_expand refused: %s", ly.name, why ? why : "");
    if (why)
        return;
    CHECK(lay.m == ly.m && lay.L == L, "%s: m / L", ly.name);
    // the value sum needs real tables: skip it where they would take 256 MB (the index is checked)
    std::vector<float> tables;
    if (L <= 5)
        tables = int_tables(ly.m, L, 99 + L);
    std::mt19937_64 rng(4096 + L);
    for (long it = 0; it < 100000; it++) {          // 100k random boards, exponents 0..18
        int8_t b[16];
        const int emax = 1 + (int)(rng() % 18);
        const int fill = (int)(rng() % 17);
        for (int k = 0; k < 16; k++)
            b[k] = ((int)(rng() % 16) < fill) ? (int8_t)(1 + rng() % emax) : 0;
        check_board<L>(ly, lay, tables, b, "random", it);
    }
    {
        int8_t b[16] = {0};                          // the empty board: every hit is entry 0
        check_board<L>(ly, lay, tables, b, "empty", 0);
        uint32_t h[8];
        header_hits<L>(load(b), lay, 0, h);
        CHECK(h[0] == 0u && h[7] == 0u, "%s: empty board hits entry 0", ly.name);
    }
    {
        // fully symmetric under all 8 transforms: corners a, edges b, centre c -> all 8 hits equal
        const int8_t b[16] = {3, 7, 7, 3, 7, 1, 1, 7, 7, 1, 1, 7, 3, 7, 7, 3};
        check_board<L>(ly, lay, tables, b, "symmetric", 0);
        for (int t = 0; t < ly.m; t++) {
            uint32_t h[8];
            header_hits<L>(load(b), lay, t, h);
            CHECK(h[0] == h[7], "%s: symmetric board, tuple %d hits differ", ly.name, t);
        }
    }
    for (int big = 16; big <= 18; big++) {           // the clamp: 16, 17, 18 share entry 15
        int8_t b[16], c[16];
        for (int k = 0; k < 16; k++) {
            b[k] = (int8_t)((k % 3 == 0) ? big : (k % 5));
            c[k] = (int8_t)((k % 3 == 0) ? 15 : (k % 5));
        }
        check_board<L>(ly, lay, tables, b, "clamp", big);
        for (int t = 0; t < ly.m; t++) {
            uint32_t hb[8], hc[8];
            header_hits<L>(load(b), lay, t, hb);
            header_hits<L>(load(c), lay, t, hc);
            CHECK(memcmp(hb, hc, sizeof hb) == 0, "%s: exponent %d does not share entry 15, tuple %d", ly.name, big, t);
        }
        int8_t all[16];
        memset(all, big, 16);
        uint32_t h[8];
        header_hits<L>(load(all), lay, 0, h);
        CHECK(h[0] == (uint32_t)r48::nt_table_size(L) - 1u && h[7] == h[0], "%s: all-%d board hits the last entry",
              ly.name, big);
    }
}

int main()
{
    for (const Layout *ly : {&kLinesSquares, &k4x6, &k3x3, &k1x2, &k8x5}) {
        switch (ly->L) {
        case 2: run_layout<2>(*ly); break;
        case 3: run_layout<3>(*ly); break;
        case 4: run_layout<4>(*ly); break;
        case 5: run_layout<5>(*ly); break;
        default: run_layout<6>(*ly); break;
        }
    }
    // the eight placed symmetries are eight different maps of the cells, each a bijection
    {
        for (int g = 0; g < 8; g++) {
            uint32_t seen = 0;
            for (int c = 0; c < 16; c++)
                seen |= 1u << r48::nt_sym_cell(g, c);
            CHECK(seen == 0xFFFFu, "sym %d is not a bijection", g);
            for (int h = 0; h < g; h++) {
                bool same = true;
                for (int c = 0; c < 16; c++)
                    same = same && r48::nt_sym_cell(g, c) == r48::nt_sym_cell(h, c);
                CHECK(!same, "syms %d and %d coincide", g, h);
            }
        }
    }
    // what nt_expand refuses
    {
        r48::NtLayout lay;
        const uint8_t ok[4] = {0, 1, 4, 5}, big[4] = {0, 1, 16, 5}, rep[4] = {0, 1, 4, 1};
        CHECK(r48::nt_expand(ok, 2, 2, lay) == nullptr && r48::nt_expand(ok, 1, 4, lay) == nullptr, "good layouts");
        CHECK(r48::nt_expand(nullptr, 1, 4, lay) != nullptr, "NULL cells");
        CHECK(r48::nt_expand(ok, 0, 4, lay) != nullptr && r48::nt_expand(ok, 9, 2, lay) != nullptr, "m out of range");
        CHECK(r48::nt_expand(ok, 1, 1, lay) != nullptr && r48::nt_expand(ok, 1, 7, lay) != nullptr, "L out of range");
        CHECK(r48::nt_expand(big, 1, 4, lay) != nullptr, "cell >= 16");
        CHECK(r48::nt_expand(rep, 1, 4, lay) != nullptr, "repeated cell");
        CHECK(r48::nt_expand(rep, 2, 2, lay) == nullptr, "a cell may repeat across tuples");
    }
    printf("ntuple_logic_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
