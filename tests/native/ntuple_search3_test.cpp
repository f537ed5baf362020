// Host build of the n-tuple network's per-board search at depth 3 (rein48_amd/csrc/r48_ntuple.h:
// nt_search_board, nt_best, nt_q_level -- the contract k_nt_search3 shares) checked against a naive
// restatement (ntuple_naive.h and here): explicit 4x4 arrays, its own line-by-line move, eight explicit board
// transforms for the value, plain recursion over the plies, float64 throughout -- a CPU test
// harness, never shipped. Build+run: tests/test_ntuple_search3_host.py (g++ -O2).
//
// The bound, with u = 2^-24, carried up the tree as (value, error, magnitude) per node:
//   a reply's score r + V: the value's 8m sequential adds are within 8m u sum |hits|, the add of
//     the reward rounds once on at most mag = |r| + sum |hits|;
//   best_k, a max over the legal replies: off by at most the largest of their errors, magnitude
//     the largest of theirs; 0 / 0 / 0 where there is no reply;
//   one level, Q_k(a) from the children's best_(k-1): s_err = sum of 9 err1 + err2 and s_mag =
//     sum of 9 mag1 + mag2 over the empty cells, d = 10 |E| (exact). The fma rounds once per cell
//     (u s_mag in all), the butterfly's 4 levels once each on partial sums bounded by s_mag
//     (4 u s_mag), the division once (u s_mag / d), the last add once (u (|r| + s_mag / d)):
//       err = ((s_err + 5 u s_mag) / d + u s_mag / d + u (|r| + s_mag / d)) (1 + 2^-16),
//       mag = |r| + s_mag / d,
//     the last factor for the products of the level's chained roundings (at most ~130).
// Depth 3 applies the level twice. Legal sets are exact; q is within err; the action is legal and
// its float64 Q is within err[action] + err[a'] of every other legal move's.
#include <random>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

using r48::Board;

static int blanks_of(const Grid &b)
{
    int n = 0;
    for (int c = 0; c < 16; c++)
        n += b.g[c >> 2][c & 3] == 0;
    return n;
}

static const double U = std::ldexp(1.0, -24);

struct Est {
    double val, err, mag;
};

struct Tally {
    long boards, big_roots, big_children, over_children, over_grandchildren, no_move_boards;
};

struct Naive {
    const Layout &ly;
    const std::vector<float> &tables;
    Tally &tally;
    int depth;   // of the whole search: a node k plies above the leaves is depth - k below the root

    Est q_level(const Grid &s, double r, int k)
    {
        double S = 0.0, s_err = 0.0, s_mag = 0.0;
        int n = 0;
        for (int c = 0; c < 16; c++) {
            if (s.g[c >> 2][c & 3])
                continue;
            n++;
            for (int e = 1; e <= 2; e++) {
                Grid child = s;
                child.g[c >> 2][c & 3] = e;
                const Est b = best(child, k - 1);
                const double w = e == 1 ? 9.0 : 1.0;
                S += w * b.val;
                s_err += w * b.err;
                s_mag += w * b.mag;
            }
        }
        const double d = 10.0 * n;
        Est q;
        q.val = r + S / d;
        q.err = ((s_err + 5.0 * U * s_mag) / d + U * s_mag / d + U * (std::fabs(r) + s_mag / d)) * (1.0 + std::ldexp(1.0, -16));
        q.mag = std::fabs(r) + s_mag / d;
        return q;
    }

    Est move_value(const Grid &after, double r, int k)
    {
        if (k >= 2)
            return q_level(after, r, k);
        double habs;
        Est q;
        q.val = r + naive_value(ly, tables, after, &habs);
        q.mag = std::fabs(r) + habs;
        q.err = 8.0 * ly.m * U * habs + U * q.mag;
        return q;
    }

    // best_k of a board that is depth - k spawns below the root
    Est best(const Grid &b, int k)
    {
        Est out = {0.0, 0.0, 0.0};
        bool have = false;
        int kids = 0;
        for (int a = 0; a < 4; a++) {
            Grid after;
            long r;
            if (!naive_move(b, a, after, r))
                continue;
            kids += 2 * blanks_of(after);
            const Est q = move_value(after, (double)r, k);
            out.val = have ? std::fmax(out.val, q.val) : q.val;
            out.err = std::fmax(out.err, q.err);
            out.mag = std::fmax(out.mag, q.mag);
            have = true;
        }
        if (k == depth - 1 && kids > 64)
            tally.big_children++;
        if (!have && k == depth - 1)
            tally.over_children++;
        if (!have && k == depth - 2)
            tally.over_grandchildren++;
        return out;
    }
};

// ---- the comparison -------------------------------------------------------------------------
static std::vector<float> make_tables(int m, int L, uint64_t seed, bool integer)
{
    std::mt19937_64 rng(seed);
    std::vector<float> t((size_t)m << (4 * L));
    for (auto &x : t)
        x = integer ? (float)((int)(rng() % 17) - 8) : (float)(((double)(rng() >> 11) / 9007199254740992.0 - 0.5) * 74.0);
    return t;
}

template <int L>
static void check_board(const Layout &ly, const r48::NtLayout &lay, const std::vector<float> &tables, const int8_t *b,
                        const char *what, long it, Tally &tally, double &worst)
{
    const Grid g = grid_of(b);
    Naive naive{ly, tables, tally, 3};
    Est want[4];
    int want_legal = 0, kids = 0;
    for (int a = 0; a < 4; a++) {
        Grid after;
        long r;
        if (!naive_move(g, a, after, r))
            continue;
        want_legal |= 1 << a;
        kids += 2 * blanks_of(after);
        want[a] = naive.move_value(after, (double)r, 3);
    }
    tally.boards++;
    tally.big_roots += kids > 64;
    tally.no_move_boards += want_legal == 0;
    float q[4];
    uint32_t legal = 99u;
    const uint32_t action = r48::nt_search_board<L>(load(b), lay, tables.data(), 3, q, legal);
    CHECK((int)legal == want_legal, "%s %s it=%ld legal %u want %d", ly.name, what, it, legal, want_legal);
    CHECK(action == r48::nt_argmax4(q[0], q[1], q[2], q[3]), "%s %s it=%ld action %u is not the first maximiser", ly.name,
          what, it, action);
    CHECK(want_legal ? ((want_legal >> action) & 1) : action == 0u, "%s %s it=%ld action %u, legal %d", ly.name, what, it,
          action, want_legal);
    for (int a = 0; a < 4; a++) {
        if (!((want_legal >> a) & 1)) {
            CHECK(std::isinf(q[a]) && q[a] < 0, "%s %s it=%ld q[%d] = %g of an illegal move", ly.name, what, it, a, q[a]);
            continue;
        }
        const double err = std::fabs((double)q[a] - want[a].val);
        CHECK(err <= want[a].err, "%s %s it=%ld q[%d] = %.9g want %.12g bound %g", ly.name, what, it, a, q[a], want[a].val,
              want[a].err);
        if (want[a].err > 0)
            worst = std::fmax(worst, err / want[a].err);
        if ((want_legal >> action) & 1)
            CHECK(want[action].val >= want[a].val - want[action].err - want[a].err,
                  "%s %s it=%ld action %u (Q %.12g) is not a maximiser: Q[%d] = %.12g", ly.name, what, it, action,
                  want[action].val, a, want[a].val);
    }
    // depths 1 and 2 keep the bits of the composition they were before depth 3 came
    for (int depth = 1; depth <= 2; depth++) {
        float q12[4], old[4];
        uint32_t lg;
        r48::nt_search_board<L>(load(b), lay, tables.data(), depth, q12, lg);
        const r48::Moves4 m = r48::move_rows4<true>(load(b));
        for (uint32_t a = 0; a < 4u; a++) {
            old[a] = -INFINITY;
            if (!((lg >> a) & 1u))
                continue;
            const Board s = r48::nt_pick(m, a);
            const uint32_t r = r48::nt_pick_reward(m, a);
            float x[16];
            for (uint32_t c = 0; c < 16u; c++)
                x[c] = r48::nt_cell_term<L>(s, c, lay, tables.data());
            old[a] = depth == 1 ? r48::nt_score<L>(s, r, lay, tables.data()) : r48::nt_q2(r, r48::nt_sum16(x), r48::blanks(s).n);
        }
        CHECK(memcmp(q12, old, sizeof old) == 0, "%s %s it=%ld depth %d bits changed", ly.name, what, it, depth);
    }
}

template <int L>
static void run_layout(const Layout &ly, bool integer, long n_random)
{
    r48::NtLayout lay;
    const char *why = r48::nt_expand(ly.cells, ly.m, L, lay);
    CHECK(why == nullptr, "%s: nt_expand refused: %s", ly.name, why ? why : "");
    if (why)
        return;
    const std::vector<float> tables = make_tables(ly.m, L, 11 + L + integer, integer);
    Tally tally = {0, 0, 0, 0, 0, 0};
    double worst = 0.0;
    std::mt19937_64 rng(4096 + L + integer);
    for (long it = 0; it < n_random; it++) {
        int8_t b[16];
        const int emax = 1 + (int)(rng() % 17);          // exponents up to 17
        const int fill = 6 + (int)(rng() % 11);          // 6..16 of 16: the sparse end is the crafted boards'
        for (int k = 0; k < 16; k++)
            b[k] = ((int)(rng() % 16) < fill) ? (int8_t)(1 + rng() % emax) : 0;
        check_board<L>(ly, lay, tables, b, "random", it, tally, worst);
    }
    const int8_t crafted[][16] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},        // empty: no move
        {0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},        // one tile: 120 children, children with more than 64
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1},        // full, no move
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 2, 1, 3},        // LEFT / RIGHT leave one blank; a 2 spawned after LEFT ends the game
        {1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12},     // only UP / DOWN
        {0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0},        // merge once
        {17, 17, 16, 0, 0, 3, 0, 0, 0, 0, 0, 0, 1, 0, 0, 17},    // reward 2^18
        {3, 7, 7, 3, 7, 1, 1, 7, 7, 1, 1, 7, 3, 7, 7, 3},        // fully symmetric: opposite moves tie
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 0},        // one blank in a corner: two legal moves, one blank after each
    };
    for (size_t k = 0; k < sizeof crafted / sizeof crafted[0]; k++)
        check_board<L>(ly, lay, tables, crafted[k], "crafted", (long)k, tally, worst);
    {
        float q[4];
        uint32_t legal;
        // integer tables: the leaves of mirrored boards are bit-equal, and the butterfly's order is invariant
        // under c -> c ^ k, so UP / DOWN (c ^ 12) and LEFT / RIGHT (c ^ 3) tie bit for bit; a transposed
        // afterstate adds the same leaves in another order and may differ in the last bit
        for (int k : {1, 7}) {
            const uint32_t act = r48::nt_search_board<L>(load(crafted[k]), lay, tables.data(), 3, q, legal);
            CHECK(legal == 15u && (!integer || (memcmp(&q[0], &q[1], 4) == 0 && memcmp(&q[2], &q[3], 4) == 0 &&
                                                (act == 0u || act == 2u))),
                  "%s: crafted board %d's mirrored moves tie bit for bit: %.9g %.9g %.9g %.9g", ly.name, k, q[0], q[1], q[2],
                  q[3]);
        }
        CHECK(r48::nt_search_board<L>(load(crafted[0]), lay, tables.data(), 3, q, legal) == 0u && legal == 0u &&
                  std::isinf(q[0]) && std::isinf(q[1]) && std::isinf(q[2]) && std::isinf(q[3]),
              "%s: the empty board", ly.name);
    }
    CHECK(tally.big_roots >= 1 && tally.big_children >= 1 && tally.over_children >= 1 && tally.over_grandchildren >= 1 &&
              tally.no_move_boards >= 2,
          "%s: the boards do not cover the ground: %ld %ld %ld %ld %ld", ly.name, tally.big_roots, tally.big_children,
          tally.over_children, tally.over_grandchildren, tally.no_move_boards);
    printf("%s %s tables: %ld boards, worst err / bound %.3g; boards with > 64 children %ld, children with > 64 %ld, "
           "game-over children %ld, game-over grandchildren %ld, boards without a move %ld\n",
           ly.name, integer ? "integer" : "float", tally.boards, worst, tally.big_roots, tally.big_children,
           tally.over_children, tally.over_grandchildren, tally.no_move_boards);
}

int main()
{
    for (const Layout *ly : {&k3x3, &kLinesSquares})
        for (int integer = 0; integer <= 1; integer++) {
            if (ly->L == 3)
                run_layout<3>(*ly, integer != 0, 40);
            else
                run_layout<4>(*ly, integer != 0, 40);
        }
    printf("ntuple_search3_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
