// Host build of the n-tuple network's per-board search at depth 4 and of the ruled wrapper
// (rein48_amd/csrc/r48_ntuple.h: nt_search_board over nt_best / nt_q_level, nt_rule_depth,
// nt_search_board_ruled -- the contract k_nt_search_ruled shares) checked against the naive
// restatement of ntuple_naive.h and here: explicit 4x4 arrays, its own line-by-line move, eight
// explicit board transforms for the value, plain recursion over the plies, float64 throughout -- a
// CPU test harness, never shipped. Build+run: tests/test_ntuple_search_ruled_host.py (g++ -O2).
//
// The bound is the 3-ply test's carried one level further. With u = 2^-24 and (value, error,
// magnitude) per node:
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
//     the last factor for the products of the level's chained roundings.
// Depth 4 applies the level three times. Legal sets are exact; q is within err; the action is legal
// and its float64 Q is within err[action] + err[a'] of every other legal move's.
//
// Depths 1 to 3 keep the bits they had: each depth k >= 2 is recomposed from calls one depth down
// (best_(k-1) of a child = the max of nt_search_board(child, k - 1)'s q over its legal moves, 0
// where it has none; then nt_fma, nt_sum16, nt_q2), which must give nt_search_board(board, k)'s
// bits for k = 2, 3 and 4; depth 1 is nt_score. The ruled wrapper equals nt_search_board at
// rule[blanks] for every board, and writes that depth also for a board without a move.
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
    long boards, nodes, over_below, no_move_boards, depth_seen[5];
};

struct Naive {
    const Layout &ly;
    const std::vector<float> &tables;
    Tally &tally;

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

    Est best(const Grid &b, int k)
    {
        Est out = {0.0, 0.0, 0.0};
        bool have = false;
        tally.nodes++;
        for (int a = 0; a < 4; a++) {
            Grid after;
            long r;
            if (!naive_move(b, a, after, r))
                continue;
            const Est q = move_value(after, (double)r, k);
            out.val = have ? std::fmax(out.val, q.val) : q.val;
            out.err = std::fmax(out.err, q.err);
            out.mag = std::fmax(out.mag, q.mag);
            have = true;
        }
        if (!have)
            tally.over_below++;
        return out;
    }
};

static std::vector<float> make_tables(int m, int L, uint64_t seed, bool integer)
{
    std::mt19937_64 rng(seed);
    std::vector<float> t((size_t)m << (4 * L));
    for (auto &x : t)
        x = integer ? (float)((int)(rng() % 17) - 8) : (float)(((double)(rng() >> 11) / 9007199254740992.0 - 0.5) * 74.0);
    return t;
}

// best_k(child) from a call at depth k: the max of its q over the legal moves, 0 where there is none
template <int L>
static float best_by_call(const Board &child, const r48::NtLayout &lay, const float *tables, int k)
{
    float q[4];
    uint32_t lg;
    r48::nt_search_board<L>(child, lay, tables, k, q, lg);
    float best = 0.0f;
    bool have = false;
    for (uint32_t a = 0; a < 4u; a++)
        if (((lg >> a) & 1u) && (!have || q[a] > best)) {
            have = true;
            best = q[a];
        }
    return best;
}

template <int L>
static void check_board(const Layout &ly, const r48::NtLayout &lay, const std::vector<float> &tables, const int8_t *b,
                        const char *what, long it, Tally &tally, double &worst)
{
    const Grid g = grid_of(b);
    const Board board = load(b);
    Naive naive{ly, tables, tally};
    Est want[4];
    int want_legal = 0;
    for (int a = 0; a < 4; a++) {
        Grid after;
        long r;
        if (!naive_move(g, a, after, r))
            continue;
        want_legal |= 1 << a;
        want[a] = naive.move_value(after, (double)r, 4);
    }
    tally.boards++;
    tally.no_move_boards += want_legal == 0;
    // the search at every depth, once: all[d] is what everything below is compared with
    float all[5][4];
    uint32_t all_legal[5], all_action[5];
    for (int depth = 1; depth <= 4; depth++) {
        all_legal[depth] = 99u;
        all_action[depth] = r48::nt_search_board<L>(board, lay, tables.data(), depth, all[depth], all_legal[depth]);
    }
    const float *q = all[4];
    const uint32_t legal = all_legal[4], action = all_action[4];
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
    // every depth from calls one depth down: depths 1..3 keep their bits, depth 4 is the same step once more
    const r48::Moves4 m = r48::move_rows4<true>(board);
    for (int depth = 1; depth <= 4; depth++) {
        float old[4];
        const float *got = all[depth];
        const uint32_t lg = all_legal[depth];
        CHECK((int)lg == want_legal, "%s %s it=%ld depth %d legal %u", ly.name, what, it, depth, lg);
        for (uint32_t a = 0; a < 4u; a++) {
            old[a] = -INFINITY;
            if (!((lg >> a) & 1u))
                continue;
            const Board s = r48::nt_pick(m, a);
            const uint32_t r = r48::nt_pick_reward(m, a);
            if (depth == 1) {
                old[a] = r48::nt_score<L>(s, r, lay, tables.data());
                continue;
            }
            float x[16];
            for (uint32_t c = 0; c < 16u; c++) {
                x[c] = 0.0f;
                if (r48::nt_cell(s, c) != 0u)
                    continue;
                Board two = s, four = s;
                r48::place(two, c, 1u, true);
                r48::place(four, c, 2u, true);
                x[c] = r48::nt_fma(9.0f, best_by_call<L>(two, lay, tables.data(), depth - 1),
                                   best_by_call<L>(four, lay, tables.data(), depth - 1));
            }
            old[a] = r48::nt_q2(r, r48::nt_sum16(x), r48::blanks(s).n);
        }
        CHECK(memcmp(got, old, sizeof old) == 0 && all_action[depth] == r48::nt_argmax4(got[0], got[1], got[2], got[3]), "%s %s it=%ld depth %d is not the step over depth %d's calls", ly.name, what,
              it, depth, depth - 1);
    }
    // the ruled wrapper: nt_search_board at rule[blanks], depth_out for every board
    const int nb = blanks_of(g);
    const uint8_t rules[][17] = {
        {4, 4, 3, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},   // NTupleNet.depth_rule(3, 1) over base 2, then 1
        {1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 1},   // every depth at some count, not monotone
        {3, 1, 4, 2, 3, 1, 4, 2, 3, 1, 4, 2, 3, 1, 4, 2, 3},
    };
    for (const auto &rule : rules) {
        CHECK(r48::nt_rule_check(rule) == nullptr, "a good rule is refused");
        const uint32_t d = r48::nt_rule_depth(rule, board);
        CHECK(d == rule[nb], "%s %s it=%ld nt_rule_depth %u, rule[%d] = %d", ly.name, what, it, d, nb, rule[nb]);
        CHECK(r48::nt_packed_rule_depth(r48::nt_rule_pack(rule), board) == d, "%s %s it=%ld the packed rule differs", ly.name,
              what, it);
        float qr[4];
        uint32_t lr = 77u;
        uint8_t dout = 0;
        const uint32_t ar = r48::nt_search_board_ruled<L>(board, lay, tables.data(), rule, qr, lr, &dout);
        CHECK(dout == rule[nb] && ar == all_action[d] && lr == all_legal[d] && memcmp(qr, all[d], sizeof qr) == 0,
              "%s %s it=%ld the ruled search is not the search at depth %d", ly.name, what, it, rule[nb]);
        if (d <= 2u)   // depth_out is nullable
            CHECK(r48::nt_search_board_ruled<L>(board, lay, tables.data(), rule, qr, lr, nullptr) == ar, "NULL depth_out");
        tally.depth_seen[dout]++;
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
    const std::vector<float> tables = make_tables(ly.m, L, 17 + L + integer, integer);
    Tally tally = {0, 0, 0, 0, {0, 0, 0, 0, 0}};
    double worst = 0.0;
    std::mt19937_64 rng(8192 + L + integer);
    for (long it = 0; it < n_random; it++) {
        int8_t b[16];
        const int emax = 2 + (int)(rng() % 16);          // exponents up to 17
        const int holes = (int)(rng() % 4);              // at most 3 blanks: a fourth ply is affordable here
        for (int k = 0; k < 16; k++)
            b[k] = (int8_t)(1 + rng() % emax);
        for (int k = 0; k < holes; k++)
            b[rng() % 16] = 0;
        check_board<L>(ly, lay, tables, b, "random", it, tally, worst);
    }
    const int8_t crafted[][16] = {
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1},        // full, no move
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 2, 1, 3},        // LEFT / RIGHT leave one blank; a 2 spawned after LEFT ends the game
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 3, 0},        // one blank in a corner: two legal moves, one blank after each
        {1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12},     // full, only UP / DOWN
        {3, 7, 7, 3, 7, 1, 1, 7, 7, 1, 1, 7, 3, 7, 7, 3},        // fully symmetric: opposite moves tie
        {17, 17, 16, 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 0, 2, 17},    // reward 2^18 on a crowded board
    };
    for (size_t k = 0; k < sizeof crafted / sizeof crafted[0]; k++)
        check_board<L>(ly, lay, tables, crafted[k], "crafted", (long)k, tally, worst);
    {
        float q[4];
        uint32_t legal;
        // integer tables: mirrored moves tie bit for bit (the butterfly's order is invariant under c -> c ^ k)
        const uint32_t act = r48::nt_search_board<L>(load(crafted[4]), lay, tables.data(), 4, q, legal);
        CHECK(legal == 15u && (!integer || (memcmp(&q[0], &q[1], 4) == 0 && memcmp(&q[2], &q[3], 4) == 0 &&
                                            (act == 0u || act == 2u))),
              "%s: the symmetric board's mirrored moves tie bit for bit: %.9g %.9g %.9g %.9g", ly.name, q[0], q[1], q[2], q[3]);
        uint8_t dout = 0;
        const uint8_t all4[17] = {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4};
        CHECK(r48::nt_search_board_ruled<L>(load(crafted[0]), lay, tables.data(), all4, q, legal, &dout) == 0u && legal == 0u &&
                  dout == 4 && std::isinf(q[0]) && std::isinf(q[1]) && std::isinf(q[2]) && std::isinf(q[3]),
              "%s: the board without a move under the all-4 rule", ly.name);
    }
    CHECK(tally.over_below >= 1 && tally.no_move_boards >= 1 && tally.depth_seen[1] >= 1 && tally.depth_seen[2] >= 1 &&
              tally.depth_seen[3] >= 1 && tally.depth_seen[4] >= 1,
          "%s: the boards do not cover the ground: %ld %ld, depths %ld %ld %ld %ld", ly.name, tally.over_below,
          tally.no_move_boards, tally.depth_seen[1], tally.depth_seen[2], tally.depth_seen[3], tally.depth_seen[4]);
    printf("%s %s tables: %ld boards, %ld nodes below them, worst err / bound %.3g; game-over nodes below %ld, boards "
           "without a move %ld; ruled depths seen 1:%ld 2:%ld 3:%ld 4:%ld\n",
           ly.name, integer ? "integer" : "float", tally.boards, tally.nodes, worst, tally.over_below, tally.no_move_boards,
           tally.depth_seen[1], tally.depth_seen[2], tally.depth_seen[3], tally.depth_seen[4]);
}

int main()
{
    {
        uint8_t bad[17] = {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2};
        CHECK(r48::nt_rule_check(nullptr) != nullptr, "a NULL rule passes");
        CHECK(r48::nt_rule_check(bad) == nullptr, "the all-2 rule is refused");
        bad[16] = 5;
        CHECK(r48::nt_rule_check(bad) != nullptr, "depth 5 passes");
        bad[16] = 2;
        bad[0] = 0;
        CHECK(r48::nt_rule_check(bad) != nullptr, "depth 0 passes");
    }
    for (const Layout *ly : {&k3x3, &kLinesSquares})
        for (int integer = 0; integer <= 1; integer++) {
            if (ly->L == 3)
                run_layout<3>(*ly, integer != 0, 20);
            else
                run_layout<4>(*ly, integer != 0, 20);
        }
    printf("ntuple_search4_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
