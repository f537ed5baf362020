// Host build of the n-tuple network's per-board search (rein48_amd/csrc/r48_ntuple.h:
// nt_search_board and the pieces the kernel shares with it) checked against a naive restatement
// (ntuple_naive.h and here): explicit 4x4 arrays, its own line-by-line move, eight explicit board transforms
// for the value, float64 throughout -- a CPU test harness, never shipped. Build+run:
// tests/test_ntuple_search_host.py (g++ -O2).
//
// Integer tables in [-8, 8]: every value, leaf and S_a is an integer, so as long as they stay below
// 2^24 (checked per board from the float64 numbers; a board that does not is counted and left out)
// the header's fp32 sums are exact in any order and only the division and the final add round:
// |q - Q64| <= 2 * 2^-23 * (|r_a| + |S_a| / (10 |E|)). Actions and legal sets are exact.
#include <random>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

using r48::Board;

struct Naive {
    int action, legal, n_empty[4];
    double q[4], s[4], r[4];
    double biggest;        // the largest |leaf| and |S_a| met: the fp32 sums are exact below 2^24
    int game_over_children, afterstates_15_empty;
};

static double naive_leaf(const Layout &ly, const std::vector<float> &tables, const Grid &child, bool &over)
{
    double best = 0.0;
    bool have = false;
    for (int a = 0; a < 4; a++) {
        Grid after;
        long r;
        if (!naive_move(child, a, after, r))
            continue;
        const double s = (double)r + naive_value(ly, tables, after);
        if (!have || s > best) {
            have = true;
            best = s;
        }
    }
    over = !have;
    return best;
}

static Naive naive_search(const Layout &ly, const std::vector<float> &tables, const int8_t *board, int depth)
{
    Naive out;
    memset(&out, 0, sizeof out);
    const Grid b = grid_of(board);
    for (int a = 0; a < 4; a++) {
        out.q[a] = -INFINITY;
        Grid s;
        long r;
        if (!naive_move(b, a, s, r))
            continue;
        out.legal |= 1 << a;
        out.r[a] = (double)r;
        if (depth == 1) {
            out.q[a] = (double)r + naive_value(ly, tables, s);
            continue;
        }
        double sum = 0.0;
        int n = 0;
        for (int c = 0; c < 16; c++) {
            if (s.g[c >> 2][c & 3])
                continue;
            n++;
            for (int e = 1; e <= 2; e++) {
                Grid child = s;
                child.g[c >> 2][c & 3] = e;
                bool over;
                const double leaf = naive_leaf(ly, tables, child, over);
                out.game_over_children += over;
                out.biggest = std::fmax(out.biggest, std::fabs(leaf));
                sum += (e == 1 ? 9.0 : 1.0) * leaf;
            }
        }
        out.afterstates_15_empty += n == 15;
        out.biggest = std::fmax(out.biggest, std::fabs(sum));
        out.s[a] = sum;
        out.n_empty[a] = n;
        out.q[a] = (double)r + sum / (10.0 * n);
    }
    out.action = 0;
    for (int a = 1; a < 4; a++)
        if (out.q[a] > out.q[out.action])
            out.action = a;
    return out;
}

// ---- the comparison -------------------------------------------------------------------------
static std::vector<float> int_tables(int m, int L, uint64_t seed, int spread)
{
    std::mt19937_64 rng(seed);
    std::vector<float> t((size_t)m << (4 * L));
    for (auto &x : t)
        x = (float)((int)(rng() % (2 * spread + 1)) - spread);
    return t;
}

struct Tally {
    long boards, left_out, game_over_children, afterstates_15_empty, ties;
};

template <int L>
static void check_board(const Layout &ly, const r48::NtLayout &lay, const std::vector<float> &tables, const int8_t *b,
                        const char *what, long it, Tally &tally)
{
    for (int depth = 1; depth <= 2; depth++) {
        const Naive want = naive_search(ly, tables, b, depth);
        float q[4];
        uint32_t legal = 99u;
        const uint32_t action = r48::nt_search_board<L>(load(b), lay, tables.data(), depth, q, legal);
        CHECK((int)legal == want.legal, "%s %s it=%ld depth %d legal %u want %d", ly.name, what, it, depth, legal, want.legal);
        if (depth == 2) {
            tally.boards++;
            tally.game_over_children += want.game_over_children;
            tally.afterstates_15_empty += want.afterstates_15_empty;
        }
        if (want.biggest >= 16777216.0) {   // the fp32 sums may round: not this test's ground
            tally.left_out++;
            continue;
        }
        CHECK((int)action == want.action, "%s %s it=%ld depth %d action %u want %d", ly.name, what, it, depth, action,
              want.action);
        int at_best = 0;
        for (int a = 0; a < 4; a++) {
            if (!((want.legal >> a) & 1)) {
                CHECK(std::isinf(q[a]) && q[a] < 0, "%s %s it=%ld depth %d q[%d] = %g of an illegal move", ly.name, what,
                      it, depth, a, q[a]);
                continue;
            }
            at_best += want.q[a] == want.q[want.action];
            const double bound = depth == 1 ? 0.0   // integers: exact
                                            : 2.0 * std::ldexp(1.0, -23) *
                                                  (std::fabs(want.r[a]) + std::fabs(want.s[a]) / (10.0 * want.n_empty[a]));
            CHECK(std::fabs((double)q[a] - want.q[a]) <= bound, "%s %s it=%ld depth %d q[%d] = %.9g want %.12g bound %g",
                  ly.name, what, it, depth, a, q[a], want.q[a], bound);
        }
        if (depth == 2 && at_best > 1)
            tally.ties++;
    }
}

template <int L>
static void run_layout(const Layout &ly, int spread, long n_random)
{
    r48::NtLayout lay;
    const char *why = r48::nt_expand(ly.cells, ly.m, L, lay);
    CHECK(why == nullptr, "%s: nt_expand refused: %s", ly.name, why ? why : "");
    if (why)
        return;
    const std::vector<float> tables = int_tables(ly.m, L, 7 + L + spread, spread);
    Tally tally = {0, 0, 0, 0, 0};
    std::mt19937_64 rng(2048 + L + spread);
    for (long it = 0; it < n_random; it++) {
        int8_t b[16];
        const int emax = 1 + (int)(rng() % 17);          // exponents up to 17
        const int fill = (int)(rng() % 17);
        for (int k = 0; k < 16; k++)
            b[k] = ((int)(rng() % 16) < fill) ? (int8_t)(1 + rng() % emax) : 0;
        check_board<L>(ly, lay, tables, b, "random", it, tally);
    }
    const int8_t crafted[][16] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},        // empty: no move
        {0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},        // one tile: afterstates with 15 blanks
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1},        // full, no move
        {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 2, 1, 3},        // LEFT / RIGHT leave one blank; a 2 spawned after LEFT ends the game
        {1, 2, 3, 4, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12},     // only UP / DOWN
        {0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0},        // merge once
        {17, 17, 16, 0, 0, 3, 0, 0, 0, 0, 0, 0, 1, 0, 0, 17},    // reward 2^18
        {3, 7, 7, 3, 7, 1, 1, 7, 7, 1, 1, 7, 3, 7, 7, 3},        // fully symmetric: opposite moves tie
    };
    const Tally before = tally;
    for (size_t k = 0; k < sizeof crafted / sizeof crafted[0]; k++)
        check_board<L>(ly, lay, tables, crafted[k], "crafted", (long)k, tally);
    {
        // the crafted boards do what their comments say, by the naive restatement
        const Naive empty = naive_search(ly, tables, crafted[0], 2), one = naive_search(ly, tables, crafted[1], 2),
                    full = naive_search(ly, tables, crafted[2], 2), near = naive_search(ly, tables, crafted[3], 2);
        CHECK(empty.legal == 0 && full.legal == 0 && empty.action == 0 && full.action == 0, "%s: boards without a move", ly.name);
        CHECK(one.legal == 15 && one.afterstates_15_empty == 4, "%s: the one-tile board", ly.name);
        CHECK((near.legal & 12) == 12 && near.n_empty[2] == 1 && near.n_empty[3] == 1 && near.game_over_children >= 1,
              "%s: the nearly-over board: legal %d, blanks %d %d, game-over children %d", ly.name, near.legal,
              near.n_empty[2], near.n_empty[3], near.game_over_children);
        float q[4];
        uint32_t legal;
        CHECK(r48::nt_search_board<L>(load(crafted[1]), lay, tables.data(), 2, q, legal) == 0u &&
                  memcmp(&q[0], &q[1], 4) == 0 && memcmp(&q[0], &q[2], 4) == 0 && memcmp(&q[0], &q[3], 4) == 0,
              "%s: the one-tile board's four moves tie bit for bit: %g %g %g %g", ly.name, q[0], q[1], q[2], q[3]);
    }
    // the 17 + 17 board's leaves hold rewards of 2^18: 150 of them pass 2^24, so it is the one left out
    CHECK(tally.left_out - before.left_out <= 1, "%s: %ld crafted boards were left out", ly.name,
          tally.left_out - before.left_out);
    CHECK(tally.left_out * 10 < tally.boards, "%s: %ld of %ld boards left out", ly.name, tally.left_out, tally.boards);
    CHECK(tally.game_over_children >= 1 && tally.afterstates_15_empty >= 1 && tally.ties >= 1,
          "%s: game-over children %ld, 15-blank afterstates %ld, ties %ld", ly.name, tally.game_over_children,
          tally.afterstates_15_empty, tally.ties);
    printf("%s spread %d: %ld boards (%ld left out: a sum reached 2^24), %ld game-over children, %ld afterstates with 15 "
           "blanks, %ld boards with tied best moves\n",
           ly.name, spread, tally.boards, tally.left_out, tally.game_over_children, tally.afterstates_15_empty, tally.ties);
}

int main()
{
    for (const Layout *ly : {&k3x3, &kLinesSquares})
        for (int spread : {8, 1}) {
            if (ly->L == 3)
                run_layout<3>(*ly, spread, 300);
            else
                run_layout<4>(*ly, spread, 300);
        }
    // the tree order of the cell sum, spelled out
    {
        float x[16];
        for (int c = 0; c < 16; c++)
            x[c] = 1.0f + (float)c * 0.37f + (c % 3 ? 1e-7f : 3e6f);
        const float lo = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
        const float hi = ((x[8] + x[9]) + (x[10] + x[11])) + ((x[12] + x[13]) + (x[14] + x[15]));
        const float want = lo + hi, got = r48::nt_sum16(x);
        CHECK(memcmp(&want, &got, 4) == 0, "nt_sum16 %.9g want %.9g", got, want);
    }
    // the k-th set bit, against a walk over the bits
    {
        std::mt19937_64 rng(64);
        for (int it = 0; it < 2000; it++) {
            uint64_t mask = rng() & rng();
            if (it < 64)
                mask = 1ull << it;
            if (it == 64)
                mask = ~0ull;
            uint32_t k = 0;
            for (uint32_t pos = 0; pos < 64; pos++)
                if ((mask >> pos) & 1u) {
                    CHECK(r48::nt_select_bit(mask, k) == pos, "nt_select_bit(%llx, %u) = %u want %u",
                          (unsigned long long)mask, k, r48::nt_select_bit(mask, k), pos);
                    k++;
                }
        }
    }
    // the argmax takes the first maximiser, and action 0 where nothing is legal
    {
        const float ninf = -INFINITY;
        CHECK(r48::nt_argmax4(ninf, ninf, ninf, ninf) == 0u, "argmax of nothing");
        CHECK(r48::nt_argmax4(ninf, 2.f, 2.f, 1.f) == 1u && r48::nt_argmax4(1.f, 1.f, 1.f, 1.f) == 0u &&
                  r48::nt_argmax4(ninf, ninf, ninf, -5.f) == 3u && r48::nt_argmax4(0.f, 1.f, 3.f, 3.f) == 2u,
              "argmax ties");
    }
    printf("ntuple_search_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
