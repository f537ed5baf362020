// Host build of the n-tuple network's ruled play contract (rein48_amd/csrc/r48_ntuple.h:
// nt_play_board_ruled, the written definition of what k_nt_play_ruled computes) checked bit for bit
// against an explicit loop written here over nt_search_board, step_draw and step_board, with the
// depth looked up from the board's bytes -- a CPU test harness, never shipped.
// Build+run: tests/test_ntuple_play_ruled_host.py (g++ -O2).
//
// Layouts 3x3 and lines-squares, float and integer tables; the rules all-1 and all-2 (which must
// also equal nt_play_board at depths 1 and 2), all-3 and a mixed rule that uses all four depths with
// depth 4 at no more than one blank (the CPU time); an even board id at step counter 0 and
// an odd one at 0xFFFFFFF0 (the uint32 add wraps inside the call); n_steps 0, 1 and 24; from a board early in a
// game, from one in mid-game and from a crowded one, where the mixed rule reaches depth 4. Then: a board
// without a move comes back as it went in under every rule, and chunked calls add up.
#include <random>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

using r48::Board;

static std::vector<float> make_tables(int m, int L, uint64_t seed, bool integer)
{
    std::mt19937_64 rng(seed);
    std::vector<float> t((size_t)m << (4 * L));
    for (auto &x : t)
        x = integer ? (float)((int)(rng() % 17) - 8) : (float)(((double)(rng() >> 11) / 9007199254740992.0 - 0.5) * 74.0);
    return t;
}

static const uint32_t K0 = 0x12345678u, K1 = 0x9ABCDEF0u;

struct Rule {
    const char *name;
    uint8_t depth[17];
    int plain;   // the depth of nt_play_board this rule must reproduce, 0: none
};

static const Rule kRules[] = {
    {"all-1", {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, 1},
    {"all-2", {2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 2},
    {"all-3", {3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3}, 0},
    {"mixed", {4, 4, 3, 3, 3, 2, 2, 2, 1, 1, 2, 1, 1, 1, 1, 1, 1}, 0},
};

struct Tally {
    long steps, changed, wrapped, finished;
    long at_depth[5];
};

static int zero_bytes(const Board &b)
{
    int8_t cell[16];
    memcpy(cell, &b, 16);
    int k = 0;
    for (int c = 0; c < 16; c++)
        k += cell[c] == 0;
    return k;
}

// the contract, spelled out: the depth from the bytes, search, draw, step -- one step
template <int L>
static r48::StepOut explicit_step(Board &b, const r48::NtLayout &lay, const float *tables, const Rule &rule, uint64_t gid,
                                  uint32_t step, Tally &tally)
{
    const int depth = rule.depth[zero_bytes(b)];
    float q[4];
    uint32_t legal;
    const uint32_t action = r48::nt_search_board<L>(b, lay, tables, depth, q, legal);
    uint32_t x, y;
    r48::step_draw(gid, step, K0, K1, x, y);
    const bool four = (x & 0x3FFFFFFFu) < r48::kFourThresh30;
    const r48::StepOut o = r48::step_board<true, false, true>(b, action, y, four);
    tally.steps++;
    tally.changed += o.changed;
    tally.at_depth[depth] += o.changed;
    CHECK(o.changed == (legal != 0u), "a step changes the board exactly where a move is legal");
    return o;
}

template <int L>
static void check_case(const Layout &ly, const r48::NtLayout &lay, const std::vector<float> &tables, const int8_t *start,
                       const Rule &rule, uint64_t gid, uint32_t step0, int n_steps, Tally &tally)
{
    Board want = load(start);
    int32_t want_len = 7, want_gain = 11;      // the in/out words are added to
    uint8_t want_done = 0x55;
    for (int t = 0; t < n_steps; t++) {
        const uint32_t step = step0 + (uint32_t)t;
        tally.wrapped += step < step0;
        const r48::StepOut o = explicit_step<L>(want, lay, tables.data(), rule, gid, step, tally);
        want_len += (int32_t)o.changed;
        want_gain += (int32_t)o.reward;
        want_done = (uint8_t)o.done;
    }
    Board got = load(start);
    int32_t len = 7, gain = 11;
    uint8_t done = 0x55;
    r48::nt_play_board_ruled<L>(got, lay, tables.data(), rule.depth, n_steps, K0, K1, gid, step0, &len, &gain, &done);
    CHECK(memcmp(&got, &want, 16) == 0, "%s %s gid %llu step0 %u n_steps %d: boards differ", ly.name, rule.name,
          (unsigned long long)gid, step0, n_steps);
    CHECK(len == want_len && gain == want_gain && done == want_done,
          "%s %s gid %llu step0 %u n_steps %d: length %d want %d, gain %d want %d, done %d want %d", ly.name, rule.name,
          (unsigned long long)gid, step0, n_steps, len, want_len, gain, want_gain, done, want_done);
    if (n_steps > 0)
        CHECK(done == r48::nt_play_done(got), "%s: done is not has_game_over of the final board", ly.name);
    tally.finished += n_steps > 0 && done;
    if (step0 == 0u)
        return;   // what follows once per rule, start and n_steps: with the odd board id and the wrapping counter
    // the outputs are optional
    Board again = load(start);
    r48::nt_play_board_ruled<L>(again, lay, tables.data(), rule.depth, n_steps, K0, K1, gid, step0, nullptr, nullptr,
                                nullptr);
    CHECK(memcmp(&again, &want, 16) == 0, "%s %s: NULL outputs change the boards", ly.name, rule.name);
    // a uniform rule of 1s or 2s is the plain play contract at that depth
    if (rule.plain) {
        Board plain = load(start);
        int32_t pl = 7, pg = 11;
        uint8_t pd = 0x55;
        r48::nt_play_board<L>(plain, lay, tables.data(), rule.plain, n_steps, K0, K1, gid, step0, &pl, &pg, &pd);
        CHECK(memcmp(&plain, &got, 16) == 0 && pl == len && pg == gain && pd == done,
              "%s %s gid %llu step0 %u n_steps %d: differs from nt_play_board at depth %d", ly.name, rule.name,
              (unsigned long long)gid, step0, n_steps, rule.plain);
    }
    // chunked calls add up: 0 + a + (n_steps - a) steps
    if (n_steps > 1) {
        const int a = n_steps / 2 + 1;
        Board parts = load(start);
        int32_t cl = 7, cg = 11;
        uint8_t cd = 0x55;
        r48::nt_play_board_ruled<L>(parts, lay, tables.data(), rule.depth, a, K0, K1, gid, step0, &cl, &cg, &cd);
        r48::nt_play_board_ruled<L>(parts, lay, tables.data(), rule.depth, n_steps - a, K0, K1, gid, step0 + (uint32_t)a,
                                    &cl, &cg, &cd);
        CHECK(memcmp(&parts, &got, 16) == 0 && cl == len && cg == gain && cd == done,
              "%s %s gid %llu step0 %u: %d + %d steps differ from %d", ly.name, rule.name, (unsigned long long)gid, step0, a,
              n_steps - a, n_steps);
    }
}

template <int L>
static void run_layout(const Layout &ly, bool integer)
{
    r48::NtLayout lay;
    const char *why = r48::nt_expand(ly.cells, ly.m, L, lay);
    CHECK(why == nullptr, "%s: nt_expand refused: %s", ly.name, why ? why : "");
    if (why)
        return;
    const std::vector<float> tables = make_tables(ly.m, L, 31 + L + integer, integer);
    const int8_t starts[][16] = {
        {0, 2, 0, 1, 2, 1, 3, 0, 0, 0, 1, 0, 2, 3, 0, 1},        // early in a game: seven blanks
        {3, 1, 0, 2, 5, 2, 1, 0, 1, 6, 3, 0, 2, 1, 0, 0},        // mid-game
        {3, 1, 4, 2, 5, 2, 1, 6, 1, 6, 3, 2, 2, 1, 5, 0},        // crowded: one blank
    };
    Tally tally = {0, 0, 0, 0, {0, 0, 0, 0, 0}};
    for (const Rule &rule : kRules) {
        CHECK(r48::nt_rule_check(rule.depth) == nullptr, "%s: the rule is refused", rule.name);
        for (const auto &start : starts)
            for (int n_steps : {0, 1, 24}) {
                // an even board id from counter 0, an odd one (beyond 32 bits) across the counter's wrap
                check_case<L>(ly, lay, tables, start, rule, 10, 0u, n_steps, tally);
                check_case<L>(ly, lay, tables, start, rule, 0x100000007ull, 0xFFFFFFF0u, n_steps, tally);
            }
        // a board without a move: unchanged, length and gain untouched, done 1
        const int8_t stuck[16] = {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1};
        Board b = load(stuck);
        int32_t len = 7, gain = 11;
        uint8_t done = 0x55;
        r48::nt_play_board_ruled<L>(b, lay, tables.data(), rule.depth, 5, K0, K1, 3, 9, &len, &gain, &done);
        CHECK(memcmp(&b, stuck, 16) == 0 && len == 7 && gain == 11 && done == 1, "%s %s: the board without a move", ly.name,
              rule.name);
    }
    CHECK(tally.wrapped > 0 && tally.changed > 300 && tally.changed < tally.steps,
          "%s: the cases do not cover the ground: %ld wrapped, %ld changed of %ld", ly.name, tally.wrapped, tally.changed,
          tally.steps);
    for (int d = 1; d <= 4; d++)
        CHECK(tally.at_depth[d] > 0, "%s: no step was searched at depth %d", ly.name, d);
    printf("%s %s tables: %ld steps compared (%ld changed the board: %ld / %ld / %ld / %ld at depths 1..4; %ld after the "
           "counter wrapped), %ld cases ended game over\n",
           ly.name, integer ? "integer" : "float", tally.steps, tally.changed, tally.at_depth[1], tally.at_depth[2],
           tally.at_depth[3], tally.at_depth[4], tally.wrapped, tally.finished);
}

int main()
{
    for (const Layout *ly : {&k3x3, &kLinesSquares})
        for (int integer = 0; integer <= 1; integer++) {
            if (ly->L == 3)
                run_layout<3>(*ly, integer != 0);
            else
                run_layout<4>(*ly, integer != 0);
        }
    printf("ntuple_play_ruled_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
