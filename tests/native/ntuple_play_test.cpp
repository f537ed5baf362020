// Host build of the n-tuple network's play contract (rein48_amd/csrc/r48_ntuple.h: nt_play_board, the
// written definition k_nt_play1 / k_nt_play2 share) checked bit for bit against an explicit loop
// written here over nt_search_board, step_draw and step_board -- a CPU test harness, never shipped.
// Build+run: tests/test_ntuple_play_host.py (g++ -O2).
//
// Layouts 3x3 and lines-squares, float and integer tables, depths 1 and 2, an even and an odd board
// id (the two halves of the Philox pair), step counters 0 and 0xFFFFFFF0 (the uint32 add wraps inside
// 300 steps), n_steps 0, 1 and 300, from a fresh game's board and from one in mid-game. Then: a board
// without a move comes back as it went in, and a game played to its end in chunks has counted its
// changing steps and summed its StepOut rewards.
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

struct Tally {
    long steps, changed, wrapped, finished, fours;
};

// the contract, spelled out: search, draw, step -- one step
template <int L>
static r48::StepOut explicit_step(Board &b, const r48::NtLayout &lay, const float *tables, int depth, uint64_t gid,
                                  uint32_t step, Tally &tally)
{
    float q[4];
    uint32_t legal;
    const uint32_t action = r48::nt_search_board<L>(b, lay, tables, depth, q, legal);
    uint32_t x, y;
    r48::step_draw(gid, step, K0, K1, x, y);
    const bool four = (x & 0x3FFFFFFFu) < r48::kFourThresh30;
    const r48::StepOut o = r48::step_board<true, false, true>(b, action, y, four);
    tally.steps++;
    tally.changed += o.changed;
    tally.fours += o.changed && four;
    CHECK(o.changed == (legal != 0u), "a step changes the board exactly where a move is legal");
    return o;
}

template <int L>
static void check_case(const Layout &ly, const r48::NtLayout &lay, const std::vector<float> &tables, const int8_t *start,
                       int depth, uint64_t gid, uint32_t step0, int n_steps, Tally &tally)
{
    Board want = load(start);
    int32_t want_len = 7, want_gain = 11;      // the in/out words are added to
    uint8_t want_done = 0x55;
    for (int t = 0; t < n_steps; t++) {
        const uint32_t step = step0 + (uint32_t)t;
        tally.wrapped += step < step0;
        const r48::StepOut o = explicit_step<L>(want, lay, tables.data(), depth, gid, step, tally);
        want_len += (int32_t)o.changed;
        want_gain += (int32_t)o.reward;
        want_done = (uint8_t)o.done;
    }
    Board got = load(start);
    int32_t len = 7, gain = 11;
    uint8_t done = 0x55;
    r48::nt_play_board<L>(got, lay, tables.data(), depth, n_steps, K0, K1, gid, step0, &len, &gain, &done);
    CHECK(memcmp(&got, &want, 16) == 0, "%s depth %d gid %llu step0 %u n_steps %d: boards differ", ly.name, depth,
          (unsigned long long)gid, step0, n_steps);
    CHECK(len == want_len && gain == want_gain && done == want_done,
          "%s depth %d gid %llu step0 %u n_steps %d: length %d want %d, gain %d want %d, done %d want %d", ly.name, depth,
          (unsigned long long)gid, step0, n_steps, len, want_len, gain, want_gain, done, want_done);
    if (n_steps > 0)
        CHECK(done == r48::nt_play_done(got), "%s: done is not has_game_over of the final board", ly.name);
    tally.finished += n_steps > 0 && done;
    // the outputs are optional
    Board again = load(start);
    r48::nt_play_board<L>(again, lay, tables.data(), depth, n_steps, K0, K1, gid, step0, nullptr, nullptr, nullptr);
    CHECK(memcmp(&again, &want, 16) == 0, "%s: NULL outputs change the boards", ly.name);
}

template <int L>
static void run_layout(const Layout &ly, bool integer)
{
    r48::NtLayout lay;
    const char *why = r48::nt_expand(ly.cells, ly.m, L, lay);
    CHECK(why == nullptr, "%s: nt_expand refused: %s", ly.name, why ? why : "");
    if (why)
        return;
    const std::vector<float> tables = make_tables(ly.m, L, 23 + L + integer, integer);
    const int8_t starts[][16] = {
        {0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},        // a fresh game
        {3, 1, 0, 2, 5, 2, 1, 0, 1, 6, 3, 0, 2, 1, 0, 0},        // mid-game
    };
    Tally tally = {0, 0, 0, 0, 0};
    for (const auto &start : starts)
        for (int depth = 1; depth <= 2; depth++)
            for (uint64_t gid : {(uint64_t)10, (uint64_t)0x100000007ull})      // even, odd (and beyond 32 bits)
                for (uint32_t step0 : {0u, 0xFFFFFFF0u})
                    for (int n_steps : {0, 1, 300})
                        check_case<L>(ly, lay, tables, start, depth, gid, step0, n_steps, tally);
    CHECK(tally.wrapped > 0 && tally.changed > 1000 && tally.fours > 0 && tally.changed < tally.steps,
          "%s: the cases do not cover the ground: %ld wrapped, %ld changed of %ld, %ld fours", ly.name, tally.wrapped,
          tally.changed, tally.steps, tally.fours);

    // a board without a move: unchanged, length and gain untouched, done 1
    for (int depth = 1; depth <= 2; depth++) {
        const int8_t stuck[16] = {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1};
        Board b = load(stuck);
        int32_t len = 7, gain = 11;
        uint8_t done = 0x55;
        r48::nt_play_board<L>(b, lay, tables.data(), depth, 5, K0, K1, 3, 9, &len, &gain, &done);
        CHECK(memcmp(&b, stuck, 16) == 0 && len == 7 && gain == 11 && done == 1, "%s depth %d: the board without a move",
              ly.name, depth);
    }

    // a game played to its end in chunks of 64 steps: length = its changing steps, gain = the sum of
    // the StepOut rewards, both from the explicit loop run until done
    long longest = 0;
    for (int depth = 1; depth <= 2; depth++) {
        const uint64_t gid = 40 + depth;
        Board want = load(starts[0]);
        Tally t2 = {0, 0, 0, 0, 0};
        long moves = 0, reward = 0;
        uint32_t over = 0;
        for (uint32_t step = 5; !over && moves < 20000; step++) {
            const r48::StepOut o = explicit_step<L>(want, lay, tables.data(), depth, gid, step, t2);
            moves += o.changed;
            reward += o.reward;
            over = o.done;
        }
        CHECK(over, "%s depth %d: the explicit game did not end in 20,000 steps", ly.name, depth);
        Board b = load(starts[0]);
        int32_t len = 0, gain = 0;
        uint8_t done = 0;
        uint32_t step = 5;
        for (int chunk = 0; !done && chunk < 400; chunk++, step += 64)
            r48::nt_play_board<L>(b, lay, tables.data(), depth, 64, K0, K1, gid, step, &len, &gain, &done);
        CHECK(done == 1 && memcmp(&b, &want, 16) == 0, "%s depth %d: the chunked game ends on another board", ly.name, depth);
        CHECK(len == moves && gain == reward, "%s depth %d: length %d want %ld, gain %d want %ld", ly.name, depth, len, moves,
              gain, reward);
        CHECK(moves > 20 && reward > 0, "%s depth %d: a game of %ld moves and reward %ld", ly.name, depth, moves, reward);
        longest = moves > longest ? moves : longest;
    }
    printf("%s %s tables: %ld steps compared (%ld changed the board, %ld spawned a 4, %ld after the counter wrapped), "
           "%ld cases ended game over; played-out games up to %ld moves\n",
           ly.name, integer ? "integer" : "float", tally.steps, tally.changed, tally.fours, tally.wrapped, tally.finished,
           longest);
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
    printf("ntuple_play_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
