// Host build of the legal-move and templated-move board logic (rein48_amd/csrc/r48_board.h:
// legal_mask, move_rows<A>, move_rows4) checked against the C oracle (oracle/r48_oracle.c) -- a
// CPU test harness, never shipped. Build+run: tests/test_moves_host.py (g++ -O2, links the
// oracle object).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../rein48_amd/csrc/r48_board.h"

extern "C" {
int orc_move(int8_t *b, int a, int64_t *reward);
int orc_game_over(const int8_t *b);
}

using r48::Board;

static Board load(const int8_t *b)
{
    Board r;
    memcpy(&r, b, 16);
    return r;
}
static void store(int8_t *b, const Board &r) { memcpy(b, &r, 16); }

static int fails = 0;
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

// the oracle's four moves of b: changed bits, moved boards, merge rewards
struct OracleMoves {
    uint32_t legal;
    int8_t after[4][16];
    int64_t reward[4];
};

static OracleMoves oracle_moves(const int8_t *b)
{
    OracleMoves o;
    o.legal = 0;
    for (int a = 0; a < 4; a++) {
        memcpy(o.after[a], b, 16);
        o.reward[a] = 0;
        const int c = orc_move(o.after[a], a, &o.reward[a]);
        const bool moved = memcmp(o.after[a], b, 16) != 0;
        CHECK((c != 0) == moved, "oracle's own changed flag a=%d", a);
        if (moved) o.legal |= 1u << a;
    }
    return o;
}

template <int A>
static void check_move_rows(const int8_t *b, const OracleMoves &o, long it)
{
    Board out;
    const uint32_t rw = r48::move_rows<A, true>(load(b), out);
    int8_t ob[16];
    store(ob, out);
    CHECK(memcmp(ob, o.after[A], 16) == 0, "move_rows<%d> board it=%ld", A, it);
    CHECK((int64_t)rw == o.reward[A], "move_rows<%d> reward it=%ld %u vs %lld", A, it, rw, (long long)o.reward[A]);
    Board out0;
    const uint32_t rw0 = r48::move_rows<A, false>(load(b), out0);
    CHECK(memcmp(&out0, &out, 16) == 0 && rw0 == 0u, "move_rows<%d, false> it=%ld", A, it);
}

int main()
{
    // 1. exhaustive: every 18^4 line placed in each of the four rows and four columns of an
    //    otherwise empty board; legal_mask's four bits vs "the oracle's move changed the board"
    {
        const int n = 18 * 18 * 18 * 18;
        for (int idx = 0; idx < n; idx++) {
            int8_t cells[4];
            int t = idx;
            for (int k = 3; k >= 0; k--) { cells[k] = (int8_t)(t % 18); t /= 18; }
            for (int vertical = 0; vertical < 2; vertical++)
                for (int slot = 0; slot < 4; slot++) {
                    int8_t b[16] = {0};
                    for (int k = 0; k < 4; k++) {
                        if (vertical) b[4 * k + slot] = cells[k]; else b[4 * slot + k] = cells[k];
                    }
                    uint32_t want = 0;
                    for (int a = 0; a < 4; a++) {
                        int8_t ob[16];
                        memcpy(ob, b, 16);
                        int64_t rw = 0;
                        orc_move(ob, a, &rw);
                        if (memcmp(ob, b, 16) != 0) want |= 1u << a;
                    }
                    const uint32_t got = r48::legal_mask(load(b));
                    CHECK(got == want, "line idx=%d vertical=%d slot=%d got %x want %x", idx, vertical, slot, got,
                          want);
                }
        }
    }
    // 2.-4. 400k random boards, cell exponents 0..17, density varied from nearly empty to full:
    //    legal_mask, move_rows<A> (board + merge reward), move_rows4, legal == 0 vs game over
    {
        std::mt19937_64 rng(20480);
        long n_full = 0, n_sparse = 0, n_over = 0;
        for (long it = 0; it < 400000; it++) {
            int8_t b[16];
            const int emax = 1 + (int)(rng() % 17);          // tiles 1..emax, emax up to 17
            const int fill = (int)(rng() % 17);               // P(tile) = fill / 16: 0 .. 1
            int tiles = 0;
            for (int k = 0; k < 16; k++) {
                b[k] = ((int)(rng() % 16) < fill) ? (int8_t)(1 + rng() % emax) : 0;
                tiles += b[k] != 0;
            }
            n_full += tiles == 16;
            n_sparse += tiles <= 2;
            const OracleMoves o = oracle_moves(b);
            const uint32_t got = r48::legal_mask(load(b));
            CHECK(got == o.legal, "random it=%ld got %x want %x", it, got, o.legal);
            check_move_rows<0>(b, o, it);
            check_move_rows<1>(b, o, it);
            check_move_rows<2>(b, o, it);
            check_move_rows<3>(b, o, it);
            const r48::Moves4 m = r48::move_rows4<true>(load(b));
            CHECK(memcmp(&m.up, o.after[0], 16) == 0 && memcmp(&m.down, o.after[1], 16) == 0 &&
                      memcmp(&m.left, o.after[2], 16) == 0 && memcmp(&m.right, o.after[3], 16) == 0,
                  "move_rows4 boards it=%ld", it);
            CHECK((int64_t)m.r_up == o.reward[0] && (int64_t)m.r_down == o.reward[1] &&
                      (int64_t)m.r_left == o.reward[2] && (int64_t)m.r_right == o.reward[3],
                  "move_rows4 rewards it=%ld", it);
            const uint32_t from_moves = (r48::differs(m.up, load(b)) ? 1u : 0u) | (r48::differs(m.down, load(b)) ? 2u : 0u) |
                                        (r48::differs(m.left, load(b)) ? 4u : 0u) | (r48::differs(m.right, load(b)) ? 8u : 0u);
            CHECK(from_moves == o.legal, "move_rows4 legal it=%ld", it);
            if (tiles > 0) {
                const bool over = orc_game_over(b) != 0;
                n_over += over;
                CHECK((got == 0u) == over, "legal == 0 vs game over it=%ld", it);
            }
        }
        // the generator must really reach both ends and some terminal boards
        CHECK(n_full > 1000 && n_sparse > 1000 && n_over > 100, "coverage full=%ld sparse=%ld over=%ld", n_full,
              n_sparse, n_over);
    }
    // 5. the all-zero board has no legal move (and is not game over)
    {
        int8_t b[16] = {0};
        CHECK(r48::legal_mask(load(b)) == 0u, "empty board legal");
        CHECK(orc_game_over(b) == 0, "empty board is not game over");
    }
    printf("moves_logic_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
