// Host check of r48::reset_lines (rein48_amd/csrc/r48_board.h) and of k_step_n's auto-reset from
// the line-form table (r48_env.hip, restated here on the host) -- a CPU test harness, never shipped.
// Build+run: tests/test_reset_lines_host.py (g++ -O2, and once more under ASan + UBSan).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../rein48_amd/csrc/r48_board.h"

using r48::Board;

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

static bool same(const Board &a, const Board &b) { return memcmp(&a, &b, 16) == 0; }

// near-full start boards: exponents 1..12, 5 % blanks (many boards are done within a few steps)
static Board near_full(std::mt19937 &g)
{
    int8_t c[16];
    for (int k = 0; k < 16; k++) c[k] = (g() % 20 == 0) ? 0 : (int8_t)(1 + g() % 12);
    Board b;
    memcpy(&b, c, 16);
    return b;
}

int main()
{
    // the kernel's LDS table: entry (a << 5) | (four << 4) | cell
    static Board rtab[128];
    for (uint32_t i = 0; i < 128; i++) rtab[i] = r48::reset_lines(i >> 5, i & 15u, (i >> 4) & 1u);

    // 1. every (a, cell, four): the table entry is the rows reset board taken to the line form of a
    //    by the transpose + select route (no kOrient), and kOrient[4a + UP] takes it back to rows
    for (uint32_t a = 0; a < 4; a++)
        for (uint32_t four = 0; four < 2; four++)
            for (uint32_t cell = 0; cell < 16; cell++) {
                Board R;
                r48::reset_board(R, cell, four != 0);
                int8_t c[16];
                memcpy(c, &R, 16);
                for (uint32_t k = 0; k < 16; k++)
                    CHECK(c[k] == (k == cell ? (four ? 2 : 1) : 0), "reset_board cell=%u four=%u k=%u", cell, four, k);
                const Board e = rtab[(a << 5) | (four << 4) | cell];
                CHECK(same(e, r48::to_lines(R, a)), "reset_lines a=%u cell=%u four=%u", a, cell, four);
                CHECK(same(r48::reorient(e, r48::kOrient[4 * a + 0]), R), "back to rows a=%u cell=%u four=%u", a, cell,
                      four);
            }

    // 2. k_step_n's random-policy loop (step_lane_pre): selector record of step t + 1 read ahead,
    //    reset from the table with no patch of that record, return to rows from the line form of
    //    the last action -- against step_board + reset_board on rows, at every step
    {
        const int n = 4096, steps = 300;
        const uint64_t seed = 0x5EED'2048ull;
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), step0 = 100;
        const int64_t off = 2;
        std::mt19937 g(11);
        long resets = 0;
        for (int i = 0; i < n; i++) {
            Board R = near_full(g), L = R;
            const uint64_t gid = (uint64_t)(off + i);
            uint32_t x, y;
            r48::step_draw(gid, step0, k0, k1, x, y);
            r48::Orient se = r48::kOrient[x >> 30];   // from rows on entry
            for (uint32_t t = 0; t < (uint32_t)steps; t++) {
                uint32_t nx, ny;
                r48::step_draw(gid, step0 + t + 1u, k0, k1, nx, ny);
                const uint32_t a = x >> 30;
                const bool four = (x & 0x3FFFFFFFu) < r48::kFourThresh30;
                const r48::Orient xe = r48::kOrient[4 * a + (nx >> 30)];   // read ahead
                L = r48::reorient(L, se);
                const r48::StepOut s = r48::step_lines<false, true>(L, a, y, four);
                if (s.done)
                    L = rtab[(a << 5) | (((y & 0x0FFFFFFFu) < r48::kFourThresh28 ? 1u : 0u) << 4) | (y >> 28)];
                se = xe;
                // reference: rows
                const r48::StepOut w = r48::step_board<false, false, true>(R, a, y, four);
                if (w.done) {
                    r48::reset_board(R, y >> 28, (y & 0x0FFFFFFFu) < r48::kFourThresh28);
                    resets++;
                }
                CHECK(s.done == w.done && s.changed == w.changed, "loop flags i=%d t=%u", i, t);
                CHECK(same(r48::reorient(L, r48::kOrient[4 * a]), R), "loop board i=%d t=%u a=%u done=%u", i, t, a,
                      w.done);
                x = nx;
                y = ny;
            }
        }
        // near-full starts alone end > 10 % of the boards within a few steps
        CHECK(resets > n / 10, "too few resets to mean anything: %ld", resets);
        printf("random-policy loop: %ld resets\n", resets);
    }

    // 3. the given-action loop (step_lane_lines): one action byte per board for all steps, bad
    //    bytes (> 3) included -- the board does not move, a dead one is reset in the line form of
    //    a & 3, the orientation the loop tracks
    {
        const int n = 4096, steps = 40;
        const uint64_t seed = 0xC0FFEEull;
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        std::mt19937 g(12);
        long resets = 0, bad_resets = 0;
        for (int i = 0; i < n; i++) {
            Board R = near_full(g), L = R;
            const uint32_t ag = (g() % 4 == 0) ? (uint32_t)(g() & 0xff) : (uint32_t)(g() & 3);
            uint32_t o = 0;
            for (uint32_t t = 0; t < (uint32_t)steps; t++) {
                uint32_t x, y;
                r48::step_draw((uint64_t)i, t, k0, k1, x, y);
                const bool four = (x & 0x3FFFFFFFu) < r48::kFourThresh30;
                const uint32_t ac = ag & 3u;
                L = r48::reorient(L, r48::kOrient[4 * o + ac]);
                o = ac;
                const r48::StepOut s = r48::step_lines<false, false>(L, ag, y, four);
                if (s.done)
                    L = rtab[(ac << 5) | (((y & 0x0FFFFFFFu) < r48::kFourThresh28 ? 1u : 0u) << 4) | (y >> 28)];
                const r48::StepOut w = r48::step_board<false, false, false>(R, ag, y, four);
                if (w.done) {
                    r48::reset_board(R, y >> 28, (y & 0x0FFFFFFFu) < r48::kFourThresh28);
                    resets++;
                    bad_resets += ag > 3u;
                }
                CHECK(s.done == w.done && s.changed == w.changed, "given flags i=%d t=%u", i, t);
                CHECK(same(r48::reorient(L, r48::kOrient[4 * o]), R), "given board i=%d t=%u a=%u", i, t, ag);
            }
        }
        CHECK(resets > n / 10 && bad_resets > 0, "too few resets: %ld (%ld with a bad byte)", resets, bad_resets);
        printf("given-action loop: %ld resets, %ld with a bad action byte\n", resets, bad_resets);
    }
    printf("reset_lines_test: %s (%d failures)\n", fails ? "FAIL" : "OK", fails);
    return fails ? 1 : 0;
}
