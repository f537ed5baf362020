// Host build of the carousel-shaping contract of rein48_amd/csrc/r48_ntuple.h (nt_carousel_host over
// nt_stage, nt_carousel_turn and nt_carousel_donor) against a naive restatement written here: the
// stage cell by cell (ntuple_stage_naive.h), Philox4x32-10 from the Random123 paper, and one call
// decided board by board from a copy of the state before it. A CPU test harness, never shipped.
// Build+run: tests/test_ntuple_carousel_host.py (g++ -O2, and once more with
// -fsanitize=address,undefined).
#include <algorithm>
#include <random>

#include "ntuple_stage_naive.h"

// ---- the naive restatement ----------------------------------------------------------------------
static void naive_philox10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the donor slot of board gid: word 0 of the block {gid lo, gid hi, ctr, 0xCA70} under the seed, times n / 2^32
static int64_t naive_donor(uint64_t seed, uint64_t gid, uint32_t ctr, int64_t n)
{
    const uint32_t c[4] = {(uint32_t)(gid & 0xFFFFFFFFu), (uint32_t)(gid >> 32), ctr, 0xCA70u};
    const uint32_t k[2] = {(uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32)};
    uint32_t w[4];
    naive_philox10(c, k, w);
    return (int64_t)(((uint64_t)w[0] * (uint64_t)n) >> 32);
}

struct State {
    int S, n;
    std::vector<int8_t> boards, pool;
    std::vector<uint8_t> has, seen, turn;
    std::vector<uint64_t> starts;
    State(int S_, int n_)
        : S(S_), n(n_), boards(16 * n_, 0), pool(16 * (S_ - 1) * n_, 0), has((S_ - 1) * n_, 0), seen(n_, 0), turn(n_, 0),
          starts(S_, 0)
    {
    }
    bool operator==(const State &o) const
    {
        return boards == o.boards && pool == o.pool && has == o.has && seen == o.seen && turn == o.turn && starts == o.starts;
    }
};

// one call, every board decided from the state as it was before the call
static void naive_call(State &st, const std::vector<uint8_t> &done, const uint8_t *cuts, uint64_t seed, int64_t gid0,
                       uint32_t ctr)
{
    const State old = st;
    const int n = st.n, n_cuts = st.S - 1;
    for (int i = 0; i < n; i++) {
        const int8_t *b = &old.boards[16 * i];
        if (done[i]) {
            int t = (old.turn[i] + 1) % st.S;
            const int8_t *from = b;
            if (t > 0) {
                const int64_t j = naive_donor(seed, (uint64_t)(gid0 + i), ctr, n);
                if (old.has[(t - 1) * n + j])
                    from = &old.pool[16 * ((t - 1) * n + j)];
                else
                    t = 0;
            }
            memcpy(&st.boards[16 * i], from, 16);
            st.turn[i] = (uint8_t)t;
            st.seen[i] = (uint8_t)naive_stage(from, cuts, n_cuts);
            st.starts[t] += 1;
        } else {
            const int s = naive_stage(b, cuts, n_cuts);
            if (s > old.seen[i]) {
                memcpy(&st.pool[16 * ((s - 1) * n + i)], b, 16);
                st.has[(s - 1) * n + i] = 1;
                st.seen[i] = (uint8_t)s;
            }
        }
    }
}

static void header_call(State &st, const std::vector<uint8_t> &done, const uint8_t *cuts, uint64_t seed, int64_t gid0,
                        uint32_t ctr, bool count = true)
{
    CHECK(r48::nt_carousel_cuts_check(cuts, st.S - 1) == nullptr, "cuts");
    r48::nt_carousel_host(st.boards.data(), st.n, done.data(), r48::nt_cuts_pack(cuts, st.S - 1), st.pool.data(),
                          st.has.data(), st.seen.data(), st.turn.data(), count ? st.starts.data() : nullptr, seed, gid0, ctr);
}

// a board with tiles below `top` under one tile `top` (top 0: empty)
static void board_with_top(std::mt19937 &rng, int top, int8_t *b)
{
    for (int c = 0; c < 16; c++)
        b[c] = (int8_t)(top > 1 ? rng() % (unsigned)top : 0u);
    b[rng() % 16u] = (int8_t)top;
}

// ---- the draw -----------------------------------------------------------------------------------
static void test_draw()
{
    // Random123's known answers for philox4x32-10
    const uint32_t zero[4] = {0, 0, 0, 0}, zkey[2] = {0, 0};
    const uint32_t pi[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, pkey[2] = {0xa4093822u, 0x299f31d0u};
    uint32_t w[4];
    naive_philox10(zero, zkey, w);
    CHECK(w[0] == 0x6627e8d5u && w[1] == 0xe169c58du && w[2] == 0xbc57ac4cu && w[3] == 0x9b00dbd8u, "KAT zero");
    naive_philox10(pi, pkey, w);
    CHECK(w[0] == 0xd16cfe09u && w[1] == 0x94fdccebu && w[2] == 0x5001e420u && w[3] == 0x24126ea1u, "KAT pi");
    // the carousel's block for (seed, gid, ctr) = (0x0123456789ABCDEF, 2^32 + 5, 7): word 0 pinned
    // (computed with the oracle's Philox), and the donors it gives
    const uint64_t seed = 0x0123456789ABCDEFull, gid = (1ull << 32) + 5u;
    const uint32_t c[4] = {5u, 1u, 7u, 0xCA70u}, k[2] = {0x89ABCDEFu, 0x01234567u};
    naive_philox10(c, k, w);
    CHECK(w[0] == 0x0fba1e1du, "pinned word 0: %08x", w[0]);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    CHECK(r48::kCarouselTag == 0xCA70u, "the tag");
    CHECK(r48::nt_carousel_donor(gid, 7u, k0, k1, 1u) == 0u, "n = 1: slot 0");
    CHECK(r48::nt_carousel_donor(gid, 7u, k0, k1, 65u) == 3u, "n = 65");
    CHECK(r48::nt_carousel_donor(gid, 7u, k0, k1, 257u) == 15u, "n = 257");
    CHECK(r48::nt_carousel_donor(gid, 7u, k0, k1, 0x7FFFFFFFu) == 131927822u, "n = 2^31 - 1");
    CHECK(r48::nt_carousel_donor(0u, 0u, k0, k1, 65u) == 40u && r48::nt_carousel_donor(64u, 0xFFFFFFFFu, k0, k1, 257u) == 242u,
          "two more pinned donors");
    std::mt19937_64 rng(3);
    for (int it = 0; it < 2000; it++) {
        const uint64_t s = rng(), g = rng();
        const uint32_t ctr = (uint32_t)rng(), n = 1u + (uint32_t)(rng() % 0x7FFFFFFFull);
        const int64_t j = naive_donor(s, g, ctr, n);
        CHECK(j >= 0 && j < (int64_t)n && (int64_t)r48::nt_carousel_donor(g, ctr, (uint32_t)s, (uint32_t)(s >> 32), n) == j,
              "donor of a random block");
    }
    // refusals: the stage cuts' rules, and at least one cut
    const uint8_t one[1] = {4}, bad0[1] = {0}, bad16[1] = {16}, same[2] = {4, 4}, four[4] = {1, 2, 3, 4};
    CHECK(r48::nt_carousel_cuts_check(one, 1) == nullptr, "one cut is fine");
    CHECK(r48::nt_carousel_cuts_check(one, 0) && r48::nt_carousel_cuts_check(nullptr, 0) && r48::nt_carousel_cuts_check(four, 4) &&
              r48::nt_carousel_cuts_check(one, -1) && r48::nt_carousel_cuts_check(nullptr, 1),
          "n_cuts outside 1..3, NULL");
    CHECK(r48::nt_carousel_cuts_check(bad0, 1) && r48::nt_carousel_cuts_check(bad16, 1) && r48::nt_carousel_cuts_check(same, 2),
          "bad cuts");
}

// ---- random chains ------------------------------------------------------------------------------
static int test_random()
{
    const uint8_t cut_sets[3][3] = {{4, 0, 0}, {3, 5, 0}, {3, 4, 6}};
    std::mt19937 rng(17);
    int calls = 0;
    for (int S = 2; S <= 4; S++)
        for (int n : {1, 2, 65}) {
            const uint8_t *cuts = cut_sets[S - 2];
            uint64_t restarts_from_pool = 0, total = 0;
            for (int chain = 0; chain < 3; chain++) {
                State a(S, n), b(S, n);
                const uint64_t seed = ((uint64_t)rng() << 32) | rng();
                const int64_t gid0 = chain == 1 ? ((int64_t)1 << 32) + 5 : (int64_t)(rng() % 1000u);
                for (int call = 0; call < 40; call++, calls++) {
                    // as an env step leaves them: a finished board is a fresh one (any non-zero byte is
                    // done), a running one has grown by up to two exponents, now and then to 15..18
                    std::vector<uint8_t> done(n);
                    for (int i = 0; i < n; i++) {
                        int8_t *b = &a.boards[16 * i];
                        done[i] = (uint8_t)(rng() % 3u == 0u ? 1 + rng() % 255u : 0u);
                        if (done[i]) {
                            memset(b, 0, 16);
                            b[rng() % 16u] = (int8_t)(1 + rng() % 2u);
                            continue;
                        }
                        int top = 0;
                        for (int c = 0; c < 16; c++)
                            top = b[c] > top ? b[c] : top;
                        const unsigned r = rng() % 16u;
                        if (r < 10u)
                            board_with_top(rng, r == 0u ? 15 + (int)(rng() % 4u) : std::min(18, top + (int)(rng() % 3u)), b);
                    }
                    b.boards = a.boards;
                    const uint32_t ctr = call < 38 ? (uint32_t)call : 0xFFFFFFFEu + (uint32_t)(call - 38);
                    const uint64_t before = a.starts[0];
                    uint64_t n_done = 0;
                    for (int i = 0; i < n; i++)
                        n_done += done[i] ? 1u : 0u;
                    header_call(a, done, cuts, seed, gid0, ctr);
                    naive_call(b, done, cuts, seed, gid0, ctr);
                    CHECK(a == b, "S %d, n %d, chain %d, call %d: the header's loop differs from the restatement", S, n, chain, call);
                    restarts_from_pool += n_done - (a.starts[0] - before);
                }
                for (uint64_t s : a.starts)
                    total += s;
            }
            CHECK(restarts_from_pool > 0, "S %d, n %d: the chains must restart from the pool (%llu of %llu starts)", S, n,
                  (unsigned long long)restarts_from_pool, (unsigned long long)total);
        }
    return calls;
}

// ---- the named cases ----------------------------------------------------------------------------
// the first ctr >= from at which board gid0 + i of a batch of n draws donor j
static uint32_t ctr_with_donor(uint64_t seed, int64_t gid0, int i, int n, int64_t j, uint32_t from = 0)
{
    uint32_t ctr = from;
    while (naive_donor(seed, (uint64_t)(gid0 + i), ctr, n) != j)
        ctr++;
    return ctr;
}

static void test_named()
{
    const uint8_t c4[1] = {4}, c15[1] = {15}, c346[3] = {3, 4, 6};
    const uint64_t seed = 99;
    std::mt19937 rng(5);
    int8_t fresh[16] = {0}, entry[16], newer[16];
    fresh[6] = 1;
    board_with_top(rng, 4, entry);
    board_with_top(rng, 5, newer);
    {   // the donor is the board's own slot
        State st(2, 2);
        memcpy(&st.boards[0], fresh, 16);
        memcpy(&st.pool[0], entry, 16);
        st.has[0] = 1;
        const uint32_t ctr = ctr_with_donor(seed, 10, 0, 2, 0);
        header_call(st, {1, 0}, c4, seed, 10, ctr);
        CHECK(!memcmp(&st.boards[0], entry, 16) && st.turn[0] == 1 && st.seen[0] == 1 && st.starts[1] == 1 && st.starts[0] == 0,
              "own slot as donor");
        CHECK(!memcmp(&st.pool[0], entry, 16) && st.has[0] == 1 && st.has[1] == 0, "the pool is as it was");
    }
    {   // the donor records into the drawn slot in the same call: the old content is read
        State st(2, 2);
        memcpy(&st.boards[0], fresh, 16);
        memcpy(&st.boards[16], newer, 16);   // slot 1's game crosses the cut in this step
        memcpy(&st.pool[16], entry, 16);
        st.has[1] = 1;
        const uint32_t ctr = ctr_with_donor(seed, 10, 0, 2, 1);
        header_call(st, {1, 0}, c4, seed, 10, ctr);
        CHECK(!memcmp(&st.boards[0], entry, 16), "the restart reads the slot's content from before the call");
        CHECK(!memcmp(&st.pool[16], newer, 16) && st.seen[1] == 1, "and the slot then holds the new entry board");
        // the same with the slot empty before the call: what is recorded in this call is not seen
        State em(2, 2);
        memcpy(&em.boards[0], fresh, 16);
        memcpy(&em.boards[16], newer, 16);
        header_call(em, {1, 0}, c4, seed, 10, ctr);
        CHECK(!memcmp(&em.boards[0], fresh, 16) && em.turn[0] == 0 && em.starts[0] == 1 && em.starts[1] == 0,
              "an empty slot filled in this call is still empty to the restart");
        CHECK(em.has[1] == 1 && !memcmp(&em.pool[16], newer, 16), "it is filled afterwards");
        // the next restart tries stage 1 again, and now finds the board
        memcpy(&em.boards[0], fresh, 16);
        const uint32_t next = ctr_with_donor(seed, 10, 0, 2, 1, ctr + 1u);
        header_call(em, {1, 0}, c4, seed, 10, next);
        CHECK(!memcmp(&em.boards[0], newer, 16) && em.turn[0] == 1 && em.starts[1] == 1, "after a fallback the slot tries stage 1 again");
    }
    {   // turn wraps from S - 1 to 0: the fresh board stays and nothing is drawn
        State st(3, 1);
        const uint8_t c35[2] = {3, 5};
        memcpy(&st.boards[0], fresh, 16);
        memcpy(&st.pool[0], entry, 16);
        memcpy(&st.pool[16], newer, 16);
        st.has[0] = st.has[1] = 1;
        st.turn[0] = 2;
        st.seen[0] = 2;
        header_call(st, {1}, c35, seed, 0, 0);
        CHECK(!memcmp(&st.boards[0], fresh, 16) && st.turn[0] == 0 && st.seen[0] == 0 && st.starts[0] == 1, "S - 1 wraps to 0");
        header_call(st, {255}, c35, seed, 0, 1);   // n = 1: the donor is slot 0
        CHECK(!memcmp(&st.boards[0], entry, 16) && st.turn[0] == 1 && st.seen[0] == 1, "then stage 1");
        memcpy(&st.boards[0], fresh, 16);
        header_call(st, {1}, c35, seed, 0, 2);
        CHECK(!memcmp(&st.boards[0], newer, 16) && st.turn[0] == 2 && st.seen[0] == 2 && st.starts[2] == 1, "then stage 2");
    }
    {   // a board that crosses a cut in this step records; one already at seen does not; starts may be NULL
        State st(2, 2);
        int8_t below[16], other[16];
        board_with_top(rng, 3, below);
        board_with_top(rng, 6, other);
        memcpy(&st.boards[0], below, 16);
        memcpy(&st.boards[16], entry, 16);
        header_call(st, {0, 0}, c4, seed, 0, 0, false);
        CHECK(st.has[0] == 0 && st.seen[0] == 0, "below the cut: nothing is recorded");
        CHECK(st.has[1] == 1 && st.seen[1] == 1 && !memcmp(&st.pool[16], entry, 16), "at the cut: recorded");
        memcpy(&st.boards[16], other, 16);
        header_call(st, {0, 0}, c4, seed, 0, 1, false);
        CHECK(st.seen[1] == 1 && !memcmp(&st.pool[16], entry, 16), "already at seen: the entry board stays");
        CHECK(st.starts[0] == 0 && st.starts[1] == 0, "no start counted");
    }
    {   // a done board never records (turn at S - 1: it restarts from the fresh board, whatever that is)
        State st(2, 1);
        memcpy(&st.boards[0], newer, 16);
        st.turn[0] = 1;
        header_call(st, {1}, c4, seed, 0, 0);
        CHECK(st.has[0] == 0 && st.turn[0] == 0 && st.seen[0] == 1 && !memcmp(&st.boards[0], newer, 16), "done: no record");
        header_call(st, {0}, c4, seed, 0, 1);
        CHECK(st.has[0] == 0, "and it started in stage 1: it has not ENTERED it");
    }
    {   // tiles of 16 and more are above every cut, as their clamp 15 is
        for (int top : {15, 16, 17, 18}) {
            State st(2, 1);
            board_with_top(rng, top, &st.boards[0]);
            header_call(st, {0}, c15, seed, 0, 0);
            CHECK(st.has[0] == 1 && st.seen[0] == 1 && !memcmp(&st.pool[0], &st.boards[0], 16), "top %d crosses cut 15", top);
            State s4(4, 1);
            board_with_top(rng, top, &s4.boards[0]);
            header_call(s4, {0}, c346, seed, 0, 0);
            CHECK(s4.seen[0] == 3 && s4.has[2] == 1 && s4.has[0] == 0 && s4.has[1] == 0 && !memcmp(&s4.pool[32], &s4.boards[0], 16),
                  "top %d enters stage 3 directly: only that stage's slot is written", top);
        }
    }
}

int main()
{
    test_draw();
    const int calls = test_random();
    test_named();
    printf("ntuple_carousel_test: %d random calls, %s (%d failures)\n", calls, fails ? "FAILED" : "OK", fails);
    return fails ? 1 : 0;
}
