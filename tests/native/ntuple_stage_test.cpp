// Host build of the multi-stage contract of rein48_amd/csrc/r48_ntuple.h: nt_stage, the staged
// value and search, and the staged update -- the header's PULL form (nt_staged_update_pull) against
// the PUSH form the kernels run, restated naively in ntuple_stage_naive.h. A CPU test harness, never
// shipped. Build+run: tests/test_ntuple_stage_host.py (g++ -O2, and once more with
// -fsanitize=address,undefined).
#include <random>

#include "ntuple_stage_naive.h"

static r48::NtLayout expand(const Layout &ly)
{
    r48::NtLayout lay;
    CHECK(r48::nt_expand(ly.cells, ly.m, ly.L, lay) == nullptr, "layout %s", ly.name);
    return lay;
}

// ---- nt_stage ---------------------------------------------------------------------------------
static void test_stage()
{
    const uint8_t cut_sets[3][3] = {{15, 0, 0}, {1, 0, 0}, {1, 2, 3}};
    const int n_cuts[3] = {1, 1, 3};
    std::mt19937 rng(11);
    for (int k = 0; k < 3; k++) {
        const uint8_t *cuts = cut_sets[k];
        CHECK(r48::nt_cuts_check(cuts, n_cuts[k]) == nullptr, "cuts %d", k);
        const r48::NtCuts packed = r48::nt_cuts_pack(cuts, n_cuts[k]);
        // the largest tile at every exponent 0..18 (so at each cut - 1, cut, cut + 1, at 15 and in
        // the clamped range 16..18), in every cell, under smaller random tiles
        for (int top = 0; top <= 18; top++)
            for (int cell = 0; cell < 16; cell++) {
                int8_t b[16];
                for (int c = 0; c < 16; c++)
                    b[c] = (int8_t)(top ? rng() % (unsigned)top : 0u);
                b[cell] = (int8_t)top;
                int want = 0;
                for (int j = 0; j < n_cuts[k]; j++)
                    want += (top < 15 ? top : 15) >= cuts[j] ? 1 : 0;
                const int got = (int)r48::nt_stage(packed, load(b));
                CHECK(got == want && got == naive_stage(b, cuts, n_cuts[k]), "cuts %d, top %d in cell %d: stage %d, want %d", k,
                      top, cell, got, want);
                if (top >= 15) {
                    b[cell] = 15;
                    CHECK(got == (int)r48::nt_stage(packed, load(b)), "cuts %d: top %d must give the stage of 15", k, top);
                }
            }
    }
    CHECK(r48::nt_stage(r48::nt_cuts_pack(nullptr, 0), load((const int8_t *)"\17\17\17\17\17\17\17\17\17\17\17\17\17\17\17\17")) == 0u,
          "no cuts: stage 0");
    // refusals
    const uint8_t bad0[1] = {0}, bad16[1] = {16}, same[2] = {4, 4}, down[2] = {5, 4}, four[4] = {1, 2, 3, 4};
    CHECK(r48::nt_cuts_check(bad0, 1) && r48::nt_cuts_check(bad16, 1), "a cut outside 1..15 is refused");
    CHECK(r48::nt_cuts_check(same, 2) && r48::nt_cuts_check(down, 2), "cuts not strictly ascending are refused");
    CHECK(r48::nt_cuts_check(four, 4) && r48::nt_cuts_check(four, -1) && r48::nt_cuts_check(nullptr, 1), "n_cuts, NULL");
    CHECK(r48::nt_cuts_check(nullptr, 0) == nullptr, "n_cuts == 0 needs no cuts");
}

// random board: tiles below `low`, and the largest tile `top` in one cell
static void random_board(std::mt19937 &rng, int low, int top, int8_t *b)
{
    for (int c = 0; c < 16; c++)
        b[c] = (int8_t)(rng() % (unsigned)low);
    b[rng() % 16u] = (int8_t)top;
}

// ---- the staged value and search: the board's stage block, the afterstate's stage --------------
template <int L>
static void test_value_and_search(const Layout &ly)
{
    const r48::NtLayout lay = expand(ly);
    const uint8_t cuts[3] = {3, 4, 6};
    const r48::NtCuts packed = r48::nt_cuts_pack(cuts, 3);
    const size_t block = (size_t)ly.m << (4 * L);
    std::vector<float> tables(4 * block);
    std::mt19937 rng(5);
    for (float &x : tables)
        x = (float)((int)(rng() % 2001u) - 1000);   // integers: every sum is exact
    for (int k = 0; k < 400; k++) {
        int8_t b[16];
        random_board(rng, 3, 2 + (int)(rng() % 6u), b);
        const r48::Board board = load(b);
        const int s = naive_stage(b, cuts, 3);
        const float v = r48::nt_value<L>(r48::nt_pack(board), lay, tables.data(), r48::nt_base<L>(packed, ly.m, board));
        CHECK(v == r48::nt_value<L>(r48::nt_pack(board), lay, tables.data() + s * block), "%s: V is not the stage block's", ly.name);
        CHECK((double)v == naive_value_staged(ly, tables, b, cuts, 3), "%s: V %a vs naive %a", ly.name, v,
              naive_value_staged(ly, tables, b, cuts, 3));
        // depth 1: q[a] = r + V(afterstate) in the AFTERSTATE's stage (a merge can cross a cut)
        float q[4];
        uint32_t legal;
        r48::nt_search_board<L>(board, lay, tables.data(), 1, q, legal, packed);
        const Grid g = grid_of(b);
        for (int a = 0; a < 4; a++) {
            Grid out;
            long r;
            if (!naive_move(g, a, out, r)) {
                CHECK(!((legal >> a) & 1u), "%s: move %d is illegal", ly.name, a);
                continue;
            }
            int8_t ab[16];
            for (int c = 0; c < 16; c++)
                ab[c] = (int8_t)out.g[c >> 2][c & 3];
            CHECK((double)q[a] == (double)r + naive_value_staged(ly, tables, ab, cuts, 3), "%s: q[%d] = %a", ly.name, a, q[a]);
        }
        // depth 2 with the policy equals the unstaged search on a net whose stages are all alike
        if (k < 40) {
            std::vector<float> alike(4 * block);
            for (int st = 0; st < 4; st++)
                std::copy(tables.begin(), tables.begin() + block, alike.begin() + st * block);
            float q0[4], q1[4];
            uint32_t l0, l1;
            const uint32_t a0 = r48::nt_search_board<L>(board, lay, tables.data(), 2, q0, l0);
            const uint32_t a1 = r48::nt_search_board<L>(board, lay, alike.data(), 2, q1, l1, packed);
            CHECK(a0 == a1 && l0 == l1 && !memcmp(q0, q1, sizeof q0), "%s: depth 2 over equal stages", ly.name);
        }
    }
}

// ---- push against pull ------------------------------------------------------------------------
// the header's pull-form arrays next to the naive push-form net
struct PullNet {
    std::vector<float> tables, tc_e, tc_a;
    std::vector<uint8_t> own;
};

template <int L>
static void compare(const Layout &ly, const StagedNet &push, const PullNet &pull, int call)
{
    for (int s = 0; s < push.S; s++)
        for (size_t e = 0; e < push.block; e++) {
            const size_t at = s * push.block + e;
            const float resolved = r48::nt_pull_read(pull.tables.data(), pull.own.data(), (int64_t)push.block, s, (int64_t)e);
            CHECK(bits(resolved) == bits(push.tables[at]), "%s call %d: (%d, %zu) pull %a, push %a", ly.name, call, s, e, resolved,
                  push.tables[at]);
            CHECK(push.own[at] == pull.own[at], "%s call %d: own (%d, %zu)", ly.name, call, s, e);
            if (!push.tc_e.empty())
                CHECK(bits(push.tc_e[at]) == bits(pull.tc_e[at]) && bits(push.tc_a[at]) == bits(pull.tc_a[at]),
                      "%s call %d: E / A (%d, %zu)", ly.name, call, s, e);
            // the invariant: an unowned entry has the bits of the stage below
            if (s >= 1 && !push.own[at])
                CHECK(bits(push.tables[at]) == bits(push.tables[at - push.block]), "%s call %d: invariant (%d, %zu)", ly.name,
                      call, s, e);
        }
}

template <int L>
static void test_push_pull(const Layout &ly, int n_cuts, bool tc, int calls)
{
    const r48::NtLayout lay = expand(ly);
    const uint8_t cuts[3] = {3, 4, 6};
    const r48::NtCuts packed = r48::nt_cuts_pack(cuts, n_cuts);
    StagedNet push(ly, n_cuts, tc);
    PullNet pull{push.tables, push.tc_e, push.tc_a, push.own};
    std::mt19937 rng(100 + 10 * L + n_cuts + (tc ? 1 : 0));
    std::uniform_real_distribution<float> u(-50.0f, 50.0f);
    for (int call = 0; call < calls; call++) {
        const int n = 1 + (int)(rng() % 24u);
        std::vector<int8_t> raw(16 * n);
        std::vector<r48::Board> boards(n);
        std::vector<float> delta(n);
        std::vector<uint8_t> valid(n);
        // the largest tile grows with the calls, so the higher stages are entered late, as in a game
        const int reach = 2 + (call * 7) / calls;
        for (int i = 0; i < n; i++) {
            random_board(rng, 3, 2 + (int)(rng() % (unsigned)reach), raw.data() + 16 * i);
            boards[i] = load(raw.data() + 16 * i);
            delta[i] = u(rng);
            valid[i] = rng() % 8u ? 1 : 0;
        }
        const bool all = rng() % 4u == 0u;   // valid == NULL: every board
        naive_update_push(ly, push, raw.data(), delta.data(), all ? nullptr : valid.data(), n, cuts, n_cuts, 0.125f);
        r48::nt_staged_update_pull<L>(boards.data(), delta.data(), all ? nullptr : valid.data(), n, lay, packed, 0.125f,
                                      pull.tables.data(), tc ? pull.tc_e.data() : nullptr, tc ? pull.tc_a.data() : nullptr,
                                      pull.own.data());
        compare<L>(ly, push, pull, call);
    }
    size_t owned = 0;
    for (size_t at = push.block; at < push.own.size(); at++)
        owned += push.own[at];
    CHECK(owned > 0, "%s: no entry above stage 0 was ever updated", ly.name);
}

// ---- the two scenarios the contract spells out ------------------------------------------------
// One call holds the first hit of (1, e) together with a hit of (0, e): (1, e) starts from the
// pre-call tables[0][e] and the push of (0, e) does not overwrite it. Then a three-stage chain in
// which (1, e) is owned and (2, e) is not.
static void test_scenarios(bool tc)
{
    const Layout &ly = k1x2;
    const r48::NtLayout lay = expand(ly);
    const uint8_t cuts[2] = {3, 5};
    const r48::NtCuts packed = r48::nt_cuts_pack(cuts, 2);
    // two boards alike but for one cell: a 1 (stage 0) or a 3 (stage 1), so most of their hits coincide
    int8_t a[16] = {1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1}, b[16];
    memcpy(b, a, 16);
    b[0] = 3;
    int8_t raw[32];
    memcpy(raw, a, 16);
    memcpy(raw + 16, b, 16);
    const std::vector<size_t> ha = naive_hits(ly, a), hb = naive_hits(ly, b);
    size_t e = ~(size_t)0;
    for (size_t x : ha)
        for (size_t y : hb)
            if (x == y)
                e = x;
    CHECK(e != ~(size_t)0, "the two boards share no entry");
    StagedNet push(ly, 2, tc);
    for (size_t k = 0; k < push.block; k++)   // a trained stage 0, promoted to the stages above
        push.tables[k] = push.tables[push.block + k] = push.tables[2 * push.block + k] = 100.0f + (float)k;
    PullNet pull{push.tables, push.tc_e, push.tc_a, push.own};
    const r48::Board boards[2] = {load(a), load(b)};
    const float delta[2] = {16.0f, -32.0f}, step = 0.5f;
    const float v0 = push.tables[e];
    auto both = [&](int first, int n) {
        naive_update_push(ly, push, raw + 16 * first, delta + first, nullptr, n, cuts, 2, step);
        r48::nt_staged_update_pull<2>(boards + first, delta + first, nullptr, n, lay, packed, step, pull.tables.data(),
                                      tc ? pull.tc_e.data() : nullptr, tc ? pull.tc_a.data() : nullptr, pull.own.data());
        compare<2>(ly, push, pull, first * 10 + n);
    };
    both(0, 2);
    // e is hit once or more by each board; every hit of a board carries the board's delta, so the
    // mean is the delta (exact in fixed point), and with no history TC runs at rate 1
    CHECK(bits(push.tables[e]) == bits(v0 + step * 16.0f), "(0, e) = %a, want %a", push.tables[e], v0 + step * 16.0f);
    CHECK(bits(push.tables[push.block + e]) == bits(v0 + step * -32.0f), "(1, e) = %a must start from the pre-call (0, e) %a",
          push.tables[push.block + e], v0);
    CHECK(push.own[push.block + e] == 1 && push.own[2 * push.block + e] == 0, "(1, e) owned, (2, e) not");
    // the chain: (2, e) follows (1, e), not (0, e)
    CHECK(bits(push.tables[2 * push.block + e]) == bits(push.tables[push.block + e]), "(2, e) must follow (1, e)");
    const float v1 = push.tables[push.block + e];
    both(0, 1);   // stage 0 alone: stops at the owned (1, e)
    CHECK(bits(push.tables[push.block + e]) == bits(v1) && bits(push.tables[2 * push.block + e]) == bits(v1),
          "an update of (0, e) reached past the owned (1, e)");
    both(1, 1);   // stage 1 alone: pushed to (2, e)
    CHECK(bits(push.tables[push.block + e]) != bits(v1), "(1, e) did not move");
    CHECK(bits(push.tables[2 * push.block + e]) == bits(push.tables[push.block + e]), "(2, e) did not follow (1, e)");
    CHECK(push.own[2 * push.block + e] == 0, "(2, e) must stay unowned");
}

int main()
{
    test_stage();
    test_value_and_search<4>(kLinesSquares);
    test_value_and_search<3>(k3x3);
    test_value_and_search<2>(k1x2);
    // L = 2 and 3, m = 1 and 2 and 3, S = 2 and 4, with and without TC
    const Layout k2x2 = {"2x2", 2, 2, {0, 1, 5, 6}};
    const Layout k1x3 = {"1x3", 1, 3, {0, 1, 4}};
    const Layout k2x3 = {"2x3", 2, 3, {0, 1, 2, 5, 9, 10}};
    for (int tc = 0; tc < 2; tc++)
        for (int n_cuts = 1; n_cuts <= 3; n_cuts += 2) {
            test_push_pull<2>(k1x2, n_cuts, tc != 0, 300);
            test_push_pull<2>(k2x2, n_cuts, tc != 0, 300);
            test_push_pull<3>(k1x3, n_cuts, tc != 0, 200);
            test_push_pull<3>(k2x3, n_cuts, tc != 0, 200);
        }
    test_scenarios(false);
    test_scenarios(true);
    printf("%s (%d failures)\n", fails ? "FAILED" : "OK", fails);
    return fails ? 1 : 0;
}
