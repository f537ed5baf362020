// Host build of the TD step's arithmetic in rein48_amd/csrc/r48_ntuple.h (nt_td_delta and
// nt_fixed_delta, the word one hit adds to acc) checked against a double-precision restatement
// written here -- a CPU test harness, never shipped. Build+run: tests/test_ntuple_fused_host.py
// (g++ -O2).
#include <random>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

// ---- the naive restatement, in double ---------------------------------------------------------
// every fp32 operation of the contract is one double operation rounded to float: the double result
// is exact, or carries 29 bits beyond the float's, so its rounding to float is the fp32 operation's
// (a double rounding would need those 29 bits to read exactly 100...0)
static float naive_delta(bool prev_done, int32_t reward, float value, float prev_value)
{
    float target = 0.0f;
    if (!prev_done)
        target = (float)((double)reward + (double)value);
    return (float)((double)target - (double)prev_value);
}

// clamp, scale by 2^16 (exact), round to nearest with ties to even -- by hand, no rint
static long long naive_fixed(float delta)
{
    double d = (double)delta;
    if (d < -1048576.0)
        d = -1048576.0;
    if (d > 1048576.0)
        d = 1048576.0;
    const double x = d * 65536.0;
    const double lo = std::floor(x), frac = x - lo;
    long long q = (long long)lo;
    if (frac > 0.5 || (frac == 0.5 && (q & 1)))
        q += 1;
    return q;
}

int main()
{
    // a prev_done row: the target is 0 whatever the move returned
    CHECK(bits(r48::nt_td_delta(1u, 64u, 123.5f, 10.25f)) == bits(-10.25f), "prev_done: target 0");
    CHECK(bits(r48::nt_td_delta(255u, 4u, -3.0f, -7.5f)) == bits(7.5f), "prev_done is any non-zero byte");
    CHECK(bits(r48::nt_td_delta(1u, 0u, 0.0f, 0.0f)) == bits(0.0f), "prev_done, all zero");
    // zero reward, negative values
    CHECK(bits(r48::nt_td_delta(0u, 0u, 5.5f, 2.25f)) == bits(3.25f), "zero reward");
    CHECK(bits(r48::nt_td_delta(0u, 0u, -5.5f, -2.25f)) == bits(-3.25f), "zero reward, negative values");
    CHECK(bits(r48::nt_td_delta(0u, 8u, -100.0f, 50.0f)) == bits(-142.0f), "negative value");
    // the sum rounds before the difference is taken: (2^24 + 1 -> 2^24) - 2^24 = 0, not 1
    CHECK(bits(r48::nt_td_delta(0u, 1u, 16777216.0f, 16777216.0f)) == bits(0.0f), "reward + value rounds first");
    {
        std::mt19937 rng(11);
        std::uniform_real_distribution<float> u(-3000.0f, 3000.0f);
        const float scales[4] = {1.0f, 1e-3f, 700.0f, 3e6f};
        for (int k = 0; k < 400000; k++) {
            const uint32_t done = (rng() & 3u) == 0u;
            const uint32_t reward = (rng() & 1u) ? 0u : 4u * (rng() % 16384u);      // merge rewards: multiples of 4
            const float s = scales[k & 3], value = s * u(rng), prev = s * u(rng);
            const float got = r48::nt_td_delta(done, reward, value, prev);
            const float want = naive_delta(done != 0u, (int32_t)reward, value, prev);
            CHECK(bits(got) == bits(want), "delta(%u, %u, %a, %a) = %a, naive %a", done, reward, value, prev, got, want);
        }
    }

    // the fixed-point word: exact cases
    CHECK(r48::nt_fixed_delta(0.0f) == 0 && r48::nt_fixed_delta(-0.0f) == 0, "zero");
    CHECK(r48::nt_fixed_delta(1.0f) == 65536 && r48::nt_fixed_delta(-2.5f) == -163840, "whole units");
    // at and beyond the clamp
    const long long top = 1ll << 36;
    CHECK(r48::nt_fixed_delta(1048576.0f) == top && r48::nt_fixed_delta(-1048576.0f) == -top, "at +-2^20");
    CHECK(r48::nt_fixed_delta(1048576.125f) == top && r48::nt_fixed_delta(-1048577.0f) == -top, "just beyond +-2^20");
    CHECK(r48::nt_fixed_delta(3e6f) == top && r48::nt_fixed_delta(-3e6f) == -top, "far beyond +-2^20");
    CHECK(r48::nt_fixed_delta(INFINITY) == top && r48::nt_fixed_delta(-INFINITY) == -top, "infinities");
    CHECK(r48::nt_fixed_delta(std::nextafterf(1048576.0f, 0.0f)) == top - 4096, "the float below 2^20 (ulp 2^-4)");
    // ties of d * 65536: k + 1/2 goes to the even neighbour, both signs
    for (int k = -9; k <= 9; k++) {
        const float d = ((float)k + 0.5f) / 65536.0f;                                // exact
        const long long want = (k & 1) ? k + 1 : k;
        CHECK(r48::nt_fixed_delta(d) == want, "tie %d + 1/2 -> %lld, got %lld", k, want, r48::nt_fixed_delta(d));
        CHECK(naive_fixed(d) == want, "the restatement's own tie rule at %d + 1/2", k);
    }
    CHECK(r48::nt_fixed_delta(123.0f + 0.5f / 65536.0f) == 123 * 65536, "a tie on a larger word goes to the even one");
    CHECK(r48::nt_fixed_delta(123.0f + 1.5f / 65536.0f) == 123 * 65536 + 2, "and up where the upper one is even");
    // below half a unit, and the nearest floats on either side of a tie
    CHECK(r48::nt_fixed_delta(0.49f / 65536.0f) == 0 && r48::nt_fixed_delta(0.51f / 65536.0f) == 1, "either side of 1/2");
    {
        const float tie = 2.5f / 65536.0f;
        CHECK(r48::nt_fixed_delta(std::nextafterf(tie, 0.0f)) == 2 && r48::nt_fixed_delta(std::nextafterf(tie, 1.0f)) == 3,
              "the floats next to the tie 2 + 1/2");
    }
    {
        std::mt19937 rng(12);
        std::uniform_real_distribution<float> u(-1.0f, 1.0f);
        const float scales[5] = {1e-4f, 1.0f, 300.0f, 1048576.0f, 4e6f};
        for (int k = 0; k < 500000; k++) {
            const float d = scales[k % 5] * u(rng);
            const long long got = r48::nt_fixed_delta(d), want = naive_fixed(d);
            CHECK(got == want, "fixed(%a) = %lld, naive %lld", d, got, want);
            CHECK(got >= -top && got <= top, "fixed(%a) = %lld outside +-2^36", d, got);
        }
        // halves of small words, where ties are dense
        for (int k = 0; k < 200000; k++) {
            const float d = (float)((int)(rng() % 4000001u) - 2000000) / 131072.0f;  // multiples of 2^-17
            CHECK(r48::nt_fixed_delta(d) == naive_fixed(d), "fixed(%a) = %lld, naive %lld", d, r48::nt_fixed_delta(d), naive_fixed(d));
        }
    }
    // the two together, as the kernel chains them
    CHECK(r48::nt_fixed_delta(r48::nt_td_delta(0u, 4u, 1.5f, 0.25f)) == 344064, "delta 5.25 -> 5.25 * 2^16");
    CHECK(r48::nt_fixed_delta(r48::nt_td_delta(1u, 4u, 1.5f, 2097152.0f)) == -top, "a prev_done row beyond the clamp");

    printf("%s (%d failures)\n", fails ? "FAILED" : "OK", fails);
    return fails ? 1 : 0;
}
