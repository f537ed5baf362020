// Host build of the temporal-coherence rule of rein48_amd/csrc/r48_ntuple.h (nt_mean, nt_tc_rate,
// nt_tc_update, nt_tc_rate_mean) checked against a naive double-precision restatement written
// here -- a CPU test harness, never shipped. Build+run: tests/test_ntuple_tc_host.py (g++ -O2).
#include <random>

#include "../../rein48_amd/csrc/r48_ntuple.h"
#include "ntuple_naive.h"

// ---- the naive restatement, in double ---------------------------------------------------------
struct Naive {
    double table, e, a;
    double rate() const
    {
        if (!(a > 0.0))
            return 1.0;
        const double r = std::fabs(e) / a;
        return r < 1.0 ? r : 1.0;
    }
    void update(double mean, double step)
    {
        const double r = rate();
        table += step * r * mean;
        e += mean;
        a += std::fabs(mean);
    }
};

int main()
{
    // no history: rate 1, and the table moves by the bits of plain apply's `table += step * mean`
    CHECK(r48::nt_tc_rate(0.0f, 0.0f) == 1.0f, "A == 0 must give rate 1");
    CHECK(r48::nt_tc_rate(5.0f, 0.0f) == 1.0f, "A == 0 must give rate 1 whatever E holds");
    {
        std::mt19937 rng(1);
        std::uniform_real_distribution<float> u(-1000.0f, 1000.0f);
        for (int k = 0; k < 100000; k++) {
            const float old = u(rng), mean = u(rng), step = 0.25f / 40.0f;
            float t = old, e = 0.0f, a = 0.0f;
            r48::nt_tc_update(t, e, a, mean, step);
            float plain = old;
            plain += step * mean;
            CHECK(bits(t) == bits(plain), "no history: %a, plain apply %a", t, plain);
            CHECK(bits(e) == bits(mean) && bits(a) == bits(std::fabs(mean)), "E, A after the first update");
        }
    }

    // nt_mean is the expression of plain apply: exact where acc / 2^16 / cnt is representable
    CHECK(r48::nt_mean(3 * 65536ll * 64, 64u) == 3.0f, "mean of 64 hits of 3");
    CHECK(r48::nt_mean(-5 * 65536ll, 2u) == -2.5f, "mean of two hits summing to -5");
    CHECK(bits(r48::nt_mean(65536ll * 64 * 7 + 64 * 3, 64u)) == bits(r48::nt_mean(65536ll * 7 + 3, 1u)),
          "64 copies give the bits of one");

    // same-sign means: |E| == A bit for bit after every update, the rate exactly 1, both signs
    for (int sign = -1; sign <= 1; sign += 2) {
        std::mt19937 rng(2 + sign);
        std::uniform_real_distribution<float> u(1e-3f, 700.0f);
        float t = 1.5f, e = 0.0f, a = 0.0f;
        Naive nv{1.5, 0.0, 0.0};
        for (int k = 0; k < 2000; k++) {
            const float mean = (float)sign * u(rng);
            CHECK(r48::nt_tc_rate(e, a) == 1.0f, "same sign, update %d: rate %a", k, r48::nt_tc_rate(e, a));
            r48::nt_tc_update(t, e, a, mean, 0.03125f);
            nv.update(mean, 0.03125);
            CHECK(bits(std::fabs(e)) == bits(a), "same sign, update %d: |E| %a, A %a", k, std::fabs(e), a);
        }
        // 2000 fp32 additions each: 2000 * 2^-24 relative on sums of one sign
        CHECK(std::fabs(t - nv.table) <= 3 * 2000 * std::ldexp(1.0, -24) * std::fabs(nv.table), "table %a vs %a", t, nv.table);
        CHECK(std::fabs(e - nv.e) <= 2000 * std::ldexp(1.0, -24) * std::fabs(nv.e), "E %a vs %a", e, nv.e);
        CHECK(std::fabs(a - nv.a) <= 2000 * std::ldexp(1.0, -24) * nv.a, "A %a vs %a", a, nv.a);
    }

    // alternating signs of one size: E is +d, 0, +d, 0, ..., A grows by d -- the rate before each
    // update never rises from one update of the same parity to the next and falls towards 0; it
    // equals the naive one to a few ulp
    {
        const float d = 3.0f;
        float t = 0.0f, e = 0.0f, a = 0.0f;
        Naive nv{0.0, 0.0, 0.0};
        float last_odd = 2.0f;
        for (int k = 0; k < 200; k++) {
            const float mean = (k & 1) ? -d : d;
            const float rate = r48::nt_tc_rate(e, a);
            CHECK(std::fabs(rate - nv.rate()) <= 4 * std::ldexp(1.0, -24), "alternating, update %d: rate %a vs %a", k, rate,
                  nv.rate());
            if (k & 1) {                                   // before an odd update E = d, A = k d: rate 1 / k
                CHECK(rate < last_odd || k == 1, "alternating, update %d: rate %a did not fall below %a", k, rate, last_odd);
                last_odd = rate;
            } else if (k > 0) {
                CHECK(rate == 0.0f, "alternating, update %d: E cancelled, rate %a", k, rate);
            }
            r48::nt_tc_update(t, e, a, mean, 0.5f);
            nv.update(mean, 0.5);
        }
        CHECK(last_odd < 0.01f, "alternating: the rate fell to %a only", last_odd);
        CHECK(std::fabs(t - nv.table) <= 200 * std::ldexp(1.0, -22) * 3.0, "alternating: table %a vs %a", t, nv.table);
    }
    // alternating signs of random sizes: E is a bounded-step random walk (|E| ~ 0.4 sqrt(k)) under
    // A ~ k, so the rate stays in [0, 1], follows the naive one, and its maximum over the last 50
    // of 400 updates is far below 1 (|E| would have to reach 35, eighty standard deviations)
    {
        std::mt19937 rng(7);
        std::uniform_real_distribution<float> u(0.5f, 1.5f);
        float t = 0.0f, e = 0.0f, a = 0.0f;
        Naive nv{0.0, 0.0, 0.0};
        float last_max = 2.0f;
        for (int blk = 0; blk < 8; blk++) {
            float mx = 0.0f;
            for (int k = 0; k < 50; k++) {
                const float mean = ((k & 1) ? -1.0f : 1.0f) * u(rng);
                const float rate = r48::nt_tc_rate(e, a);
                CHECK(rate >= 0.0f && rate <= 1.0f, "rate %a outside [0, 1]", rate);
                CHECK(std::fabs(rate - nv.rate()) <= 1e-5, "random alternating: rate %a vs %a", rate, nv.rate());
                mx = rate > mx ? rate : mx;
                r48::nt_tc_update(t, e, a, mean, 0.5f);
                nv.update(mean, 0.5);
            }
            CHECK(blk > 0 || mx == 1.0f, "the first update runs at rate 1, the block's max is %a", mx);
            last_max = mx;
        }
        CHECK(last_max < 0.1f, "random alternating: the rate is still %a after 350 updates", last_max);
        CHECK(std::fabs(t - nv.table) <= 1e-4, "random alternating: table %a vs %a", t, nv.table);
    }

    // mean == 0 changes nothing, with and without history
    {
        const float cases[3][3] = {{2.5f, 0.0f, 0.0f}, {-7.25f, 3.0f, 9.0f}, {1e-3f, -4.0f, 4.0f}};
        for (const auto &c : cases) {
            float t = c[0], e = c[1], a = c[2];
            r48::nt_tc_update(t, e, a, r48::nt_mean(0, 17u), 0.125f);
            CHECK(bits(t) == bits(c[0]) && bits(e) == bits(c[1]) && bits(a) == bits(c[2]), "mean 0 changed (%a, %a, %a)", c[0],
                  c[1], c[2]);
        }
    }

    // the clamp: |E| above A (set by hand, the rule itself never does it) still gives rate 1
    CHECK(r48::nt_tc_rate(10.0f, 4.0f) == 1.0f && r48::nt_tc_rate(-10.0f, 4.0f) == 1.0f, "the clamp at 1");
    CHECK(r48::nt_tc_rate(-2.0f, 4.0f) == 0.5f && r48::nt_tc_rate(2.0f, 4.0f) == 0.5f, "rate |E| / A = 1 / 2");
    {
        float t = 1.0f, e = -10.0f, a = 4.0f;
        r48::nt_tc_update(t, e, a, 8.0f, 0.25f);
        CHECK(t == 3.0f && e == -2.0f && a == 12.0f, "clamped update: (%a, %a, %a)", t, e, a);
    }

    // nt_tc_rate_mean: the mean over a board's 8m hits in the header's order against the naive mean
    {
        const uint8_t cells[2 * 3] = {0, 1, 2, 5, 9, 10};
        r48::NtLayout lay;
        CHECK(r48::nt_expand(cells, 2, 3, lay) == nullptr, "layout");
        const size_t size = 2 * 4096;
        std::vector<float> E(size, 0.0f), A(size, 0.0f);
        int8_t raw[16] = {1, 2, 3, 0, 0, 4, 5, 1, 2, 2, 0, 17, 3, 1, 0, 6};
        r48::Board b;
        memcpy(&b, raw, 16);
        const r48::NtBoard nb = r48::nt_pack(b);
        CHECK(r48::nt_tc_rate_mean<3>(nb, lay, E.data(), A.data()) == 1.0f, "a fresh net has rate 1");
        std::mt19937 rng(3);
        std::uniform_real_distribution<float> u(0.0f, 1.0f);
        for (size_t k = 0; k < size; k++) {
            A[k] = u(rng) < 0.2f ? 0.0f : 10.0f * u(rng);
            E[k] = A[k] * (2.0f * u(rng) - 1.0f);
        }
        double want = 0.0;
        for (int p = 0; p < 16; p++) {
            const uint32_t at = r48::nt_entry<3>(nb, lay, p);
            want += Naive{0.0, E[at], A[at]}.rate();
        }
        const float got = r48::nt_tc_rate_mean<3>(nb, lay, E.data(), A.data());
        CHECK(std::fabs(got - want / 16.0) <= 16 * std::ldexp(1.0, -24), "rate mean %a vs %a", got, want / 16.0);
    }

    printf("%s (%d failures)\n", fails ? "FAILED" : "OK", fails);
    return fails ? 1 : 0;
}
