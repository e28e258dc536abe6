// Stand-alone check of the rule that picks the shadow copy's encoding (adelie_amd/csrc/shadow_kind_host.hpp), built with
// -fsanitize=address,undefined by tests/test_shadow_kind_host.py.  Fixed cases, then random inputs against a direct restatement;
// exits non-zero on the first disagreement.
#include "../../adelie_amd/csrc/shadow_kind_host.hpp"
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    CHECK(shadow_kind_parse(nullptr) == kShadowAuto && shadow_kind_parse("auto") == kShadowAuto && shadow_kind_parse("") == kShadowAuto);
    CHECK(shadow_kind_parse("f32") == kShadowF32 && shadow_kind_parse("q15") == kShadowQ15 && shadow_kind_parse("Q15") == kShadowAuto);

    // the size rule: n p 4 >= min_bytes
    const int64_t gib = int64_t(1) << 30;
    CHECK(kShadowMinBytesDefault == gib);
    CHECK(shadow_q15_wanted(kShadowAuto, 100000, 10000, gib));          // the headline: 4e9 bytes
    CHECK(!shadow_q15_wanted(kShadowAuto, 5000, 37, gib) && !shadow_q15_wanted(kShadowAuto, 1000, 4100, gib));
    CHECK(shadow_q15_wanted(kShadowAuto, 16384, 16384, gib));           // exactly 2^30
    CHECK(!shadow_q15_wanted(kShadowAuto, 16384, 16383, gib));
    CHECK(shadow_q15_wanted(kShadowAuto, 1, 1, 4) && !shadow_q15_wanted(kShadowAuto, 1, 1, 5));
    CHECK(shadow_q15_wanted(kShadowAuto, 1, 1, 0) && shadow_q15_wanted(kShadowAuto, 1, 1, -7));
    CHECK(shadow_q15_wanted(kShadowQ15, 1, 1, gib) && !shadow_q15_wanted(kShadowF32, 100000, 10000, 0));
    CHECK(!shadow_q15_wanted(kShadowAuto, 0, 10, 0) && !shadow_q15_wanted(kShadowAuto, 10, 0, 0));
    const int64_t big = std::numeric_limits<int64_t>::max();
    CHECK(!shadow_q15_wanted(kShadowAuto, 100000, 10000, big));         // no overflow on the way
    CHECK(shadow_q15_wanted(kShadowAuto, big, big, big));

    // the error rule: at least 7/8 of the columns within 2^-11 of their norm
    {
        std::vector<double> err(16, 1.0 / 4096), nrm(16, 1.0);
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 16) == kShadowQ15);
        err[0] = err[1] = 1.0 / 1024;                                   // 14 of 16 good: exactly 7/8
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 16) == kShadowQ15);
        err[2] = 1.0 / 1024;                                            // 13 of 16
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 16) == kShadowF32);
        CHECK(shadow_kind_pick(kShadowQ15, err.data(), nrm.data(), 16) == kShadowQ15);
        err.assign(16, 0.0);
        CHECK(shadow_kind_pick(kShadowF32, err.data(), nrm.data(), 16) == kShadowF32);
        nrm.assign(16, 0.0);                                            // zero columns are good
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 16) == kShadowQ15);
        err.assign(16, 1e-310);                                         // stored as zeros though not zero: bad
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 16) == kShadowF32);
        err.assign(16, std::numeric_limits<double>::quiet_NaN());
        nrm.assign(16, 1.0);
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 16) == kShadowF32);
        CHECK(shadow_kind_pick(kShadowAuto, err.data(), nrm.data(), 0) == kShadowQ15); // (never asked: p >= 1 where it is called)
        const double e1 = 1.0 / 2048, n1 = 1.0;                         // the boundary itself is good
        CHECK(shadow_kind_pick(kShadowAuto, &e1, &n1, 1) == kShadowQ15);
    }

    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> u(0, 1);
    for (int it = 0; it < 20000; ++it) {
        const int64_t n = 1 + int64_t(200000 * u(rng)), p = 1 + int64_t(20000 * u(rng));
        const int64_t mb = int64_t(std::ldexp(u(rng), int(34 * u(rng))));
        const int forced = int(3 * u(rng)) - 1;
        const bool want = forced == kShadowQ15 || (forced == kShadowAuto && (long double)n * (long double)p * 4.0L >= (long double)mb);
        CHECK(shadow_q15_wanted(forced, n, p, mb) == want);
        const int64_t pc = 1 + int64_t(40 * u(rng));
        const size_t pcs = size_t(pc);
        std::vector<double> err(pcs), nrm(pcs);
        int64_t good = 0;
        const double frac_bad = u(rng) * 0.3;
        for (int64_t j = 0; j < pc; ++j) {
            nrm[size_t(j)] = std::ldexp(0.5 + u(rng), int(600 * u(rng)) - 300);
            const bool bad = u(rng) < frac_bad;
            err[size_t(j)] = nrm[size_t(j)] * (bad ? (1.0 / 2048) * (1.01 + 5 * u(rng)) : (1.0 / 2048) * 0.99 * u(rng));
            good += !bad;
        }
        const int expect = forced >= 0 ? forced : (8 * good >= 7 * pc ? kShadowQ15 : kShadowF32);
        CHECK(shadow_kind_pick(forced, err.data(), nrm.data(), pc) == expect);
    }
    std::printf(fails ? "shadow_kind: %d check(s) FAILED\n" : "shadow_kind: ok\n", fails);
    return fails ? 1 : 0;
}
