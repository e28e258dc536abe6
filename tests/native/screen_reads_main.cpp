// Stand-alone check of the pivot rule's reading of the sorted scores and of the depth rule around it
// (adelie_amd/csrc/screen_reads_host.hpp), built with -fsanitize=address,undefined by tests/test_screen_reads_host.py.
// 20 000 random score sets; for every M from 0 to G, pivot_read on the sorted top M is held against pivot_read on all G and
// against a direct restatement of the positions the rule reads.  Exits non-zero on the first disagreements.
#include "../../adelie_amd/csrc/screen_reads_host.hpp"
#include <cstdio>
#include <random>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

using Pair = std::pair<double, int64_t>;

// The rule as screen() had it inline, on all G sorted pairs, recording every position it reads; lowest: the smallest of them
struct Ref {
    std::vector<int64_t> append;
    int64_t lowest;
};
static Ref reference(const std::vector<Pair>& keyed, int64_t subset_size, double slack, int64_t nna, const std::vector<char>& in_s) {
    const int64_t G = int64_t(keyed.size());
    Ref r;
    r.lowest = G - subset_size;
    std::vector<double> sub(size_t(subset_size), 0.0), mses(size_t(subset_size), 0.0), ind(size_t(subset_size), 0.0);
    for (int64_t i = 0; i < subset_size; ++i) {
        sub[size_t(i)] = keyed[size_t(G - subset_size + i)].first;
        ind[size_t(i)] = double(i);
    }
    const int64_t full_pivot_idx = G - subset_size + search_pivot(ind, sub, mses);
    for (int64_t ii = G - 1; ii >= full_pivot_idx; --ii) {
        r.lowest = std::min(r.lowest, ii);
        const int64_t i = keyed[size_t(ii)].second;
        if (in_s[size_t(i)]) continue;
        r.append.push_back(i);
    }
    int64_t count = 0;
    for (int64_t ii = full_pivot_idx - 1; ii >= 0; --ii) {
        if (count >= slack * nna) break;
        r.lowest = std::min(r.lowest, ii);
        const int64_t i = keyed[size_t(ii)].second;
        if (in_s[size_t(i)]) continue;
        r.append.push_back(i);
        ++count;
    }
    return r;
}

int main() {
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> u(0, 1);
    int64_t n_short = 0, n_ok = 0, G_max = 0;
    for (int it = 0; it < 20000; ++it) {
        // most sets are small, so that every M from 0 to G is affordable; one in 250 is large, the last one G = 20 000
        int64_t G = 1 + int64_t(64 * u(rng));
        if (it % 250 == 249) G = 1 + int64_t(std::exp(u(rng) * std::log(20000.0)));
        if (it == 19999) G = 20000;
        G = std::min<int64_t>(G, 20000);
        G_max = std::max(G_max, G);
        const double cap = 0.1 + u(rng);
        const int kind = it % 4; // 0: screen groups scattered, 1: clustered at the top, 2: clustered + many ties at the cap, 3: none
        const int64_t n_screen = kind == 3 ? 0 : std::min<int64_t>(int64_t(u(rng) * double(G) * 0.6), 300);
        std::vector<char> in_s(size_t(G), 0);
        std::vector<Pair> keyed(size_t(G), Pair(0.0, 0));
        for (int64_t g = 0; g < G; ++g) {
            double s = cap * u(rng) * 1.3;
            if (kind == 2 && u(rng) < 0.3) s = cap;
            if (u(rng) < 0.05) s = std::floor(s * 8) / 8; // ties below the cap as well
            keyed[size_t(g)] = Pair(std::min(s, cap), g);
        }
        std::sort(keyed.begin(), keyed.end());
        for (int64_t k = 0; k < n_screen; ++k) {
            // clustered: the top positions (active groups tie at the cap); scattered: anywhere
            const int64_t pos = kind == 0 ? int64_t(u(rng) * double(G)) : G - 1 - int64_t(u(rng) * u(rng) * double(std::min<int64_t>(G, 2 * n_screen + 1)));
            in_s[size_t(keyed[size_t(std::max<int64_t>(0, std::min(pos, G - 1)))].second)] = 1;
        }
        int64_t old_size = 0;
        for (char c : in_s) old_size += c;
        const int64_t nna = int64_t(51 * u(rng)) % 51;
        const int64_t subset_min = int64_t(3 * u(rng)); // (0 included: the rule then reads the top position alone)
        const int64_t subset_size = pivot_subset_size(old_size, G, 0.1, subset_min);
        const double slack = 1.25;
        auto is_s = [&](int64_t i) { return in_s[size_t(i)] != 0; };
        std::vector<int64_t> full, part;
        const PivotRead rf = pivot_read(keyed.data(), G, G, subset_size, slack, nna, is_s, full);
        const Ref ref = reference(keyed, subset_size, slack, nna, in_s);
        CHECK(rf.sufficient);
        CHECK(full == ref.append);
        CHECK(rf.reads == G - ref.lowest);
        CHECK(rf.reads <= pivot_need(old_size, nna, G, 0.1, subset_min, slack) || rf.reads == G);
        for (int64_t M = 0; M <= G; ++M) {
            const PivotRead rp = pivot_read(keyed.data() + (G - M), M, G, subset_size, slack, nna, is_s, part);
            const bool want = ref.lowest >= G - M; // no read below position G - M
            CHECK(rp.sufficient == want);
            if (rp.sufficient) {
                CHECK(part == full);
                CHECK(rp.reads == rf.reads);
                ++n_ok;
            } else {
                ++n_short;
            }
        }
    }
    CHECK(G_max == 20000 && n_short > 0 && n_ok > 0);

    // the threshold depth at its edges
    CHECK(filter_depth(1, 0, 0.25) == 1 && filter_depth(1, 5, 0.25) == 1 && filter_depth(0, 5, 0.25) == 0);
    CHECK(filter_depth(10000, 100, 0.25) == 125 + kDepthExtra);
    CHECK(filter_depth(10000, 100, 0.0) == 100);                  // the test hook: the prediction itself
    CHECK(filter_depth(10000, 0, 0.0) == 1);
    CHECK(filter_depth(100, 90, 0.25) == 100 && filter_depth(100, 1000000, 0.25) == 100); // D >= G
    CHECK(filter_depth(10000, -3, 0.25) == kDepthExtra);
    CHECK(pivot_subset_size(0, 1, 0.1, 1) == 1 && pivot_subset_size(0, 10, 0.1, 0) == 0 && pivot_subset_size(100, 50, 0.1, 1) == 50);
    CHECK(pivot_subset_size(100, 10000, 0.1, 1) == 110);
    CHECK(predict_reads(110, 0, 0, 4, 1.25) == 110 + 10);         // no call has read yet: twice the groups asked for
    CHECK(predict_reads(110, 0, 0, 0, 1.25) == 110 + 4);
    CHECK(predict_reads(110, 130, 99, 4, 1.25) == 110 + 31);      // the last call's walk below its subset
    CHECK(predict_reads(110, 90, 99, 4, 1.25) == 110);
    {
        std::vector<double> s{0.5, 0.1, 0.9, 0.9, 0.3};
        std::vector<double> a = s, b = s, c = s, d = s, e;
        CHECK(depth_score(a, 1) == 0.9 && depth_score(b, 2) == 0.9 && depth_score(c, 3) == 0.5);
        CHECK(depth_score(d, 5) == 0.1);
        d = s;
        CHECK(depth_score(d, 99) == 0.1 && depth_score(d, 0) == 0.9); // D >= G, D < 1
        CHECK(depth_score(e, 3) == std::numeric_limits<double>::infinity());
        std::vector<double> one{0.25};
        CHECK(depth_score(one, filter_depth(1, 7, 0.25)) == 0.25);   // G = 1
    }
    // the hinted selection: the plain one's value whatever the hint, the scores untouched
    for (int it = 0; it < 2000; ++it) {
        const int64_t G = 1 + int64_t(300 * u(rng));
        std::vector<double> s(size_t(G), 0.0), scratch;
        for (double& x : s) x = u(rng) < 0.2 ? 0.5 : u(rng);
        const std::vector<double> kept = s;
        const int64_t D = int64_t(u(rng) * double(G + 3)) - 1;
        std::vector<double> plain = s;
        const double want = depth_score(plain, D);
        const double hint = it % 5 == 0 ? 0.0 : (it % 5 == 1 ? 2.0 : u(rng));
        CHECK(depth_score_hinted(s, D, hint, scratch) == want);
        CHECK(s == kept);
    }
    // an empty screen set: the rule reads its minimal subset and the walk
    {
        std::vector<Pair> k{{0.1, 0}, {0.2, 1}, {0.3, 2}, {0.4, 3}};
        std::vector<int64_t> app;
        auto none = [](int64_t) { return false; };
        const PivotRead r = pivot_read(k.data(), 4, 4, pivot_subset_size(0, 4, 0.1, 1), 1.25, 1, none, app);
        CHECK(r.sufficient && r.reads == 3 && app.size() == 3 && app[0] == 3 && app[1] == 2 && app[2] == 1);
        const PivotRead r2 = pivot_read(k.data() + 2, 2, 4, 1, 1.25, 1, none, app);
        CHECK(!r2.sufficient);
        const PivotRead r3 = pivot_read(k.data() + 1, 3, 4, 1, 1.25, 1, none, app);
        CHECK(r3.sufficient && r3.reads == 3 && app.size() == 3);
        const PivotRead r4 = pivot_read(k.data(), 4, 4, 1, 1.25, 50, none, app); // the list ends before the walk is done
        CHECK(r4.sufficient && r4.reads == 4 && app.size() == 4);
        const PivotRead r5 = pivot_read(k.data() + 1, 3, 4, 1, 1.25, 50, none, app);
        CHECK(!r5.sufficient);
        const PivotRead r6 = pivot_read(k.data() + 4, 0, 4, 0, 1.25, 1, none, app);
        CHECK(!r6.sufficient);
    }
    // the byte rule: n (8 exact + elem (p - skipped)) against rho 8 n p, for designs of at least 2^28 bytes
    const int64_t N = 100000;
    CHECK(!filter_bytes_eligible(0, N, 0, 0, 2.0) && !filter_bytes_eligible(0, 0, 10000, 0, 2.0));
    CHECK(filter_bytes_eligible(0, N, 10000, 0, 2.0) && filter_bytes_eligible(0, N, 10000, 0, 4.0));
    CHECK(filter_bytes_eligible(3499, N, 10000, 0, 2.0) && !filter_bytes_eligible(3500, N, 10000, 0, 2.0)); // 0.25 + x / p < 0.6
    CHECK(filter_bytes_eligible(999, N, 10000, 0, 4.0) && !filter_bytes_eligible(1000, N, 10000, 0, 4.0));
    CHECK(filter_bytes_eligible(4000, N, 10000, 4000, 2.0) && !filter_bytes_eligible(6000, N, 10000, 20000, 2.0));
    CHECK(filter_bytes_eligible(-5, N, 10000, 0, 2.0) && !filter_bytes_eligible(10000, N, 10000, 10000, 2.0));
    CHECK(filter_bytes_eligible(7000, N, 10000, 0, 2.0, 1.0) && !filter_bytes_eligible(0, N, 10000, 0, 2.0, 0.25));
    CHECK(filter_bytes_eligible(200, 9000, 200, 0, 4.0));                                   // 14 MB: not held to the rule
    CHECK(!filter_bytes_eligible(4096, 8192, 4096, 0, 4.0) && filter_bytes_eligible(4096, 8191, 4096, 0, 4.0)); // 2^28 bytes
    // the list capacity of the rule: never below the parent's
    CHECK(filter_depth_list_cap(10000) == 5000 && filter_depth_list_cap(37) == 1024 && filter_depth_list_cap(0) == 1024);
    for (int64_t p = 0; p < 100000; p += 997) CHECK(filter_depth_list_cap(p) >= filter_list_cap(p));
    if (fails) std::printf("screen_reads: %d check(s) FAILED\n", fails);
    else std::printf("screen_reads: ok (%lld sufficient, %lld short)\n", (long long)n_ok, (long long)n_short);
    return fails ? 1 : 0;
}
