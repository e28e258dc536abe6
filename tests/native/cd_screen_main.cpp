// Stand-alone check of the host-only decisions of the screen-set coordinate descents (adelie_amd/csrc/cd_screen_host.hpp):
// the admission of a KKT round and the validation of a warm start.  Built with -fsanitize=address,undefined by
// tests/test_cd_screen_host.py.  Every expected value is written out by hand.  Exits non-zero on the first disagreements.
#include "../../adelie_amd/csrc/cd_screen_host.hpp"
#include <cstdio>
#include <cstring>
#include <limits>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

using Idx = std::vector<int64_t>;

// one admission in the dtype T; `members` as 0 / 1 flags
template <class T>
static bool admit(std::vector<T> viols, std::vector<uint8_t> members, int64_t kappa, Idx& added) {
    added = Idx{99, 98}; // (left-overs of an earlier round must not survive)
    return cd_screen_admit<T>(viols.data(), int64_t(viols.size()), members.data(), kappa, added);
}

template <class T>
static void admission() {
    const T inf = std::numeric_limits<T>::infinity();
    Idx added;
    // ties go to the lower index
    CHECK(!admit<T>({1, 3, 3, 2}, {0, 0, 0, 0}, 2, added) && added == (Idx{1, 2}));
    CHECK(!admit<T>({1, 3, 3, 2}, {0, 0, 0, 0}, 4, added) && added == (Idx{1, 2, 3, 0}));
    CHECK(!admit<T>({7, 7, 7, 7, 7}, {0, 1, 0, 0, 0}, 3, added) && added == (Idx{0, 2, 3}));
    // -inf (an infinite penalty) sorts last and is no violator; +inf sorts first
    CHECK(!admit<T>({-inf, inf, T(0.5), -inf, inf}, {0, 0, 0, 0, 1}, 5, added) && added == (Idx{1, 2}));
    CHECK(!admit<T>({-inf, inf, T(0.5), -inf, inf}, {0, 0, 0, 0, 0}, 5, added) && added == (Idx{1, 4, 2}));
    CHECK(admit<T>({-inf, -inf}, {0, 0}, 1, added) && added.empty());
    // kappa = 1, kappa = the number of violators, kappa above it
    CHECK(!admit<T>({T(0.1), T(0.9), T(0.5)}, {0, 0, 0}, 1, added) && added == (Idx{1}));
    CHECK(!admit<T>({T(0.1), -1, T(0.5)}, {0, 0, 0}, 2, added) && added == (Idx{2, 0}));
    CHECK(!admit<T>({T(0.1), -1, T(0.5)}, {0, 0, 0}, 10, added) && added == (Idx{2, 0}));
    // every violator already a member: the round passes and admits nothing
    CHECK(admit<T>({2, -1, 3}, {1, 0, 1}, 4, added) && added.empty());
    CHECK(admit<T>({2, 0, 3}, {1, 0, 1}, 4, added) && added.empty()); // (a violation of exactly 0 is none)
    CHECK(admit<T>({T(-0.0), 0}, {0, 0}, 4, added) && added.empty());
    // one violator left when kappa is exhausted: not admitted, and the round does not pass
    CHECK(!admit<T>({5, 4, 3}, {0, 0, 0}, 2, added) && added == (Idx{0, 1}));
    CHECK(!admit<T>({3, 9, 4, 5}, {0, 1, 0, 0}, 2, added) && added == (Idx{3, 2}));
    // p = 1
    CHECK(!admit<T>({1}, {0}, 1, added) && added == (Idx{0}));
    CHECK(admit<T>({1}, {1}, 1, added) && added.empty());
    CHECK(admit<T>({0}, {0}, 1, added) && added.empty());
    CHECK(admit<T>({-2}, {0}, 3, added) && added.empty());
}

static const char* const kScreen = "screen";
static const char* const kActive = "active";
static const char* validate(Idx screen, Idx active, int64_t p) {
    return cd_screen_warm_start_error(screen.data(), int64_t(screen.size()), active.data(), int64_t(active.size()), p, kScreen, kActive);
}

int main() {
    admission<double>();
    admission<float>();

    CHECK(validate({}, {}, 3) == nullptr);
    CHECK(validate({2, 0, 1}, {1, 2}, 3) == nullptr);
    CHECK(validate({2, 0}, {0, 2}, 3) == nullptr);
    CHECK(validate({0}, {0}, 1) == nullptr);
    CHECK(validate({1, 2, 1}, {}, 3) == kScreen);    // a duplicate
    CHECK(validate({0, 3}, {}, 3) == kScreen);       // out of range
    CHECK(validate({-1}, {}, 3) == kScreen);
    CHECK(validate({1}, {}, 1) == kScreen);
    CHECK(validate({2, 0}, {1}, 3) == kActive);      // an active index that is no member
    CHECK(validate({}, {0}, 3) == kActive);
    CHECK(validate({2, 0}, {0, 0}, 3) == kActive);   // an active duplicate
    CHECK(validate({2, 0}, {3}, 3) == kActive);      // an active index out of range
    CHECK(validate({2, 0}, {-1}, 3) == kActive);
    CHECK(validate({1, 1}, {5}, 3) == kScreen);      // (the screen set is judged first)

    if (fails) std::printf("cd_screen: %d check(s) FAILED\n", fails);
    else std::printf("cd_screen: ok\n");
    return fails ? 1 : 0;
}
