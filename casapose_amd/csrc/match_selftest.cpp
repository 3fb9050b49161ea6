// Stand-alone self-test of match_math.h on the host, meant to be built with -fsanitize=address,undefined (make match-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs the assignment rule of the instance evaluator -- what lane 0 of match_assign_kernel
// (pose_match.hip) carries out per (image, object) -- over hand-made cost matrices and against a plain restatement (sort all pairs by cost, g,
// e; take every pair whose two sides are free) on random ones.  The cost matrices and the two outputs live in vectors of exactly the sizes the
// rule is given, so that an index past them is an AddressSanitizer report.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <tuple>
#include <vector>

#include "match_math.h"
#include "selftest.h"

namespace {

constexpr double INF = std::numeric_limits<double>::infinity();
constexpr double NaN = std::numeric_limits<double>::quiet_NaN();

struct Result {
    std::vector<int> est, gt;
    int matched;
};

Result run(const std::vector<double>& cost, int estimates, int instances, int stride, unsigned live) {
    Result r{std::vector<int>((size_t)estimates, 77), std::vector<int>((size_t)instances, 77), 0};
    r.matched = cp_match::greedy_match(cost.data(), estimates, instances, stride, live, r.est.data(), r.gt.data());
    return r;
}

// the restatement: every finite pair, ordered by (cost, g, e); a pair is taken when both of its sides are still free
Result restated(const std::vector<double>& cost, int estimates, int instances, int stride, unsigned live) {
    Result r{std::vector<int>((size_t)estimates), std::vector<int>((size_t)instances, -1), 0};
    std::vector<std::tuple<double, int, int>> pairs;
    for (int e = 0; e < estimates; ++e) {
        r.est[(size_t)e] = (live >> e) & 1u ? -1 : -2;
        for (int g = 0; g < instances; ++g)
            if (((live >> e) & 1u) && std::isfinite(cost[(size_t)(e * stride + g)])) pairs.emplace_back(cost[(size_t)(e * stride + g)], g, e);
    }
    std::sort(pairs.begin(), pairs.end());
    for (const auto& [c, g, e] : pairs) {
        (void)c;
        if (r.est[(size_t)e] != -1 || r.gt[(size_t)g] != -1) continue;
        r.est[(size_t)e] = g, r.gt[(size_t)g] = e, ++r.matched;
    }
    return r;
}

bool same(const Result& a, const Result& b) { return a.est == b.est && a.gt == b.gt && a.matched == b.matched; }

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

}  // namespace

int main() {
    int cases = 0;
    {   // plain 2 x 2: the diagonal is cheaper
        const Result r = run({1.0, 5.0, 6.0, 2.0}, 2, 2, 2, 3u);
        EXPECT(r.est == std::vector<int>({0, 1}) && r.gt == std::vector<int>({0, 1}) && r.matched == 2, "2 x 2 diagonal");
        ++cases;
    }
    {   // greedy is not optimal: (e0, g0) = 1 is taken first and leaves (e1, g1) = 100; the optimum is (e0, g1), (e1, g0) at 2 + 2
        const Result r = run({1.0, 2.0, 2.0, 100.0}, 2, 2, 2, 3u);
        EXPECT(r.est == std::vector<int>({0, 1}) && r.gt == std::vector<int>({0, 1}), "greedy takes the smallest cost first");
        ++cases;
    }
    {   // ties: all costs equal -> g 0 goes to e 0, g 1 to e 1 (smaller g first, then smaller e)
        const Result r = run({3.0, 3.0, 3.0, 3.0, 3.0, 3.0}, 3, 2, 2, 7u);
        EXPECT(r.est == std::vector<int>({0, 1, -1}) && r.gt == std::vector<int>({0, 1}) && r.matched == 2, "ties go to g, then e");
        ++cases;
    }
    {   // a tie between (e1, g0) and (e0, g1): the smaller g wins, so g 0 takes e 1
        const Result r = run({9.0, 1.0, 1.0, 9.0}, 2, 2, 2, 3u);
        EXPECT(r.est == std::vector<int>({1, 0}) && r.gt == std::vector<int>({1, 0}), "tie across pairs: smaller g first");
        ++cases;
    }
    {   // two identical estimates, one instance: slot 0 matches, slot 1 is the false positive
        const Result r = run({4.0, 4.0}, 2, 1, 1, 3u);
        EXPECT(r.est == std::vector<int>({0, -1}) && r.gt == std::vector<int>({0}) && r.matched == 1, "duplicate estimates");
        ++cases;
    }
    {   // empty slots: e 0 is empty whatever its cost says
        const Result r = run({0.0, 0.0, 5.0, 7.0, 6.0, 1.0}, 3, 2, 2, 6u);
        EXPECT(r.est == std::vector<int>({-2, 0, 1}) && r.gt == std::vector<int>({1, 2}) && r.matched == 2, "an empty slot is never matched");
        ++cases;
    }
    {   // no ground truth: the row stride still is the full width
        const Result r = run({1.0, 2.0, 3.0, 4.0}, 2, 0, 2, 3u);
        EXPECT(r.est == std::vector<int>({-1, -1}) && r.gt.empty() && r.matched == 0, "count = 0");
        ++cases;
    }
    {   // ground truth and no estimate
        const Result r = run({1.0, 2.0}, 1, 2, 2, 0u);
        EXPECT(r.est == std::vector<int>({-2}) && r.gt == std::vector<int>({-1, -1}) && r.matched == 0, "no estimate");
        ++cases;
    }
    {   // non-finite costs are never matched, and do not end the search early
        const Result r = run({NaN, INF, NaN, 2.0, INF, NaN}, 3, 2, 2, 7u);
        EXPECT(r.est == std::vector<int>({-1, 1, -1}) && r.gt == std::vector<int>({-1, 1}) && r.matched == 1, "non-finite costs");
        ++cases;
    }
    {   // count smaller than the stride: column 1 is not an instance
        const Result r = run({5.0, 0.0, 4.0, 0.0}, 2, 1, 2, 3u);
        EXPECT(r.est == std::vector<int>({-1, 0}) && r.gt == std::vector<int>({1}), "columns beyond the count are not read as instances");
        ++cases;
    }
    // random matrices of every shape up to 16 x 16, with ties (costs drawn from a few integers), holes and empty slots, against the restatement
    uint32_t seed = 12345u;
    for (int estimates = 1; estimates <= cp_match::MAX_SIDE; ++estimates)
        for (int instances = 0; instances <= cp_match::MAX_SIDE; ++instances)
            for (int rep = 0; rep < 4; ++rep) {
                const int stride = instances + (int)(lcg(seed) >> 30);   // the rule may see fewer instances than the matrix is wide
                std::vector<double> cost((size_t)(estimates * std::max(stride, 1)));
                for (double& c : cost) {
                    const uint32_t v = lcg(seed) >> 24;
                    c = v < 16 ? (v < 8 ? INF : NaN) : (double)(v % 12);
                }
                const unsigned live = (lcg(seed) >> 8) & ((1u << estimates) - 1u);
                const Result a = run(cost, estimates, instances, std::max(stride, 1), live), b = restated(cost, estimates, instances, std::max(stride, 1), live);
                EXPECT(same(a, b), "random %d x %d (rep %d) differs from the restatement", estimates, instances, rep);
                ++cases;
            }
    {   // float costs go through the same template
        const std::vector<float> cost = {1.f, 2.f, 2.f, 100.f};
        std::vector<int> est(2), gt(2);
        const int m = cp_match::greedy_match(cost.data(), 2, 2, 2, 3u, est.data(), gt.data());
        EXPECT(m == 2 && est == std::vector<int>({0, 1}), "float costs");
        ++cases;
    }
    SELFTEST_END("match_selftest", "%d cases", cases);
}
