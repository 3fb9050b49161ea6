// Stand-alone self-test of the uncertainty-weighted PnP of pnp_math.h on the host, meant to be built with -fsanitize=address,undefined
// (make wpnp-selftest) and run on the CPU.  It is never loaded into Python.  It runs the body of cp_pnp_weighted_host_f64
// (solve_batch_weighted_serial) into heap buffers of exactly the output sizes, so that a write past poses [pairs][12], info [pairs][4],
// cost [pairs][2] or weighted [pairs] is an AddressSanitizer report: n = 5 and n = 16, a singular covariance with floor 0 and a NaN covariance
// (both fall back to the unweighted solve, bit for bit, with weighted = 0), a zero covariance rescued by the floor, an affine with rotation
// and scale, and a skipped pair.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnp_math.h"
#include "selftest.h"

using namespace cp_pnp;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}
static double uniform(double a, double b) { return a + (b - a) * uniform(); }
static double normal() { return std::sqrt(-2.0 * std::log(1.0 - uniform())) * std::cos(6.283185307179586 * uniform()); }

static const float K[9] = {572.4114f, 0.f, 325.2611f, 0.f, 573.57043f, 242.04899f, 0.f, 0.f, 1.f};

struct Batch {   // every array has exactly the size the entry point documents
    int pairs, n;
    std::vector<float> xy, xyz, cov, poses, cost;
    std::vector<int32_t> solve, info, weighted;
    std::vector<double> R, t;
    Batch(int pairs_, int n_)
        : pairs(pairs_), n(n_), xy((size_t)pairs_ * n_ * 2), xyz((size_t)pairs_ * n_ * 3), cov((size_t)pairs_ * n_ * 3), poses((size_t)pairs_ * 12, 7.f),
          cost((size_t)pairs_ * 2, 7.f), solve(pairs_, 1), info((size_t)pairs_ * 4, 7), weighted(pairs_, 7), R((size_t)pairs_ * 9), t((size_t)pairs_ * 3) {}
};

// pair `pr`: n points in +-60 mm, a random pose, per point a covariance with axes (s_major, s_minor) px at a random angle and noise drawn from it
static void fill_pair(Batch& B, int pr, double s_major, double s_minor) {
    const int n = B.n;
    float* xyz = &B.xyz[(size_t)pr * n * 3];
    for (int i = 0; i < 3 * n; ++i) xyz[i] = i < 3 ? 0.f : (float)uniform(-60.0, 60.0);
    double axis[3] = {normal(), normal(), normal()};
    const double len = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]), angle = uniform(0.2, 2.8);
    for (double& a : axis) a *= angle / len;
    double* R = &B.R[(size_t)pr * 9];
    double* t = &B.t[(size_t)pr * 3];
    rodrigues(axis, R);
    t[0] = uniform(-150, 150); t[1] = uniform(-100, 100); t[2] = uniform(600, 1200);
    for (int i = 0; i < n; ++i) {
        double cam[3];
        for (int d = 0; d < 3; ++d) cam[d] = R[3 * d] * xyz[3 * i] + R[3 * d + 1] * xyz[3 * i + 1] + R[3 * d + 2] * xyz[3 * i + 2] + t[d];
        const double th = uniform(0.0, 3.141592653589793), c = std::cos(th), s = std::sin(th);
        const double a = (i % 3 == 0 ? s_major : s_minor) * normal(), b = s_minor * normal();
        const double va = (i % 3 == 0 ? s_major * s_major : s_minor * s_minor), vb = s_minor * s_minor;
        B.xy[((size_t)pr * n + i) * 2] = (float)(K[0] * cam[0] / cam[2] + K[2] + c * a - s * b);
        B.xy[((size_t)pr * n + i) * 2 + 1] = (float)(K[4] * cam[1] / cam[2] + K[5] + s * a + c * b);
        float* q = &B.cov[((size_t)pr * n + i) * 3];
        q[0] = (float)(c * c * va + s * s * vb);
        q[1] = (float)(c * s * (va - vb));
        q[2] = (float)(s * s * va + c * c * vb);
    }
}

static std::vector<uint8_t> table_for(int n, int& H) {
    std::vector<uint8_t> table;
    for (int a = 0; a < n && (int)table.size() < 5 * MAX_HYPOTHESES; ++a)
        for (int b = a + 1; b < n; ++b)
            for (int c = b + 1; c < n; ++c)
                for (int d = c + 1; d < n; ++d)
                    for (int e = d + 1; e < n && (int)table.size() < 5 * MAX_HYPOTHESES; ++e) {
                        const uint8_t row[5] = {(uint8_t)a, (uint8_t)b, (uint8_t)c, (uint8_t)d, (uint8_t)e};
                        table.insert(table.end(), row, row + 5);
                    }
    H = (int)table.size() / 5;
    return table;
}

static void run(Batch& B, const std::vector<uint8_t>& table, int H, const double* affine, double floor_) {
    solve_batch_weighted_serial(B.xy.data(), B.xyz.data(), K, 0, affine, B.solve.data(), table.data(), 1, B.pairs, B.n, H, 12.0, B.cov.data(), floor_,
                                B.poses.data(), B.info.data(), B.cost.data(), B.weighted.data());
}

static bool proper(const float* pose) {
    const double det = pose[0] * (pose[5] * pose[10] - pose[6] * pose[9]) - pose[1] * (pose[4] * pose[10] - pose[6] * pose[8]) +
                       pose[2] * (pose[4] * pose[9] - pose[5] * pose[8]);
    return std::fabs(det - 1.0) < 1e-5 && pose[11] > 0.f;
}

int main() {
    int cases = 0;
    for (int n : {5, 9, 16}) {
        int H;
        const std::vector<uint8_t> table = table_for(n, H);
        EXPECT(H >= 1 && H <= MAX_HYPOTHESES, "%d hypotheses for %d points", H, n);
        // pairs: 0 usable, 1 skipped, 2 singular covariance (floor 0), 3 NaN covariance, 4 usable
        Batch B(5, n);
        for (int pr = 0; pr < 5; ++pr) fill_pair(B, pr, 4.0, 0.3);
        B.solve[1] = 0;
        {   // rank one: (1, 2, 4) = v v^T for v = (1, 2)
            float* q = &B.cov[((size_t)2 * n + 1) * 3];
            q[0] = 1.f; q[1] = 2.f; q[2] = 4.f;
        }
        B.cov[((size_t)3 * n + 2) * 3 + 1] = NAN;
        run(B, table, H, nullptr, 0.0);
        const int want_w[5] = {1, 0, 0, 0, 1};
        for (int pr = 0; pr < 5; ++pr) {
            EXPECT(B.weighted[pr] == want_w[pr], "n %d pair %d: weighted %d", n, pr, B.weighted[pr]);
            if (pr == 1) {
                bool zero = true;
                for (int i = 0; i < 12; ++i) zero = zero && B.poses[12 * pr + i] == 0.f;
                EXPECT(zero && B.info[4 * pr] == SKIPPED && B.info[4 * pr + 1] == -1, "n %d: the skipped pair has status %d", n, B.info[4 * pr]);
                continue;
            }
            EXPECT(B.info[4 * pr] == OK && proper(&B.poses[12 * pr]) && B.cost[2 * pr + 1] <= B.cost[2 * pr] && B.info[4 * pr + 3] >= 1 &&
                       B.info[4 * pr + 3] <= LM_ITERS,
                   "n %d pair %d: status %d, cost %g -> %g, %d LM iterations", n, pr, B.info[4 * pr], (double)B.cost[2 * pr], (double)B.cost[2 * pr + 1],
                   B.info[4 * pr + 3]);
            // the unweighted solve of the same pair: the fall-backs equal it bit for bit, the weighted pairs do not (anisotropic covariances)
            float pose[12], cost[2];
            int32_t info[4];
            solve_pair_serial(&B.xy[(size_t)pr * n * 2], &B.xyz[(size_t)pr * n * 3], K, nullptr, n, table.data(), H, 12.0, pose, info, cost);
            const bool same = std::memcmp(pose, &B.poses[12 * pr], sizeof pose) == 0 && std::memcmp(cost, &B.cost[2 * pr], sizeof cost) == 0 &&
                              std::memcmp(info, &B.info[4 * pr], sizeof info) == 0;
            EXPECT(same == (want_w[pr] == 0), "n %d pair %d: equal to the unweighted solve %d, weighted %d", n, pr, (int)same, want_w[pr]);
            ++cases;
        }
        // a zero covariance: unusable with floor 0, rescued by the floor -- and then, being isotropic, the unweighted optimum
        Batch Z(1, n);
        fill_pair(Z, 0, 0.3, 0.3);
        std::fill(Z.cov.begin(), Z.cov.end(), 0.f);
        run(Z, table, H, nullptr, 0.0);
        EXPECT(Z.weighted[0] == 0 && Z.info[0] == OK, "n %d zero covariance, floor 0: weighted %d status %d", n, Z.weighted[0], Z.info[0]);
        const std::vector<float> plain = Z.poses;
        run(Z, table, H, nullptr, 1.0 / 12.0);
        double d = 0.0;
        for (int i = 0; i < 12; ++i) d = std::fmax(d, std::fabs(Z.poses[i] - plain[i]) / std::fmax(1.0, std::fabs(plain[i])));
        EXPECT(Z.weighted[0] == 1 && Z.info[0] == OK && d <= 1e-5, "n %d zero covariance with the floor: weighted %d status %d, pose differs by %.3g", n,
               Z.weighted[0], Z.info[0], d);
        // an affine with rotation and scale: crop pixels p = M^-1 (x - c) with covariance M^-1 Sigma M^-T give the image-pixel pose
        Batch A(1, n), C(1, n);
        fill_pair(A, 0, 4.0, 0.3);
        C = A;
        const double ang = 0.3, sc = 1.25, affine[6] = {std::cos(ang) / sc, std::sin(ang) / sc, 31.0, -std::sin(ang) / sc, std::cos(ang) / sc, -17.0};
        const double Mi[4] = {std::cos(ang) * sc, -std::sin(ang) * sc, std::sin(ang) * sc, std::cos(ang) * sc};   // M^-1
        for (int i = 0; i < n; ++i) {
            const double x = A.xy[2 * i] - affine[2], y = A.xy[2 * i + 1] - affine[5];
            C.xy[2 * i] = (float)(Mi[0] * x + Mi[1] * y);
            C.xy[2 * i + 1] = (float)(Mi[2] * x + Mi[3] * y);
            const double s00 = A.cov[3 * i], s01 = A.cov[3 * i + 1], s11 = A.cov[3 * i + 2];
            const double t00 = Mi[0] * s00 + Mi[1] * s01, t01 = Mi[0] * s01 + Mi[1] * s11, t10 = Mi[2] * s00 + Mi[3] * s01, t11 = Mi[2] * s01 + Mi[3] * s11;
            C.cov[3 * i] = (float)(t00 * Mi[0] + t01 * Mi[1]);
            C.cov[3 * i + 1] = (float)(t00 * Mi[2] + t01 * Mi[3]);
            C.cov[3 * i + 2] = (float)(t10 * Mi[2] + t11 * Mi[3]);
        }
        run(A, table, H, nullptr, 0.0);
        run(C, table, H, affine, 0.0);
        d = 0.0;
        for (int i = 0; i < 12; ++i) d = std::fmax(d, std::fabs(C.poses[i] - A.poses[i]) / std::fmax(1.0, std::fabs(A.poses[i])));
        EXPECT(A.weighted[0] == 1 && C.weighted[0] == 1 && C.info[0] == OK && d <= 1e-4, "n %d affine: weighted %d / %d, status %d, relative pose difference %.3g",
               n, A.weighted[0], C.weighted[0], C.info[0], d);
        cases += 3;
    }
    SELFTEST_END("wpnp_selftest", "%d solves for n = 5, 9, 16: weighted, skipped, singular, NaN, floor-rescued and affine pairs", cases);
}
