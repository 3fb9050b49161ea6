// Stand-alone self-test of pnp_math.h on the host, meant to be built with -fsanitize=address,undefined (make pnp-selftest) and run on the CPU.
// It is never loaded into Python.  The cases follow tests/test_pnp_twin_host.py: nine points in +-60 mm with the first at the origin, a rotation
// of 0.2..2.8 rad, t = (+-150, +-100, 600..1200) mm, the LINEMOD intrinsics; noise-free poses against the ground truth, noisy and outlier
// cases for a finite pose that LM did not make worse and the expected consensus, and the three bounded failures (equal 2-D points, collinear
// 3-D points, a NaN keypoint), which must return the zero pose with a status.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

struct Case {
    float xy[18], xyz[27];
    double R[9], t[3];
};

static Case make_case(double sigma, int outliers) {
    Case c;
    for (int i = 0; i < 27; ++i) c.xyz[i] = i < 3 ? 0.f : (float)uniform(-60.0, 60.0);
    double axis[3] = {normal(), normal(), normal()};
    const double len = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]), angle = uniform(0.2, 2.8);
    for (double& a : axis) a *= angle / len;
    rodrigues(axis, c.R);
    c.t[0] = uniform(-150, 150); c.t[1] = uniform(-100, 100); c.t[2] = uniform(600, 1200);
    for (int i = 0; i < 9; ++i) {
        double cam[3];
        for (int d = 0; d < 3; ++d) cam[d] = c.R[3 * d] * c.xyz[3 * i] + c.R[3 * d + 1] * c.xyz[3 * i + 1] + c.R[3 * d + 2] * c.xyz[3 * i + 2] + c.t[d];
        double u = K[0] * cam[0] / cam[2] + K[2] + sigma * normal(), v = K[4] * cam[1] / cam[2] + K[5] + sigma * normal();
        if (i >= 9 - outliers) {
            const double a = uniform(0.0, 6.283185307179586), r = uniform(40.0, 80.0);
            u += r * std::cos(a);
            v += r * std::sin(a);
        }
        c.xy[2 * i] = (float)u;
        c.xy[2 * i + 1] = (float)v;
    }
    return c;
}

int main() {
    std::vector<uint8_t> table;
    for (int a = 0; a < 9; ++a)
        for (int b = a + 1; b < 9; ++b)
            for (int c = b + 1; c < 9; ++c)
                for (int d = c + 1; d < 9; ++d)
                    for (int e = d + 1; e < 9; ++e) {
                        const uint8_t row[5] = {(uint8_t)a, (uint8_t)b, (uint8_t)c, (uint8_t)d, (uint8_t)e};
                        table.insert(table.end(), row, row + 5);
                    }
    const int H = (int)table.size() / 5;
    EXPECT(H == 126, "%d hypotheses for 9 points", H);
    float pose[12], cost[2];
    int32_t info[4];
    // 1. noise-free: the ground truth, up to the fp32 rounding of the keypoints (3e-5 px: < 1e-3 mm in depth at 1200 mm) and of the output
    for (int k = 0; k < 8; ++k) {
        const Case c = make_case(0.0, 0);
        solve_pair_serial(c.xy, c.xyz, K, nullptr, 9, table.data(), H, 12.0, pose, info, cost);
        double dR = 0.0, dt = 0.0;
        for (int r = 0; r < 3; ++r) {
            for (int j = 0; j < 3; ++j) dR = std::fmax(dR, std::fabs(pose[4 * r + j] - c.R[3 * r + j]));
            dt = std::fmax(dt, std::fabs(pose[4 * r + 3] - c.t[r]));
        }
        EXPECT(info[0] == OK && info[2] == 9 && dR <= 4e-6 && dt <= 2e-3, "noise-free case %d: status %d, %d inliers, |dR| %.3g, |dt| %.3g", k, info[0],
               info[2], dR, dt);
    }
    // 2. noise and outliers: a finite proper rotation in front of the camera, the planted outliers at most lost, LM never worse than its start
    for (int k = 0; k < 18; ++k) {
        const int outliers = k % 3;
        const Case c = make_case(k % 2 ? 0.5 : 0.0, outliers);
        solve_pair_serial(c.xy, c.xyz, K, nullptr, 9, table.data(), H, 12.0, pose, info, cost);
        const double det = pose[0] * (pose[5] * pose[10] - pose[6] * pose[9]) - pose[1] * (pose[4] * pose[10] - pose[6] * pose[8]) +
                           pose[2] * (pose[4] * pose[9] - pose[5] * pose[8]);
        EXPECT(info[0] == OK && info[2] >= 9 - outliers && info[1] >= 0 && info[1] < H && info[3] >= 1 && info[3] <= LM_ITERS && cost[1] <= cost[0] &&
                   std::fabs(det - 1.0) < 1e-5 && pose[11] > 0.f,
               "case %d with %d outliers: status %d, winner %d, %d inliers, %d LM iterations, cost %g -> %g, det %g, t_z %g", k, outliers, info[0],
               info[1], info[2], info[3], (double)cost[0], (double)cost[1], det, (double)pose[11]);
    }
    // 5. bounded failures: the zero pose and a status, and the call returns
    for (int kind = 0; kind < 3; ++kind) {
        Case c = make_case(0.5, 0);
        if (kind == 0)
            for (int i = 0; i < 9; ++i) { c.xy[2 * i] = 311.5f; c.xy[2 * i + 1] = 207.25f; }
        else if (kind == 1)
            for (int i = 0; i < 9; ++i) {
                const float s = -60.f + 15.f * i;
                c.xyz[3 * i] = 0.6f * s; c.xyz[3 * i + 1] = -0.3f * s; c.xyz[3 * i + 2] = 0.74f * s;
            }
        else
            c.xy[8] = NAN;
        solve_pair_serial(c.xy, c.xyz, K, nullptr, 9, table.data(), H, 12.0, pose, info, cost);
        bool zero = true;
        for (float v : pose) zero = zero && v == 0.f;
        EXPECT(zero && info[0] == (kind == 2 ? NONFINITE_INPUT : DEGENERATE), "failure kind %d: status %d, zero pose %d", kind, info[0], (int)zero);
    }
    // a crop->image affine is applied to the keypoints: shifting the crop and undoing it in the affine gives the same pose, up to the
    // fp32 rounding of the shifted keypoints
    {
        Case c = make_case(0.5, 1);
        float ref[12];
        solve_pair_serial(c.xy, c.xyz, K, nullptr, 9, table.data(), H, 12.0, ref, info, cost);
        for (int i = 0; i < 9; ++i) { c.xy[2 * i] -= 64.f; c.xy[2 * i + 1] -= 32.f; }
        const double affine[6] = {1.0, 0.0, 64.0, 0.0, 1.0, 32.0};
        solve_pair_serial(c.xy, c.xyz, K, affine, 9, table.data(), H, 12.0, pose, info, cost);
        double d = 0.0;
        for (int i = 0; i < 12; ++i) d = std::fmax(d, std::fabs(pose[i] - ref[i]) / std::fmax(1.0, std::fabs(ref[i])));
        EXPECT(info[0] == OK && d <= 1e-5, "affine: status %d, relative pose difference %.3g", info[0], d);
    }
    SELFTEST_END("pnp_selftest", "8 noise-free, 18 noisy / outlier, 3 bounded-failure cases, 1 affine case; %d hypotheses each", H);
}
