// Stand-alone self-test of bpnp_math.h on the host, meant to be built with -fsanitize=address,undefined (make bpnp-selftest) and run on the CPU.
// It is never loaded into Python.  The cases follow pnp_selftest.cpp (points in +-60 mm, a rotation of 0.2..2.8 rad, t = (+-150, +-100, 600..1200)
// mm, the LINEMOD intrinsics) with 0.5 px noise on every keypoint -- a noise-free optimum has |r - p'| ~ 1e-6 px and no meaningful unit vector --
// and ground-truth projections 2 px away.  Checked: a finite loss, gradient and proper pose for kp = 5, 9 and 16, with planted outliers, an
// unavailable pair, a collapsed vote, a NaN keypoint and a crop affine; the batch rules (na, counts, zeros for pairs that are not solved); and
// the gradient against central differences of the loss with the PnP re-solved.  The batch loop below is cp_bpnp_loss_host_f64's, restated here
// because that entry point lives in a HIP translation unit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bpnp_math.h"
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
static const float IDENTITY[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};

struct Pair {
    int n;
    float yx[2 * MAX_POINTS], gt[2 * MAX_POINTS], xyz[3 * MAX_POINTS];
};

// keypoints (y, x) in crop pixels such that `affine` maps them to the noisy projections
static Pair make_pair(int n, int outliers, const float* affine) {
    Pair c;
    c.n = n;
    for (int i = 0; i < 3 * n; ++i) c.xyz[i] = i < 3 ? 0.f : (float)uniform(-60.0, 60.0);
    double axis[3] = {normal(), normal(), normal()}, R[9];
    const double len = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]), angle = uniform(0.2, 2.8);
    for (double& a : axis) a *= angle / len;
    rodrigues(axis, R);
    const double t[3] = {uniform(-150, 150), uniform(-100, 100), uniform(600, 1200)};
    const double det = (double)affine[0] * affine[4] - (double)affine[1] * affine[3];
    for (int i = 0; i < n; ++i) {
        double cam[3];
        for (int d = 0; d < 3; ++d) cam[d] = R[3 * d] * c.xyz[3 * i] + R[3 * d + 1] * c.xyz[3 * i + 1] + R[3 * d + 2] * c.xyz[3 * i + 2] + t[d];
        double u = K[0] * cam[0] / cam[2] + K[2] + 0.5 * normal(), v = K[4] * cam[1] / cam[2] + K[5] + 0.5 * normal();
        c.gt[2 * i] = (float)(u + 2.0 * normal());
        c.gt[2 * i + 1] = (float)(v + 2.0 * normal());
        if (i >= n - outliers) {
            const double a = uniform(0.0, 6.283185307179586), r = uniform(40.0, 80.0);
            u += r * std::cos(a);
            v += r * std::sin(a);
        }
        const double du = u - affine[2], dv = v - affine[5];
        c.yx[2 * i + 1] = (float)((affine[4] * du - affine[1] * dv) / det);   // x
        c.yx[2 * i] = (float)((affine[0] * dv - affine[3] * du) / det);       // y
    }
    return c;
}

struct Result {
    double loss;
    int solved, unsolved;
    std::vector<float> g, poses;
    std::vector<int32_t> info;
};

static Result run(const std::vector<Pair>& pairs, const std::vector<float>& avail, const float* affine, const std::vector<uint8_t>& table, double weight) {
    const int n = pairs[0].n, np = (int)pairs.size(), H = (int)table.size() / SET_POINTS;
    std::vector<double> gd((size_t)np * 2 * n), pl(np);
    Result r;
    r.g.resize((size_t)np * 2 * n);
    r.poses.resize((size_t)np * 12);
    r.info.resize((size_t)np * 4);
    for (int p = 0; p < np; ++p) {
        if (avail[p] == 0.f) {
            zero_pair(SKIPPED, n, &gd[(size_t)p * 2 * n], &pl[p], &r.poses[(size_t)p * 12], &r.info[(size_t)p * 4]);
            continue;
        }
        bpnp_pair_serial(pairs[p].yx, pairs[p].gt, affine, pairs[p].xyz, K, n, table.data(), H, 12.0, 12.5, &gd[(size_t)p * 2 * n], &pl[p],
                         &r.poses[(size_t)p * 12], &r.info[(size_t)p * 4]);
    }
    r.solved = r.unsolved = 0;
    double total = 0.0;
    for (int p = 0; p < np; ++p) {
        const bool ok = avail[p] != 0.f && r.info[4 * p] == OK;
        if (ok) total += pl[p];
        r.solved += ok ? 1 : 0;
        r.unsolved += (avail[p] != 0.f && !ok) ? 1 : 0;
    }
    r.loss = r.solved > 0 ? total / r.solved : 0.0;
    for (size_t i = 0; i < gd.size(); ++i) {
        const size_t p = i / (2 * n);
        r.g[i] = finished_gradient(gd[i], avail[p] != 0.f && r.info[4 * p] == OK, weight, r.solved);
    }
    return r;
}

// every 5-subset of n points in lexicographic order, at most 256 of them (the first 256 where device_pnp.hypothesis_table samples)
static std::vector<uint8_t> make_table(int n) {
    std::vector<uint8_t> table;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            for (int c = b + 1; c < n; ++c)
                for (int d = c + 1; d < n; ++d)
                    for (int e = d + 1; e < n; ++e) {
                        if ((int)table.size() / SET_POINTS >= MAX_HYPOTHESES) return table;
                        const uint8_t row[5] = {(uint8_t)a, (uint8_t)b, (uint8_t)c, (uint8_t)d, (uint8_t)e};
                        table.insert(table.end(), row, row + 5);
                    }
    return table;
}

static bool all_zero(const float* v, int count) {
    for (int i = 0; i < count; ++i)
        if (v[i] != 0.f) return false;
    return true;
}

static bool good_pair(const Result& r, int p, int n) {
    const float* pose = &r.poses[(size_t)p * 12];
    const double det = pose[0] * (pose[5] * pose[10] - pose[6] * pose[9]) - pose[1] * (pose[4] * pose[10] - pose[6] * pose[8]) +
                       pose[2] * (pose[4] * pose[9] - pose[5] * pose[8]);
    bool fin = true, any = false;
    for (int i = 0; i < 2 * n; ++i) {
        fin = fin && std::isfinite(r.g[(size_t)p * 2 * n + i]);
        any = any || r.g[(size_t)p * 2 * n + i] != 0.f;
    }
    return r.info[4 * p] == OK && fin && any && std::fabs(det - 1.0) < 1e-5 && pose[11] > 0.f && r.info[4 * p + 3] >= 1 && r.info[4 * p + 3] <= LM_ITERS;
}

int main() {
    int cases = 0;
    // 1. kp = 5, 9, 16; 0..2 planted outliers (none for kp = 5: five points are one hypothesis)
    for (int n : {5, 9, 16}) {
        const std::vector<uint8_t> table = make_table(n);
        std::vector<Pair> pairs;
        for (int k = 0; k < 4; ++k) pairs.push_back(make_pair(n, n == 5 ? 0 : k % 3, IDENTITY));
        const Result r = run(pairs, std::vector<float>(4, 1.f), IDENTITY, table, 1.0);
        cases += 4;
        EXPECT(r.solved == 4 && r.unsolved == 0 && std::isfinite(r.loss) && r.loss > 0.0, "kp %d: %d solved, %d unsolved, loss %g", n, r.solved, r.unsolved, r.loss);
        for (int p = 0; p < 4; ++p)
            // (five noisy points are a single hypothesis, which may have few inliers: the solve then starts from EPnP on all points)
            EXPECT(good_pair(r, p, n) && (n == 5 || r.info[4 * p + 2] >= n - p % 3), "kp %d pair %d: status %d, %d inliers, %d LM iterations", n, p,
                   r.info[4 * p], r.info[4 * p + 2], r.info[4 * p + 3]);
    }
    const std::vector<uint8_t> table9 = make_table(9);
    // 2. an unavailable pair, a collapsed vote and a NaN keypoint among solved pairs; all pairs unavailable
    {
        std::vector<Pair> pairs;
        for (int k = 0; k < 5; ++k) pairs.push_back(make_pair(9, k % 2, IDENTITY));
        for (int i = 0; i < 9; ++i) { pairs[2].yx[2 * i] = 207.25f; pairs[2].yx[2 * i + 1] = 311.5f; }
        pairs[3].yx[8] = NAN;
        const Result r = run(pairs, {1.f, 0.f, 1.f, 1.f, 1.f}, IDENTITY, table9, 0.5);
        cases += 5;
        EXPECT(r.solved == 2 && r.unsolved == 2 && std::isfinite(r.loss), "mixed batch: %d solved, %d unsolved, loss %g", r.solved, r.unsolved, r.loss);
        EXPECT(good_pair(r, 0, 9) && good_pair(r, 4, 9), "mixed batch: status %d and %d", r.info[0], r.info[16]);
        EXPECT(r.info[4] == SKIPPED && r.info[8] == DEGENERATE && r.info[12] == NONFINITE_INPUT, "mixed batch: status %d %d %d", r.info[4], r.info[8], r.info[12]);
        for (int p = 1; p <= 3; ++p)
            EXPECT(all_zero(&r.g[(size_t)p * 18], 18) && all_zero(&r.poses[(size_t)p * 12], 12), "mixed batch: pair %d is not zero", p);
        const Result none = run(pairs, std::vector<float>(5, 0.f), IDENTITY, table9, 1.0);
        EXPECT(none.solved == 0 && none.unsolved == 0 && none.loss == 0.0 && all_zero(none.g.data(), (int)none.g.size()), "all unavailable: %d solved, loss %g",
               none.solved, none.loss);
    }
    // 3. a crop affine (shift, rotation, scale): the gradient against central differences of the loss, the PnP re-solved at every perturbed point
    {
        const float affine[6] = {0.79f, -0.11f, 37.5f, 0.11f, 0.79f, -12.25f};
        std::vector<Pair> pairs = {make_pair(9, 0, affine), make_pair(9, 1, affine)};
        const std::vector<float> avail(2, 1.f);
        const Result r = run(pairs, avail, affine, table9, 1.0);
        cases += 2;
        EXPECT(r.solved == 2 && good_pair(r, 0, 9) && good_pair(r, 1, 9), "affine: %d solved", r.solved);
        const float h = 0.0009765625f;   // 2^-10 px: exact on fp32 coordinates below 2^13
        double worst = 0.0, largest = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int i = 0; i < 18; i += 4) {
                std::vector<Pair> up = pairs, down = pairs;
                up[p].yx[i] += h;
                down[p].yx[i] -= h;
                const double num = (run(up, avail, affine, table9, 1.0).loss - run(down, avail, affine, table9, 1.0).loss) / (2.0 * (double)h);
                worst = std::fmax(worst, std::fabs(num - (double)r.g[(size_t)p * 18 + i]));
                largest = std::fmax(largest, std::fabs(num));
            }
        EXPECT(largest > 0.0 && worst < 2e-2 * largest, "affine: gradient differs from central differences by %.3g of %.3g", worst, largest);
    }
    SELFTEST_END("bpnp_selftest", "%d pairs: kp 5, 9 and 16, outliers, an unavailable pair, a collapsed vote, a NaN keypoint, a crop affine with central differences", cases);
}
