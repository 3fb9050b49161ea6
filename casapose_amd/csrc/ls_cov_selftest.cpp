// Stand-alone self-test of ls_cov_math.h on the host, meant to be built with -fsanitize=address,undefined (make ls-cov-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs what the moments pass of ls_vote.hip adds per (pixel, keypoint) and the finish per (image,
// slot, keypoint) over known answers, every refusal and the (x, y) order of the output, and sweeps 2 x 2 systems to see that the rule factored
// out of cp_lsr::solve (cp_lsr::well_posed) leaves that solve's decisions and values what they were.  The sums live in buffers of exactly five
// doubles, cov and stat in buffers of exactly three and two floats, so that an index past them is an AddressSanitizer report.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ls_cov_math.h"
#include "selftest.h"

namespace {

constexpr int H = 40;

// one line: the pixel at (y, x) pixels, direction (dy, dx) not normalised, weight w; added to s against the estimate (py, px) pixels
void add(std::vector<double>& s, double y, double x, double dy, double dx, float w, float py, float px, float rscale) {
    const float cy = (float)y / (float)H, cx = (float)x / (float)H;
    const float nrm = std::sqrt((float)(dy * dy + dx * dx));
    const float ny = nrm > 0.f ? (float)dy / nrm : 0.f, nx = nrm > 0.f ? (float)dx / nrm : 0.f;
    const cp_lsc::Moment m = cp_lsc::moment(py / (float)H, px / (float)H, cy, cx, ny, nx, w, rscale);
    s[0] += (double)((1.0f - ny * ny) * m.omega);
    s[1] += (double)((0.0f - ny * nx) * m.omega);
    s[2] += (double)((1.0f - nx * nx) * m.omega);
    s[3] += (double)m.q;
    s[4] += (double)m.wall;
}

// cp_lsr::solve as it stood before the rule was factored out, word for word
bool solve_before(const double* s, double plain_trace, double& p0, double& p1) {
    const double a = s[0], b = s[1], c = s[2], t0 = s[3], t1 = s[4];
    const double half_tr = 0.5 * (a + c), half_df = 0.5 * (a - c);
    const double rad = sqrt(half_df * half_df + b * b);
    const double l1 = half_tr + rad, l2 = half_tr - rad;
    const double rcond = 10.0 * 2.0 * 2.220446049250313e-16;
    const double smax = fmax(fabs(l1), fabs(l2));
    if (!(smax > 0.0)) return false;
    if (!(fabs(l2) > rcond * smax && fabs(l1) > rcond * smax)) return false;
    if (!(l2 > 0.0 && l1 < cp_lsr::CP_LS_ROBUST_MAX_COND * l2)) return false;
    if (!(a + c >= cp_lsr::CP_LS_ROBUST_MIN_KEPT * plain_trace)) return false;
    const double det = a * c - b * b;
    p0 = (c * t0 - b * t1) / det;
    p1 = (a * t1 - b * t0) / det;
    return true;
}

bool all_nan(const std::vector<float>& c) { return std::isnan(c[0]) && std::isnan(c[1]) && std::isnan(c[2]); }

}  // namespace

int main() {
    std::vector<float> cov(3), stat(2);
    // 1. what one pixel adds: the estimate (0.05, 0.3) normalised above the line of the pixel at the origin pointing along x
    {
        cp_lsc::Moment m = cp_lsc::moment(0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, 2.f, 0.f);
        EXPECT(m.omega == 2.f && std::fabs(m.q - 2.f * 0.05f * 0.05f) < 1e-9f && m.wall == 2.f, "no cut-off: omega = w, q = w d^2 (%g %g %g)", m.omega, m.q, m.wall);
        m = cp_lsc::moment(0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, 2.f, 10.f);   // half the cut-off: rho = 0.5625
        EXPECT(std::fabs(m.omega - 1.125f) < 1e-6f && std::fabs(m.q - 1.125f * 0.0025f) < 1e-8f && m.wall == 2.f, "half the cut-off (%g %g %g)", m.omega, m.q, m.wall);
        EXPECT(m.omega == 2.f * cp_lsr::rho(0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, 10.f), "rho is cp_lsr::rho itself");
        m = cp_lsc::moment(0.25f, 0.3f, 0.f, 0.f, 0.f, 1.f, 2.f, 10.f);
        EXPECT(m.omega == 0.f && m.q == 0.f && m.wall == 2.f, "beyond the cut-off: nothing but Wall");
        for (float rs : {0.f, 10.f}) {
            m = cp_lsc::moment(0.05f, 0.3f, 0.f, 0.f, 0.f, 0.f, 2.f, rs);
            EXPECT(m.omega == 0.f && m.q == 0.f && m.wall == 0.f, "a zero direction takes no part (rscale %g)", rs);
        }
        m = cp_lsc::moment(-0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, 2.f, 10.f);
        EXPECT(std::fabs(m.omega - 1.125f) < 1e-6f, "the sign of the distance");
    }
    // 2. a known answer: 64 pixels on a circle of radius 10 around (20, 20), every line delta = 0.5 px off the centre
    {
        const float rs[2] = {0.f, cp_lsr::rho_scale(H, 4.f)};
        for (int k = 0; k < 2; ++k) {
            std::vector<double> s(5, 0.0);
            for (int i = 0; i < 64; ++i) {
                const double t = 2.0 * M_PI * i / 64.0, off = std::asin(0.5 / 10.0);   // every direction turned alike: the set of directions stays uniform, sum n n^T = 32 I
                add(s, 20.0 + 10.0 * std::sin(t), 20.0 + 10.0 * std::cos(t), -std::sin(t + off), -std::cos(t + off), 1.5f, 20.f, 20.f, rs[k]);
            }
            const bool ok = cp_lsc::finish(s.data(), true, H, cov.data(), stat.data());
            const double rho = k ? (1.0 - 1.0 / 64.0) * (1.0 - 1.0 / 64.0) : 1.0;   // (1 - (0.5 / 4)^2)^2
            EXPECT(ok && std::fabs(cov[0] - 0.5) < 1e-3 && std::fabs(cov[2] - 0.5) < 1e-3 && std::fabs(cov[1]) < 1e-3, "the ring: Sigma = 2 delta^2 I (%g %g %g)", cov[0], cov[1], cov[2]);
            EXPECT(std::fabs(stat[0] - 0.25) < 1e-3 && std::fabs(stat[1] - rho) < 1e-4, "the ring: sigma2 = delta^2, kept = rho (%g %g)", stat[0], stat[1]);
            EXPECT(std::fabs(s[4] - 96.0) < 1e-9, "Wall is the weight before reweighting (%g)", s[4]);
        }
    }
    // 3. the (x, y) order: pixels left of the keypoint, rays along x, the keypoint 1 px off every line: long along x
    {
        std::vector<double> s(5, 0.0);
        for (int i = 0; i < 20; ++i)
            for (int j = 0; j < 5; ++j) {
                const double y = 10.0 + i, x = 2.0 + j, ty = 20.0 - y, tx = 60.0 - x, r = std::sqrt(ty * ty + tx * tx), off = std::asin((i % 2 ? 1.0 : -1.0) / r);
                const double a = std::atan2(ty, tx) + off;
                add(s, y, x, std::sin(a), std::cos(a), 1.f, 20.f, 60.f, 0.f);
            }
        const bool ok = cp_lsc::finish(s.data(), true, H, cov.data(), stat.data());
        EXPECT(ok && cov[0] > 20.f * cov[2] && cov[2] > 0.f, "sxx comes first and is the long axis (%g %g %g)", cov[0], cov[1], cov[2]);
        const double k = (double)H * H * s[3] / (s[0] * s[2] - s[1] * s[1]);
        EXPECT(cov[0] == (float)(k * s[0]) && cov[1] == (float)(-(k * s[1])) && cov[2] == (float)(k * s[2]), "cov = (Sigma[1][1], Sigma[0][1], Sigma[0][0]) of the (y, x) matrix");
        EXPECT(std::fabs(stat[0] - 1.0) < 1e-3 && stat[1] == 1.f, "sigma2 = 1 px^2, all kept (%g %g)", stat[0], stat[1]);
        // 4. every refusal, on these sums and on hand-written ones
        EXPECT(!cp_lsc::finish(s.data(), false, H, cov.data(), stat.data()) && all_nan(cov) && stat[0] == 0.f && stat[1] == 0.f, "an estimate that is not finite");
        std::vector<double> low(s);
        low[4] = 8.5 * (s[0] + s[2]);
        EXPECT(!cp_lsc::finish(low.data(), true, H, cov.data(), stat.data()) && all_nan(cov) && stat[1] > 0.f && stat[1] < 0.125f, "kept below 1/8 (%g)", stat[1]);
        low[4] = 8.0 * (s[0] + s[2]);
        EXPECT(cp_lsc::finish(low.data(), true, H, cov.data(), stat.data()) && stat[1] == 0.125f, "kept exactly 1/8 is taken");
    }
    {
        const std::vector<double> empty(5, 0.0), rank_one{0.0, 0.0, 5.0, 0.1, 5.0}, thin{1.0, 0.0, 0.9e-6, 0.1, 1.0}, fair{1.0, 0.0, 1.1e-6, 0.1, 1.0},
            nan{NAN, 0.0, 1.0, 0.1, 1.0}, negative{-1.0, 0.0, -1.0, 0.1, 1.0};
        EXPECT(!cp_lsc::finish(empty.data(), true, H, cov.data(), stat.data()) && all_nan(cov) && stat[0] == 0.f && stat[1] == 0.f, "an empty slot");
        EXPECT(!cp_lsc::finish(rank_one.data(), true, H, cov.data(), stat.data()) && all_nan(cov) && stat[1] == 1.f, "parallel directions: rank one");
        EXPECT(!cp_lsc::finish(thin.data(), true, H, cov.data(), stat.data()) && all_nan(cov), "condition number above 1e6");
        EXPECT(cp_lsc::finish(fair.data(), true, H, cov.data(), stat.data()) && !all_nan(cov), "condition number below 1e6");
        EXPECT(!cp_lsc::finish(nan.data(), true, H, cov.data(), stat.data()) && all_nan(cov), "NaN sums");
        EXPECT(!cp_lsc::finish(negative.data(), true, H, cov.data(), stat.data()) && all_nan(cov) && stat[0] == 0.f, "W not > 0");
    }
    // 5. the factored rule: cp_lsr::solve decides and computes what it did, on a sweep of systems around every threshold
    int swept = 0, taken = 0;
    {
        const double diag[] = {0.0, 1e-300, 1e-9, 0.9e-6, 1.0e-6, 1.1e-6, 1e-3, 0.5, 1.0, 3.0, 1e6, 1.1e6, -1.0, NAN, INFINITY};
        const double offd[] = {0.0, 1e-7, -1e-3, 0.5, -0.999, 1.0, 2.0, NAN};
        const double traces[] = {0.0, 1.0, 7.9, 8.0, 8.1, 1e9, NAN};
        for (double a : diag)
            for (double c : diag)
                for (double b : offd)
                    for (double tr : traces) {
                        const double s[5] = {a, b, c, 0.7, -0.3};
                        double p0 = 7.0, p1 = 7.0, q0 = 7.0, q1 = 7.0;
                        const bool now = cp_lsr::solve(s, tr, p0, p1), before = solve_before(s, tr, q0, q1);
                        ++swept;
                        taken += now;
                        if (now != before || std::memcmp(&p0, &q0, sizeof p0) || std::memcmp(&p1, &q1, sizeof p1)) EXPECT(false, "the solve changed at a = %g b = %g c = %g trace = %g", a, b, c, tr);
                        const bool wp = cp_lsr::well_posed(a, b, c);
                        if (now && !wp) EXPECT(false, "a system the solve takes is well posed (a = %g b = %g c = %g)", a, b, c);
                    }
        EXPECT(taken > 100 && taken < swept / 2, "the sweep takes and refuses (%d of %d taken)", taken, swept);
    }
    SELFTEST_END("ls_cov_selftest", "the moment of one pixel with and without a cut-off, zero directions; the ring (Sigma = 2 delta^2 I); the (x, y) order; every refusal: "
                                    "estimate not finite, kept below 1/8, empty, rank one, condition 1e6, NaN, W <= 0; the factored rule over %d systems (%d taken)", swept, taken);
}
