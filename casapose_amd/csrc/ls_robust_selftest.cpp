// Stand-alone self-test of ls_robust_math.h on the host, meant to be built with -fsanitize=address,undefined (make ls-robust-selftest) and run on
// the CPU.  It is never loaded into Python.  It runs the weight and the solve rule of the robust voter -- what the reweighted passes of
// ls_vote.hip carry out per term and per (image, slot, keypoint) -- over a small planted scene: two touching discs, every pixel pointing exactly
// at its own disc's keypoints, a few pixels beside the contact handed to the neighbour's slot.  The sums live in buffers of exactly
// [slots][kp][5] doubles, so that an index past them is an AddressSanitizer report.
#include <cmath>
#include <cstdint>
#include <vector>

#include "ls_robust_math.h"
#include "selftest.h"

namespace {

constexpr int H = 40, W = 64, KP = 3, SLOTS = 3;   // slot 3 is the rank-one slot
constexpr float CUTOFF = 4.f;

struct Scene {
    std::vector<uint8_t> slot;        // [H][W], 0 = background
    std::vector<float> dir;           // [H][W][KP][2] (dy, dx), not normalised
    double kp[SLOTS][KP][2];          // planted keypoints (y, x) in pixels
};

// the five terms of one keypoint of one pixel with weight w: R = w (I - n n^T) and R c, in fp32 and summed in fp64 as the voter does
void add_terms(double* a, float ny, float nx, float w, float cy, float cx) {
    const float r00 = (1.0f - ny * ny) * w, r01 = (0.0f - ny * nx) * w, r11 = (1.0f - nx * nx) * w;
    a[0] += r00, a[1] += r01, a[2] += r11;
    a[3] += r00 * cy + r01 * cx, a[4] += r01 * cy + r11 * cx;
}

// one pass over the slot map: plain with est == nullptr, otherwise reweighted against est [SLOTS][KP][2] in pixels
std::vector<double> accumulate(const Scene& s, const float* est) {
    std::vector<double> sums((size_t)SLOTS * KP * 5, 0.0);
    const float scale = cp_lsr::rho_scale(H, CUTOFF);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int lab = s.slot[(size_t)y * W + x];
            if (lab == 0) continue;
            const float cy = ((float)y + 0.5f) / (float)H, cx = ((float)x + 0.5f) / (float)H;
            for (int j = 0; j < KP; ++j) {
                const float dy = s.dir[(((size_t)y * W + x) * KP + j) * 2], dx = s.dir[(((size_t)y * W + x) * KP + j) * 2 + 1];
                const float nrm = std::sqrt(dy * dy + dx * dx);
                const float ny = nrm > 0.f ? dy / nrm : 0.f, nx = nrm > 0.f ? dx / nrm : 0.f;
                float w = 1.f;
                if (est) {
                    const float* p = est + ((size_t)(lab - 1) * KP + j) * 2;
                    w *= cp_lsr::rho(p[0] / (float)H, p[1] / (float)H, cy, cx, ny, nx, scale);
                }
                add_terms(&sums[((size_t)(lab - 1) * KP + j) * 5], ny, nx, w, cy, cx);
            }
        }
    return sums;
}

// the plain solve of a regular system (the self-test's slots 1 and 2), in pixels
void plain_solve(const double* s, float* out) {
    const double det = s[0] * s[2] - s[1] * s[1];
    out[0] = (float)((s[2] * s[3] - s[1] * s[4]) / det) * (float)H;
    out[1] = (float)((s[0] * s[4] - s[1] * s[3]) / det) * (float)H;
}

// the solve of a reweighted pass over all slots: how many keypoints kept the value of the pass before
int robust_solve(const std::vector<double>& plain, const std::vector<double>& again, std::vector<float>& kp) {
    int kept_back = 0;
    for (int i = 0; i < SLOTS * KP; ++i) {
        double p0, p1;
        if (cp_lsr::solve(&again[(size_t)i * 5], plain[(size_t)i * 5] + plain[(size_t)i * 5 + 2], p0, p1))
            kp[2 * i] = (float)p0 * (float)H, kp[2 * i + 1] = (float)p1 * (float)H;
        else
            ++kept_back;
    }
    return kept_back;
}

double worst_error(const Scene& s, const std::vector<float>& kp, int slots) {
    double e = 0.0;
    for (int o = 0; o < slots; ++o)
        for (int j = 0; j < KP; ++j)
            for (int c = 0; c < 2; ++c) e = std::fmax(e, std::fabs((double)kp[((size_t)o * KP + j) * 2 + c] - s.kp[o][j][c]));
    return e;
}

}  // namespace

int main() {
    // 1. the weight
    {
        const float sc = cp_lsr::rho_scale(40, 4.f);   // = 10: a distance of 0.1 normalised is the cut-off
        EXPECT(sc == 10.f, "scale %g", sc);
        // the pixel at the origin pointing along x; the estimate d above its line
        EXPECT(cp_lsr::rho(0.f, 0.7f, 0.f, 0.f, 0.f, 1.f, sc) == 1.f, "on the line: rho = 1");
        EXPECT(cp_lsr::rho(0.f, -0.7f, 0.f, 0.f, 0.f, 1.f, sc) == 1.f, "on the line behind the pixel: rho = 1 (lines, not rays)");
        EXPECT(std::fabs(cp_lsr::rho(0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, sc) - 0.5625f) < 1e-6f, "half the cut-off: (1 - 1/4)^2");
        EXPECT(cp_lsr::rho(-0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, sc) == cp_lsr::rho(0.05f, 0.3f, 0.f, 0.f, 0.f, 1.f, sc), "the sign of the distance");
        EXPECT(cp_lsr::rho(0.1f, 0.3f, 0.f, 0.f, 0.f, 1.f, sc) < 1e-12f, "at the cut-off: 0 (continuous)");
        EXPECT(cp_lsr::rho(0.25f, 0.3f, 0.f, 0.f, 0.f, 1.f, sc) == 0.f, "beyond the cut-off: exactly 0");
        EXPECT(cp_lsr::rho(0.f, 0.3f, 0.f, 0.f, 0.f, 0.f, sc) == 0.f, "a zero direction: 0");
        EXPECT(cp_lsr::rho(NAN, 0.3f, 0.f, 0.f, 0.f, 1.f, sc) == 0.f, "a NaN estimate: 0");
        EXPECT(cp_lsr::rho(INFINITY, 0.3f, 0.f, 0.f, 0.f, 1.f, sc) == 0.f, "an infinite estimate: 0");
    }
    // 2. the solve rule on hand-written systems
    {
        double p0 = 7.0, p1 = 7.0;
        const double regular[5] = {2.0, 0.0, 1.0, 1.0, 0.25};
        EXPECT(cp_lsr::solve(regular, 3.0, p0, p1) && p0 == 0.5 && p1 == 0.25, "a regular system: (%g, %g)", p0, p1);
        p0 = p1 = 7.0;
        EXPECT(cp_lsr::solve(regular, 24.0, p0, p1) && p0 == 0.5, "exactly 1/8 of the plain weight is kept");
        p0 = p1 = 7.0;
        EXPECT(!cp_lsr::solve(regular, 24.5, p0, p1) && p0 == 7.0 && p1 == 7.0, "below 1/8 of the plain weight: refused, p untouched");
        const double rank_one[5] = {0.0, 0.0, 5.0, 0.0, 2.0};   // every direction (1, 0): R = diag(0, w)
        EXPECT(!cp_lsr::solve(rank_one, 5.0, p0, p1) && p0 == 7.0, "rank one: refused");
        const double empty[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        EXPECT(!cp_lsr::solve(empty, 0.0, p0, p1) && p0 == 7.0, "an empty slot: refused");
        const double thin[5] = {1.0, 0.0, 0.9e-6, 1.0, 1.0};
        const double fair[5] = {1.0, 0.0, 1.1e-6, 1.0, 1.0};
        EXPECT(!cp_lsr::solve(thin, 1.0, p0, p1) && p0 == 7.0, "condition number above 1e6: refused");
        EXPECT(cp_lsr::solve(fair, 1.0, p0, p1) && p0 == 1.0, "condition number below 1e6: taken");
        const double nan[5] = {NAN, 0.0, 1.0, 1.0, 1.0};
        p0 = 7.0;
        EXPECT(!cp_lsr::solve(nan, 1.0, p0, p1) && p0 == 7.0, "NaN sums: refused");
    }
    // 3. the planted scene: discs of radius 12 around (20, 19) and (20, 43) touch at x = 31; slot 3 is a block whose directions are all (1, 0)
    Scene s;
    s.slot.assign((size_t)H * W, 0);
    s.dir.assign((size_t)H * W * KP * 2, 0.f);
    const double centre[2][2] = {{20.0, 19.0}, {20.0, 43.0}};
    const double offs[KP][2] = {{0.0, 0.0}, {-6.0, 5.0}, {7.0, -4.0}};
    for (int o = 0; o < 2; ++o)
        for (int j = 0; j < KP; ++j) s.kp[o][j][0] = centre[o][0] + offs[j][0], s.kp[o][j][1] = centre[o][1] + offs[j][1];
    for (int j = 0; j < KP; ++j) s.kp[2][j][0] = s.kp[2][j][1] = 0.0;
    int stray = 0, size[2] = {0, 0};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const double py = y + 0.5, px = x + 0.5;
            int own = -1;
            for (int o = 0; o < 2; ++o)
                if ((py - centre[o][0]) * (py - centre[o][0]) + (px - centre[o][1]) * (px - centre[o][1]) <= 144.0 && (o == 0 ? px < 31.0 : px >= 31.0)) own = o;
            if (own < 0) continue;
            ++size[own];
            // the pixels of disc 2 in columns 31 and 32, rows 17 .. 22, are handed to slot 1: they keep their own disc's directions
            const bool moved = own == 1 && x <= 32 && y >= 17 && y <= 22;
            stray += moved;
            s.slot[(size_t)y * W + x] = (uint8_t)(moved ? 1 : own + 1);
            for (int j = 0; j < KP; ++j) {
                s.dir[(((size_t)y * W + x) * KP + j) * 2] = (float)(s.kp[own][j][0] - py);
                s.dir[(((size_t)y * W + x) * KP + j) * 2 + 1] = (float)(s.kp[own][j][1] - px);
            }
        }
    for (int y = 0; y < 4; ++y)
        for (int x = 56; x < 64; ++x) {
            s.slot[(size_t)y * W + x] = 3;
            for (int j = 0; j < KP; ++j) s.dir[(((size_t)y * W + x) * KP + j) * 2] = 1.f;
        }
    EXPECT(stray == 12 && size[0] > 200 && size[1] > 200, "the scene: %d stray pixels, discs of %d and %d", stray, size[0], size[1]);

    const std::vector<double> plain = accumulate(s, nullptr);
    std::vector<float> kp((size_t)SLOTS * KP * 2, 0.f);
    for (int i = 0; i < 2 * KP; ++i) plain_solve(&plain[(size_t)i * 5], &kp[2 * i]);
    for (int j = 0; j < KP; ++j) kp[((size_t)2 * KP + j) * 2] = 3.f, kp[((size_t)2 * KP + j) * 2 + 1] = 5.f;   // the rank-one slot's value of the pass before
    const double e0 = worst_error(s, kp, 2);
    EXPECT(e0 > 0.25, "the plain solve is off: %.4f px", e0);
    double e = e0;
    std::vector<double> again;
    for (int pass = 1; pass <= 2; ++pass) {
        again = accumulate(s, kp.data());
        const int back = robust_solve(plain, again, kp);
        EXPECT(back == KP, "pass %d: only the rank-one slot's %d keypoints keep their value (%d did)", pass, KP, back);
        e = worst_error(s, kp, 2);
    }
    EXPECT(e < 0.05 && e < 0.1 * e0, "two passes bring it back: %.4f px after %.4f px", e, e0);
    for (int j = 0; j < KP; ++j)
        EXPECT(kp[((size_t)2 * KP + j) * 2] == 3.f && kp[((size_t)2 * KP + j) * 2 + 1] == 5.f, "the rank-one slot keeps its previous value");
    // the share of the plain weight kept by slot 1: its own pixels in full, the strays (12 of size[0] + 12) mostly gone
    const double share = (again[0] + again[2]) / (plain[0] + plain[2]);
    EXPECT(share > (double)size[0] / (size[0] + 12) - 1e-3 && share < 1.0, "slot 1 kept %.4f of its weight", share);
    // 4. a slot that loses more than 7/8 of its weight keeps the value of the pass before: slot 2 against an estimate 30 px off
    {
        std::vector<float> far(kp);
        for (int j = 0; j < KP; ++j) far[((size_t)KP + j) * 2] += 30.f;
        const std::vector<double> lost = accumulate(s, far.data());
        const std::vector<float> before(far);
        robust_solve(plain, lost, far);
        const double kept = (lost[(size_t)KP * 5] + lost[(size_t)KP * 5 + 2]) / (plain[(size_t)KP * 5] + plain[(size_t)KP * 5 + 2]);
        EXPECT(kept > 0.0 && kept < 0.125, "slot 2 keeps %.4f of its weight against an estimate 30 px off", kept);
        for (int j = 0; j < KP; ++j) EXPECT(far[((size_t)KP + j) * 2] == before[((size_t)KP + j) * 2], "slot 2 keeps the value of the pass before");
    }
    SELFTEST_END("ls_robust_selftest", "the weight on and off the line, at and beyond the cut-off, zero directions, NaN; the solve rule: regular, 1/8 of the "
                                       "weight, rank one, empty, condition 1e6; two discs with %d stray pixels: plain %.3f px, two passes %.4f px", stray, e0, e);
}
