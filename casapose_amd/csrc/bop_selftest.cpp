// Stand-alone self-test of bop_math.h on the host, meant to be built with -fsanitize=address,undefined (make bop-selftest) and run on the CPU.
// It is never loaded into Python.  It runs pair_errors_serial -- the loop the two kernels of bop_errors.hip carry out -- on buffers of exactly
// the input and output sizes, so that any index past them is an AddressSanitizer report, on cases worked out by hand: the identity symmetry, a
// 180 degree discrete symmetry, padded vertices and symmetries, the zero pose, and a projective z of exactly 0.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bop_math.h"
#include "selftest.h"

using namespace cp_bop;

static const float IDENT[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
static const float RZ180[12] = {-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0};
static const float K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};

struct Out {
    float e[2];
    std::vector<float> per;
};

// exact-size copies of every input: a read past a mesh's `count` vertices or an object's `sym_count` transforms leaves its array
static Out run(const std::vector<float>& points, int count, const std::vector<float>& syms, int sym_count, int smax, const float* est, const float* gt,
               const float* k) {
    float* p = (float*)std::malloc((size_t)count * 3 * sizeof(float) + 1);
    float* s = (float*)std::malloc((size_t)sym_count * 12 * sizeof(float) + 1);
    float* rec = (float*)std::malloc(PAIR_FLOATS * sizeof(float));
    std::memcpy(p, points.data(), (size_t)count * 3 * sizeof(float));
    std::memcpy(s, syms.data(), (size_t)sym_count * 12 * sizeof(float));
    std::memset(rec, 0, PAIR_FLOATS * sizeof(float));
    std::memcpy(rec, est, 12 * sizeof(float));
    std::memcpy(rec + 12, gt, 12 * sizeof(float));
    std::memcpy(rec + 24, k, 9 * sizeof(float));
    Out o;
    o.per.assign((size_t)smax * 2, -1.f);
    pair_errors_serial(p, count, s, sym_count, smax, rec, o.e, o.per.data());
    std::free(p);
    std::free(s);
    std::free(rec);
    return o;
}

static std::vector<float> cat(const float* a, const float* b = nullptr) {
    std::vector<float> v(a, a + 12);
    if (b) v.insert(v.end(), b, b + 12);
    return v;
}

int main() {
    // two vertices on the x axis, 1000 mm in front of the camera
    const std::vector<float> bar = {10, 0, 0, -10, 0, 0};
    const float gt[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1000};
    // 1. identity symmetry, the estimate 3 mm to the right and 4 mm up: every vertex is 5 mm off, and (500 * 3 / 1000, 500 * 4 / 1000) pixels
    {
        const float est[12] = {1, 0, 0, 3, 0, 1, 0, 4, 0, 0, 1, 1000};
        const Out o = run(bar, 2, cat(IDENT), 1, 1, est, gt, K);
        EXPECT(o.e[0] == 5.f && std::fabs(o.e[1] - 2.5f) < 1e-4f, "identity: (%g, %g), expected (5, 2.5)", o.e[0], o.e[1]);
        EXPECT(o.per[0] == o.e[0] && o.per[1] == o.e[1], "identity: the per-symmetry entry is not the result");
    }
    // 2. the estimate is the ground truth turned by 180 degrees about z: 20 mm and 500 * 20 / 1000 = 10 px under the identity, 0 under Rz(180)
    {
        const float est[12] = {-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 1000};
        const Out one = run(bar, 2, cat(IDENT), 1, 1, est, gt, K);
        EXPECT(one.e[0] == 20.f && std::fabs(one.e[1] - 10.f) < 1e-4f, "180 degrees without its symmetry: (%g, %g), expected (20, 10)", one.e[0], one.e[1]);
        const Out two = run(bar, 2, cat(IDENT, RZ180), 2, 2, est, gt, K);
        EXPECT(two.e[0] == 0.f && two.e[1] == 0.f, "180 degrees with its symmetry: (%g, %g), expected (0, 0)", two.e[0], two.e[1]);
        EXPECT(two.per[0] == 20.f && two.per[2] == 0.f && two.per[3] == 0.f, "180 degrees: per-symmetry maxima %g, %g, %g", two.per[0], two.per[2], two.per[3]);
    }
    // 3. a symmetry with a translation composes as R_ t_s + t_: the ground truth turned by 90 degrees about z, the symmetry shifts by (0, 7, 0),
    //    which the ground truth turns into (-7, 0, 0)
    {
        const float gtz[12] = {0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1000};
        const float shift[12] = {1, 0, 0, 0, 0, 1, 0, 7, 0, 0, 1, 0};
        float m[12];
        for (int e = 0; e < 12; ++e) m[e] = compose_entry(gtz, shift, e);
        const float want[12] = {0, -1, 0, -7, 1, 0, 0, 0, 0, 0, 1, 1000};
        EXPECT(std::memcmp(m, want, sizeof m) == 0, "composition with a translation: t = (%g, %g, %g)", m[3], m[7], m[11]);
        const float est[12] = {0, -1, 0, -7, 1, 0, 0, 0, 0, 0, 1, 1000};
        const Out o = run(bar, 2, cat(IDENT, shift), 2, 2, est, gtz, K);
        EXPECT(o.e[0] == 0.f && o.per[0] == 7.f, "shifted symmetry: min %g, identity %g", o.e[0], o.per[0]);
    }
    // 4. padding: the arrays hold 2 vertices and 1 symmetry; smax = 3 leaves two per-symmetry entries at +inf
    {
        const float est[12] = {1, 0, 0, 3, 0, 1, 0, 4, 0, 0, 1, 1000};
        const Out o = run(bar, 2, cat(IDENT), 1, 3, est, gt, K);
        EXPECT(o.e[0] == 5.f, "padding: %g", o.e[0]);
        for (int i = 2; i < 6; ++i) EXPECT(std::isinf(o.per[i]) && o.per[i] > 0, "padding: per-symmetry entry %d is %g, expected +inf", i, o.per[i]);
        // a third vertex far off raises the maximum only when it is counted
        const std::vector<float> three = {10, 0, 0, -10, 0, 0, 0, 300, 0};
        const float rot[12] = {0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1000};
        const Out a = run(three, 2, cat(IDENT), 1, 1, rot, gt, K), b = run(three, 3, cat(IDENT), 1, 1, rot, gt, K);
        EXPECT(std::fabs(a.e[0] - 14.142136f) < 1e-5f && std::fabs(b.e[0] - 424.26407f) < 1e-4f, "counted vertices: %g and %g", a.e[0], b.e[0]);
    }
    // 5. no estimate: the zero pose, a pose whose entries cancel below 1e-4, a pose that is not finite, an object without vertices
    {
        const float zero[12] = {0};
        const float cancel[12] = {1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0};
        float nan[12];
        std::memcpy(nan, gt, sizeof nan);
        nan[5] = NAN;
        for (const float* est : {zero, cancel, (const float*)nan}) {
            const Out o = run(bar, 2, cat(IDENT), 1, 1, est, gt, K);
            EXPECT(std::isinf(o.e[0]) && std::isinf(o.e[1]) && std::isinf(o.per[0]) && std::isinf(o.per[1]), "no estimate: (%g, %g)", o.e[0], o.e[1]);
        }
        const Out o = run(bar, 0, cat(IDENT), 1, 1, gt, gt, K);
        EXPECT(std::isinf(o.e[0]) && std::isinf(o.e[1]), "an object without vertices: (%g, %g)", o.e[0], o.e[1]);
        EXPECT(!no_estimate(gt) && no_estimate(zero), "no_estimate");
    }
    // 6. projective z exactly 0 under the estimated pose: its pixel is (0, 0), so the 2-D error is |ground-truth pixel| = |(320, 240)| = 400
    {
        const std::vector<float> one = {0, 0, -5};
        const float est[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 5}, far[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 905};
        const Out o = run(one, 1, cat(IDENT), 1, 1, est, far, K);
        EXPECT(o.e[0] == 900.f && std::fabs(o.e[1] - 400.f) < 1e-3f, "z = 0: (%g, %g), expected (900, 400)", o.e[0], o.e[1]);
    }
    SELFTEST_END("bop_selftest", "identity, a 180 degree symmetry, a symmetry with a translation, padded vertices and symmetries, no estimate, z = 0");
}
