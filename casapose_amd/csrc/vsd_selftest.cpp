// Stand-alone self-test of vsd_math.h on the host, meant to be built with -fsanitize=address,undefined (make vsd-selftest) and run on the CPU.
// It is never loaded into Python.  It runs vsd_serial -- the loop the kernel of vsd.hip carries out -- on buffers of exactly the input and output
// sizes, so that any index past them is an AddressSanitizer report, on cases worked out by hand.  The image is 6 x 8 with f = 1000 and the
// principal point at its centre, so c lies in [1, 1.00001]: no case's comparison comes closer than 1 % to its threshold.
#include <cmath>
#include <cstring>
#include <vector>

#include "selftest.h"
#include "vsd_math.h"

using namespace cp_vsd;

constexpr int H = 6, W = 8;
static const double CAM[4] = {1000.0, 1000.0, 3.5, 2.5};
static const double TAUS[10] = {0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5};

struct Scene {
    std::vector<uint32_t> planes;
    std::vector<int32_t> records;
    std::vector<float> depth;
    explicit Scene(int nplanes, float sensor) : planes((size_t)nplanes * H * W, EMPTY), records((size_t)nplanes * RECORD, -1), depth((size_t)H * W, sensor) {}
    // columns [x0, x1] x rows [y0, y1] of a plane at depth z, and its record's box
    void fill(int plane, int x0, int y0, int x1, int y1, float z) {
        uint32_t bits;
        std::memcpy(&bits, &z, sizeof bits);
        for (int i = y0; i <= y1; ++i)
            for (int j = x0; j <= x1; ++j) planes[((size_t)plane * H + i) * W + j] = bits;
        const int32_t box[4] = {x0, y0, x1 - x0, y1 - y0};
        std::memcpy(&records[(size_t)plane * RECORD + R_BOX_OBJ], box, sizeof box);
    }
    void sensor(int x0, int y0, int x1, int y1, float z) {
        for (int i = y0; i <= y1; ++i)
            for (int j = x0; j <= x1; ++j) depth[(size_t)i * W + j] = z;
    }
    // one pair (image, estimate plane, ground-truth plane) into a buffer of exactly 2 + ntau integers, pre-filled with rubbish
    std::vector<int32_t> run(int image, int e, int g, int ntau = 10, const double* taus = TAUS, double diameter = 100.0, int images = 1) const {
        const std::vector<int32_t> pair = {image, e, g, 12345};
        const std::vector<double> cams(CAM, CAM + 4), dia(1, diameter), t(taus, taus + ntau);
        std::vector<int32_t> counts((size_t)(2 + ntau), -7);
        vsd_serial(planes.data(), records.data(), (int)(records.size() / RECORD), H, W, depth.data(), cams.data(), images, pair.data(), dia.data(), 1, 15.0,
                   t.data(), ntau, counts.data());
        return counts;
    }
};

// counts == (uni, inter, `per` at the first `reached` taus, 0 at the others)
static bool is(const std::vector<int32_t>& c, int uni, int inter, int reached, int per) {
    if (c[0] != uni || c[1] != inter) return false;
    for (size_t k = 2; k < c.size(); ++k)
        if (c[k] != ((int)k - 2 < reached ? per : 0)) return false;
    return true;
}

#define EXPECT_COUNTS(c, uni, inter, reached, per, what) \
    EXPECT(is(c, uni, inter, reached, per), what ": counts (%d, %d, %d, ..., %d)", (c)[0], (c)[1], (c)[2], (c).back())

int main() {
    // 1. the estimate equals the ground truth, 16 pixels at the sensor's depth: all visible, cost 0
    {
        Scene s(2, 1000.f);
        s.fill(0, 2, 1, 5, 4, 1000.f);
        s.fill(1, 2, 1, 5, 4, 1000.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 16, 16, 0, 0, "estimate == ground truth");
        // the estimate 32 mm behind: more than delta behind the sensor, visible only through vis_g; cost 0.32 c reaches 0.05 .. 0.30
        s.fill(0, 2, 1, 5, 4, 1032.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 16, 16, 6, 16, "estimate 0.32 diameters behind");
        // 8. ntau = 1, into three integers
        const double below = 0.3, above = 0.35;
        EXPECT_COUNTS(s.run(0, 0, 1, 1, &below), 16, 16, 1, 16, "ntau = 1, tau below the cost");
        EXPECT_COUNTS(s.run(0, 0, 1, 1, &above), 16, 16, 0, 0, "ntau = 1, tau above the cost");
        EXPECT_COUNTS(s.run(0, 0, 1, 10, TAUS, 0.0), 0, 0, 0, 0, "diameter 0");
    }
    // 2. an occluder 100 mm in front of the ground truth over columns 2-3 (8 of the 16 pixels)
    {
        Scene s(2, 1000.f);
        s.sensor(2, 1, 3, 4, 900.f);
        s.fill(0, 2, 1, 5, 4, 1000.f);
        s.fill(1, 2, 1, 5, 4, 1000.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 8, 8, 0, 0, "occluder, estimate == ground truth");
        // the estimate at 905: 5 mm behind the occluder, so visible there (union only); elsewhere both are visible and 0.95 diameters apart
        s.fill(0, 2, 1, 5, 4, 905.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 16, 8, 10, 8, "occluder, estimate in front");
    }
    // 3. missing sensor depth (0, negative, NaN): a ground truth 100 mm behind a valid sensor depth is invisible, behind a missing one visible
    {
        Scene s(2, 1000.f);
        s.fill(0, 2, 1, 5, 4, 1132.f);
        s.fill(1, 2, 1, 5, 4, 1100.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 0, 0, 0, 0, "behind a valid sensor depth");
        for (float missing : {0.f, -1.f, NAN}) {
            s.sensor(0, 0, W - 1, H - 1, missing);
            EXPECT_COUNTS(s.run(0, 0, 1), 16, 16, 6, 16, "missing sensor depth");
        }
        s.sensor(2, 1, 5, 4, 1000.f);
        s.sensor(4, 1, 5, 4, 0.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 8, 8, 6, 8, "sensor depth missing over half of the object");
    }
    // 4. disjoint renders: 4 pixels each, no intersection
    {
        Scene s(2, 1000.f);
        s.fill(0, 0, 1, 1, 2, 1000.f);
        s.fill(1, 6, 1, 7, 2, 1000.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 8, 0, 0, 0, "disjoint renders");
    }
    // 5. both planes empty; one empty
    {
        Scene s(2, 1000.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 0, 0, 0, 0, "both planes empty");
        s.fill(1, 2, 1, 5, 4, 1000.f);
        EXPECT_COUNTS(s.run(0, 0, 1), 16, 0, 0, 0, "empty estimate");
        EXPECT_COUNTS(s.run(0, 1, 0), 16, 0, 0, 0, "empty ground truth");
    }
    // 6. indices out of range: nothing is read (the buffers end where the valid indices end)
    {
        Scene s(2, 1000.f);
        s.fill(0, 2, 1, 5, 4, 1000.f);
        s.fill(1, 2, 1, 5, 4, 1000.f);
        EXPECT_COUNTS(s.run(0, 2, 1), 0, 0, 0, 0, "estimate plane 2 of 2");
        EXPECT_COUNTS(s.run(0, 0, -1), 0, 0, 0, 0, "ground-truth plane -1");
        EXPECT_COUNTS(s.run(0, 0x7fffffff, 1), 0, 0, 0, 0, "estimate plane 2^31 - 1");
        EXPECT_COUNTS(s.run(1, 0, 1), 0, 0, 0, 0, "image 1 of 1");
        EXPECT_COUNTS(s.run(-1, 0, 1), 0, 0, 0, 0, "image -1");
    }
    // 7. boxes that cross the border are clipped: (-2, -3, 5, 5) -> columns 0-3 x rows 0-2, (6, 4, 10, 10) -> columns 6-7 x rows 4-5; a box
    //    wholly outside is empty; corners near the end of int32 do not overflow
    {
        Scene s(3, 1000.f);
        s.fill(0, 0, 0, 3, 2, 1000.f);
        s.fill(1, 6, 4, 7, 5, 1000.f);
        const int32_t a[4] = {-2, -3, 5, 5}, b[4] = {6, 4, 10, 10}, out[4] = {W, H, 3, 3}, huge[4] = {0x7ffffff0, 0x7ffffff0, 0x7ffffff0, 0x7ffffff0};
        std::memcpy(&s.records[0 * RECORD + R_BOX_OBJ], a, sizeof a);
        std::memcpy(&s.records[1 * RECORD + R_BOX_OBJ], b, sizeof b);
        EXPECT_COUNTS(s.run(0, 0, 0), 12, 12, 0, 0, "a box across the top-left corner");
        EXPECT_COUNTS(s.run(0, 1, 1), 4, 4, 0, 0, "a box across the bottom-right corner");
        EXPECT_COUNTS(s.run(0, 0, 1), 16, 0, 0, 0, "both: the union is the whole image");
        std::memcpy(&s.records[2 * RECORD + R_BOX_OBJ], out, sizeof out);
        EXPECT_COUNTS(s.run(0, 2, 2), 0, 0, 0, 0, "a box outside the image");
        std::memcpy(&s.records[2 * RECORD + R_BOX_OBJ], huge, sizeof huge);
        EXPECT_COUNTS(s.run(0, 2, 2), 0, 0, 0, 0, "a box near the end of int32");
    }
    SELFTEST_END("vsd_selftest", "estimate == ground truth, an occluder, missing sensor depth, disjoint renders, empty planes, indices out of range, "
                                 "boxes across the border, ntau = 1, diameter 0");
}
