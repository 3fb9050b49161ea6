// Stand-alone self-test of verify_math.h on the host, meant to be built with -fsanitize=address,undefined (make verify-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs verify_serial -- the loop the kernels of pose_verify.hip carry out -- on buffers of exactly the
// input and output sizes, so that any index past them is an AddressSanitizer report, on a case worked out by hand (tests/verify_cases.py
// states the same 5 x 7 case and its derivation).
#include <cmath>
#include <cstring>
#include <vector>

#include "selftest.h"
#include "verify_math.h"

using namespace cp_verify;

constexpr int H = 5, W = 7, LD = 4, DIR_OFF = 1;

static uint32_t bits(float z) {
    uint32_t b;
    std::memcpy(&b, &z, sizeof b);
    return b;
}

struct Scene {
    std::vector<uint32_t> planes;
    std::vector<int32_t> records, inst_counts;
    std::vector<uint8_t> labels;
    std::vector<float> field;
    int imax;
    Scene(int frames, int instances_max)
        : planes((size_t)frames * instances_max * H * W, EMPTY), records((size_t)frames * instances_max * RECORD, -1), inst_counts((size_t)frames, instances_max),
          labels((size_t)H * W, 0), field((size_t)H * W * LD, NAN), imax(instances_max) {}
    void fill(int plane, int x0, int y0, int x1, int y1, float z) {
        for (int i = y0; i <= y1; ++i)
            for (int j = x0; j <= x1; ++j) planes[((size_t)plane * H + i) * W + j] = bits(z);
        const int32_t box[4] = {x0, y0, x1 - x0, y1 - y0};
        std::memcpy(&records[(size_t)plane * RECORD + R_BOX_OBJ], box, sizeof box);
    }
    void word(int plane, int i, int j, float z) { planes[((size_t)plane * H + i) * W + j] = bits(z); }
    void direction(int i, int j, float dy, float dx) {
        field[((size_t)i * W + j) * LD + DIR_OFF] = dy;
        field[((size_t)i * W + j) * LD + DIR_OFF + 1] = dx;
    }
    // one job into a buffer of exactly 8 integers and a histogram of exactly 256, both pre-filled with rubbish
    std::vector<int32_t> run(int image, int plane, int label, double ky, double kx, double cos_min = 0.6, int images = 1) const {
        const std::vector<int32_t> job = {image, plane, label, 12345};
        const std::vector<double> kp = {ky, kx};
        std::vector<int32_t> counts(COUNTS, -7), hist((size_t)images * BINS, -9);
        verify_serial(planes.data(), records.data(), (int)(records.size() / RECORD), H, W, inst_counts.data(), (int)inst_counts.size(), imax, labels.data(),
                      field.data(), images, LD, DIR_OFF, 1, kp.data(), job.data(), 1, 0.5, cos_min, counts.data(), hist.data());
        return counts;
    }
};

static bool is(const std::vector<int32_t>& c, const int (&want)[COUNTS]) {
    for (int k = 0; k < COUNTS; ++k)
        if (c[k] != want[k]) return false;
    return true;
}

#define EXPECT_COUNTS(c, what, ...)                                                                                                          \
    do {                                                                                                                                     \
        const int want_[COUNTS] = {__VA_ARGS__};                                                                                             \
        const std::vector<int32_t> got_ = (c);                                                                                               \
        EXPECT(is(got_, want_), what ": counts (%d, %d, %d, %d, %d, %d, %d, %d)", got_[0], got_[1], got_[2], got_[3], got_[4], got_[5], got_[6], got_[7]); \
    } while (0)

static Scene hand() {
    Scene s(1, 2);
    s.fill(0, 1, 1, 4, 3, 2.0f);
    s.fill(1, 3, 2, 6, 4, 1.5f);
    s.word(1, 2, 3, 2.0f);   // plane 0's very word: the lower plane keeps the pixel
    s.word(1, 3, 4, 3.0f);   // behind plane 0
    const uint8_t lab[H][W] = {{1, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 1, 2, 0, 0}, {0, 1, 1, 1, 2, 2, 2}, {0, 1, 1, 2, 1, 2, 2}, {1, 0, 0, 2, 2, 2, 2}};
    std::memcpy(s.labels.data(), lab, sizeof lab);
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) s.direction(i, j, (float)(0.25 - (i + 0.5)), (float)(6.75 - (j + 0.5)));   // the ray to job B's keypoint
    s.direction(1, 2, 2.f, 2.f);                          // on the ray to (2.5, 3.5)
    s.direction(1, 3, -1.f, 0.f);                         // opposite
    s.direction(2, 1, std::nextafterf(4.f, 0.f), 3.f);    // cos a hair above 3 / 5
    s.direction(2, 2, std::nextafterf(4.f, 8.f), 3.f);    // a hair below
    s.direction(2, 3, 1.f, 0.f);                          // the keypoint at this pixel's centre
    s.direction(3, 1, 0.f, 0.f);
    s.direction(3, 2, NAN, 1.f);
    s.direction(3, 4, INFINITY, 1.f);
    return s;
}

int main() {
    // 1. the hand case: two overlapping planes, equal words on one pixel, a pixel under label 0 and one under another label, eight directions
    {
        const Scene s = hand();
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "job A", 12, 2, 8, 1, 1, 10, 4, 2);
        EXPECT_COUNTS(s.run(0, 1, 2, 0.25, 6.75), "job B", 12, 2, 10, 0, 0, 11, 10, 10);
        // cos_min 0: every pair that does not point away; cos_min 1: only the direction exactly on the ray
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5, 0.0), "cos_min 0", 12, 2, 8, 1, 1, 10, 4, 3);
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5, 1.0), "cos_min 1", 12, 2, 8, 1, 1, 10, 4, 1);
        // a label that is not in the map: everything visible lies on another label or on background
        EXPECT_COUNTS(s.run(0, 0, 9, 2.5, 3.5), "label 9", 12, 2, 0, 1, 9, 0, 0, 0);
        // a keypoint that is not finite makes no pair
        EXPECT_COUNTS(s.run(0, 0, 1, NAN, 3.5), "NaN keypoint", 12, 2, 8, 1, 1, 10, 0, 0);
        EXPECT_COUNTS(s.run(0, 0, 1, 1e200, 3.5), "a keypoint whose e.e overflows", 12, 2, 8, 1, 1, 10, 0, 0);
    }
    // 2. the frame's instance count bounds the planes that may hide: with one instance, plane 1 hides nothing of plane 0
    {
        Scene s = hand();
        s.inst_counts[0] = 1;
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "one instance", 12, 0, 8, 1, 3, 10, 4, 2);
        s.inst_counts[0] = -5;
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "a negative instance count", 12, 0, 8, 1, 3, 10, 4, 2);
        s.inst_counts[0] = 0x7fffffff;   // clamped to instances_max: no plane beyond the frame is read
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "an instance count of 2^31 - 1", 12, 2, 8, 1, 1, 10, 4, 2);
    }
    // 3. indices out of range leave zeros and read nothing (the buffers end where the valid indices end)
    {
        const Scene s = hand();
        EXPECT_COUNTS(s.run(1, 0, 1, 2.5, 3.5), "image 1 of 1", 0, 0, 0, 0, 0, 0, 0, 0);
        EXPECT_COUNTS(s.run(-1, 0, 1, 2.5, 3.5), "image -1", 0, 0, 0, 0, 0, 0, 0, 0);
        EXPECT_COUNTS(s.run(0, 2, 1, 2.5, 3.5), "plane 2 of 2", 0, 0, 0, 0, 0, 0, 0, 0);
        EXPECT_COUNTS(s.run(0, -1, 1, 2.5, 3.5), "plane -1", 0, 0, 0, 0, 0, 0, 0, 0);
        EXPECT_COUNTS(s.run(0, 0x7fffffff, 1, 2.5, 3.5), "plane 2^31 - 1", 0, 0, 0, 0, 0, 0, 0, 0);
        EXPECT_COUNTS(s.run(0, 0, 0, 2.5, 3.5), "label 0", 0, 0, 0, 0, 0, 0, 0, 0);
        EXPECT_COUNTS(s.run(0, 0, 256, 2.5, 3.5), "label 256", 0, 0, 0, 0, 0, 0, 0, 0);
        Scene t = hand();
        t.inst_counts.pop_back();   // no frame at all: plane 0's frame lies beyond inst_counts
        EXPECT_COUNTS(t.run(0, 0, 1, 2.5, 3.5), "a frame beyond inst_counts", 0, 0, 0, 0, 0, 0, 0, 0);
    }
    // 4. boxes: an empty one still counts the label's pixels; one across the border is clipped; corners near the end of int32 do not overflow
    {
        Scene s = hand();
        const int32_t none[4] = {-1, -1, -1, -1}, across[4] = {-2, -3, 5, 5}, huge[4] = {0x7ffffff0, 0x7ffffff0, 0x7ffffff0, 0x7ffffff0};
        std::memcpy(&s.records[R_BOX_OBJ], none, sizeof none);
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "an empty box", 0, 0, 0, 0, 0, 10, 0, 0);
        std::memcpy(&s.records[R_BOX_OBJ], huge, sizeof huge);
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "a box near the end of int32", 0, 0, 0, 0, 0, 10, 0, 0);
        std::memcpy(&s.records[R_BOX_OBJ], across, sizeof across);   // columns 0-3 x rows 0-2: (1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3) of the plane
        EXPECT_COUNTS(s.run(0, 0, 1, 2.5, 3.5), "a box across the top-left corner", 6, 0, 5, 1, 0, 10, 4, 2);
        // plane 1's box shrunk to column 4: it is read there only, so (3, 3) is no longer hidden
        Scene t = hand();
        const int32_t column[4] = {4, 2, 0, 2};
        std::memcpy(&t.records[RECORD + R_BOX_OBJ], column, sizeof column);
        EXPECT_COUNTS(t.run(0, 0, 1, 2.5, 3.5), "a hiding plane is read inside its box only", 12, 1, 8, 1, 2, 10, 4, 2);
    }
    SELFTEST_END("verify_selftest", "the 5 x 7 hand case, cos_min 0 and 1, keypoints that are not finite, instance counts, indices out of range, "
                                    "empty, clipped and huge boxes, a hiding plane's own box");
}
