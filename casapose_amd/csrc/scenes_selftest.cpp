// Stand-alone self-test of scene_math.h on the host, meant to be built with -fsanitize=address,undefined (make scenes-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs render_image_serial -- the loop cp_render_scenes_host_f32 runs per record -- into buffers of
// exactly the output sizes, so that any index past an image is an AddressSanitizer report, and checks what can be known in closed form: the
// label of a pixel on an object's optical axis, the background elsewhere, the order of two overlapping objects, the counts against the label
// map, the one-hot rows, the value range, the noise-free image being a function of the record alone and the noise a function of (seed, pixel).
// Cases: an odd width, an object cut by the image border, an object behind the camera plane, two objects overlapping, oc = 1 and oc = 13 (the
// largest the tests use).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scene_math.h"
#include "selftest.h"

using namespace cp_scene;

static const double FX = 572.4114, FY = 573.57043, CX = 325.2611, CY = 242.04899;

struct Object {
    double u, v, z, axes[3], colour[3], angle;   // the centre projects to frame pixel (u, v) at depth z
};

static std::vector<double> make_record(int oc, int hc, int wc, uint64_t seed, const std::vector<Object>& objects) {
    std::vector<double> rec(record_words(oc), 0.0);
    rec[W_HC] = hc; rec[W_WC] = wc; rec[W_FX] = FX; rec[W_FY] = FY; rec[W_CX] = CX; rec[W_CY] = CY;
    __builtin_memcpy(&rec[W_SEED], &seed, sizeof seed);
    rec[W_COUNT] = (double)objects.size();
    for (size_t o = 0; o < objects.size(); ++o) {
        double* obj = &rec[HEADER + OBJECT * o];
        const Object& ob = objects[o];
        const double c = std::cos(ob.angle), s = std::sin(ob.angle);   // a rotation about z, then about x
        const double Rz[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, Rx[9] = {1, 0, 0, 0, c, -s, 0, s, c};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) obj[O_R + 3 * i + j] = Rx[3 * i] * Rz[j] + Rx[3 * i + 1] * Rz[3 + j] + Rx[3 * i + 2] * Rz[6 + j];
        obj[O_T] = (ob.u - CX) * ob.z / FX;
        obj[O_T + 1] = (ob.v - CY) * ob.z / FY;
        obj[O_T + 2] = ob.z;
        for (int i = 0; i < 3; ++i) { obj[O_INV + i] = 1.0 / ob.axes[i]; obj[O_COLOUR + i] = ob.colour[i]; }
    }
    return rec;
}

struct Image {
    int H, W, oc;
    std::vector<float> img, seg;
    std::vector<uint8_t> label;
    std::vector<int32_t> counts;
    int at(int y, int x) const { return label[(size_t)y * W + x]; }
};

static Image render(const std::vector<double>& rec, int oc, int H, int W, int noise) {
    Image r{H, W, oc, std::vector<float>((size_t)H * W * 3), std::vector<float>((size_t)H * W * (oc + 1)), std::vector<uint8_t>((size_t)H * W),
            std::vector<int32_t>(oc)};
    std::vector<double> der((size_t)DERIVED * oc);
    render_image_serial(rec.data(), oc, H, W, noise, der.data(), r.img.data(), r.label.data(), r.seg.data(), r.counts.data());
    return r;
}

// what holds for every image: labels within the object count, counts and one-hot rows equal to the label map, values in [-1, 1]
static void check_consistent(const char* name, const Image& r, int n) {
    std::vector<int32_t> counted(r.oc, 0);
    bool labels = true, onehot = true, range = true;
    for (size_t p = 0; p < r.label.size(); ++p) {
        const int lab = r.label[p];
        labels = labels && lab <= n;
        if (lab > 0 && lab <= r.oc) counted[lab - 1] += 1;
        for (int k = 0; k <= r.oc; ++k) onehot = onehot && r.seg[p * (r.oc + 1) + k] == (k == lab ? 1.f : 0.f);
        for (int c = 0; c < 3; ++c) range = range && r.img[3 * p + c] >= -1.f && r.img[3 * p + c] <= 1.f;
    }
    EXPECT(labels && onehot && range, "%s: labels %d, one-hot rows %d, value range %d", name, (int)labels, (int)onehot, (int)range);
    for (int o = 0; o < r.oc; ++o) EXPECT(counted[o] == r.counts[o], "%s: counts[%d] = %d, the label map has %d", name, o, r.counts[o], counted[o]);
}

static const Object UNIT = {0, 0, 900.0, {50.0, 40.0, 60.0}, {0.8, 0.5, 0.2}, 0.3};
static Object object_at(double u, double v, double z, double scale = 1.0) {
    Object o = UNIT;
    o.u = u; o.v = v; o.z = z;
    o.angle = 0.3 + 0.001 * z;
    for (double& a : o.axes) a *= scale;
    return o;
}

int main() {
    int cases = 0;
    // 1. an odd width, oc = 1: the object's optical axis hits it, a far corner is background; noise-free twice gives the same bits
    {
        const int H = 21, W = 37, hc = 100, wc = 200;
        const std::vector<double> rec = make_record(1, hc, wc, 7u, {object_at(wc + 18.5, hc + 10.5, 900.0, 0.15)});
        const Image a = render(rec, 1, H, W, 0), b = render(rec, 1, H, W, 0), c = render(rec, 1, H, W, 1);
        ++cases;
        check_consistent("odd width", a, 1);
        check_consistent("odd width, noisy", c, 1);
        EXPECT(a.at(10, 18) == 1 && a.at(0, 0) == 0 && a.at(H - 1, W - 1) == 0, "odd width: centre %d, corners %d %d", a.at(10, 18), a.at(0, 0), a.at(H - 1, W - 1));
        EXPECT(a.img == b.img && a.label == b.label && a.label == c.label, "odd width: two renderings differ");
        // the centre pixel looks down the axis: its normal is along the ray, its shade is 0.55 + 0.45 |n_z| of the rotated ellipsoid, within [0.55, 1]
        const float v = a.img[3 * (10 * W + 18)];
        EXPECT(v >= (float)(0.8 * 0.55 * 2 - 1) - 1e-6f && v <= (float)(0.8 * 2 - 1) + 1e-6f, "odd width: centre value %g", (double)v);
        // the noise is small, not zero, and a function of (seed, pixel): another seed changes it, the same seed does not
        const Image c2 = render(rec, 1, H, W, 1), d = render(make_record(1, hc, wc, 8u, {object_at(wc + 18.5, hc + 10.5, 900.0, 0.15)}), 1, H, W, 1);
        double worst = 0.0;
        int moved = 0;
        for (size_t i = 0; i < a.img.size(); ++i) {
            worst = std::fmax(worst, std::fabs((double)c.img[i] - (double)a.img[i]));
            moved += c.img[i] != d.img[i];
        }
        EXPECT(c.img == c2.img && worst > 0.01 && worst < 0.5 && moved > (int)a.img.size() / 2, "odd width: noise max %g, %d values moved by the seed", worst, moved);
    }
    // 2. an object cut by the image border: its centre lies outside the crop, part of it inside
    {
        const int H = 24, W = 40, hc = 50, wc = 60;
        const Image a = render(make_record(1, hc, wc, 1u, {object_at(wc - 10.0, hc + 12.0, 700.0, 0.4)}), 1, H, W, 1);
        ++cases;
        check_consistent("border", a, 1);
        EXPECT(a.at(12, 0) == 1 && a.at(12, W - 1) == 0 && a.counts[0] > 0 && a.counts[0] < H * W / 2, "border: edge %d, far side %d, %d pixels", a.at(12, 0),
               a.at(12, W - 1), a.counts[0]);
    }
    // 3. an object behind the camera plane (both intersections have s <= 0) beside one in front: only the one in front is drawn
    {
        const int H = 32, W = 32, hc = 0, wc = 0;
        Object behind = object_at(16.0, 16.0, -900.0), front = object_at(16.0, 16.0, 1000.0, 0.2);
        const Image a = render(make_record(2, hc, wc, 2u, {behind, front}), 2, H, W, 0);
        ++cases;
        check_consistent("behind", a, 2);
        EXPECT(a.counts[0] == 0 && a.counts[1] > 0 && a.at(16, 16) == 2 && a.at(0, 0) == 0, "behind: counts %d %d, centre %d", a.counts[0], a.counts[1], a.at(16, 16));
    }
    // 4. two objects overlapping: the nearer one wins whichever index it has
    {
        const int H = 48, W = 64, hc = 200, wc = 280;
        const Object near_ = object_at(wc + 30.0, hc + 24.0, 700.0, 0.3), far_ = object_at(wc + 36.0, hc + 24.0, 1000.0, 0.5);
        const Image a = render(make_record(2, hc, wc, 3u, {near_, far_}), 2, H, W, 1), b = render(make_record(2, hc, wc, 3u, {far_, near_}), 2, H, W, 1);
        ++cases;
        check_consistent("overlap", a, 2);
        check_consistent("overlap, swapped", b, 2);
        EXPECT(a.at(24, 30) == 1 && b.at(24, 30) == 2 && a.counts[0] == b.counts[1] && a.counts[1] == b.counts[0] && a.counts[1] > 0,
               "overlap: %d / %d at the near centre, counts %d %d and %d %d", a.at(24, 30), b.at(24, 30), a.counts[0], a.counts[1], b.counts[0], b.counts[1]);
        // the far object is larger on screen than what stays visible of it: it is occluded somewhere
        const Image alone = render(make_record(2, hc, wc, 3u, {object_at(0, 0, -900.0), far_}), 2, H, W, 0);
        EXPECT(alone.counts[1] > a.counts[1], "overlap: the far object shows %d pixels alone and %d behind the near one", alone.counts[1], a.counts[1]);
    }
    // 5. oc = 13 at the full frame's width, a record with fewer objects than oc, and a record whose count word is not a count
    {
        const int oc = 13, H = 30, W = 640;
        std::vector<Object> objects;
        for (int o = 0; o < oc; ++o) objects.push_back(object_at(40.0 + 45.0 * o, 15.0, 800.0 + 20.0 * o, 0.4));
        const Image a = render(make_record(oc, 0, 0, 4u, objects), oc, H, W, 1);
        ++cases;
        check_consistent("oc 13", a, oc);
        for (int o = 0; o < oc; ++o) EXPECT(a.counts[o] > 0 && a.at(15, 40 + 45 * o) == o + 1, "oc 13: object %d has %d pixels", o, a.counts[o]);
        objects.resize(5);
        const Image few = render(make_record(oc, 0, 0, 4u, objects), oc, H, W, 1);
        check_consistent("oc 13, 5 objects", few, 5);
        EXPECT(few.counts[4] > 0 && few.counts[5] == 0, "oc 13, 5 objects: counts %d %d", few.counts[4], few.counts[5]);
        std::vector<double> bad = make_record(oc, 0, 0, 4u, objects);
        for (double word : {-1.0, 14.0, (double)NAN, 1e300}) {
            bad[W_COUNT] = word;
            const Image none = render(bad, oc, H, W, 0);
            check_consistent("oc 13, bad count", none, 0);
        }
    }
    SELFTEST_END("scenes_selftest", "%d scenes: an odd width, an object cut by the border, one behind the camera, two overlapping, oc = 1 and 13", cases);
}
