// Stand-alone self-test of contour_math.h on the host, meant to be built with -fsanitize=address,undefined (make contour-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs edt_serial and step_serial -- the loops the kernels of mask_contour.hip carry out -- on buffers
// of exactly the input and output sizes, so that any index past them is an AddressSanitizer report.
//   1. a 5 x 5 field worked out by hand, without and with an occlusion edge
//   2. a four-pixel contour worked out by hand: e, the counts, sum e . e and the translation entries of the sums
//   3. the failure statuses and the refusals of both entry points (a refused job's indices would land outside the buffers)
//   4. a 40 x 72 patch (three tiles, the last one part full): the field against a naive loop over all seeds, one step against a naive double
//      loop over pixel(): equal counts, every sum within N 2^-52 sum |term|, the same pose from either set of sums to 1e-9, and the same
//      bytes whatever the workspaces held before
#include <cstring>
#include <vector>

#include "contour_math.h"
#include "selftest.h"

using namespace cp_contour;
using cp_icp::absd;
using cp_icp::R_BOX_OBJ;
using cp_icp::RECORD;

static uint32_t bits_of(float z) {
    uint32_t b;
    std::memcpy(&b, &z, sizeof b);
    return b;
}

struct Field {
    std::vector<uint16_t> planes, rows;
    std::vector<int32_t> status;
};

// jobs [(image, label)] over labels [images][H][W]; every buffer has exactly the size the call may touch
static Field field_of(const std::vector<uint8_t>& labels, int images, int H, int W, const std::vector<int32_t>& jobs, int G, unsigned char fill = 0xA5) {
    const int n = (int)jobs.size() / 2;
    Field f;
    f.planes.assign((size_t)n * H * W, 0x5A5A);
    f.rows.assign(edt_workspace_bytes(n, H, W) / sizeof(uint16_t), 0);
    std::memset(f.rows.data(), fill, f.rows.size() * sizeof(uint16_t));
    f.status.assign(n, -7);
    std::vector<uint8_t> flags((size_t)W);
    edt_serial(labels.data(), images, H, W, jobs.data(), n, G, f.planes.data(), f.status.data(), f.rows.data(), flags.data());
    return f;
}

struct Scene {
    int H, W;
    std::vector<uint32_t> planes;
    std::vector<int32_t> records;
    std::vector<uint16_t> fields;
    std::vector<double> cams, poses;
    double sample = 0.0;   // the sample offset
    Scene(int h, int w, double f, double cx, double cy)
        : H(h), W(w), planes((size_t)h * w, EMPTY), records(RECORD, -1), cams{f, f, cx, cy}, poses{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1000} {}
    void box(int x0, int y0, int x1, int y1) {
        const int32_t b[4] = {x0, y0, x1 - x0, y1 - y0};
        std::memcpy(&records[R_BOX_OBJ], b, sizeof b);
    }
    struct Out {
        int32_t status;
        double stats[4];
        std::vector<double> pose, partials;
    };
    Out run(int image, int plane, int field, int gate, int min_pixels = 4, int update = 1, unsigned char fill = 0xA5) const {
        const std::vector<int32_t> job = {image, plane, field, gate};
        Out o;
        o.pose = poses;
        o.partials.assign(workspace_bytes<Contour>(1, H, W) / sizeof(double), 0.0);
        std::memset(o.partials.data(), fill, o.partials.size() * sizeof(double));
        o.status = -1;
        for (double& s : o.stats) s = -1.0;
        const Contour::Args a = {planes.data(), records.data(), 1, H, W, fields.data(), 1, cams.data(), 1, job.data(), sample};
        step_serial<Contour>(a, 1, 1e-6, min_pixels, update, o.pose.data(), o.stats, &o.status, o.partials.data());
        return o;
    }
};

int main() {
    // 1. label 1 on the middle 3 x 3 of a 5 x 5 image, G = 2: its ring of eight is the seeds (the centre has no background neighbour)
    {
        std::vector<uint8_t> lab(25, 0);
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 3; ++x) lab[y * 5 + x] = 1;
        const uint16_t want[25] = {2, 1, 1, 1, 2, 1, 0, 0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1, 2, 1, 1, 1, 2};
        const Field f = field_of(lab, 1, 5, 5, {0, 1}, 2);
        EXPECT(f.status[0] == ST_OK && std::memcmp(f.planes.data(), want, sizeof want) == 0, "5 x 5: the field differs from the hand-worked one");
        const Field g1 = field_of(lab, 1, 5, 5, {0, 1}, 1);
        EXPECT(std::memcmp(g1.planes.data(), want, sizeof want) == 0, "5 x 5, G = 1: the clamp is 2, the largest value of the field");
        for (int y = 1; y <= 3; ++y) lab[y * 5 + 4] = 2;   // label 2 on the right: (3, 2) borders label 2, not background
        const Field f2 = field_of(lab, 1, 5, 5, {0, 1}, 2);
        const uint16_t row2[5] = {1, 0, 1, 1, 2};
        EXPECT(std::memcmp(f2.planes.data() + 10, row2, sizeof row2) == 0 && f2.planes[1 * 5 + 3] == 0 && f2.planes[3 * 5 + 3] == 0,
               "5 x 5 with an occlusion edge: row 2 is %d %d %d %d %d", f2.planes[10], f2.planes[11], f2.planes[12], f2.planes[13], f2.planes[14]);
        const Field none = field_of(lab, 1, 5, 5, {0, 7}, 2);
        bool all = true;
        for (uint16_t v : none.planes) all = all && v == 5;
        EXPECT(all, "a label that is not in the map gives G G + 1 everywhere");
        // 3a. refusals write nothing: their image index would land outside `lab`
        const Field bad = field_of(lab, 1, 5, 5, {1, 1, -1, 1, 0, 0, 0, 256, 0, 1}, 2);
        EXPECT(bad.status[0] == ST_REFUSED && bad.status[1] == ST_REFUSED && bad.status[2] == ST_REFUSED && bad.status[3] == ST_REFUSED && bad.status[4] == ST_OK,
               "refusals: %d %d %d %d %d", bad.status[0], bad.status[1], bad.status[2], bad.status[3], bad.status[4]);
        bool untouched = true;
        for (int k = 0; k < 100; ++k) untouched = untouched && bad.planes[k] == 0x5A5A && bad.rows[k] == 0xA5A5;
        EXPECT(untouched && std::memcmp(bad.planes.data() + 100, f2.planes.data(), 50) == 0, "a refused job's plane or rows were written");
    }
    // 2. 8 x 8, f = 1000, principal point (0, 0), depth 1000: X = x, Y = y.  The plane is hit on (3..4, 3..4): four contour pixels.  Label 1 on
    //    (4..5, 3..4), all four of them seeds.  e = (-1, -1/4), (-1/4, -1/4), (-1, 1/4), (-1/4, 1/4) at (3,3), (4,3), (3,4), (4,4);
    //    a = b = 1, so g_3 = ex and g_4 = ey: b_3 = 2.5, b_4 = 0; sum e . e = 2 (1 + 1/16) + 2 (1/8) = 2.375
    {
        Scene s(8, 8, 1000.0, 0.0, 0.0);
        std::vector<uint8_t> lab(64, 0);
        for (int y = 3; y <= 4; ++y)
            for (int x = 3; x <= 4; ++x) s.planes[y * 8 + x] = bits_of(1000.f), lab[y * 8 + x + 1] = 1;
        s.box(3, 3, 4, 4);
        s.fields = field_of(lab, 1, 8, 8, {0, 1}, 3).planes;
        const Camera cam = {1000.0, 1000.0, 0.0, 0.0};
        Terms t;
        const uint16_t* D = s.fields.data();
        EXPECT(D[3 * 8 + 3] == 1 && D[3 * 8 + 2] == 4 && D[2 * 8 + 3] == 2 && D[4 * 8 + 3] == 1 && D[3 * 8 + 4] == 0, "four pixels: the field around (3, 3)");
        const int kind = pixel(bits_of(1000.f), EMPTY, bits_of(1000.f), EMPTY, bits_of(1000.f), 1, 4, 0, 2, 1, 3, 3, cam, 3, t);
        EXPECT(kind == 2 && t.g[3] == -1.0 && t.g[4] == -0.25 && t.ee == 1.0625, "four pixels: (3, 3) gives kind %d, g %g %g, ee %g", kind, t.g[3], t.g[4], t.ee);
        EXPECT(pixel(bits_of(1000.f), bits_of(1.f), bits_of(1.f), bits_of(1.f), bits_of(1.f), 0, 0, 0, 0, 0, 3, 3, cam, 3, t) == 0, "an inner pixel is no contour");
        EXPECT(pixel(bits_of(1000.f), EMPTY, bits_of(1.f), bits_of(1.f), bits_of(1.f), 1, 10, 0, 2, 1, 3, 3, cam, 3, t) == 1, "a neighbour past the gate: unused");
        const Scene::Out o = s.run(0, 0, 0, 3);
        const double* p = o.partials.data();
        EXPECT(o.stats[0] == 4.0 && o.stats[2] == 4.0 && o.stats[3] == 2.375 && p[SUMS] == 4.0 && p[SUMS + 1] == 4.0 && p[N_A + N_B] == 2.375,
               "four pixels: used %g, contour %g, see %g", o.stats[0], o.stats[2], o.stats[3]);
        EXPECT(p[N_A + 3] == 2.5 && p[N_A + 4] == 0.0, "four pixels: b_3 = %g, b_4 = %g", p[N_A + 3], p[N_A + 4]);
        EXPECT(absd(p[15] - (2.0 / 1.0625 + 1.0)) < 1e-15 && absd(o.stats[1] * o.stats[1] - 2.375 / 4.0) < 1e-15, "four pixels: A_33 = %.17g, rms %g", p[15], o.stats[1]);
        Scene half = s;      // sampled at + 0.5 with the principal point at 0.5: the same rays, the same sums
        half.sample = 0.5, half.cams[2] = half.cams[3] = 0.5;
        EXPECT(half.run(0, 0, 0, 3).partials == o.partials, "four pixels: a sample offset is a shift of the principal point");
        // 3b. the statuses
        const Scene::Out few = s.run(0, 0, 0, 3, 5);
        EXPECT(few.status == ST_FEW && few.stats[0] == 4.0 && few.stats[2] == 4.0 && few.pose == s.poses, "5 pixels asked for: status %d", few.status);
        const Scene::Out tight = s.run(0, 0, 0, 1);     // D2 = 4 at (2, y) is past a gate of 1: the left two are unused
        EXPECT(tight.stats[0] == 2.0 && tight.stats[2] == 4.0 && tight.status == ST_FEW, "gate 1: %g of %g pixels used", tight.stats[0], tight.stats[2]);
        const int bad[8][4] = {{1, 0, 0, 3}, {-1, 0, 0, 3}, {0, 1, 0, 3}, {0, -5, 0, 3}, {0, 0, 1, 3}, {0, 0, -1, 3}, {0, 0, 0, 0}, {0, 0, 0, 256}};
        for (const auto& b : bad) {
            const Scene::Out r = s.run(b[0], b[1], b[2], b[3]);
            EXPECT(r.status == ST_REFUSED && r.stats[0] == 0.0 && r.stats[3] == 0.0 && r.pose == s.poses, "job (%d, %d, %d, %d): status %d", b[0], b[1], b[2],
                   b[3], r.status);
        }
        Scene e(8, 8, 1000.0, 0.0, 0.0);   // an empty record and a box outside the clipped image
        e.fields = s.fields;
        EXPECT(e.run(0, 0, 0, 3).status == ST_FEW, "an empty box has no pixels");
        e.box(0, 0, 0, 7);
        EXPECT(e.run(0, 0, 0, 3).status == ST_FEW, "a box in column 0 has no pixels");
        // a contour on its seeds: label 1 on (1..6, 2..4), the plane hit on (3..4, 2), in the label's upper edge.  D2 is 0 to the left and right
        // and 1 above and below: e = 0 at both pixels, which are counted and add nothing
        Scene z(8, 8, 1000.0, 0.0, 0.0);
        std::vector<uint8_t> wide(64, 0);
        for (int y = 2; y <= 4; ++y)
            for (int x = 1; x <= 6; ++x) wide[y * 8 + x] = 1;
        z.planes[2 * 8 + 3] = z.planes[2 * 8 + 4] = bits_of(1000.f);
        z.box(3, 2, 4, 2);
        z.fields = field_of(wide, 1, 8, 8, {0, 1}, 3).planes;
        const Scene::Out on = z.run(0, 0, 0, 3, 2);
        bool zero = true;
        for (int k = 0; k < SUMS; ++k) zero = zero && on.partials[k] == 0.0;
        EXPECT(on.stats[0] == 2.0 && on.stats[2] == 2.0 && on.stats[1] == 0.0 && zero && on.status == ST_SINGULAR && on.pose == z.poses,
               "on the seeds: used %g, status %d", on.stats[0], on.status);
    }
    // 4. a patch
    {
        const int H = 40, W = 72, G = 6;
        std::vector<uint8_t> lab((size_t)H * W, 0);
        Scene s(H, W, 300.0, 35.3, 19.6);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const double u = x - 33.0, v = y - 21.0;
                if (u * u / 900.0 + v * v / 260.0 < 1.0 && (x * 7 + y * 13) % 61 != 0) lab[(size_t)y * W + x] = 1;      // an ellipse with pinholes
                if ((x - 60) * (x - 60) + (y - 12) * (y - 12) < 120) lab[(size_t)y * W + x] = 2;                        // a disc over its right end
                const double a = x - 35.5, b = y - 19.0;
                if (a * a / 800.0 + b * b / 300.0 < 1.0 && (x * 5 + y * 11) % 47 != 0)
                    s.planes[(size_t)y * W + x] = bits_of((float)(1000.0 + 0.8 * a - 0.5 * b + 0.02 * a * b));
            }
        const Field f = field_of(lab, 1, H, W, {0, 1, 0, 2}, G);
        long long seeds = 0;
        for (int l = 1; l <= 2; ++l)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    int best = G * G + 1;
                    for (int sy = 0; sy < H; ++sy)
                        for (int sx = 0; sx < W; ++sx)
                            if (is_seed(lab.data(), H, W, sx, sy, l)) {
                                const int d = (sx - x) * (sx - x) + (sy - y) * (sy - y);
                                best = d < best ? d : best;
                                seeds += (x == 0 && y == 0);
                            }
                    EXPECT(f.planes[((size_t)(l - 1) * H + y) * W + x] == best, "patch: label %d, D2(%d, %d) = %d, naively %d", l, x, y,
                           f.planes[((size_t)(l - 1) * H + y) * W + x], best);
                }
        EXPECT(seeds > 150, "patch: %lld seeds", seeds);
        const Field f0 = field_of(lab, 1, H, W, {0, 1, 0, 2}, G, 0x00);
        EXPECT(f0.planes == f.planes, "patch: the field depends on what the workspace held");
        s.fields.assign(f.planes.begin(), f.planes.begin() + (size_t)H * W);
        s.box(0, 0, W - 1, H - 1);
        const Scene::Out o = s.run(0, 0, 0, G, 24);
        Job j;
        int fieldno, gate;
        const int32_t job[4] = {0, 0, 0, G};
        EXPECT(job_setup(job, s.records.data(), 1, 1, 1, H, W, j, fieldno, gate) && j.tiles == 3 && j.total == 38 * 70, "patch: %d tiles of %d pixels", j.tiles,
               j.total);
        const Camera cam = {s.cams[0], s.cams[1], s.cams[2], s.cams[3]};
        double naive[SUMS] = {0}, mag[SUMS] = {0};
        long long used = 0, contour = 0;
        for (int y = 1; y <= H - 2; ++y)
            for (int x = 1; x <= W - 2; ++x) {
                const size_t at = (size_t)y * W + x;
                const uint16_t* D = s.fields.data();
                Terms t;
                const int kind = pixel(s.planes[at], s.planes[at - 1], s.planes[at + 1], s.planes[at - W], s.planes[at + W], D[at], D[at - 1], D[at + 1],
                                       D[at - W], D[at + W], x, y, cam, G, t);
                contour += kind != 0;
                if (kind != 2) continue;
                double one[SUMS] = {0};
                add_terms(t, one);
                for (int k = 0; k < SUMS; ++k) naive[k] += one[k], mag[k] += absd(one[k]);
                ++used;
            }
        double sums[SUMS];
        long long got[2];
        add_tiles<2>(o.partials.data(), j.tiles, sums, got);
        const long long got_used = got[0], got_contour = got[1];
        EXPECT(got_used == used && got_contour == contour && used > 60 && contour > used && o.stats[0] == (double)used && o.stats[2] == (double)contour,
               "patch: %lld of %lld pixels, the naive loop has %lld of %lld", got_used, got_contour, used, contour);
        for (int k = 0; k < SUMS; ++k)
            EXPECT(absd(sums[k] - naive[k]) <= (double)used * 2.220446049250313e-16 * mag[k], "patch: sum %d is %.17g, serially %.17g", k, sums[k], naive[k]);
        double pose[12], st[4];
        for (int k = 0; k < 12; ++k) pose[k] = s.poses[k];
        const int code = solve_update(naive, used, contour, 1e-6, 24, 1, pose, st);
        EXPECT(code == ST_OK && o.status == ST_OK, "patch: status %d, from the naive sums %d", o.status, code);
        bool moved = false;
        for (int k = 0; k < 12; ++k) {
            EXPECT(absd(pose[k] - o.pose[k]) <= 1e-9 * (1.0 + absd(pose[k])), "patch: pose word %d is %.17g, from the naive sums %.17g", k, o.pose[k], pose[k]);
            moved = moved || o.pose[k] != s.poses[k];
        }
        EXPECT(moved, "patch: the pose did not move");
        const Scene::Out again = s.run(0, 0, 0, G, 24, 1, 0xFF), zero = s.run(0, 0, 0, G, 24, 1, 0x00);
        EXPECT(again.pose == o.pose && zero.pose == o.pose && std::memcmp(again.stats, o.stats, sizeof o.stats) == 0 &&
                   std::memcmp(zero.stats, o.stats, sizeof o.stats) == 0,
               "patch: the result depends on what the workspace held");
        EXPECT(std::memcmp(again.partials.data(), o.partials.data(), (size_t)j.tiles * PARTIAL<Contour> * sizeof(double)) == 0, "patch: the tile records differ");
        const Scene::Out eval = s.run(0, 0, 0, G, 24, 0);
        EXPECT(eval.status == ST_OK && eval.pose == s.poses && eval.stats[1] == o.stats[1], "patch: update = 0 writes stats and status only");
    }
    SELFTEST_END("contour_selftest", "a hand-worked 5 x 5 field and four-pixel contour, the statuses and refusals, a 40 x 72 patch against naive loops");
}
