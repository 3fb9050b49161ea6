// Stand-alone self-test of icp_math.h on the host, meant to be built with -fsanitize=address,undefined (make icp-selftest) and run on the CPU.
// It is never loaded into Python.  It runs step_serial -- the loop the kernels of depth_icp.hip carry out -- on buffers of exactly the input and
// output sizes, so that any index past them is an AddressSanitizer report.
//   1. a fronto-parallel quad worked out by hand: 48 pixels, n = (0, 0, 1), r = 2, J = (p_y, -p_x, 0, 0, 0, 1); the matrix is singular
//   2. the two failure statuses and the three refusals
//   3. one step on a smooth 40 x 72 patch with holes (three tiles, the last one part full) against a naive double loop over pixel(): equal
//      counts, every sum within N 2^-52 sum |term| of the serial sum, the same pose from either set of sums to 1e-9, an orthonormal rotation,
//      and the same bytes whatever the workspace held before
#include <cstring>
#include <vector>

#include "icp_math.h"
#include "selftest.h"

using namespace cp_icp;

static uint32_t bits_of(float z) {
    uint32_t b;
    std::memcpy(&b, &z, sizeof b);
    return b;
}

struct Scene {
    int H, W;
    std::vector<uint32_t> planes;
    std::vector<int32_t> records;
    std::vector<float> depth;
    std::vector<double> cams, poses;
    Scene(int h, int w, double f, float sensor)
        : H(h), W(w), planes((size_t)h * w, EMPTY), records(RECORD, -1), depth((size_t)h * w, sensor), cams{f, f, w / 2.0 - 0.5, h / 2.0 - 0.5},
          poses{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1000} {}
    void box(int x0, int y0, int x1, int y1) {
        const int32_t b[4] = {x0, y0, x1 - x0, y1 - y0};
        std::memcpy(&records[R_BOX_OBJ], b, sizeof b);
    }
    struct Out {
        int32_t status;
        double stats[4];
        std::vector<double> pose, partials;
    };
    // one job into buffers of exactly the sizes the step may touch; fill: what the workspace holds before
    Out run(int image, int plane, double gate, int min_pixels = 8, double damping = 1e-6, int update = 1, unsigned char fill = 0xA5, int images = 1,
            int nplanes = 1) const {
        const std::vector<int32_t> job = {image, plane, 777, -777};
        const std::vector<double> gates(1, gate);
        Out o;
        o.pose = poses;
        o.partials.assign(workspace_bytes<Depth>(1, H, W) / sizeof(double), 0.0);
        std::memset(o.partials.data(), fill, o.partials.size() * sizeof(double));
        o.status = -1;
        for (double& s : o.stats) s = -1.0;
        const Depth::Args a = {planes.data(), records.data(), nplanes, H, W, depth.data(), cams.data(), images, job.data(), gates.data(), 0.75};
        step_serial<Depth>(a, 1, damping, min_pixels, update, o.pose.data(), o.stats, &o.status, o.partials.data());
        return o;
    }
};

int main() {
    // 1. 12 x 16, f = 1000, principal point (7.5, 5.5): depth 1000 over columns 3-12 x rows 2-9, the sensor 2 mm behind it.  The pixels with four
    //    hit neighbours are columns 4-11 x rows 3-8: 48.  p_R - p_L = (2, 0, 0), p_D - p_U = (0, 2, 0): n = (0, 0, 1), r = 2, J = (p_y, -p_x, 0, 0, 0, 1)
    //    with p_x = x - 7.5, p_y = y - 5.5 (z / f = 1).  sum p_y^2 = 8 * 2 (0.25 + 2.25 + 6.25) = 140, sum p_x^2 = 6 * 2 (0.25 + 2.25 + 6.25 + 12.25) = 252.
    {
        Scene s(12, 16, 1000.0, 1002.f);
        for (int y = 2; y <= 9; ++y)
            for (int x = 3; x <= 12; ++x) s.planes[(size_t)y * 16 + x] = bits_of(1000.f);
        s.box(3, 2, 12, 9);
        const Scene::Out o = s.run(0, 0, 40.0);
        const double* p = o.partials.data();
        EXPECT(o.stats[0] == 48.0 && o.stats[1] == 2.0, "quad: %g pixels, rms %g", o.stats[0], o.stats[1]);
        EXPECT(p[0] == 140.0 && p[6] == 252.0 && p[1] == 0.0 && p[20] == 48.0 && p[N_A + 5] == 96.0 && p[N_A + N_B] == 192.0 && p[SUMS] == 48.0,
               "quad: sums %g %g %g %g %g %g %g", p[0], p[6], p[1], p[20], p[N_A + 5], p[N_A + N_B], p[SUMS]);
        EXPECT(p[11] == 0.0 && p[15] == 0.0 && p[18] == 0.0, "quad: the third to fifth diagonal entries are %g %g %g", p[11], p[15], p[18]);
        EXPECT(o.status == ST_SINGULAR && o.pose == s.poses, "quad: status %d (a zero pivot is ST_SINGULAR and leaves the pose)", o.status);
        // 2. the failure statuses: too few pixels; a sensor outside the gate; refusals read nothing (their indices would land outside the buffers)
        const Scene::Out few = s.run(0, 0, 40.0, 49);
        EXPECT(few.status == ST_FEW && few.stats[0] == 48.0 && few.pose == s.poses, "49 pixels asked for: status %d", few.status);
        const Scene::Out gated = s.run(0, 0, 2.0);
        EXPECT(gated.status == ST_FEW && gated.stats[0] == 0.0 && gated.stats[1] == 0.0, "gate 2 mm: status %d, %g pixels", gated.status, gated.stats[0]);
        const int bad[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -5}};
        for (const auto& b : bad) {
            const Scene::Out r = s.run(b[0], b[1], 40.0);
            EXPECT(r.status == ST_REFUSED && r.stats[0] == 0.0 && r.stats[3] == 0.0 && r.pose == s.poses, "job (%d, %d): status %d", b[0], b[1], r.status);
        }
        const double gates[3] = {0.0, -1.0, __builtin_nan("")};
        for (double g : gates) EXPECT(s.run(0, 0, g).status == ST_REFUSED, "gate %g is refused", g);
        Scene e(12, 16, 1000.0, 1002.f);   // an empty record and a box outside the clipped image
        EXPECT(e.run(0, 0, 40.0).status == ST_FEW, "an empty box has no pixels");
        e.box(0, 0, 0, 11);
        EXPECT(e.run(0, 0, 40.0).status == ST_FEW, "a box in column 0 has no pixels");
    }
    // 3. a smooth patch
    {
        const int H = 40, W = 72;
        Scene s(H, W, 300.0, 0.f);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const double u = x - 36.0, v = y - 20.0;
                const double z = 1000.0 + 0.8 * u - 0.5 * v + 0.02 * u * v + 0.015 * u * u + 0.03 * v * v;
                if ((x * 7 + y * 13) % 29 != 0) s.planes[(size_t)y * W + x] = bits_of((float)z);
                s.depth[(size_t)y * W + x] = (x * 5 + y * 3) % 31 == 0 ? 0.f : (float)(z + 3.0 + 0.02 * u - 0.03 * v);
            }
        s.box(0, 0, W - 1, H - 1);
        const Scene::Out o = s.run(0, 0, 40.0);
        Job j;
        const int32_t job[4] = {0, 0, 0, 0};
        EXPECT(job_setup(job, 40.0, s.records.data(), 1, 1, H, W, j) && j.tiles == 3 && j.total == 38 * 70, "patch: %d tiles of %d pixels", j.tiles, j.total);
        const Camera cam = {s.cams[0], s.cams[1], s.cams[2], s.cams[3]};
        double naive[SUMS] = {0}, mag[SUMS] = {0};
        long long count = 0;
        for (int y = 1; y <= H - 2; ++y)
            for (int x = 1; x <= W - 2; ++x) {
                const size_t at = (size_t)y * W + x;
                Terms t;
                if (!pixel(s.planes[at], s.planes[at - 1], s.planes[at + 1], s.planes[at - W], s.planes[at + W], s.depth[at], x, y, cam, 40.0, 30.0, t)) continue;
                double one[SUMS] = {0};
                add_terms(t, one);
                for (int k = 0; k < SUMS; ++k) naive[k] += one[k], mag[k] += absd(one[k]);
                ++count;
            }
        double sums[SUMS];
        long long got;
        add_tiles<1>(o.partials.data(), j.tiles, sums, &got);
        EXPECT(got == count && count > 2000 && o.stats[0] == (double)count, "patch: %lld pixels, the naive loop has %lld", got, count);
        for (int k = 0; k < SUMS; ++k)
            EXPECT(absd(sums[k] - naive[k]) <= (double)count * 2.220446049250313e-16 * mag[k], "patch: sum %d is %.17g, serially %.17g", k, sums[k], naive[k]);
        double pose[12], st[4];
        for (int k = 0; k < 12; ++k) pose[k] = s.poses[k];
        const int code = solve_update(naive, count, 1e-6, 8, 1, pose, st);
        EXPECT(code == ST_OK && o.status == ST_OK, "patch: status %d, from the naive sums %d", o.status, code);
        bool moved = false;
        for (int k = 0; k < 12; ++k) {
            EXPECT(absd(pose[k] - o.pose[k]) <= 1e-9 * (1.0 + absd(pose[k])), "patch: pose word %d is %.17g, from the naive sums %.17g", k, o.pose[k], pose[k]);
            moved = moved || o.pose[k] != s.poses[k];
        }
        EXPECT(moved && o.stats[3] > 1.0 && o.stats[3] < 10.0, "patch: the sensor is about 3 mm behind the render, |v| = %g", o.stats[3]);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double ra[3] = {o.pose[4 * a], o.pose[4 * a + 1], o.pose[4 * a + 2]}, rb[3] = {o.pose[4 * b], o.pose[4 * b + 1], o.pose[4 * b + 2]};
                EXPECT(absd(dot3(ra, rb) - (a == b ? 1.0 : 0.0)) < 1e-14, "patch: R R^T [%d][%d] = %.17g", a, b, dot3(ra, rb));
            }
        const Scene::Out again = s.run(0, 0, 40.0, 8, 1e-6, 1, 0xFF), zero = s.run(0, 0, 40.0, 8, 1e-6, 1, 0x00);
        EXPECT(again.pose == o.pose && zero.pose == o.pose && std::memcmp(again.stats, o.stats, sizeof o.stats) == 0 &&
                   std::memcmp(zero.stats, o.stats, sizeof o.stats) == 0,
               "patch: the result depends on what the workspace held");
        EXPECT(std::memcmp(again.partials.data(), o.partials.data(), (size_t)j.tiles * PARTIAL<Depth> * sizeof(double)) == 0, "patch: the tile records differ");
        const Scene::Out eval = s.run(0, 0, 40.0, 8, 1e-6, 0);
        EXPECT(eval.status == ST_OK && eval.pose == s.poses && eval.stats[3] == o.stats[3], "patch: update = 0 writes stats and status only");
    }
    SELFTEST_END("icp_selftest", "a hand-worked quad, the failure statuses and refusals, one step on a 40 x 72 patch against a naive loop");
}
