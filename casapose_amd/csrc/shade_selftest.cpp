// Stand-alone self-test of shade_math.h on the host, meant to be built with -fsanitize=address,undefined (make shade-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs render_shaded_serial -- the loop cp_render_shaded_host_f32 runs -- into buffers of exactly the
// output and workspace sizes, so that any index past them is an AddressSanitizer report, and checks what can be known in closed form: the label
// map against mask_math.h's render_serial on the same scene, the shade of a square facing the camera, the albedo at a pixel the vertex colours
// fix, the keys of covered and empty pixels.
// Cases: W = 37, a frame with zero instances, a vertex behind the near plane, a quad larger than the image, an invalid object index, null
// colors, null background, null depth.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "selftest.h"
#include "shade_math.h"

using namespace cp_shade;

static const double F = 100.0;   // focal length; the principal point is given per case

struct Instance {
    int obj, label;
    double tx, ty, tz;   // identity rotation
};

struct Case {
    int objects, Vmax, Tmax, frames, imax, H, W;
    std::vector<float> verts, flat;
    std::vector<uint8_t> colors;
    std::vector<int32_t> vert_counts, faces, face_counts, inst_counts, inst_obj, inst_label;
    std::vector<double> cams, poses, lights;
    std::vector<float> img, depth;
    std::vector<uint8_t> label, mask_label, background;
    std::vector<int32_t> dropped;
    std::vector<uint64_t> keys;
    size_t at(int f, int i, int j) const { return ((size_t)f * H + i) * W + j; }
};

// object 0: the square [-1, 1]^2 in the plane z = 0 as two triangles of opposite winding; object 1: the same square and a triangle that reaches
// 50 behind it.  Vertex colours: 255 red at vertex 0, 255 green at 1, 255 blue at 2, white at 3.
static Case make_case(int frames, int imax, int H, int W, double cx, double cy, const std::vector<std::vector<Instance>>& inst) {
    Case s{2, 6, 3, frames, imax, H, W};
    s.verts.assign((size_t)s.objects * s.Vmax * 3, 0.f);
    s.colors.assign((size_t)s.objects * s.Vmax * 3, 0);
    s.faces.assign((size_t)s.objects * s.Tmax * 3, 0);
    const float sq[5][3] = {{-1, -1, 0}, {1, -1, 0}, {1, 1, 0}, {-1, 1, 0}, {0, 0, -50}};
    const uint8_t col[5][3] = {{255, 0, 0}, {0, 255, 0}, {0, 0, 255}, {255, 255, 255}, {9, 9, 9}};
    for (int o = 0; o < 2; ++o)
        for (int v = 0; v < 5; ++v)
            for (int c = 0; c < 3; ++c) {
                s.verts[((size_t)o * s.Vmax + v) * 3 + c] = sq[v][c];
                s.colors[((size_t)o * s.Vmax + v) * 3 + c] = col[v][c];
            }
    const int32_t f[3][3] = {{0, 1, 2}, {0, 3, 2}, {0, 1, 4}};
    for (int o = 0; o < 2; ++o)
        for (int t = 0; t < 3; ++t)
            for (int c = 0; c < 3; ++c) s.faces[((size_t)o * s.Tmax + t) * 3 + c] = f[t][c];
    s.vert_counts = {4, 5};
    s.face_counts = {2, 3};
    s.flat = {0.25f, 0.5f, 0.75f, 0.9f, 0.1f, 0.3f};
    s.inst_counts.assign(frames, 0);
    s.inst_obj.assign((size_t)frames * imax, 0);
    s.inst_label.assign((size_t)frames * imax, 0);
    s.poses.assign((size_t)frames * imax * 12, 0.0);
    for (int fr = 0; fr < frames; ++fr) {
        s.cams.insert(s.cams.end(), {F, F, cx, cy});
        s.lights.insert(s.lights.end(), {0.0, 0.0, -1.0, 0.25, 0.5, 0.0, 3.0, 5.0});
        const uint64_t seed = 1234567u + fr;
        __builtin_memcpy(&s.lights[(size_t)fr * FRAME_WORDS + F_SEED], &seed, sizeof seed);
        s.inst_counts[fr] = (int32_t)inst[fr].size();
        for (size_t k = 0; k < inst[fr].size(); ++k) {
            const size_t slot = (size_t)fr * imax + k;
            s.inst_obj[slot] = inst[fr][k].obj;
            s.inst_label[slot] = inst[fr][k].label;
            double* P = &s.poses[slot * 12];
            P[0] = P[5] = P[10] = 1.0;
            P[3] = inst[fr][k].tx, P[7] = inst[fr][k].ty, P[11] = inst[fr][k].tz;
        }
    }
    return s;
}

// renders into buffers of exactly the output sizes; then the label map of mask_math.h's renderer on the same scene
static void render(Case& s, double near, double far, double offset, bool colors, bool background, bool depth, int noise) {
    const size_t px = (size_t)s.frames * s.H * s.W;
    s.img.assign(px * 3, 77.f);
    s.label.assign(px, 77);
    s.depth.assign(depth ? px : 0, 77.f);
    s.dropped.assign(s.frames, 77);
    s.keys.assign(workspace_bytes(s.frames, s.H, s.W) / sizeof(uint64_t), 77);
    s.background.assign(background ? px * 3 : 0, 51);   // 51 / 255 = 0.2
    const Scene sc = {s.verts.data(), s.vert_counts.data(), s.Vmax, s.faces.data(), s.face_counts.data(), s.Tmax, s.objects, s.cams.data(),
                      s.inst_counts.data(), s.inst_obj.data(), s.inst_label.data(), s.poses.data(), s.imax, s.H, s.W, near, cp_mask::sample_origin(offset),
                      colors ? s.colors.data() : nullptr, s.flat.data()};
    render_shaded_serial(sc, s.frames, far, s.lights.data(), background ? s.background.data() : nullptr, noise, s.img.data(), s.label.data(),
                         depth ? s.depth.data() : nullptr, s.dropped.data(), s.keys.data());
    s.mask_label.assign(px, 78);
    std::vector<int32_t> records((size_t)s.frames * s.imax * cp_mask::RECORD);
    std::vector<uint32_t> planes(cp_mask::workspace_bytes(s.frames, s.imax, s.H, s.W) / sizeof(uint32_t));
    cp_mask::render_serial(s.verts.data(), s.vert_counts.data(), s.Vmax, s.faces.data(), s.face_counts.data(), s.Tmax, s.objects, s.cams.data(),
                           s.inst_counts.data(), s.inst_obj.data(), s.inst_label.data(), s.poses.data(), s.frames, s.imax, s.H, s.W, near, far, offset,
                           s.mask_label.data(), records.data(), planes.data());
}

static void check_common(const char* name, const Case& s) {
    bool same = true, keys = true, range = true;
    for (size_t p = 0; p < s.label.size(); ++p) {
        same = same && s.label[p] == s.mask_label[p];
        keys = keys && (s.keys[p] == KEY_EMPTY) == (s.label[p] == 0);
        for (int c = 0; c < 3; ++c) range = range && s.img[3 * p + c] >= -1.f && s.img[3 * p + c] <= 1.f;
        if (!s.depth.empty()) keys = keys && (s.depth[p] == 0.f) == (s.label[p] == 0);
    }
    EXPECT(same, "%s: the label map is not mask_math.h's", name);
    EXPECT(keys, "%s: a key or a depth disagrees with the label map", name);
    EXPECT(range, "%s: a channel outside [-1, 1]", name);
}

static bool close(float got, double want) { return std::fabs((double)got - want) <= 2.4e-7; }

int main() {
    int cases = 0;
    // 1. W = 37, three frames with 0, 1 and 2 instances, vertex colours, a supplied background, depth.  The square at depth 10 covers columns
    //    8 .. 27 and rows 0 .. 19 (masks_selftest.cpp); facing the camera under l = (0, 0, -1) it shades with ambient + diffuse = 0.75.
    {
        Case s = make_case(3, 2, 21, 37, 18.0, 10.0, {{}, {{0, 255, 0, 0, 10}}, {{0, 5, 0, 0, 10}, {0, 9, 0.5, 0, 8}}});
        render(s, 1.0, 100.0, 0.5, true, true, true, 0);
        ++cases;
        check_common("odd width", s);
        bool empty = true;
        for (int p = 0; p < s.H * s.W; ++p) empty = empty && s.label[p] == 0 && close(s.img[3 * p], 0.2 * 2 - 1) && s.keys[p] == KEY_EMPTY;
        EXPECT(empty && s.dropped[0] == 0, "zero instances: the frame is not the background alone");
        // the sample (8.5, 0.5) is the square's point (-0.95, -0.95): bilinear in the triangle (0, 3, 2) or (0, 1, 2); on the diagonal x = y both
        // give lambda_0 = 0.975, lambda_2 = 0.025: red 0.975, green 0, blue 0.025, times 0.75
        const size_t p = s.at(1, 0, 8);
        EXPECT(s.label[p] == 255 && close(s.depth[p], 10.0) && close(s.img[3 * p], 0.975 * 0.75 * 2 - 1) && close(s.img[3 * p + 1], -1.0) &&
                   close(s.img[3 * p + 2], 0.025 * 0.75 * 2 - 1),
               "vertex colours: label %d depth %g rgb %.9g %.9g %.9g", s.label[p], s.depth[p], s.img[3 * p], s.img[3 * p + 1], s.img[3 * p + 2]);
        EXPECT((s.keys[p] >> 32) == 0x41200000u && ((s.keys[p] >> 24) & 255) == 0 && (s.keys[p] & 0xffffff) == 0, "the diagonal pixel's key %llx",
               (unsigned long long)s.keys[p]);   // depth 10.0f, instance 0, and of the two triangles that share the diagonal the lower index
        EXPECT(s.label[s.at(2, 10, 24)] == 9 && close(s.depth[s.at(2, 10, 24)], 8.0), "overlap: the nearer square does not win");
    }
    // 2. null colors, null background, null depth, noise: flat colours, the wave, 16 threads' worth of Philox per pixel; W a multiple of 4
    {
        Case s = make_case(1, 1, 21, 40, 18.0, 10.0, {{{0, 1, 0, 0, 10}}});
        render(s, 1.0, 100.0, 0.0, false, false, false, 0);
        ++cases;
        check_common("flat colour", s);
        const size_t p = s.at(0, 10, 18), b = s.at(0, 10, 35);
        EXPECT(close(s.img[3 * p], 0.25 * 0.75 * 2 - 1) && close(s.img[3 * p + 1], 0.5 * 0.75 * 2 - 1) && close(s.img[3 * p + 2], 0.75 * 0.75 * 2 - 1),
               "flat colour: %.9g %.9g %.9g", s.img[3 * p], s.img[3 * p + 1], s.img[3 * p + 2]);
        const double wave = 0.35 + (0.1 * std::sin((35 + 5.0 + 0.5) / 37.0)) * std::cos((10 + 3.0 + 0.5) / 53.0);
        EXPECT(s.label[b] == 0 && close(s.img[3 * b], wave * 2 - 1) && s.img[3 * b] == s.img[3 * b + 2], "the wave: %.9g against %.9g", s.img[3 * b], wave * 2 - 1);
        std::vector<float> clean = s.img;
        render(s, 1.0, 100.0, 0.0, false, false, false, 1);
        check_common("noise", s);
        double worst = 0.0, moved = 0.0;
        for (size_t q = 0; q < clean.size(); ++q) {
            const double d = std::fabs((double)clean[q] - s.img[q]);
            worst = d > worst ? d : worst, moved += d > 0.0;
        }
        EXPECT(worst < 0.3 && moved > 0.9 * clean.size(), "noise: largest change %g, %g of %zu channels moved", worst, moved, clean.size());
    }
    // 3. a vertex behind the near plane (object 1's third triangle, dropped whole and counted per instance that draws it), two identical
    //    instances (the lower index wins), an instance naming object 7 and one with label 256 (they render nothing and drop nothing)
    {
        Case s = make_case(2, 4, 24, 40, 20.0, 12.0, {{{1, 7, 0, 0, 10}, {1, 9, 0, 0, 10}, {7, 3, 0, 0, 10}, {0, 256, 0, 0, 10}}, {{0, 4, 0, 0, 10}, {0, 6, 0, 0, 300}}});
        render(s, 1.0, 100.0, 0.5, true, false, true, 1);
        ++cases;
        check_common("behind / invalid", s);
        EXPECT(s.dropped[0] == 2 && s.dropped[1] == 0 && s.label[s.at(0, 12, 20)] == 7, "behind / tie: dropped %d %d, label %d", s.dropped[0], s.dropped[1],
               s.label[s.at(0, 12, 20)]);
        EXPECT(((s.keys[s.at(0, 12, 20)] >> 24) & 255) == 0, "two identical instances: instance %d wins", (int)((s.keys[s.at(0, 12, 20)] >> 24) & 255));
    }
    // 4. a quad larger than the image: every pixel covered, one key each
    {
        Case s = make_case(1, 2, 9, 13, 6.0, 4.0, {{{0, 2, 0, 0, 1.5}, {0, 3, 1e9, 0, 1.5}}});
        render(s, 1.0, 100.0, 0.5, true, true, true, 0);
        ++cases;
        check_common("full frame", s);
        bool all = true;
        for (size_t p = 0; p < s.label.size(); ++p) all = all && s.label[p] == 2;
        EXPECT(all && s.dropped[0] == 2, "full frame: not every pixel is the quad's, or %d dropped", s.dropped[0]);
    }
    SELFTEST_END("shade_selftest", "%d scenes: W = 37, zero instances, a vertex behind the near plane, a quad larger than the image, an invalid object, "
                 "null colors, null background, null depth", cases);
}
