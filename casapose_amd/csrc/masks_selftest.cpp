// Stand-alone self-test of mask_math.h on the host, meant to be built with -fsanitize=address,undefined (make masks-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs render_serial -- the loop cp_render_masks_host_u8 runs -- into buffers of exactly the output
// and workspace sizes, so that any index past them is an AddressSanitizer report, and checks what can be known in closed form: the pixels of an
// axis-aligned square facing the camera, the records against the label map, the order of two overlapping squares and the tie rule.
// Cases: a degenerate triangle, a frame with zero instances, a vertex behind the camera, a width that is no multiple of 4, a label of 255.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mask_math.h"
#include "selftest.h"

using namespace cp_mask;


static const double F = 100.0;   // focal length; the principal point is given per case

struct Instance {
    int obj, label;
    double tx, ty, tz;   // identity rotation
};

struct Scene {
    int objects, Vmax, Tmax, frames, imax, H, W;
    std::vector<float> verts;
    std::vector<int32_t> vert_counts, faces, face_counts, inst_counts, inst_obj, inst_label;
    std::vector<double> cams, poses;
    std::vector<uint8_t> label;
    std::vector<int32_t> records;
    int at(int f, int i, int j) const { return label[((size_t)f * H + i) * W + j]; }
    const int32_t* rec(int f, int k) const { return &records[((size_t)f * imax + k) * RECORD]; }
};

// object 0: a unit square in the plane z = 0 (two triangles of opposite winding) plus a zero-area triangle and a repeated vertex;
// object 1: the same square with one more triangle that reaches behind the camera
static Scene make_scene(int frames, int imax, int H, int W, double cx, double cy, const std::vector<std::vector<Instance>>& inst) {
    Scene s{2, 6, 4, frames, imax, H, W};
    s.verts.assign((size_t)s.objects * s.Vmax * 3, 0.f);
    s.faces.assign((size_t)s.objects * s.Tmax * 3, 0);
    const float sq[5][3] = {{-1, -1, 0}, {1, -1, 0}, {1, 1, 0}, {-1, 1, 0}, {0, 0, -50}};
    for (int o = 0; o < 2; ++o)
        for (int v = 0; v < 5; ++v)
            for (int c = 0; c < 3; ++c) s.verts[((size_t)o * s.Vmax + v) * 3 + c] = sq[v][c];
    const int32_t f0[4][3] = {{0, 1, 2}, {0, 3, 2}, {0, 2, 2}, {1, 1, 1}}, f1[3][3] = {{0, 1, 2}, {0, 3, 2}, {0, 1, 4}};
    for (int t = 0; t < 4; ++t)
        for (int c = 0; c < 3; ++c) s.faces[(size_t)t * 3 + c] = f0[t][c];
    for (int t = 0; t < 3; ++t)
        for (int c = 0; c < 3; ++c) s.faces[((size_t)s.Tmax + t) * 3 + c] = f1[t][c];
    s.vert_counts = {4, 5};
    s.face_counts = {4, 3};
    s.inst_counts.assign(frames, 0);
    s.inst_obj.assign((size_t)frames * imax, 0);
    s.inst_label.assign((size_t)frames * imax, 0);
    s.poses.assign((size_t)frames * imax * 12, 0.0);
    for (int f = 0; f < frames; ++f) {
        s.cams.insert(s.cams.end(), {F, F, cx, cy});
        s.inst_counts[f] = (int32_t)inst[f].size();
        for (size_t k = 0; k < inst[f].size(); ++k) {
            const size_t slot = (size_t)f * imax + k;
            s.inst_obj[slot] = inst[f][k].obj;
            s.inst_label[slot] = inst[f][k].label;
            double* P = &s.poses[slot * 12];
            P[0] = P[5] = P[10] = 1.0;
            P[3] = inst[f][k].tx, P[7] = inst[f][k].ty, P[11] = inst[f][k].tz;
        }
    }
    return s;
}

static void render(Scene& s, double near, double far, double offset) {
    s.label.assign((size_t)s.frames * s.H * s.W, 77);
    s.records.assign((size_t)s.frames * s.imax * RECORD, 77);
    std::vector<uint32_t> planes(workspace_bytes(s.frames, s.imax, s.H, s.W) / sizeof(uint32_t));
    render_serial(s.verts.data(), s.vert_counts.data(), s.Vmax, s.faces.data(), s.face_counts.data(), s.Tmax, s.objects, s.cams.data(),
                  s.inst_counts.data(), s.inst_obj.data(), s.inst_label.data(), s.poses.data(), s.frames, s.imax, s.H, s.W, near, far, offset,
                  s.label.data(), s.records.data(), planes.data());
}

// what holds for every frame: px_count_visib and bbox_visib are those of the label map (labels are distinct per frame in these scenes)
static void check_consistent(const char* name, const Scene& s) {
    for (int f = 0; f < s.frames; ++f)
        for (int k = 0; k < s.imax; ++k) {
            const int32_t* r = s.rec(f, k);
            if (k >= s.inst_counts[f]) {
                EXPECT(r[R_ALL] == 0 && r[R_VISIB] == 0 && r[R_BOX_OBJ] == -1 && r[R_BOX_VISIB + 3] == -1 && r[R_DROPPED] == 0, "%s: unused slot %d.%d is not empty", name, f, k);
                continue;
            }
            int n = 0, x0 = s.W, y0 = s.H, x1 = -1, y1 = -1;
            for (int i = 0; i < s.H; ++i)
                for (int j = 0; j < s.W; ++j)
                    if (s.at(f, i, j) == s.inst_label[(size_t)f * s.imax + k] && s.at(f, i, j) != 0) {
                        ++n;
                        x0 = j < x0 ? j : x0, y0 = i < y0 ? i : y0, x1 = j > x1 ? j : x1, y1 = i > y1 ? i : y1;
                    }
            EXPECT(r[R_VISIB] == n && r[R_VISIB] <= r[R_ALL], "%s: %d.%d counts %d visible, the label map has %d (all %d)", name, f, k, r[R_VISIB], n, r[R_ALL]);
            if (n) EXPECT(r[R_BOX_VISIB] == x0 && r[R_BOX_VISIB + 1] == y0 && r[R_BOX_VISIB + 2] == x1 - x0 && r[R_BOX_VISIB + 3] == y1 - y0, "%s: %d.%d visible box", name, f, k);
            else EXPECT(r[R_BOX_VISIB] == -1 && r[R_BOX_VISIB + 2] == -1, "%s: %d.%d empty visible box", name, f, k);
        }
}

int main() {
    int cases = 0;
    // 1. W = 37 (no multiple of 4), three frames with 0, 1 and 2 instances; object 0 carries a zero-area and a one-vertex triangle; label 255.
    //    The square [-1, 1]^2 at depth 10 projects to [cx - 10, cx + 10] x [cy - 10, cy + 10]: with cx = 18, cy = 10 and sample_offset 0.5 the
    //    samples j + 0.5 inside are j = 8 .. 27, rows 0 .. 19 -- 20 x 20 pixels, closed edges included by none (no sample lies on an edge).
    {
        Scene s = make_scene(3, 2, 21, 37, 18.0, 10.0, {{}, {{0, 255, 0, 0, 10}}, {{0, 5, 0, 0, 10}, {0, 9, 0.5, 0, 8}}});
        render(s, 1.0, 100.0, 0.5);
        ++cases;
        check_consistent("odd width", s);
        bool empty = true;
        for (int p = 0; p < s.H * s.W; ++p) empty = empty && s.label[p] == 0;
        EXPECT(empty, "zero instances: the frame is not all background");
        const int32_t* r = s.rec(1, 0);
        EXPECT(r[R_ALL] == 400 && r[R_VISIB] == 400 && r[R_BOX_OBJ] == 8 && r[R_BOX_OBJ + 1] == 0 && r[R_BOX_OBJ + 2] == 19 && r[R_BOX_OBJ + 3] == 19 && r[R_DROPPED] == 0,
               "label 255: all %d visib %d box %d %d %d %d dropped %d", r[R_ALL], r[R_VISIB], r[R_BOX_OBJ], r[R_BOX_OBJ + 1], r[R_BOX_OBJ + 2], r[R_BOX_OBJ + 3], r[R_DROPPED]);
        EXPECT(s.at(1, 10, 18) == 255 && s.at(1, 10, 7) == 0 && s.at(1, 10, 8) == 255 && s.at(1, 10, 27) == 255 && s.at(1, 10, 28) == 0 && s.at(1, 20, 18) == 0,
               "label 255: the square's pixels");
        // frame 2: the nearer square (depth 8, label 9) covers the farther one's centre and wins there; part of the farther stays visible
        const int32_t *a = s.rec(2, 0), *b = s.rec(2, 1);
        EXPECT(s.at(2, 10, 24) == 9 && a[R_ALL] == 400 && a[R_VISIB] < 400 && a[R_VISIB] > 0 && b[R_VISIB] == b[R_ALL] && b[R_ALL] > 400, "overlap: %d, far %d / %d, near %d / %d",
               s.at(2, 10, 24), a[R_VISIB], a[R_ALL], b[R_VISIB], b[R_ALL]);
    }
    // 2. sample_offset 0: samples at integers, the closed edges count: columns 8 .. 28, rows 0 .. 20 of a 21-row image
    {
        Scene s = make_scene(1, 1, 21, 38, 18.0, 10.0, {{{0, 1, 0, 0, 10}}});
        render(s, 1.0, 100.0, 0.0);
        ++cases;
        check_consistent("offset 0", s);
        const int32_t* r = s.rec(0, 0);
        EXPECT(r[R_ALL] == 21 * 21 && r[R_BOX_OBJ] == 8 && r[R_BOX_OBJ + 2] == 20 && r[R_BOX_OBJ + 3] == 20, "offset 0: all %d box %d %d", r[R_ALL], r[R_BOX_OBJ], r[R_BOX_OBJ + 2]);
    }
    // 3. a vertex behind the camera: object 1's third triangle reaches z = 10 - 50 and is dropped whole; the square is still drawn.  Two
    //    identical instances: the lower index wins everywhere.  An instance naming object 7 and one with label 256 render nothing.  Depth range.
    {
        Scene s = make_scene(2, 4, 24, 40, 20.0, 12.0, {{{1, 7, 0, 0, 10}, {1, 9, 0, 0, 10}, {7, 3, 0, 0, 10}, {0, 256, 0, 0, 10}}, {{0, 4, 0, 0, 10}, {0, 6, 0, 0, 300}}});
        render(s, 1.0, 100.0, 0.5);
        ++cases;
        const int32_t *a = s.rec(0, 0), *b = s.rec(0, 1), *c = s.rec(0, 2), *d = s.rec(0, 3);
        EXPECT(a[R_DROPPED] == 1 && b[R_DROPPED] == 1 && a[R_ALL] == 400 && b[R_ALL] == 400 && a[R_VISIB] == 400 && b[R_VISIB] == 0 && b[R_BOX_VISIB] == -1,
               "behind / tie: dropped %d %d, all %d %d, visible %d %d", a[R_DROPPED], b[R_DROPPED], a[R_ALL], b[R_ALL], a[R_VISIB], b[R_VISIB]);
        EXPECT(c[R_ALL] == 0 && d[R_ALL] == 0 && c[R_DROPPED] == 0 && s.at(0, 12, 20) == 7, "invalid instances rendered: %d %d", c[R_ALL], d[R_ALL]);
        EXPECT(s.rec(1, 0)[R_ALL] == 400 && s.rec(1, 1)[R_ALL] == 0, "far plane: %d pixels at depth 300 with far = 100", s.rec(1, 1)[R_ALL]);
    }
    // 4. a quad larger than the image (every pixel covered), and one that projects beyond the representable range (dropped, not drawn)
    {
        Scene s = make_scene(1, 2, 9, 13, 6.0, 4.0, {{{0, 2, 0, 0, 1.5}, {0, 3, 1e9, 0, 1.5}}});
        render(s, 1.0, 100.0, 0.5);
        ++cases;
        check_consistent("full frame", s);
        EXPECT(s.rec(0, 0)[R_ALL] == 9 * 13 && s.rec(0, 0)[R_BOX_OBJ + 2] == 12 && s.rec(0, 1)[R_ALL] == 0 && s.rec(0, 1)[R_DROPPED] == 4, "full frame: %d pixels, %d dropped",
               s.rec(0, 0)[R_ALL], s.rec(0, 1)[R_DROPPED]);
    }
    SELFTEST_END("masks_selftest", "%d scenes: a degenerate triangle, zero instances, a vertex behind the camera, an odd width, label 255", cases);
}
