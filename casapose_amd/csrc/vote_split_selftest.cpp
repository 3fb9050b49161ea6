// Stand-alone self-test of vote_split_math.h on the host, meant to be built with -fsanitize=address,undefined -ffp-contract=off
// (make vote_split-selftest) and run on the CPU.  It is never loaded into Python.  It runs the serial loops of the header -- what the kernels of
// vote_split.hip carry out -- on buffers of exactly the input and output sizes, so that any index past them is an AddressSanitizer report, on
// cases worked out by hand.
#include <cmath>
#include <cstring>
#include <vector>

#include "selftest.h"
#include "vote_split_math.h"

using namespace cp_vs;

// an h x w image with a record of two floats per pixel (dy, dx); one object unless said otherwise
struct Image {
    int h, w;
    std::vector<uint8_t> labels;
    std::vector<float> field;
    Image(int h_, int w_) : h(h_), w(w_), labels((size_t)h_ * w_, 0), field((size_t)h_ * w_ * 2, 0.f) {}
    void put(int y, int x, int label, float dy, float dx) {
        labels[(size_t)y * w + x] = (uint8_t)label;
        field[((size_t)y * w + x) * 2] = dy, field[((size_t)y * w + x) * 2 + 1] = dx;
    }
    std::vector<int32_t> acc(int objects, int cell, int stride) const {
        const int gh = (h + cell - 1) / cell, gw = (w + cell - 1) / cell;
        std::vector<int32_t> a((size_t)objects * gh * gw, -7);
        accumulate_serial(labels.data(), field.data(), 2, 0, h, w, objects, cell, stride, a.data());
        return a;
    }
};

static long long total(const std::vector<int32_t>& a) {
    long long s = 0;
    for (int32_t v : a) s += v;
    return s;
}

int main() {
    // 1. rays to the four edges of an 8 x 12 image at cell 4 (grid 2 x 3), from pixel (5, 6) in cell (1, 1)
    {
        Image im(8, 12);
        im.put(5, 6, 1, 1.f, 0.f);   // down: a = 5.5, 9.5 -> one step
        std::vector<int32_t> a = im.acc(1, 4, 1);
        EXPECT(a[1 * 3 + 1] == 1 && total(a) == 1, "down: cell (1,1) once, total %lld", total(a));
        im.put(5, 6, 1, -1.f, 0.f);   // up: a = 5.5, 1.5, -2.5
        a = im.acc(1, 4, 1);
        EXPECT(a[1 * 3 + 1] == 1 && a[0 * 3 + 1] == 1 && total(a) == 2, "up: cells (1,1), (0,1), total %lld", total(a));
        im.put(5, 6, 1, 0.f, 2.f);   // right: a = 6.5, 10.5, 14.5
        a = im.acc(1, 4, 1);
        EXPECT(a[1 * 3 + 1] == 1 && a[1 * 3 + 2] == 1 && total(a) == 2, "right: cells (1,1), (1,2), total %lld", total(a));
        im.put(5, 6, 1, 0.f, -0.5f);   // left: a = 6.5, 2.5, -1.5
        a = im.acc(1, 4, 1);
        EXPECT(a[1 * 3 + 1] == 1 && a[1 * 3 + 0] == 1 && total(a) == 2, "left: cells (1,1), (1,0), total %lld", total(a));
        // |dy| == |dx|: y is the major axis, m = -1; from (5, 6) up and to the right: (5.5, 6.5), (1.5, 10.5), (-2.5, ..)
        im.put(5, 6, 1, -3.f, 3.f);
        a = im.acc(1, 4, 1);
        EXPECT(a[1 * 3 + 1] == 1 && a[0 * 3 + 2] == 1 && total(a) == 2, "diagonal: cells (1,1), (0,2), total %lld", total(a));
        // the minor axis leaves first: x major, m = 0.75: (6.5, 5.5), then (10.5, 8.5) with 8.5 >= h
        im.put(5, 6, 1, 3.f, 4.f);
        a = im.acc(1, 4, 1);
        EXPECT(a[1 * 3 + 1] == 1 && total(a) == 1, "minor axis leaves: total %lld", total(a));
    }
    // 2. pixels that do not vote: zero, NaN and infinite directions, a label above `objects`, a stride that skips the pixel
    {
        Image im(8, 12);
        im.put(2, 2, 1, 0.f, 0.f);
        im.put(2, 4, 1, NAN, 1.f);
        im.put(2, 6, 1, 1.f, INFINITY);
        im.put(4, 4, 3, 1.f, 0.f);   // objects = 2
        im.put(3, 2, 1, 1.f, 0.f);   // row 3: skipped at stride 2
        im.put(4, 3, 2, 1.f, 0.f);   // column 3: skipped at stride 2
        std::vector<int32_t> a = im.acc(2, 4, 2);
        EXPECT(total(a) == 0, "nothing votes at stride 2: total %lld", total(a));
        a = im.acc(2, 4, 1);   // at stride 1 the last two vote: (3, 2) down -> cells (0,0), (1,0); (4, 3) of object 2 -> cell (1,0)
        EXPECT(a[0] == 1 && a[3] == 1 && a[6 + 3] == 1 && total(a) == 3, "stride 1: total %lld", total(a));
    }
    // 3. a grid that does not divide the image: 5 x 7 at cell 2 -> 3 x 4; the last pixel's own cell is (2, 3)
    {
        Image im(5, 7);
        im.put(4, 6, 1, 1.f, 1.f);
        std::vector<int32_t> a = im.acc(1, 2, 1);
        EXPECT(a[2 * 4 + 3] == 1 && total(a) == 1, "ragged grid: total %lld", total(a));
        im.put(4, 6, 1, -1.f, -1.f);   // (4.5, 6.5), (2.5, 4.5), (0.5, 2.5), (-1.5, ..)
        a = im.acc(1, 2, 1);
        EXPECT(a[2 * 4 + 3] == 1 && a[1 * 4 + 2] == 1 && a[0 * 4 + 1] == 1 && total(a) == 3, "ragged grid, diagonal: total %lld", total(a));
    }
    // 4. peaks on a hand-written 4 x 5 grid, R = 3 into tables of exactly R rows
    {
        const int gh = 4, gw = 5;
        std::vector<int32_t> g((size_t)gh * gw, 0);
        g[0 * gw + 0] = 9;            // a corner: the window and the centroid are clipped
        g[0 * gw + 1] = 3;
        g[3 * gw + 4] = 9;            // equal votes: the smaller index (0, 0) ranks first
        g[3 * gw + 3] = 9;            // a plateau inside one window: (3, 3) has the smaller index and suppresses (3, 4)
        g[1 * gw + 2] = 2;            // below min_votes
        std::vector<int32_t> inst(3 * 4, -7);
        std::vector<float> pk(3 * 2, -7.f);
        int np = peaks_serial(g.data(), gh, gw, 4, 3, 3, 25, 1, inst.data(), pk.data());
        EXPECT(np == 2, "two peaks (got %d)", np);
        EXPECT(inst[1] == 9 && inst[2] == 0 && inst[3] == 0 && inst[5] == 9 && inst[6] == 3 && inst[7] == 3, "ranks: (0,0) then (3,3)");
        EXPECT(inst[8] == 0 && inst[9] == 0 && inst[10] == -1 && inst[11] == -1 && pk[4] == 0.f && pk[5] == 0.f, "rank 2 is empty");
        // centroid at (0, 0): cells (0,0) = 9 and (0,1) = 3: y = 12 / 12 * 2 = 2, x = (9 + 9) / 12 * 2 = 3
        EXPECT(pk[0] == 2.f && pk[1] == 3.f, "corner centroid (%g, %g)", pk[0], pk[1]);
        // centroid at (3, 3): cells (3,3) = 9, (3,4) = 9: y = 7 * 18 / 18 * 2 = 14, x = (7 * 9 + 9 * 9) / 18 * 2 = 16
        EXPECT(pk[2] == 14.f && pk[3] == 16.f, "edge centroid (%g, %g)", pk[2], pk[3]);
        // the cut: rel_percent 100 keeps equal votes only; a peak of 8 votes is dropped at 100 and kept at 88
        g[3 * gw + 3] = 8, g[3 * gw + 4] = 0;
        np = peaks_serial(g.data(), gh, gw, 4, 3, 3, 100, 1, inst.data(), pk.data());
        EXPECT(np == 1 && inst[5] == 0 && inst[6] == -1, "cut at 100 %% (np %d)", np);
        np = peaks_serial(g.data(), gh, gw, 4, 3, 3, 88, 1, inst.data(), pk.data());
        EXPECT(np == 2 && inst[5] == 8, "kept at 88 %% (np %d)", np);
        // more candidates than R: R = 1 keeps the first
        std::vector<int32_t> one(4, -7);
        std::vector<float> pk1(2, -7.f);
        np = peaks_serial(g.data(), gh, gw, 4, 1, 3, 0, 1, one.data(), pk1.data());
        EXPECT(np == 1 && one[1] == 9 && one[2] == 0 && one[3] == 0, "R = 1");
        // an empty grid
        std::vector<int32_t> none((size_t)gh * gw, 0);
        np = peaks_serial(none.data(), gh, gw, 4, 3, 1, 0, 4, inst.data(), pk.data());
        EXPECT(np == 0 && inst[2] == -1 && inst[6] == -1 && inst[10] == -1 && inst[1] == 0, "an empty grid has no peak");
    }
    // 5. assignment: two peaks at (10, 10) and (10, 30); a pixel at (10, 18) pointing left takes rank 0, pointing right rank 1
    {
        const float peaks[4] = {10.5f, 10.5f, 10.5f, 30.5f};
        EXPECT(assign_rank(10, 18, 0.f, -1.f, peaks, 2, 4.f) == 0, "pointing left");
        EXPECT(assign_rank(10, 18, 0.f, 1.f, peaks, 2, 4.f) == 1, "pointing right");
        EXPECT(assign_rank(10, 18, 1.f, 0.f, peaks, 2, 4.f) == -1, "pointing down: both peaks are behind or beside, 8 and 12 px away");
        EXPECT(assign_rank(10, 12, 0.f, 0.f, peaks, 2, 4.f) == 0, "no direction, 2 px from rank 0");
        EXPECT(assign_rank(10, 12, NAN, 1.f, peaks, 2, 4.f) == 0, "NaN direction, 2 px from rank 0");
        EXPECT(assign_rank(10, 20, 0.f, 0.f, peaks, 2, 4.f) == -1, "no direction, 10 px from both");
        EXPECT(assign_rank(10, 20, -1.f, 0.f, peaks, 0, 4.f) == -1, "no peaks");
        // a tie: (10, 20) pointing up-left and up-right symmetrically -- with a zero direction both are 10 px away; gate 10 -> the lower rank
        EXPECT(assign_rank(10, 20, 0.f, 0.f, peaks, 2, 10.f) == 0, "a tie goes to the lower rank");
        // the line of sight passes 3 px from rank 1: inside the gate of 4, outside a gate of 2
        EXPECT(assign_rank(13, 18, 0.f, 1.f, peaks, 2, 4.f) == 1 && assign_rank(13, 18, 0.f, 1.f, peaks, 2, 2.f) == -1, "the gate");
        EXPECT(peak_dist2(13, 18, 0.f, 1.f, 10.5f, 30.5f) == 9.f, "dist2 = 9");
    }
    SELFTEST_END("vote_split_selftest", "rays to the four edges, the diagonal, the minor axis leaving, directions that do not vote, a ragged grid, "
                                        "peak order, plateau, clipping, the cut, R, assignment and its gate");
}
