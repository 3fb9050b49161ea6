// Stand-alone self-test of model_math.h on the host, meant to be built with -fsanitize=address,undefined (make models-selftest) and run on the
// CPU.  It is never loaded into Python.  It runs prep_serial -- the loop cp_model_prep_host_f32 runs -- on buffers of exactly the input, output
// and workspace sizes, so that any index past them is an AddressSanitizer report, and checks it against a plain restatement: all pairs for the
// diameter, a first-maximum loop for the picks.  Cases: sizes around the tile (1, 2, 255, 256, 257, 513, 1000), objects of very different sizes in
// one call with an invalid one between them, a cube (ties), identical vertices, and the pair <-> tile map for every pair of 300 tiles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "model_math.h"
#include "selftest.h"

using namespace cp_model;


static uint32_t rng_state = 12345u;
static float rnd() {   // a small LCG: values in [950, 1050), far from the zeros a padded vertex would hold
    rng_state = rng_state * 1664525u + 1013904223u;
    return 950.0f + 100.0f * (float)(rng_state >> 8) / 16777216.0f;
}

struct Out {
    std::vector<double> diam;
    std::vector<float> box, kps;
    std::vector<int32_t> idx, status;
};

static Out run(const std::vector<float>& verts, const std::vector<long long>& offsets, const std::vector<int32_t>& counts, int K) {
    const int objects = (int)counts.size();
    const long long total = (long long)verts.size() / 3;
    Out o;
    o.diam.assign(objects, -1.0);
    o.box.assign((size_t)objects * 6, -1.f);
    o.kps.assign((size_t)objects * K * 3, -1.f);
    o.idx.assign((size_t)objects * (K - 1), -1);
    o.status.assign(objects, -1);
    std::vector<int64_t> ws(workspace_bytes(objects, total) / 8);
    // exact-size copies of the inputs: a read past an object's vertices that leaves the array is reported
    float* v = (float*)std::malloc(verts.size() * sizeof(float));
    std::memcpy(v, verts.data(), verts.size() * sizeof(float));
    prep_serial(v, total, offsets.data(), counts.data(), objects, K, o.diam.data(), o.box.data(), o.kps.data(), o.idx.data(), o.status.data(), ws.data());
    std::free(v);
    return o;
}

// the plain restatement for one valid object
static void check_object(const char* what, const float* P, int n, int K, const Out& o, int obj) {
    double best = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double d = dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], P[3 * j], P[3 * j + 1], P[3 * j + 2]);
            if (d > best) best = d;
        }
    EXPECT(o.diam[obj] == best, "%s: diameter_sq %.17g, all pairs give %.17g", what, o.diam[obj], best);
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = P[a];
    for (int i = 1; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            if (P[3 * i + a] < mn[a]) mn[a] = P[3 * i + a];
            if (P[3 * i + a] > mx[a]) mx[a] = P[3 * i + a];
        }
    double c[3];
    for (int a = 0; a < 3; ++a) {
        EXPECT(o.box[6 * obj + a] == mn[a] && o.box[6 * obj + 3 + a] == mx[a], "%s: box axis %d", what, a);
        c[a] = 0.5 * ((double)mn[a] + (double)mx[a]);
        EXPECT(o.kps[(size_t)obj * K * 3 + a] == (float)c[a], "%s: centre axis %d", what, a);
    }
    std::vector<double> m(n);
    for (int i = 0; i < n; ++i) m[i] = dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], c[0], c[1], c[2]);
    int status = ST_OK;
    for (int k = 1; k < K; ++k) {
        int j = 0;
        for (int i = 1; i < n; ++i)
            if (m[i] > m[j]) j = i;
        const float* kp = &o.kps[((size_t)obj * K + k) * 3];
        if (!(m[j] > 0.0)) {
            status = ST_TOO_FEW;
            for (int r = k; r < K; ++r) {
                const float* z = &o.kps[((size_t)obj * K + r) * 3];
                EXPECT(z[0] == 0.f && z[1] == 0.f && z[2] == 0.f && o.idx[(size_t)obj * (K - 1) + r - 1] == 0, "%s: pick %d is not zero", what, r);
            }
            break;
        }
        EXPECT(o.idx[(size_t)obj * (K - 1) + k - 1] == j, "%s: pick %d is vertex %d, expected %d", what, k, o.idx[(size_t)obj * (K - 1) + k - 1], j);
        EXPECT(kp[0] == P[3 * j] && kp[1] == P[3 * j + 1] && kp[2] == P[3 * j + 2], "%s: keypoint %d is not vertex %d", what, k, j);
        for (int i = 0; i < n; ++i) {
            const double d = dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], P[3 * j], P[3 * j + 1], P[3 * j + 2]);
            if (d < m[i]) m[i] = d;
        }
    }
    EXPECT(o.status[obj] == status, "%s: status %d, expected %d", what, o.status[obj], status);
}

int main() {
    // the pair <-> tile map: every pair of 300 tiles in order, and the last pair of the largest object
    {
        int64_t p = 0;
        for (int tb = 0; tb < 300; ++tb)
            for (int ta = 0; ta <= tb; ++ta, ++p) {
                int a, b;
                tile_of_pair(p, a, b);
                if (a != ta || b != tb) EXPECT(false, "tile_of_pair(%lld) = (%d, %d), expected (%d, %d)", (long long)p, a, b, ta, tb);
            }
        const int T = tiles(MAX_VERTICES);
        int a, b;
        tile_of_pair(tile_pairs(MAX_VERTICES) - 1, a, b);
        EXPECT(a == T - 1 && b == T - 1 && tile_pairs(MAX_VERTICES) == (int64_t)T * (T + 1) / 2, "the last pair of 2^22 vertices is (%d, %d)", a, b);
        tile_of_pair((int64_t)(T - 1) * T / 2, a, b);
        EXPECT(a == 0 && b == T - 1, "the first pair of the last row is (%d, %d)", a, b);
    }
    // single objects around the tile size
    for (int n : {1, 2, 255, 256, 257, 513, 1000}) {
        std::vector<float> v((size_t)n * 3);
        for (float& x : v) x = rnd();
        char what[32];
        std::snprintf(what, sizeof what, "n = %d", n);
        for (int K : {2, 9, 32}) check_object(what, v.data(), n, K, run(v, {0}, {n}, K), 0);
    }
    // four objects in one call: 300 vertices, an invalid count, 700 vertices and 5; the objects do not start at multiples of anything
    {
        const std::vector<int32_t> counts = {300, 0, 700, 5};
        const std::vector<long long> offsets = {0, 300, 300, 1000};
        std::vector<float> v((size_t)1005 * 3);
        for (float& x : v) x = rnd();
        const int K = 9;
        const Out o = run(v, offsets, counts, K);
        check_object("mixed/0", v.data(), 300, K, o, 0);
        check_object("mixed/2", v.data() + 900, 700, K, o, 2);
        check_object("mixed/3", v.data() + 3000, 5, K, o, 3);
        EXPECT(o.status[1] == ST_BAD_COUNT && o.diam[1] == 0.0, "an object of no vertices has status %d", o.status[1]);
        for (int a = 0; a < 6; ++a) EXPECT(o.box[6 + a] == 0.f, "an invalid object's box is not zero");
        // ranges that leave the array are refused, not read
        const Out bad = run(v, {0, 900, -1}, {300, 200, 10}, K);
        EXPECT(bad.status[0] == ST_OK && bad.status[1] == ST_BAD_COUNT && bad.status[2] == ST_BAD_COUNT, "out-of-range vertex ranges: %d %d %d",
               bad.status[0], bad.status[1], bad.status[2]);
        const Out big = run(v, {0}, {MAX_VERTICES + 1}, K);
        EXPECT(big.status[0] == ST_BAD_COUNT, "N above 2^22 has status %d", big.status[0]);
    }
    // a cube: four diagonals tie for the diameter; every corner is sqrt(3) from the centre and at least 2 from every other corner, so all
    // remaining corners tie at every pick and the picks are the corners in index order
    {
        std::vector<float> v;
        for (int i = 0; i < 8; ++i)
            for (int a = 0; a < 3; ++a) v.push_back(1000.f + ((i >> (2 - a)) & 1 ? 1.f : -1.f));
        const Out o = run(v, {0}, {8}, 9);
        check_object("cube", v.data(), 8, 9, o, 0);
        EXPECT(o.diam[0] == 12.0 && o.idx[0] == 0 && o.idx[1] == 1 && o.idx[7] == 7 && o.status[0] == ST_OK, "cube: diameter_sq %g, picks %d %d .. %d", o.diam[0], o.idx[0], o.idx[1],
               o.idx[7]);
        const Out few = run(v, {0}, {8}, 10);   // nine picks from eight vertices
        check_object("cube, K = 10", v.data(), 8, 10, few, 0);
        EXPECT(few.status[0] == ST_TOO_FEW, "nine picks from eight vertices: status %d", few.status[0]);
    }
    // identical vertices
    {
        std::vector<float> v(3 * 40, 1000.f);
        const Out o = run(v, {0}, {40}, 9);
        check_object("identical", v.data(), 40, 9, o, 0);
        EXPECT(o.status[0] == ST_TOO_FEW && o.diam[0] == 0.0 && o.kps[0] == 1000.f && o.kps[3] == 0.f, "identical vertices: status %d", o.status[0]);
    }
    SELFTEST_END("models_selftest", "the pair <-> tile map, sizes around the tile, four objects of mixed sizes with an invalid one, a cube, identical vertices");
}
