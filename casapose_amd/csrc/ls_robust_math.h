// The robust form of the least-squares voter (cp_ls_vote_slots_robust_f32, ls_vote.hip): the weight of one (pixel, keypoint) term in a
// reweighted pass and the rule that accepts or refuses a reweighted 2 x 2 system, as __host__ __device__ code free of HIP types.  The kernels
// of ls_vote.hip and the stand-alone self-test (ls_robust_selftest.cpp) call the same functions.  Nothing here calls a library beyond <math.h>.
//
// The LS objective of a keypoint is sum_i w_i dist(p, line_i)^2 over the slot's pixels, line_i the line through the pixel's centre c_i along its
// unit direction n_i.  A reweighted pass multiplies every term by rho_i = rho(dist(p_prev, line_i)), p_prev the estimate of the pass before:
// the residual of the objective itself, so the weight falls exactly where the term's pull is wrong, and a pixel far from the keypoint whose
// line still passes through it keeps its full weight.  (A weight on the distance |p - c| would reject far pixels, which are the well-aimed
// ones; a weight on the angle would reject near ones for a sub-pixel miss.)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LSR_HD __host__ __device__ __forceinline__
#else
#define LSR_HD inline
#endif

namespace cp_lsr {

constexpr double CP_LS_ROBUST_MIN_KEPT = 0.125;   // a reweighted system must keep this share of the plain system's weight (its trace)
constexpr double CP_LS_ROBUST_MAX_COND = 1e6;     // and its condition number must stay below this
constexpr int CP_LS_ROBUST_MAX_PASSES = 8;

// what the entry point computes once per call and hands to every term: H / cutoff, both in fp32
LSR_HD float rho_scale(int h, float cutoff_px) { return (float)h / cutoff_px; }

// Tukey's biweight of the perpendicular distance of the estimate p = (py, px) from the line of the pixel with centre c = (cy, cx) and unit
// direction n = (ny, nx), everything in the voter's normalised coordinates (pixels / H):
//     e = p - c;   t = (e_y n_x - e_x n_y) * scale   (= r / cutoff, r the signed distance in pixels);   u = t^2;   rho = u < 1 ? (1 - u)^2 : 0
// rho is continuous at the cut-off and so is its first derivative.  A zero direction (n = (0, 0): divide_no_nan's result for d = 0) is no line
// and has no distance: rho = 0, the pixel takes no part in a reweighted pass.  (The plain pass counts it as w I, a pull towards its own centre.)
// There is no "behind the ray" rule: the objective is about lines.  A NaN estimate gives 0.
LSR_HD float rho(float py, float px, float cy, float cx, float ny, float nx, float scale) {
    if (ny == 0.f && nx == 0.f) return 0.f;
    const float ey = py - cy, ex = px - cx;
    const float t = (ey * nx - ex * ny) * scale;
    const float u = t * t;
    const float k = 1.0f - u;
    return u < 1.0f ? k * k : 0.f;
}

// The solve rule of a reweighted pass for one (image, slot, keypoint): s = (S00, S01, S11, T0, T1) are the reweighted sums, plain_trace is
// S00 + S11 of the plain sums.  Every term has trace w rho (ny^2 + nx^2 = 1), so the trace of a system is the weight it holds and
// trace(s) / plain_trace the share of the plain weight the pass kept.  The new value p (normalised coordinates) is taken when
//   - the system passes the rank rule of the plain solve (both eigenvalues above 20 eps(fp64) of the larger one, which is > 0),
//   - its condition number l1 / l2 is below CP_LS_ROBUST_MAX_COND, and
//   - trace(s) >= CP_LS_ROBUST_MIN_KEPT * plain_trace;
// otherwise false is returned and p is not written: the keypoint keeps the value of the pass before.  The rule keeps no state, so the next
// pass starts from the same estimate, sums the same terms and decides the same.
//
// well_posed is the first two conditions on the matrix [[a, b], [b, c]] alone; the covariance of ls_cov_math.h asks it of its normal matrix.
LSR_HD bool well_posed(double a, double b, double c) {
    const double half_tr = 0.5 * (a + c), half_df = 0.5 * (a - c);
    const double rad = sqrt(half_df * half_df + b * b);
    const double l1 = half_tr + rad, l2 = half_tr - rad;   // l1 >= l2 (PSD up to rounding)
    const double rcond = 10.0 * 2.0 * 2.220446049250313e-16;
    const double smax = fmax(fabs(l1), fabs(l2));
    if (!(smax > 0.0)) return false;                                       // empty (or NaN)
    if (!(fabs(l2) > rcond * smax && fabs(l1) > rcond * smax)) return false;   // rank one
    return l2 > 0.0 && l1 < CP_LS_ROBUST_MAX_COND * l2;
}

LSR_HD bool solve(const double* s, double plain_trace, double& p0, double& p1) {
    const double a = s[0], b = s[1], c = s[2], t0 = s[3], t1 = s[4];
    if (!well_posed(a, b, c)) return false;
    if (!(a + c >= CP_LS_ROBUST_MIN_KEPT * plain_trace)) return false;
    const double det = a * c - b * b;
    p0 = (c * t0 - b * t1) / det;
    p1 = (a * t1 - b * t0) / det;
    return true;
}

}  // namespace cp_lsr
