// A covariance per (image, slot, keypoint) from the least-squares voter's own objective (cp_ls_slot_covariance_f32, ls_vote.hip): what one pixel
// adds to the five sums of the moments pass, and the finish that turns the sums into a 2 x 2 covariance, as __host__ __device__ code free of
// HIP types.  The kernels of ls_vote.hip and the stand-alone self-test (ls_cov_selftest.cpp) call the same functions.  Nothing here calls a
// library beyond <math.h>.
//
// The LS objective of a keypoint is sum_i w_i d_i(p)^2, d_i(p) the signed distance of p from the line of pixel i (centre c_i, unit direction
// n_i); its normal matrix is A = sum_i w_i (I - n_i n_i^T).  For an estimate p handed in from outside (the covariance is a function of the
// keypoints given; it keeps no state and reads nothing an earlier pass summed) the pass sums, over the slot's pixels with a non-zero direction,
//     omega_i = w_i rho_i            rho_i = cp_lsr::rho of d_i(p) when a cut-off is given, otherwise 1
//     A  = sum omega_i (I - n_i n_i^T)         Q = sum omega_i d_i^2         Wall = sum w_i
// everything in the voter's normalised coordinates (pixels / H), and the finish gives
//     W = trace A = sum omega_i      sigma2 = H^2 Q / W  (px^2)      kept = W / Wall      Sigma = sigma2 (A / W)^-1 = H^2 Q A^-1.
// Sigma is the covariance of ONE vote of average weight: the scale of a hypothesis scatter, long along the rays of a keypoint far from the
// mask.  It is deliberately not the standard error of the estimate (Sigma over the effective number of pixels): that one is far below the
// 1/12 px^2 floor of the weighted PnP for any slot worth solving, and weighting by it changes nothing.
// A truncated Tukey residual underestimates sigma2 (the pixels beyond the cut-off hold the largest residuals and have weight 0, the ones near
// it are weighted down); that is not corrected.
// A zero direction (n = (0, 0)) is no line: such a pixel takes no part in any of the five sums, with or without a cut-off.  (The plain vote
// counts it as w I.)
#pragma once
#include "ls_robust_math.h"

namespace cp_lsc {

// What one (pixel, keypoint) adds, in fp32 and in cp_lsr::rho's order: e = p - c, d = e_y n_x - e_x n_y, omega = w * rho, q = omega * (d * d).
// p = (py, px) is the estimate, c = (cy, cx) the pixel's centre, n = (ny, nx) its unit direction or (0, 0), all normalised; rscale = H / cutoff
// (cp_lsr::rho_scale) or 0 for no cut-off.  The caller forms the matrix terms from omega as it forms them from w, adds q to Q and wall to Wall.
struct Moment { float omega, q, wall; };
LSR_HD Moment moment(float py, float px, float cy, float cx, float ny, float nx, float w, float rscale) {
    if (ny == 0.f && nx == 0.f) return {0.f, 0.f, 0.f};
    const float ey = py - cy, ex = px - cx;
    const float d = ey * nx - ex * ny;
    const float r = rscale > 0.f ? cp_lsr::rho(py, px, cy, cx, ny, nx, rscale) : 1.0f;
    const float omega = w * r;
    return {omega, omega * (d * d), w};
}

// The finish of one (image, slot, keypoint) in fp64.  s = (A00, A01, A11, Q, Wall) in the voter's (y, x) order and normalised coordinates,
// p_finite says whether both coordinates of the estimate were finite, h is the image height.  cov = (sxx, sxy, syy) in (x, y) PIXELS, the order
// the weighted PnP reads: (Sigma[1][1], Sigma[0][1], Sigma[0][0]) of the (y, x) matrix.  stat = (sigma2 in px^2, kept); (0, 0) where W is not
// > 0 or the estimate is not finite.  Returns false, and three NaNs in cov (which the weighted PnP refuses, so that the pair is solved
// unweighted and says so), when
//   - the estimate is not finite, or W is not > 0,
//   - A fails the rank rule or the condition bound of the robust solve (cp_lsr::well_posed), or
//   - kept < CP_LS_ROBUST_MIN_KEPT.
LSR_HD bool finish(const double* s, bool p_finite, int h, float* cov, float* stat) {
    const double a = s[0], b = s[1], c = s[2], q = s[3], wall = s[4];
    const double w = a + c, hh = (double)h * (double)h;
    const float nan = NAN;
    cov[0] = cov[1] = cov[2] = nan;
    stat[0] = stat[1] = 0.f;
    if (!p_finite || !(w > 0.0)) return false;
    const double kept = wall > 0.0 ? w / wall : 0.0;
    stat[0] = (float)(hh * q / w);
    stat[1] = (float)kept;
    if (!cp_lsr::well_posed(a, b, c)) return false;
    if (!(w >= cp_lsr::CP_LS_ROBUST_MIN_KEPT * wall)) return false;
    const double k = hh * q / (a * c - b * b);      // Sigma = k [[c, -b], [-b, a]]
    cov[0] = (float)(k * a);
    cov[1] = (float)(-(k * b));
    cov[2] = (float)(k * c);
    return true;
}

}  // namespace cp_lsc
