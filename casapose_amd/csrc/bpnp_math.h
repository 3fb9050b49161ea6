// BPnP keypoint loss on top of pnp_math.h: training.bpnp_reprojection_loss_host restated for one (image, object) pair in fp64, shared by the
// device kernels (bpnp.hip), the host twin (cp_bpnp_loss_host_f64) and the stand-alone self-test (bpnp_selftest.cpp).
//
//   p' = T(p)                      voted keypoints (y, x) in crop pixels through the fp32 crop->image affine
//   y  = argmin sum |pi(y) - p'|^2 the PnP optimum: consensus EPnP + LM (pnp_math.h, before its fp32 rounding), then LM again with 30
//                                  iterations and a relative stop of 1e-14, the optimum the implicit function theorem differentiates
//   r  = pi(y), e = (|r - p'| + |gt - r|) / 2, l = cap(smoothL1(e)), the pair's loss = mean_j l
//   d loss / d p' = g_direct + J v,  H v = J^T g_r,  H = d(J^T r)/dy by central differences of residual_normal's g (pnp.bpnp_backward): it
//                                  holds the second-order term sum r_i d2 pi_i / dy2 that the Gauss-Newton J^T J lacks
// The stages are separate functions because the kernel gives them to different lanes: the 12 evaluations g(y +- h e_k) and the per-keypoint
// terms are independent.  bpnp_pair_serial strings them together for one pair.  Every loop has a fixed trip count.
#pragma once
#include "pnp_math.h"

namespace cp_pnp {

constexpr int TIGHT_LM_ITERS = 30;
constexpr double TIGHT_LM_EPS = 1e-14, HESSIAN_STEP = 1e-6;

// keypoint i of a pair: (y, x) crop pixels through the fp32 affine (x' = a0 x + a1 y + a2, y' = a3 x + a4 y + a5), the fp32 model point, and
// the fp32 ground-truth projection (x, y) in image pixels
PNP_HD void load_point_yx(Problem& P, double* gt, int i, const float* yx, const float* xyz, const float* gt_xy, const float* affine) {
    const double y = (double)yx[2 * i], x = (double)yx[2 * i + 1];
    P.x[2 * i] = (double)affine[0] * x + (double)affine[1] * y + (double)affine[2];
    P.x[2 * i + 1] = (double)affine[3] * x + (double)affine[4] * y + (double)affine[5];
    for (int d = 0; d < 3; ++d) P.X[3 * i + d] = (double)xyz[3 * i + d];
    gt[2 * i] = (double)gt_xy[2 * i];
    gt[2 * i + 1] = (double)gt_xy[2 * i + 1];
}

// a pair without a loss: the zero pose, a status, no gradient
PNP_HD void zero_pair(int status, int n, double* g_yx, double* loss, float* pose, int32_t* info) {
    for (int i = 0; i < 12; ++i) pose[i] = 0.f;
    info[0] = status; info[1] = -1; info[2] = 0; info[3] = 0;
    for (int i = 0; i < 2 * n; ++i) g_yx[i] = 0.0;
    *loss = 0.0;
}

// the tightened optimum from the consensus: y = (rvec, t) in fp64; iters = the iterations of the first LM (info[3] of cp_pnp_f64)
PNP_HD bool tightened_optimum(const Problem& P, const Score& sc, double* y, int& iters) {
    double c2[2];
    if (!consensus_pose(P, sc, y, c2, iters)) return false;
    refine_lm(P, y, c2, TIGHT_LM_ITERS, TIGHT_LM_EPS);
    bool fin = finite(c2[0]) && finite(c2[1]);
    for (int i = 0; i < 6; ++i) fin = fin && finite(y[i]);
    return fin;
}

// evaluation e = 2 k + s of the central differences: g = J^T r at y + h e_k (s = 0) or y - h e_k (s = 1), h = 1e-6 max(1, |y_k|)
PNP_HD double hessian_step(const double* y, int k) { return HESSIAN_STEP * dmax(1.0, fabs(y[k])); }
PNP_HD void shifted_gradient(const Problem& P, const double* y, int e, double* g) {
    double q[6], A[36];
    for (int i = 0; i < 6; ++i) q[i] = y[i];
    const int k = e >> 1;
    const double h = hessian_step(y, k);
    q[k] = (e & 1) ? y[k] - h : y[k] + h;
    residual_normal(P, q, A, g);
}

// what keypoint j contributes: its loss, d loss / d r and the explicit d loss / d p' (both without 1 / na), and its Jacobian rows
struct PointTerm {
    double l, g_r[2], g_direct[2], ju[6], jv[6];
};

PNP_HD void point_term(const Problem& P, const double* gt, const double* y, const double* R, const double* Jl, int j, double max_pixel_error, PointTerm& T) {
    double ru, rv;
    point_residual(P, y, R, Jl, j, ru, rv, T.ju, T.jv);
    const double r[2] = {ru + P.x[2 * j], rv + P.x[2 * j + 1]};
    const double d1[2] = {r[0] - P.x[2 * j], r[1] - P.x[2 * j + 1]}, d2[2] = {gt[2 * j] - r[0], gt[2 * j + 1] - r[1]};
    const double n1 = sqrt(d1[0] * d1[0] + d1[1] * d1[1]), n2 = sqrt(d2[0] * d2[0] + d2[1] * d2[1]);
    const double e = 0.5 * (n1 + n2);
    double l = e < 1.0 ? 0.5 * e * e : e - 0.5, slope = e < 1.0 ? e : 1.0;
    if (l > max_pixel_error) {
        l = max_pixel_error + (l - max_pixel_error) * 0.01;
        slope *= 0.01;
    }
    T.l = l;
    const double cf = slope / (double)P.n * 0.5;   // d loss / d n1 = d loss / d n2
    for (int d = 0; d < 2; ++d) {
        const double u1 = n1 > 0.0 ? d1[d] / n1 : 0.0, u2 = n2 > 0.0 ? d2[d] / n2 : 0.0;
        T.g_r[d] = cf * (u1 - u2);
        T.g_direct[d] = -cf * u1;
    }
}

// H from the 12 shifted gradients G[e][6], symmetrised; H v = g_pose.  false: H is singular or v is not finite
PNP_HD bool implicit_solve(const double* y, const double* G, const double* g_pose, double* v) {
    double D[36], H[36], b[6];
    for (int k = 0; k < 6; ++k) {
        const double h = hessian_step(y, k);
        for (int a = 0; a < 6; ++a) D[a * 6 + k] = (G[(2 * k) * 6 + a] - G[(2 * k + 1) * 6 + a]) / (2.0 * h);
    }
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) H[a * 6 + c] = 0.5 * (D[a * 6 + c] + D[c * 6 + a]);
    for (int a = 0; a < 6; ++a) b[a] = g_pose[a];
    if (!solve_pivoted<6>(H, b, v, false)) return false;
    bool fin = true;
    for (int a = 0; a < 6; ++a) fin = fin && finite(v[a]);
    return fin;
}

// keypoint j's d loss / d (y, x) in crop pixels, without weight / na: g_direct + J v, back through the 2x2 linear part of the affine
PNP_HD void point_gradient(const PointTerm& T, const double* v, const float* affine, double* g_yx) {
    double gX = T.g_direct[0], gY = T.g_direct[1];
    for (int a = 0; a < 6; ++a) {
        gX += T.ju[a] * v[a];
        gY += T.jv[a] * v[a];
    }
    g_yx[0] = gX * (double)affine[1] + gY * (double)affine[4];
    g_yx[1] = gX * (double)affine[0] + gY * (double)affine[3];
}

// [R | t] of y as fp32, negated when t_z < 0 (pnp.pnp's sign rule)
PNP_HD void pose_from_optimum(const double* y, const double* R, float* pose) {
    const double sgn = y[5] < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) pose[r * 4 + c] = (float)(sgn * R[r * 3 + c]);
        pose[r * 4 + 3] = (float)(sgn * y[3 + r]);
    }
}

// the whole of one pair, serially: what bpnp_pair_kernel's block computes.  g_yx [n][2] (y, x) without weight / na.
PNP_HD void bpnp_pair_serial(const float* coords_yx, const float* gt_xy, const float* affine, const float* xyz, const float* K, int n, const uint8_t* table,
                             int H, double reprojection_error, double max_pixel_error, double* g_yx, double* loss, float* pose, int32_t* info) {
    Problem P;
    double gt[MAX_POINTS * 2];
    P.n = n;
    for (int i = 0; i < 9; ++i) P.K[i] = (double)K[i];
    for (int i = 0; i < n; ++i) load_point_yx(P, gt, i, coords_yx, xyz, gt_xy, affine);
    const int status = check_problem(P);
    if (status != OK) {
        zero_pair(status, n, g_yx, loss, pose, info);
        return;
    }
    Score best;
    const int winner = consensus_serial(P, table, H, reprojection_error, best);
    double y[6], R[9], Jl[9], G[72], g_pose[6], v[6];
    int iters = 0;
    if (!tightened_optimum(P, best, y, iters)) {
        zero_pair(NO_SOLUTION, n, g_yx, loss, pose, info);
        return;
    }
    for (int e = 0; e < 12; ++e) shifted_gradient(P, y, e, G + 6 * e);
    rotation_and_left_jacobian(y, R, Jl);
    PointTerm T[MAX_POINTS];
    double total = 0.0;
    for (int a = 0; a < 6; ++a) g_pose[a] = 0.0;
    for (int j = 0; j < n; ++j) {
        point_term(P, gt, y, R, Jl, j, max_pixel_error, T[j]);
        total += T[j].l;
        for (int a = 0; a < 6; ++a) g_pose[a] += T[j].ju[a] * T[j].g_r[0] + T[j].jv[a] * T[j].g_r[1];
    }
    if (!implicit_solve(y, G, g_pose, v) || !finite(total)) {
        zero_pair(NO_SOLUTION, n, g_yx, loss, pose, info);
        return;
    }
    for (int j = 0; j < n; ++j) point_gradient(T[j], v, affine, g_yx + 2 * j);
    *loss = total / n;
    pose_from_optimum(y, R, pose);
    info[0] = OK; info[1] = winner; info[2] = best.count < 0 ? 0 : best.count; info[3] = iters;
}

// the batch's ending, for element i of pair `pair`: weight / na x the un-normalised gradient of a solved pair, 0 for every other
PNP_HD float finished_gradient(double g, bool solved, double weight, int na) { return solved ? (float)(weight / (double)na * g) : 0.f; }

}  // namespace cp_pnp
