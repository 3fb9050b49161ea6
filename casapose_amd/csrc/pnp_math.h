// PnP arithmetic shared by the device kernels (pnp.hip; bpnp.hip through bpnp_math.h), their host twins (cp_pnp_host_f64,
// cp_bpnp_loss_host_f64) and the stand-alone self-tests (pnp_selftest.cpp, bpnp_selftest.cpp):
// casapose_amd/pose_estimation/pnp.py restated function by function in fp64, as __host__ __device__ code without any library call beyond
// <math.h>.  Everything is bounded: the Jacobi sweeps, the Gauss-Newton steps, the LM iterations and the damping retries have fixed trip
// counts, and a non-finite intermediate ends in a status word, never in another round.
//
// Where pnp.py calls LAPACK this file uses a cyclic Jacobi eigen-solver (the 12x12 M^T M, the 3x3 control-point covariance, Horn's 4x4
// quaternion matrix for the absolute orientation) and pivoted normal equations for the small least-squares problems.  A 5-point minimal
// set gives a 10x12 system whose null space has dimension >= 2; Jacobi returns another basis of it than LAPACK, so single hypotheses differ
// from pnp.py.  The final pose does not: it is the LM optimum of the all-point reprojection error reached from the consensus pose.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ inline
#else
#define PNP_HD inline
#endif

namespace cp_pnp {

constexpr int MAX_POINTS = 16, MIN_POINTS = 5, SET_POINTS = 5, MAX_HYPOTHESES = 256;
constexpr int JACOBI_SWEEPS = 30, GN_STEPS = 10, LM_ITERS = 20, LM_TRIES = 10;
constexpr double LM_EPS = 1e-10;

// info[0] of cp_pnp_f64: anything but OK comes with the zero pose
enum Status { OK = 0, SKIPPED = 1, NONFINITE_INPUT = 2, DEGENERATE = 3, NO_SOLUTION = 4 };

PNP_HD bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN
PNP_HD double dmax(double a, double b) { return a > b ? a : b; }

// ---- cyclic Jacobi: A [N*N] symmetric (destroyed) -> eigenvalues w ascending, eigenvectors in the columns of V ------------------------
template <int N>
PNP_HD void jacobi_eigh(double* A, double* V, double* w) {
    double total = 0.0;
    for (int i = 0; i < N * N; ++i) {
        V[i] = (i / N == i % N) ? 1.0 : 0.0;
        total += A[i] * A[i];
    }
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < N; ++p)
            for (int q = p + 1; q < N; ++q) off += A[p * N + q] * A[p * N + q];
        if (!(off > 1e-36 * total)) break;   // converged (or NaN: nothing below would repair it)
#pragma unroll 1
        for (int p = 0; p < N - 1; ++p) {
#pragma unroll 1
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) {   // A <- A J
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {   // A <- J^T A
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; ++k) {   // V <- V J
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
        }
    }
    for (int i = 0; i < N; ++i) w[i] = A[i * N + i];
    for (int i = 0; i < N - 1; ++i) {   // selection sort, ascending
        int m = i;
        for (int j = i + 1; j < N; ++j)
            if (w[j] < w[m]) m = j;
        if (m != i) {
            const double tw = w[i];
            w[i] = w[m];
            w[m] = tw;
            for (int k = 0; k < N; ++k) {
                const double tv = V[k * N + i];
                V[k * N + i] = V[k * N + m];
                V[k * N + m] = tv;
            }
        }
    }
}

// ---- small dense solves ---------------------------------------------------------------------------------------------------------------
// Gaussian elimination with full pivoting on the M x M system A x = b (A, b destroyed).  least_squares: a pivot below 1e-13 of the first
// one ends the elimination and the remaining unknowns are 0 (a basic solution where np.linalg.lstsq gives the minimum-norm one);
// otherwise a zero or non-finite pivot returns false, as np.linalg.solve raises.
template <int M>
PNP_HD bool solve_pivoted(double* A, double* b, double* x, bool least_squares) {
    int perm[M];
    for (int i = 0; i < M; ++i) perm[i] = i;
    int rank = M;
    double first = 0.0;
    for (int k = 0; k < M; ++k) {
        int pr = k, pc = k;
        double best = -1.0;
        for (int i = k; i < M; ++i)
            for (int j = k; j < M; ++j) {
                const double a = fabs(A[i * M + j]);
                if (a > best) { best = a; pr = i; pc = j; }
            }
        if (k == 0) first = best;
        if (!finite(best) || best < 0.0) return false;
        if (least_squares ? !(best > 1e-13 * first) : best == 0.0) {
            if (!least_squares) return false;
            rank = k;
            break;
        }
        if (pr != k) {
            for (int j = 0; j < M; ++j) { const double t = A[k * M + j]; A[k * M + j] = A[pr * M + j]; A[pr * M + j] = t; }
            const double t = b[k]; b[k] = b[pr]; b[pr] = t;
        }
        if (pc != k) {
            for (int i = 0; i < M; ++i) { const double t = A[i * M + k]; A[i * M + k] = A[i * M + pc]; A[i * M + pc] = t; }
            const int t = perm[k]; perm[k] = perm[pc]; perm[pc] = t;
        }
        const double inv = 1.0 / A[k * M + k];
        for (int i = k + 1; i < M; ++i) {
            const double f = A[i * M + k] * inv;
            for (int j = k; j < M; ++j) A[i * M + j] -= f * A[k * M + j];
            b[i] -= f * b[k];
        }
    }
    double y[M];
    for (int i = 0; i < M; ++i) y[i] = 0.0;
    for (int k = rank - 1; k >= 0; --k) {
        double s = b[k];
        for (int j = k + 1; j < rank; ++j) s -= A[k * M + j] * y[j];
        y[k] = s / A[k * M + k];
    }
    for (int i = 0; i < M; ++i) x[perm[i]] = y[i];
    return true;
}

// min |J x - r| for a ROWS x COLS system through the normal equations J^T J x = J^T r
template <int ROWS, int COLS>
PNP_HD void least_squares(const double* J, const double* r, double* x) {
    double A[COLS * COLS], g[COLS];
    for (int a = 0; a < COLS; ++a) {
        for (int b = 0; b < COLS; ++b) {
            double s = 0.0;
            for (int i = 0; i < ROWS; ++i) s += J[i * COLS + a] * J[i * COLS + b];
            A[a * COLS + b] = s;
        }
        double s = 0.0;
        for (int i = 0; i < ROWS; ++i) s += J[i * COLS + a] * r[i];
        g[a] = s;
    }
    if (!solve_pivoted<COLS>(A, g, x, true))
        for (int a = 0; a < COLS; ++a) x[a] = 0.0;
}

// ---- rotations ------------------------------------------------------------------------------------------------------------------------
PNP_HD void skew(const double* v, double* S) {
    S[0] = 0.0; S[1] = -v[2]; S[2] = v[1];
    S[3] = v[2]; S[4] = 0.0; S[5] = -v[0];
    S[6] = -v[1]; S[7] = v[0]; S[8] = 0.0;
}
PNP_HD void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// pnp.rodrigues: axis-angle -> R
PNP_HD void rodrigues(const double* r, double* R) {
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    double Kx[9], K2[9];
    if (th < 1e-12) {
        skew(r, Kx);
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + Kx[i];
        return;
    }
    const double k[3] = {r[0] / th, r[1] / th, r[2] / th};
    skew(k, Kx);
    mul3(Kx, Kx, K2);
    const double s = sin(th), c1 = 1.0 - cos(th);
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + s * Kx[i] + c1 * K2[i];
}

// pnp.rodrigues_inverse: R -> axis-angle, with the branches near 0 and near pi
PNP_HD void rodrigues_inverse(const double* R, double* r) {
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double th = acos(c);
    const double w[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    if (th < 1e-8) {
        for (int i = 0; i < 3; ++i) r[i] = 0.5 * w[i];
        return;
    }
    if (3.141592653589793 - th < 1e-6) {   // the axis from the symmetric part
        double A[9];
        for (int i = 0; i < 9; ++i) A[i] = (R[i] + (i % 4 == 0 ? 1.0 : 0.0)) * 0.5;
        int m = 0;
        if (A[4] > A[m * 4]) m = 1;
        if (A[8] > A[m * 4]) m = 2;
        const double d = sqrt(dmax(A[m * 4], 1e-300));
        double ax[3] = {A[m] / d, A[3 + m] / d, A[6 + m] / d};
        if (ax[0] * w[0] + ax[1] * w[1] + ax[2] * w[2] < 0.0)
            for (int i = 0; i < 3; ++i) ax[i] = -ax[i];
        for (int i = 0; i < 3; ++i) r[i] = ax[i] * th;
        return;
    }
    const double f = th / (2.0 * sin(th));
    for (int i = 0; i < 3; ++i) r[i] = w[i] * f;
}

// ---- the problem of one (image, object) pair --------------------------------------------------------------------------------------------
struct Problem {
    int n;
    double X[MAX_POINTS * 3], x[MAX_POINTS * 2], K[9];
};

struct Pose {
    double R[9], t[3];
};

// pnp._reproj_error for point i: pixel = (K cam).xy / cam.z with |z| clamped away from 0
PNP_HD double reproj_error(const Problem& P, int i, const Pose& q) {
    const double* X = P.X + 3 * i;
    const double cx = q.R[0] * X[0] + q.R[1] * X[1] + q.R[2] * X[2] + q.t[0];
    const double cy = q.R[3] * X[0] + q.R[4] * X[1] + q.R[5] * X[2] + q.t[1];
    double z = q.R[6] * X[0] + q.R[7] * X[1] + q.R[8] * X[2] + q.t[2];
    const double cz = z;
    if (fabs(z) < 1e-12) z = 1e-12;
    const double u = (P.K[0] * cx + P.K[1] * cy + P.K[2] * cz) / z - P.x[2 * i];
    const double v = (P.K[3] * cx + P.K[4] * cy + P.K[5] * cz) / z - P.x[2 * i + 1];
    return sqrt(u * u + v * v);
}

// ---- EPnP (pnp.epnp) on the points idx[0..m) of P -------------------------------------------------------------------------------------
// pnp._pose_from_betas: control points in the camera frame = sum beta_k v_k; depth sign; absolute orientation.  The rotation that maximises
// sum (R X_i) . pc_i is the largest eigenvector of Horn's quaternion matrix: the same R as pnp.py's SVD with its det < 0 repair.
PNP_HD void pose_from_betas(const double* betas, int nb, const double* V, const double* al, const Problem& P, const uint8_t* idx, int m, Pose& out) {
    double cc[12], pc[MAX_POINTS * 3];
    for (int i = 0; i < 12; ++i) {
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s += betas[k] * V[i * 12 + k];
        cc[i] = s;
    }
    double zs = 0.0;
    for (int i = 0; i < m; ++i)
        for (int d = 0; d < 3; ++d) {
            double s = 0.0;
            for (int j = 0; j < 4; ++j) s += al[i * 4 + j] * cc[3 * j + d];
            pc[3 * i + d] = s;
            if (d == 2) zs += s;
        }
    if (zs / m < 0.0)
        for (int i = 0; i < 3 * m; ++i) pc[i] = -pc[i];
    double mc[3] = {0.0, 0.0, 0.0}, mw[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < m; ++i)
        for (int d = 0; d < 3; ++d) {
            mc[d] += pc[3 * i + d];
            mw[d] += P.X[3 * idx[i] + d];
        }
    for (int d = 0; d < 3; ++d) {
        mc[d] /= m;
        mw[d] /= m;
    }
    double S[9];   // S[a][b] = sum X_a pc_b
    for (int i = 0; i < 9; ++i) S[i] = 0.0;
    for (int i = 0; i < m; ++i)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[a * 3 + b] += (P.X[3 * idx[i] + a] - mw[a]) * (pc[3 * i + b] - mc[b]);
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                    Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                    Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                    Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
    double Q[16], ev[4];
    jacobi_eigh<4>(N, Q, ev);
    double qw = Q[3], qx = Q[7], qy = Q[11], qz = Q[15];
    const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw /= qn; qx /= qn; qy /= qn; qz /= qn;
    double* R = out.R;
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[1] = 2.0 * (qx * qy - qw * qz);       R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz);       R[4] = 1.0 - 2.0 * (qx * qx + qz * qz); R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy);       R[7] = 2.0 * (qy * qz + qw * qx);       R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    for (int d = 0; d < 3; ++d) out.t[d] = mc[d] - (R[3 * d] * mw[0] + R[3 * d + 1] * mw[1] + R[3 * d + 2] * mw[2]);
}

// the residuals rho_p - |sum beta_k dv[k][p]|^2 of the six control-point distances and their Jacobian; Gauss-Newton on the betas
template <int NB>
PNP_HD void gauss_newton(double* betas, const double* dv, const double* rho) {
#pragma unroll 1
    for (int it = 0; it < GN_STEPS; ++it) {
        double res[6], J[6 * NB], step[NB];
        for (int p = 0; p < 6; ++p) {
            double d[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < NB; ++k)
                for (int c = 0; c < 3; ++c) d[c] += betas[k] * dv[(k * 6 + p) * 3 + c];
            res[p] = -(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - rho[p]);
            for (int k = 0; k < NB; ++k) {
                const double* e = dv + (k * 6 + p) * 3;
                J[p * NB + k] = 2.0 * (e[0] * d[0] + e[1] * d[1] + e[2] * d[2]);
            }
        }
        least_squares<6, NB>(J, res, step);
        double n2 = 0.0;
        for (int k = 0; k < NB; ++k) {
            betas[k] += step[k];
            n2 += step[k] * step[k];
        }
        if (!(sqrt(n2) >= 1e-12)) break;
    }
}

PNP_HD bool epnp(const Problem& P, const uint8_t* idx, int m, Pose& best) {
    const double fu = P.K[0], fv = P.K[4], uc = P.K[2], vc = P.K[5];
    // pnp._control_points: the centroid and the three principal directions scaled by the standard deviations
    double cws[12], c0[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < m; ++i)
        for (int d = 0; d < 3; ++d) c0[d] += P.X[3 * idx[i] + d];
    for (int d = 0; d < 3; ++d) c0[d] /= m;
    {
        double C[9], E[9], w[3];
        for (int i = 0; i < 9; ++i) C[i] = 0.0;
        for (int i = 0; i < m; ++i)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) C[a * 3 + b] += (P.X[3 * idx[i] + a] - c0[a]) * (P.X[3 * idx[i] + b] - c0[b]);
        for (int i = 0; i < 9; ++i) C[i] /= m;
        jacobi_eigh<3>(C, E, w);
        for (int d = 0; d < 3; ++d) cws[d] = c0[d];
        for (int i = 0; i < 3; ++i) {
            const double s = sqrt(dmax(w[i], 0.0));
            for (int d = 0; d < 3; ++d) cws[3 * (i + 1) + d] = c0[d] + s * E[d * 3 + i];
        }
    }
    // pnp._barycentric
    double al[MAX_POINTS * 4];
    {
        double A[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) A[r * 3 + c] = cws[3 * (c + 1) + r] - cws[r];
        double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
        if (fabs(det) < 1e-12) {
            A[0] += 1e-9; A[4] += 1e-9; A[8] += 1e-9;
            det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
        }
        const double inv[9] = {(A[4] * A[8] - A[5] * A[7]) / det, (A[2] * A[7] - A[1] * A[8]) / det, (A[1] * A[5] - A[2] * A[4]) / det,
                               (A[5] * A[6] - A[3] * A[8]) / det, (A[0] * A[8] - A[2] * A[6]) / det, (A[2] * A[3] - A[0] * A[5]) / det,
                               (A[3] * A[7] - A[4] * A[6]) / det, (A[1] * A[6] - A[0] * A[7]) / det, (A[0] * A[4] - A[1] * A[3]) / det};
        for (int i = 0; i < m; ++i) {
            const double d[3] = {P.X[3 * idx[i]] - cws[0], P.X[3 * idx[i] + 1] - cws[1], P.X[3 * idx[i] + 2] - cws[2]};
            double s = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double a = inv[r * 3] * d[0] + inv[r * 3 + 1] * d[1] + inv[r * 3 + 2] * d[2];
                al[i * 4 + r + 1] = a;
                s += a;
            }
            al[i * 4] = 1.0 - s;
        }
    }
    // M^T M of the 2m x 12 system, accumulated row by row; its eigenvectors, ascending
    double MtM[144], V[144], w[12];
    for (int i = 0; i < 144; ++i) MtM[i] = 0.0;
#pragma unroll 1
    for (int i = 0; i < m; ++i) {
        double r0[12], r1[12];
        const double du = uc - P.x[2 * idx[i]], dv_ = vc - P.x[2 * idx[i] + 1];
        for (int j = 0; j < 4; ++j) {
            const double a = al[i * 4 + j];
            r0[3 * j] = a * fu; r0[3 * j + 1] = 0.0;    r0[3 * j + 2] = a * du;
            r1[3 * j] = 0.0;    r1[3 * j + 1] = a * fv; r1[3 * j + 2] = a * dv_;
        }
        for (int a = 0; a < 12; ++a)
            for (int b = 0; b < 12; ++b) MtM[a * 12 + b] += r0[a] * r0[b] + r1[a] * r1[b];
    }
    jacobi_eigh<12>(MtM, V, w);
    // differences of the control points of v_0..v_3 and of the world control points over the six pairs
    const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
    double rho[6], dv[4 * 6 * 3];
    for (int p = 0; p < 6; ++p) {
        double s = 0.0;
        for (int d = 0; d < 3; ++d) {
            const double e = cws[3 * pa[p] + d] - cws[3 * pb[p] + d];
            s += e * e;
        }
        rho[p] = s;
        for (int k = 0; k < 4; ++k)
            for (int d = 0; d < 3; ++d) dv[(k * 6 + p) * 3 + d] = V[(3 * pa[p] + d) * 12 + k] - V[(3 * pb[p] + d) * 12 + k];
    }
#define CP_PNP_DOT(k, l, p) (dv[((k)*6 + (p)) * 3] * dv[((l)*6 + (p)) * 3] + dv[((k)*6 + (p)) * 3 + 1] * dv[((l)*6 + (p)) * 3 + 1] + \
                             dv[((k)*6 + (p)) * 3 + 2] * dv[((l)*6 + (p)) * 3 + 2])
    double cand[3][3];
    {   // N = 1: beta^2 |dv0|^2 = rho
        double num = 0.0, den = 0.0;
        for (int p = 0; p < 6; ++p) {
            const double d = CP_PNP_DOT(0, 0, p);
            num += sqrt(d * rho[p]);
            den += d;
        }
        cand[0][0] = num / dmax(den, 1e-300);
    }
    {   // N = 2: linear in (b00, b01, b11)
        double L[18], b[3];
        for (int p = 0; p < 6; ++p) {
            L[p * 3] = CP_PNP_DOT(0, 0, p);
            L[p * 3 + 1] = 2.0 * CP_PNP_DOT(0, 1, p);
            L[p * 3 + 2] = CP_PNP_DOT(1, 1, p);
        }
        least_squares<6, 3>(L, rho, b);
        if (b[0] < 0.0)
            for (int i = 0; i < 3; ++i) b[i] = -b[i];
        cand[1][0] = sqrt(dmax(b[0], 0.0));
        cand[1][1] = sqrt(fabs(b[2])) * (b[1] >= 0.0 ? 1.0 : -1.0);
    }
    {   // N = 3: linear in (b00, b01, b02, b11, b12, b22)
        double L[36], b[6];
        for (int p = 0; p < 6; ++p) {
            L[p * 6] = CP_PNP_DOT(0, 0, p);
            L[p * 6 + 1] = 2.0 * CP_PNP_DOT(0, 1, p);
            L[p * 6 + 2] = 2.0 * CP_PNP_DOT(0, 2, p);
            L[p * 6 + 3] = CP_PNP_DOT(1, 1, p);
            L[p * 6 + 4] = 2.0 * CP_PNP_DOT(1, 2, p);
            L[p * 6 + 5] = CP_PNP_DOT(2, 2, p);
        }
        least_squares<6, 6>(L, rho, b);
        if (b[0] < 0.0)
            for (int i = 0; i < 6; ++i) b[i] = -b[i];
        cand[2][0] = sqrt(dmax(b[0], 0.0));
        cand[2][1] = sqrt(fabs(b[3])) * (b[1] >= 0.0 ? 1.0 : -1.0);
        cand[2][2] = sqrt(fabs(b[5])) * (b[2] >= 0.0 ? 1.0 : -1.0);
    }
#undef CP_PNP_DOT
    gauss_newton<1>(cand[0], dv, rho);
    gauss_newton<2>(cand[1], dv, rho);
    gauss_newton<3>(cand[2], dv, rho);
    bool found = false;
    double best_err = 0.0;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        Pose q;
        pose_from_betas(cand[c], c + 1, V, al, P, idx, m, q);
        double err = 0.0;
        for (int i = 0; i < m; ++i) err += reproj_error(P, idx[i], q);
        err /= m;
        if (finite(err) && (!found || err < best_err)) {
            best = q;
            best_err = err;
            found = true;
        }
    }
    return found;
}

// ---- LM on the all-point reprojection error in (rvec, t) (pnp.refine_lm) ------------------------------------------------------------------
// R(rvec) and the left Jacobian J_l of the rotation: R(rvec + d) ~ exp(J_l d) R
PNP_HD void rotation_and_left_jacobian(const double* p, double* R, double* Jl) {
    double Kx[9], K2[9];
    rodrigues(p, R);
    const double th = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    if (th < 1e-8) {
        skew(p, Kx);
        for (int i = 0; i < 9; ++i) Jl[i] = (i % 4 == 0 ? 1.0 : 0.0) + 0.5 * Kx[i];
    } else {
        const double k[3] = {p[0] / th, p[1] / th, p[2] / th};
        skew(k, Kx);
        mul3(Kx, Kx, K2);
        const double a = (1.0 - cos(th)) / th, b = 1.0 - sin(th) / th;
        for (int i = 0; i < 9; ++i) Jl[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * Kx[i] + b * K2[i];
    }
}

// point i of pnp._residual_and_jacobian: the residual (ru, rv) = projection - keypoint and its two Jacobian rows in (rvec, t)
PNP_HD void point_residual(const Problem& P, const double* p, const double* R, const double* Jl, int i, double& ru, double& rv, double* ju, double* jv) {
    const double fu = P.K[0], fv = P.K[4], sk = P.K[1];
    const double* X = P.X + 3 * i;
    const double Xr[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2], R[3] * X[0] + R[4] * X[1] + R[5] * X[2], R[6] * X[0] + R[7] * X[1] + R[8] * X[2]};
    const double cx = Xr[0] + p[3], cy = Xr[1] + p[4], z = Xr[2] + p[5];
    ru = fu * cx / z + P.K[2] + sk * cy / z - P.x[2 * i];
    rv = fv * cy / z + P.K[5] - P.x[2 * i + 1];
    const double du[3] = {fu / z, sk / z, -(fu * cx + sk * cy) / (z * z)}, dv[3] = {0.0, fv / z, -fv * cy / (z * z)};
    double S[9], D[9];   // d cam / d rvec = -[Xr]x J_l
    skew(Xr, S);
    mul3(S, Jl, D);
    for (int c = 0; c < 3; ++c) {
        ju[c] = -(du[0] * D[c] + du[1] * D[3 + c] + du[2] * D[6 + c]);
        jv[c] = -(dv[0] * D[c] + dv[1] * D[3 + c] + dv[2] * D[6 + c]);
        ju[3 + c] = du[c];
        jv[3 + c] = dv[c];
    }
}

// pnp._residual_and_jacobian, folded into the normal equations: cost = r.r, A = J^T J, g = J^T r
PNP_HD double residual_normal(const Problem& P, const double* p, double* A, double* g) {
    double R[9], Jl[9];
    rotation_and_left_jacobian(p, R, Jl);
    for (int i = 0; i < 36; ++i) A[i] = 0.0;
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    double cost = 0.0;
#pragma unroll 1
    for (int i = 0; i < P.n; ++i) {
        double ru, rv, ju[6], jv[6];
        point_residual(P, p, R, Jl, i, ru, rv, ju, jv);
        cost += ru * ru + rv * rv;
        for (int a = 0; a < 6; ++a) {
            g[a] += ju[a] * ru + jv[a] * rv;
            for (int b = 0; b < 6; ++b) A[a * 6 + b] += ju[a] * ju[b] + jv[a] * jv[b];
        }
    }
    return cost;
}

// ---- uncertainty-weighted LM (cp_pnp_weighted_f64): per point the lower Cholesky factor L of its 2x2 keypoint covariance -----------------
struct Whitening {
    double l00[MAX_POINTS], l10[MAX_POINTS], l11[MAX_POINTS];
};

// point i's factor from cov3 = (sxx, sxy, syy) in the pixels of points_xy: Sigma = cov + floor I, through the linear part M = [[a0, a1], [a3, a4]]
// of the crop->image affine Sigma' = M Sigma M^T, then Sigma' = L L^T.  false: Sigma' is non-finite or has no positive pivots
PNP_HD bool load_whitening(Whitening& W, int i, const float* cov3, double floor, const double* affine) {
    double s00 = (double)cov3[0] + floor, s01 = (double)cov3[1], s11 = (double)cov3[2] + floor;
    if (affine) {
        const double a = affine[0], b = affine[1], c = affine[3], d = affine[4];
        const double t00 = a * s00 + b * s01, t01 = a * s01 + b * s11, t10 = c * s00 + d * s01, t11 = c * s01 + d * s11;   // M Sigma
        s00 = t00 * a + t01 * b;
        s01 = t00 * c + t01 * d;
        s11 = t10 * c + t11 * d;
    }
    W.l00[i] = W.l11[i] = 1.0;
    W.l10[i] = 0.0;
    if (!(finite(s00) && finite(s01) && finite(s11)) || !(s00 > 0.0)) return false;
    const double l00 = sqrt(s00), l10 = s01 / l00, piv = s11 - l10 * l10;
    if (!(piv > 0.0) || !finite(l10) || !finite(piv)) return false;
    W.l00[i] = l00;
    W.l10[i] = l10;
    W.l11[i] = sqrt(piv);
    return true;
}

// residual_normal with every point's residual and Jacobian rows whitened by L^-1: cost = the Mahalanobis reprojection error
PNP_HD double residual_normal_weighted(const Problem& P, const Whitening& W, const double* p, double* A, double* g) {
    double R[9], Jl[9];
    rotation_and_left_jacobian(p, R, Jl);
    for (int i = 0; i < 36; ++i) A[i] = 0.0;
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    double cost = 0.0;
#pragma unroll 1
    for (int i = 0; i < P.n; ++i) {
        double ru, rv, ju[6], jv[6];
        point_residual(P, p, R, Jl, i, ru, rv, ju, jv);
        const double l00 = W.l00[i], l10 = W.l10[i], l11 = W.l11[i];
        ru = ru / l00;
        rv = (rv - l10 * ru) / l11;
        for (int a = 0; a < 6; ++a) {
            ju[a] = ju[a] / l00;
            jv[a] = (jv[a] - l10 * ju[a]) / l11;
        }
        cost += ru * ru + rv * rv;
        for (int a = 0; a < 6; ++a) {
            g[a] += ju[a] * ru + jv[a] * rv;
            for (int b = 0; b < 6; ++b) A[a * 6 + b] += ju[a] * ju[b] + jv[a] * jv[b];
        }
    }
    return cost;
}

// lam 1e-3, x0.1 on success, x10 on failure, <= 10 tries per iteration, at most max_iters iterations (pnp.pnp: 20), relative stop eps
// (pnp.pnp: 1e-10).  p = (rvec, t) in and out; returns the iterations entered; cost[0] = the squared error at the start, cost[1] at the end.
// WEIGHTED: the same schedule on residual_normal_weighted (W may be null otherwise); the unweighted instantiation never touches W.
template <bool WEIGHTED>
PNP_HD double lm_residual(const Problem& P, const Whitening* W, const double* p, double* A, double* g) {
    if constexpr (WEIGHTED) return residual_normal_weighted(P, *W, p, A, g);
    else return residual_normal(P, p, A, g);
}

template <bool WEIGHTED>
PNP_HD int refine_lm_t(const Problem& P, const Whitening* W, double* p, double* cost2, int max_iters, double eps) {
    double A[36], g[6], A2[36], g2[6], B[36], rhs[6], step[6], q[6];
    double lam = 1e-3, cost = lm_residual<WEIGHTED>(P, W, p, A, g);
    cost2[0] = cost;
    int iters = 0;
#pragma unroll 1
    for (int it = 0; it < max_iters; ++it) {
        ++iters;
        bool improved = false, done = false;
#pragma unroll 1
        for (int t = 0; t < LM_TRIES; ++t) {
            for (int i = 0; i < 36; ++i) B[i] = A[i];
            for (int i = 0; i < 6; ++i) {
                B[i * 7] += lam * dmax(A[i * 7], 1e-12);
                rhs[i] = -g[i];
            }
            if (!solve_pivoted<6>(B, rhs, step, false)) {
                lam *= 10.0;
                continue;
            }
            for (int i = 0; i < 6; ++i) q[i] = p[i] + step[i];
            const double c2 = lm_residual<WEIGHTED>(P, W, q, A2, g2);
            if (finite(c2) && c2 < cost) {
                for (int i = 0; i < 6; ++i) { p[i] = q[i]; g[i] = g2[i]; }
                for (int i = 0; i < 36; ++i) A[i] = A2[i];
                lam = dmax(lam * 0.1, 1e-12);
                done = (cost - c2) < eps * dmax(cost, 1e-30);
                cost = c2;
                improved = true;
                break;
            }
            lam *= 10.0;
        }
        if (!improved || done) break;
    }
    cost2[1] = cost;
    return iters;
}

PNP_HD int refine_lm(const Problem& P, double* p, double* cost2, int max_iters = LM_ITERS, double eps = LM_EPS) {
    return refine_lm_t<false>(P, nullptr, p, cost2, max_iters, eps);
}

// ---- one pair: load, hypotheses, consensus, final solve ---------------------------------------------------------------------------------
// point i of a pair: fp32 crop pixels through the optional crop->image affine (x' = a0 x + a1 y + a2, y' = a3 x + a4 y + a5), fp32 model point
PNP_HD void load_point(Problem& P, int i, const float* xy, const float* xyz, const double* affine) {
    const double x = (double)xy[2 * i], y = (double)xy[2 * i + 1];
    P.x[2 * i] = affine ? affine[0] * x + affine[1] * y + affine[2] : x;
    P.x[2 * i + 1] = affine ? affine[3] * x + affine[4] * y + affine[5] : y;
    for (int d = 0; d < 3; ++d) P.X[3 * i + d] = (double)xyz[3 * i + d];
}

// OK, or why this pair has no pose: a non-finite input, 2-D points that all coincide (a collapsed vote), 3-D points on one line
PNP_HD int check_problem(const Problem& P) {
    double m2[2] = {0.0, 0.0}, c0[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 9; ++i)
        if (!finite(P.K[i])) return NONFINITE_INPUT;
    for (int i = 0; i < P.n; ++i) {
        for (int d = 0; d < 2; ++d) {
            if (!finite(P.x[2 * i + d])) return NONFINITE_INPUT;
            m2[d] += P.x[2 * i + d];
        }
        for (int d = 0; d < 3; ++d) {
            if (!finite(P.X[3 * i + d])) return NONFINITE_INPUT;
            c0[d] += P.X[3 * i + d];
        }
    }
    double var2 = 0.0, C[9], E[9], w[3];
    for (int i = 0; i < 9; ++i) C[i] = 0.0;
    for (int i = 0; i < P.n; ++i) {
        for (int d = 0; d < 2; ++d) {
            const double e = P.x[2 * i + d] - m2[d] / P.n;
            var2 += e * e;
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) C[a * 3 + b] += (P.X[3 * i + a] - c0[a] / P.n) * (P.X[3 * i + b] - c0[b] / P.n);
    }
    if (!(var2 / P.n > 1e-12)) return DEGENERATE;
    jacobi_eigh<3>(C, E, w);
    if (!(w[1] > 1e-10 * w[2])) return DEGENERATE;
    return OK;
}

// what one hypothesis contributes to the consensus; count -1 marks a hypothesis without a pose
struct Score {
    int count;
    double sse;
    uint32_t mask;
};

// the total order of the consensus: most inliers, then the smallest sum of squared inlier errors, then the lowest hypothesis index
PNP_HD bool better(int ca, double sa, int ia, int cb, double sb, int ib) {
    if (ca != cb) return ca > cb;
    if (sa != sb) return sa < sb;
    return ia < ib;
}

PNP_HD Score score_hypothesis(const Problem& P, const uint8_t* set, double reprojection_error) {
    Score s = {-1, 0.0, 0u};
    uint8_t idx[SET_POINTS];
    for (int j = 0; j < SET_POINTS; ++j) {
        if ((int)set[j] >= P.n) return s;
        idx[j] = set[j];
    }
    Pose q;
    if (!epnp(P, idx, SET_POINTS, q)) return s;
    s.count = 0;
    for (int i = 0; i < P.n; ++i) {
        const double e = reproj_error(P, i, q);
        if (e <= reprojection_error) {
            ++s.count;
            s.sse += e * e;
            s.mask |= 1u << i;
        }
    }
    return s;
}

PNP_HD void zero_outputs(int status, float* pose, int32_t* info, float* cost) {
    for (int i = 0; i < 12; ++i) pose[i] = 0.f;
    info[0] = status; info[1] = -1; info[2] = 0; info[3] = 0;
    cost[0] = cost[1] = 0.f;
}

// EPnP on the consensus set (all points when it has fewer than 5, as pnp.pnp_rvec_t), then LM over all points: p = (rvec, t) in fp64,
// c2 = the squared error before and after LM.  false: no finite pose
// WEIGHTED: the final LM minimises the Mahalanobis error under W; the consensus set and both EPnP calls are the unweighted ones
template <bool WEIGHTED>
PNP_HD bool consensus_pose_t(const Problem& P, const Whitening* W, const Score& sc, double* p, double* c2, int& iters) {
    uint8_t idx[MAX_POINTS];
    int m = 0;
    if (sc.count >= SET_POINTS)
        for (int i = 0; i < P.n; ++i)
            if (sc.mask >> i & 1u) idx[m++] = (uint8_t)i;
    Pose q;
    bool ok = m >= SET_POINTS && epnp(P, idx, m, q);
    if (!ok) {
        for (int i = 0; i < P.n; ++i) idx[i] = (uint8_t)i;
        ok = epnp(P, idx, P.n, q);
    }
    if (!ok) return false;
    rodrigues_inverse(q.R, p);
    for (int d = 0; d < 3; ++d) p[3 + d] = q.t[d];
    iters = refine_lm_t<WEIGHTED>(P, W, p, c2, LM_ITERS, LM_EPS);
    bool fin = finite(c2[0]) && finite(c2[1]);
    for (int i = 0; i < 6; ++i) fin = fin && finite(p[i]);
    return fin;
}

PNP_HD bool consensus_pose(const Problem& P, const Score& sc, double* p, double* c2, int& iters) {
    return consensus_pose_t<false>(P, nullptr, sc, p, c2, iters);
}

// consensus_pose, then pnp.pnp's ending: (rvec, t) rounded to fp32, the pose negated when t_z < 0, a non-finite result replaced by the zero pose
template <bool WEIGHTED>
PNP_HD void finish_pair_t(const Problem& P, const Whitening* W, int winner, const Score& sc, float* pose, int32_t* info, float* cost) {
    double p[6], c2[2], R[9];
    int iters = 0;
    if (!consensus_pose_t<WEIGHTED>(P, W, sc, p, c2, iters)) {
        zero_outputs(NO_SOLUTION, pose, info, cost);
        return;
    }
    for (int i = 0; i < 6; ++i) p[i] = (double)(float)p[i];
    rodrigues(p, R);
    const double sgn = p[5] < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) pose[r * 4 + c] = (float)(sgn * R[r * 3 + c]);
        pose[r * 4 + 3] = (float)(sgn * p[3 + r]);
    }
    info[0] = OK; info[1] = winner; info[2] = sc.count < 0 ? 0 : sc.count; info[3] = iters;
    cost[0] = (float)c2[0];
    cost[1] = (float)c2[1];
}

PNP_HD void finish_pair(const Problem& P, int winner, const Score& sc, float* pose, int32_t* info, float* cost) {
    finish_pair_t<false>(P, nullptr, winner, sc, pose, info, cost);
}

// the consensus over the H hypotheses of the table, serially: what the kernels' blocks find with one thread per hypothesis
PNP_HD int consensus_serial(const Problem& P, const uint8_t* table, int H, double reprojection_error, Score& best) {
    best = {-2, 0.0, 0u};
    int winner = -1;
    for (int h = 0; h < H; ++h) {
        const Score s = score_hypothesis(P, table + SET_POINTS * h, reprojection_error);
        if (winner < 0 || better(s.count, s.sse, h, best.count, best.sse, winner)) {
            best = s;
            winner = h;
        }
    }
    return winner;
}

// the whole of one pair, serially: what the kernel's block computes with one thread per hypothesis
PNP_HD void solve_pair_serial(const float* xy, const float* xyz, const float* K, const double* affine, int n, const uint8_t* table, int H,
                              double reprojection_error, float* pose, int32_t* info, float* cost) {
    Problem P;
    P.n = n;
    for (int i = 0; i < 9; ++i) P.K[i] = (double)K[i];
    for (int i = 0; i < n; ++i) load_point(P, i, xy, xyz, affine);
    const int status = check_problem(P);
    if (status != OK) {
        zero_outputs(status, pose, info, cost);
        return;
    }
    Score best;
    const int winner = consensus_serial(P, table, H, reprojection_error, best);
    finish_pair(P, winner, best, pose, info, cost);
}

// solve_pair_serial with the final LM weighted by the keypoint covariances cov [n][3]; *weighted = 1 when every point's covariance was usable,
// otherwise 0 and the pair is solved exactly as solve_pair_serial solves it
PNP_HD void solve_pair_weighted_serial(const float* xy, const float* xyz, const float* K, const double* affine, const float* cov, double cov_floor,
                                       int n, const uint8_t* table, int H, double reprojection_error, float* pose, int32_t* info, float* cost,
                                       int32_t* weighted) {
    Problem P;
    Whitening W;
    P.n = n;
    for (int i = 0; i < 9; ++i) P.K[i] = (double)K[i];
    bool usable = true;
    for (int i = 0; i < n; ++i) {
        load_point(P, i, xy, xyz, affine);
        usable = load_whitening(W, i, cov + 3 * i, cov_floor, affine) && usable;
    }
    *weighted = 0;
    const int status = check_problem(P);
    if (status != OK) {
        zero_outputs(status, pose, info, cost);
        return;
    }
    Score best;
    const int winner = consensus_serial(P, table, H, reprojection_error, best);
    if (usable) finish_pair_t<true>(P, &W, winner, best, pose, info, cost);
    else finish_pair_t<false>(P, nullptr, winner, best, pose, info, cost);
    *weighted = usable ? 1 : 0;
}

// every pair of a batch, serially: the body of cp_pnp_weighted_host_f64 (pnp.hip) after its argument checks, and what wpnp_selftest.cpp runs
PNP_HD void solve_batch_weighted_serial(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine,
                                        const int32_t* solve, const uint8_t* table, int b, int oc, int n, int H, double reprojection_error,
                                        const float* cov, double cov_floor, float* poses, int32_t* info, float* cost, int32_t* weighted) {
    for (int pair = 0; pair < b * oc; ++pair) {
        float* pose = poses + (size_t)pair * 12;
        int32_t* inf = info + (size_t)pair * 4;
        float* cst = cost + (size_t)pair * 2;
        if (solve[pair] == 0) {
            zero_outputs(SKIPPED, pose, inf, cst);
            weighted[pair] = 0;
            continue;
        }
        const int image = pair / oc;
        solve_pair_weighted_serial(points_xy + (size_t)pair * n * 2, points_3d + (size_t)pair * n * 3, K + (k_per_image ? (size_t)image * 9 : 0),
                                   affine ? affine + (size_t)image * 6 : nullptr, cov + (size_t)pair * n * 3, cov_floor, n, table, H,
                                   reprojection_error, pose, inf, cst, weighted + pair);
    }
}

}  // namespace cp_pnp
