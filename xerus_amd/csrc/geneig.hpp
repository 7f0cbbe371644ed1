// The small generalised symmetric eigenproblem of a LOBPCG step (als_eig.hip): the smallest pair of H c = theta G c
// for the Gram pair G = S^T S, H = S^T M S of k = 2 or 3 basis vectors, in registers. One function for the kernel
// and for the host diagnostic xrs_geneig_lowest, so that its pivot rule can be tested without a GPU.
//
// The pencil is scaled to unit diagonal of G, G is Cholesky-factored, and the reduced k x k symmetric matrix
// L^-1 H L^-T is diagonalised by cyclic Jacobi. A squared Cholesky pivot below kGeneigPivotMin means that the last
// basis vector adds (numerically) nothing to the span: for k = 3 it is dropped and the 2 x 2 problem solved; if
// that fails too, or a value is not finite, the result is a breakdown.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace xrs {

constexpr double kGeneigPivotMin = 1e-8;   // the rounding error of the reduced problem grows like eps / pivot
constexpr int kGeneigSweeps = 10;          // (a 3 x 3 Jacobi iteration converges quadratically: 4-5 sweeps)
constexpr double kGeneigSkip = 1e-20;      // off-diagonal entries below this fraction of the diagonal are zero

__host__ __device__ inline bool geneig_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for NaN)

// the smallest pair of the leading k x k pencil of the full symmetric (finite) g, h; false: pivot rule or not finite
__host__ __device__ inline bool geneig_try(int k, const double (&g)[3][3], const double (&h)[3][3], double* theta, double* c) {
    double d[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < 3; ++i) {
        if (i >= k) break;
        if (!(g[i][i] > 0.0)) return false;
        d[i] = 1.0 / sqrt(g[i][i]);
    }
    double gs[3][3] = {}, hs[3][3] = {};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i < k && j < k) {
                gs[i][j] = g[i][j] * d[i] * d[j];
                hs[i][j] = h[i][j] * d[i] * d[j];
            }
    // Cholesky of the unit-diagonal Gram matrix
    double low[3][3] = {};
    low[0][0] = 1.0;
    low[1][0] = gs[0][1];
    const double p1 = 1.0 - low[1][0] * low[1][0];
    if (!(p1 >= kGeneigPivotMin)) return false;
    low[1][1] = sqrt(p1);
    if (k == 3) {
        low[2][0] = gs[0][2];
        low[2][1] = (gs[1][2] - low[2][0] * low[1][0]) / low[1][1];
        const double p2 = 1.0 - low[2][0] * low[2][0] - low[2][1] * low[2][1];
        if (!(p2 >= kGeneigPivotMin)) return false;
        low[2][2] = sqrt(p2);
    }
    // a = L^-1 Hs L^-T
    double w[3][3] = {}, a[3][3] = {};
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i)
            if (i < k && j < k) {
                double s = hs[i][j];
                for (int m = 0; m < i; ++m) s -= low[i][m] * w[m][j];
                w[i][j] = s / low[i][i];
            }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i < k && j < k) {
                double s = w[i][j];
                for (int m = 0; m < j; ++m) s -= a[i][m] * low[j][m];
                a[i][j] = s / low[j][j];
            }
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (j < k) a[i][j] = a[j][i] = 0.5 * (a[i][j] + a[j][i]);
    // cyclic Jacobi
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < kGeneigSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (q >= k) continue;
                const double apq = a[p][q];
                if (fabs(apq) <= kGeneigSkip * (fabs(a[p][p]) + fabs(a[q][q]))) {
                    a[p][q] = a[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double tau = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = t * cs;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
                for (int m = 0; m < 3; ++m)
                    if (m < k && m != p && m != q) {
                        const double amp = a[m][p], amq = a[m][q];
                        a[m][p] = a[p][m] = cs * amp - sn * amq;
                        a[m][q] = a[q][m] = sn * amp + cs * amq;
                    }
                for (int m = 0; m < 3; ++m)
                    if (m < k) {
                        const double vmp = v[m][p], vmq = v[m][q];
                        v[m][p] = cs * vmp - sn * vmq;
                        v[m][q] = sn * vmp + cs * vmq;
                    }
            }
        if (!rotated) break;
    }
    double lowest = a[0][0], y[3] = {v[0][0], v[1][0], v[2][0]};
    for (int i = 1; i < 3; ++i)
        if (i < k && a[i][i] < lowest) {
            lowest = a[i][i];
            for (int m = 0; m < 3; ++m) y[m] = v[m][i];
        }
    // coefficients: z = L^-T y, c = D z, scaled to unit G-norm, first coefficient non-negative
    double z[3] = {0.0, 0.0, 0.0}, co[3];
    for (int i = 2; i >= 0; --i)
        if (i < k) {
            double s = y[i];
            for (int m = i + 1; m < 3; ++m)
                if (m < k) s -= low[m][i] * z[m];
            z[i] = s / low[i][i];
        }
    for (int i = 0; i < 3; ++i) co[i] = z[i] * d[i];
    double nrm2 = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i < k && j < k) nrm2 += co[i] * g[i][j] * co[j];
    if (!(nrm2 > 0.0 && geneig_finite(nrm2))) return false;
    double scale = 1.0 / sqrt(nrm2);
    if (co[0] < 0.0) scale = -scale;
    for (int i = 0; i < 3; ++i) co[i] *= scale;
    double th = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (i < k && j < k) th += co[i] * h[i][j] * co[j];
    if (!(geneig_finite(th) && geneig_finite(co[0]) && geneig_finite(co[1]) && geneig_finite(co[2]))) return false;
    *theta = th;
    for (int i = 0; i < 3; ++i) c[i] = co[i];
    return true;
}

// G, H: the upper triangles, row by row, of the k x k pencil (k = 2: 00 01 11; k = 3: 00 01 02 11 12 22). Returns the
// number of basis vectors used (k, or k - 1 after dropping the last one) with *theta and c[0..2] (unused
// coefficients 0), or 0 on breakdown (*theta and c untouched).
__host__ __device__ inline int geneig_lowest(int k, const double* G, const double* H, double* theta, double* c) {
    double g[3][3] = {}, h[3][3] = {};
    int at = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j)
            if (j < k) {
                if (!(geneig_finite(G[at]) && geneig_finite(H[at]))) return 0;
                g[i][j] = g[j][i] = G[at];
                h[i][j] = h[j][i] = H[at];
                ++at;
            }
    if (k == 3 && geneig_try(3, g, h, theta, c)) return 3;
    if (geneig_try(2, g, h, theta, c)) return 2;
    return 0;
}

}  // namespace xrs
