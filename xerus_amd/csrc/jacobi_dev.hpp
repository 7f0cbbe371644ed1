// Device code shared by the one-sided Jacobi kernels (svd.hip, svd_batched.hip): 1/x and
// sqrt(x) from the hardware estimates, the rotation parameters and the stopping tolerance (every kernel), and the
// one-workgroup solve of k_jacobi_vt_lds, k_jacobi_vt_global and k_svd_batched: the circle-tournament pairing
// (circle_pair), the sweep / round loop with its stopping rule (jacobi_sweeps) and the row norms ranked
// descending (jacobi_rank_rows). What rotates a row pair stays with each kernel: rotate_pair in svd.hip, rotate_rows (the
// rows carry their accumulated rotations) in svd_batched.hip. The DPP lane-group sums (dpp, gsum<G>) come from
// reduce_dev.hpp. Internal linkage: each kernel file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include "reduce_dev.hpp"

namespace xrs {

namespace {

// 1/x and sqrt(x) to ~1 ulp from the hardware estimates + Newton steps (rotation parameters only need
// to be mutually consistent; no IEEE division / square-root sequences in the per-round critical path)
__device__ __forceinline__ double frcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}
__device__ __forceinline__ double fsqrt(double x) {   // x > 0
    double y = __builtin_amdgcn_rsq(x);
    double h = 0.5 * y;
    double g = x * y;
    double r = fma(-g, h, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    r = fma(-g, h, 0.5);
    return fma(g, r, g);
}

// Jacobi rotation zeroing the (i,j) entry of [[a c][c b]]: t = tan(theta) = sign(b - a) 2c /
// (|b - a| + sqrt((b - a)^2 + 4 c^2)) (the smaller root), c = 1/sqrt(1+t^2), s = t c, tau = s / (1 + c)
__device__ __forceinline__ void rotation(double a, double b, double c, double& s, double& tau, double& tn) {
    const double dd = b - a;
    const double hh = fsqrt(fma(dd, dd, 4.0 * c * c));
    tn = copysign(2.0, dd) * c * frcp(fabs(dd) + hh);
    const double qq = fsqrt(fma(tn, tn, 1.0));   // 1 / cos
    s = tn * frcp(qq);
    tau = tn * frcp(1.0 + qq);   // = s / (1 + cos); Rutishauser: x' = x - s (y + tau x), y' = y + s (x - tau y)
}
__device__ __forceinline__ void rotation(double a, double b, double c, double& s, double& tau) {
    double tn;
    rotation(a, b, c, s, tau, tn);
}

// dgesvj's stopping rule: rows i, j count as orthogonal when |w_i . w_j| <= tol ||w_i|| ||w_j||, tol = sqrt(q) u
__device__ __forceinline__ double jacobi_tol(int q) { return sqrt(double(q)) * 1.1102230246251565e-16; }

// Circle tournament of P (even) players: position 0 is fixed, the others move on by one per round, so the
// pairs (position t, position P-1-t), t < P/2, of rounds 0 .. P-2 meet every two players once. i, j: the
// players at positions t and P-1-t of round r (no integer divisions).
__device__ __forceinline__ void circle_pair(int t, int r, int P, int& i, int& j) {
    i = 0;
    if (t > 0) {
        i = t + r;
        i = i >= P ? i - (P - 1) : i;
    }
    j = P - 1 - t + r;
    j = j >= P ? j - (P - 1) : j;
}

// The sweeps of a one-workgroup solve on p rows by nt threads (all of them call this): per round the groups of
// G lanes take the pairs of circle_pair -- rot(i, j, lane) -> rotated? -- with one barrier per round, until a
// sweep went by without a rotation or max_sweeps are done. rotated: a word of LDS.
struct JacobiSweeps {
    int sweeps;
    bool converged;
};
template <int G, class Rot>
__device__ __forceinline__ JacobiSweeps jacobi_sweeps(int p, int nt, int max_sweeps, int* rotated, Rot rot) {
    const int tid = threadIdx.x, g = tid / G, l = tid % G, groups = nt / G;
    const int P = (p + 1) & ~1;
    JacobiSweeps r{0, false};
    for (; r.sweeps < max_sweeps && !r.converged; ++r.sweeps) {
        if (tid == 0) *rotated = 0;
        __syncthreads();
        for (int round = 0; round < P - 1; ++round) {
            for (int t = g; t < P / 2; t += groups) {
                int i, j;
                circle_pair(t, round, P, i, j);
                if (i >= p || j >= p) continue;   // (odd p: the bye)
                if (rot(i, j, l) && l == 0) *rotated = 1;
            }
            __syncthreads();
        }
        r.converged = *rotated == 0;
        __syncthreads();
    }
    return r;
}

// After the sweeps: sn[i] = the norm of row i of W (row stride ld) over its q data columns, rk[i] = its rank
// in descending order (ties by index: a stable order). sn, rk: p entries of LDS each, valid on return.
template <int G>
__device__ __forceinline__ void jacobi_rank_rows(const double* __restrict__ W, size_t ld, int p, int q, int nt, double* sn, int* rk) {
    const int tid = threadIdx.x, g = tid / G, l = tid % G, groups = nt / G;
    for (int i = g; i < p; i += groups) {
        const double* wi = W + size_t(i) * ld;
        double a = 0.0;
        for (int k = l; k < q; k += G) a = fma(wi[k], wi[k], a);
        a = gsum<G>(a);
        if (l == 0) sn[i] = sqrt(a);
    }
    __syncthreads();
    for (int i = tid; i < p; i += nt) {
        const double si = sn[i];
        int r = 0;
        for (int j = 0; j < p; ++j) r += (sn[j] > si) || (sn[j] == si && j < i);
        rk[i] = r;
    }
    __syncthreads();
}

}  // namespace

}  // namespace xrs
