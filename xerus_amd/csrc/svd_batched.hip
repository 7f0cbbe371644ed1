// Batched thin SVD: one launch factors `batch` small m x n matrices, one workgroup per matrix.
//
// Method (that of svd.hip's k_jacobi_vt_lds, per workgroup; the pairing, the sweep loop and the ranking of the row
// norms are the same code: jacobi_dev.hpp): one-sided Jacobi on the rows of the wide orientation
// W (p x q, p = min(m, n) <= q = max(m, n); W = A or A^T), resident in LDS for the whole solve. Round-robin
// pairing of the P = p rounded up to even players, a 16-lane group per pair with the lane's elements of both
// rows in registers, DPP-butterfly dot products, Rutishauser rotations, dgesvj's stopping rule
// |w_i . w_j| <= sqrt(q) u ||w_i|| ||w_j||. Unlike that kernel every row also carries, behind its q data
// columns, its row of the accumulated rotation product J (p identity columns at the start: the ACC layout of
// svd.hip's block kernel), so J W = diag(S) V and the p x p factor (U for a wide A, Vt for a tall one) is
// J^T resp. J: a product of rotations, orthonormal by construction and never divided by S.
//
// Workgroups are independent: no grid barrier, no spin on global memory, a fixed sweep bound. Each takes
// max |A_b| during the load, scales its entries by the exact power of two 2^-ilogb(max |A_b|) with ldexp
// (elementwise.hpp's range rule, per member) and scales S back, so members of very different magnitude
// share a batch. status[b] = sweeps, or -1 (see the certificate below); the driver recomputes the -1
// members through svd() and re-orthonormalises their factors (k_orthonormalise).
#include <climits>
#include <cmath>
#include <vector>

#include "jacobi_dev.hpp"
#include "smallla.hpp"
#include "svd_batched.hpp"

namespace xrs {

namespace {

constexpr int SB_G = 16;                  // lanes per row pair (one DPP row)
constexpr int SB_THREADS = 512;           // at most: 32 pairs in flight (p = 64 in one pass per round)
constexpr int SB_WIDTH = 512;             // p + q at most: 32 doubles per lane and row
constexpr size_t SB_LDS = 160 * 1024;     // LDS of a gfx950 compute unit
constexpr int SB_SWEEPS = 40;             // jacobi_vt's default bound
constexpr double SB_U = 1.1102230246251565e-16;

// row stride: >= p + q and 16 mod 32 doubles, so the two row pairs that share a 32-lane LDS access group
// (adjacent players: adjacent rows) fall on disjoint halves of the 64 banks
__host__ __device__ inline int sb_ld(int wt) { return ((wt + 15) / 32) * 32 + 16; }

// One Jacobi step on rows wi, wj = [w (q) | j (p)] by a 16-lane group (lane l): both rows in registers
// (wt = p + q <= 16 E), the dot products over the q data columns only, the rotation applied to all wt.
template <int E>
__device__ __forceinline__ bool rotate_rows(double* __restrict__ wi, double* __restrict__ wj, int q, int wt, int l, double tol2) {
    double x[E], y[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = l + e * SB_G;
        x[e] = k < wt ? wi[k] : 0.0;
        y[e] = k < wt ? wj[k] : 0.0;
    }
    double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const bool data = l + e * SB_G < q;
        const double xe = data ? x[e] : 0.0, ye = data ? y[e] : 0.0;
        a = fma(xe, xe, a);
        b = fma(ye, ye, b);
        c = fma(xe, ye, c);
    }
    a = gsum<SB_G>(a);
    b = gsum<SB_G>(b);
    c = gsum<SB_G>(c);
    if (!(c * c > tol2 * a * b)) return false;
    double s, tau;
    rotation(a, b, c, s, tau);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = l + e * SB_G;
        const double xe = x[e], ye = y[e];
        if (k < wt) {
            wi[k] = xe - s * fma(tau, xe, ye);
            wj[k] = ye + s * fma(-tau, ye, xe);
        }
    }
    return true;
}

// LDS (dynamic, sized by the driver from (m, n)): W p x ld | sn p | red 8 (doubles) | rk p | rotated (ints)
template <int E>
__global__ void __launch_bounds__(SB_THREADS) k_svd_batched(const double* __restrict__ A, int m, int n, int max_sweeps,
                                                            double* __restrict__ U, double* __restrict__ S,
                                                            double* __restrict__ Vt, int* __restrict__ status) {
    extern __shared__ double sb_lds[];
    const bool tall = m > n;
    const int p = tall ? n : m, q = tall ? m : n, wt = p + q, ld = sb_ld(wt);
    double* const W = sb_lds;
    double* const sn = W + p * ld;
    double* const red = sn + p;
    int* const rk = reinterpret_cast<int*>(red + 8);
    int* const rotated = rk + p;
    const int NT = blockDim.x, tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const double* __restrict__ Ab = A + b * size_t(m) * n;

    // max |A_b| (NaNs are skipped: they reach the norms below and fail the certificate)
    double mx = 0.0;
    for (int e = tid; e < m * n; e += NT) {
        const double v = fabs(Ab[e]);
        mx = v > mx ? v : mx;
    }
    mx = wave_max_gt(mx);
    wave_partials(mx, red);
    mx = red[0];
    for (int i = 1; i < NT / 64; ++i) mx = red[i] > mx ? red[i] : mx;
    const int ex = (mx > 0.0 && mx <= 1.7976931348623157e308) ? ilogb(mx) : 0;

    // W = 2^-ex A (wide) or its transpose (tall), read along A's rows; then the identity columns
    for (int e = tid; e < m * n; e += NT) {
        const int r = e / n, c = e - r * n;
        const double v = ldexp(Ab[e], -ex);
        if (tall) W[c * ld + r] = v;
        else W[r * ld + c] = v;
    }
    for (int e = tid; e < p * p; e += NT) {
        const int i = e / p, j = e - i * p;
        W[i * ld + q + j] = i == j ? 1.0 : 0.0;
    }

    const double tol = jacobi_tol(q);
    const double tol2 = tol * tol;
    const JacobiSweeps done = jacobi_sweeps<SB_G>(p, NT, max_sweeps, rotated, [&](int i, int j, int l) {
        return rotate_rows<E>(W + i * ld, W + j * ld, q, wt, l, tol2);
    });

    // singular values = row norms of the data columns, ranked descending
    jacobi_rank_rows<SB_G>(W, size_t(ld), p, q, NT, sn, rk);
    for (int i = tid; i < p; i += NT) S[b * p + rk[i]] = ldexp(sn[i], ex);
    // Certificate. The stopping rule leaves |w_i . w_j| <= tol ||w_i|| ||w_j||, tol = sqrt(q) u, unrotated:
    // each of the other p - 1 rows may keep a component of up to tol ||w_j|| <= tol s_max along the direction
    // of row i, (p - 1) tol s_max in all. A row whose norm does not exceed that sum need hold nothing else,
    // so its normalisation is not a trustworthy singular vector (and a zero row has none): the member counts
    // as numerically rank-deficient unless s_min > p tol s_max. (All-zero and NaN members fail the comparison.)
    if (tid == 0) {
        double smin = sn[0], smax = sn[0];
        for (int i = 1; i < p; ++i) {
            smin = sn[i] < smin ? sn[i] : smin;
            smax = sn[i] > smax ? sn[i] : smax;
        }
        const bool full = smin > double(p) * tol * smax;
        status[b] = (done.converged && full) ? done.sweeps : -1;
    }
    // J W = diag(sn) V: wide A = J^T diag(sn) V (U = J^T, Vt = V), tall A = V^T diag(sn) J (U = V^T, Vt = J)
    double* __restrict__ Ub = U + b * size_t(m) * p;
    double* __restrict__ Vb = Vt + b * size_t(p) * n;
    if (tall) {
        for (int e = tid; e < p * q; e += NT) {
            const int k = e / p, i = e - k * p;
            const double s = sn[i];
            Ub[k * p + rk[i]] = s > 0.0 ? W[i * ld + k] / s : 0.0;
        }
        for (int e = tid; e < p * p; e += NT) {
            const int i = e / p, i2 = e - i * p;
            Vb[rk[i] * p + i2] = W[i * ld + q + i2];
        }
    } else {
        for (int e = tid; e < p * q; e += NT) {
            const int i = e / q, k = e - i * q;
            const double s = sn[i];
            Vb[rk[i] * q + k] = s > 0.0 ? W[i * ld + k] / s : 0.0;
        }
        for (int e = tid; e < p * p; e += NT) {
            const int i2 = e / p, i = e - i2 * p;
            Ub[i2 * p + rk[i]] = W[i * ld + q + i2];
        }
    }
}

// Orthonormal bases for a recomputed member. svd()'s Jacobi routes normalise the rows of one factor by S, so
// an exactly rank-deficient member comes back with a zero vector for a singular value that is exactly zero, and
// (measured on an exactly rank-2 16 x 16 member) with unit vectors that are not mutually orthogonal for the
// singular values at rounding level. The k vectors x_r (length n, element c of vector r at X[r * rs + c * cs],
// ordered by descending singular value) are therefore taken through Gram-Schmidt in that order: x_z is
// projected against x_0 .. x_{z-1} and normalised, three times (each pass on a unit vector: whatever fraction of
// x_z survives the first pass, the last one starts from a vector that is orthogonal to O(sqrt(u)) and leaves
// O(u)). Vectors that were orthonormal move by O(u); a defective one belongs to a singular value of rounding
// size, so U S Vt is unchanged to O(u ||A||). A vector that is zero, or lies exactly in the span of its
// predecessors to working precision (remainder < sqrt(u)), is replaced by the coordinate vector e_c of the
// column c in which those have the least weight (its remainder has norm^2 >= 1 / n). One workgroup; k <= 256 (the envelope: p <= q, p + q <= 512).
constexpr int CB_THREADS = 256, CB_MAXK = 256;

// Workgroup barrier that also orders global memory: the threads hand the vectors to one another through
// global memory, and __syncthreads() alone only fences LDS (a store may still be in flight behind it).
__device__ __forceinline__ void cb_sync() {
    __threadfence_block();
    __syncthreads();
}

__device__ __forceinline__ double cb_block_sum(double v, double* red4) {
    v = wave_sum(v);
    cb_sync();   // (red4 may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    cb_sync();
    return sum_pairwise4(red4);
}

// (X is not __restrict__: other threads write what this one reads, across the barriers)
__global__ void __launch_bounds__(CB_THREADS) k_orthonormalise(double* X, int k, int n, int rs, int cs) {
    __shared__ double d[CB_MAXK];
    __shared__ double red4[4], best_v[CB_THREADS / 64];
    __shared__ int best_c[CB_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WAVES = CB_THREADS / 64;
    auto at = [&](int r, int c) -> double& { return X[size_t(r) * rs + size_t(c) * cs]; };
    for (int z = 0; z < k; ++z) {
        double nn = 0.0;
        for (int c = tid; c < n; c += CB_THREADS) nn = fma(at(z, c), at(z, c), nn);
        nn = cb_block_sum(nn, red4);   // (the same bits in every thread: the branches below are uniform)
        for (int attempt = 0; attempt < 2; ++attempt) {
            if (!(nn > 0.0)) {
                // e_c of the column with the least weight in x_0 .. x_{z-1} (ties: the first)
                double bv = 2.0;
                int bc = n;
                for (int c = tid; c < n; c += CB_THREADS) {
                    double s = 0.0;
                    for (int r = 0; r < z; ++r) s = fma(at(r, c), at(r, c), s);
                    if (s < bv) {
                        bv = s;
                        bc = c;
                    }
                }
                wave_arg_best(bv, bc, [](double a, double b) { return a < b; });
                cb_sync();   // (best_* may still be read from an earlier vector)
                if (lane == 0) {
                    best_v[wave] = bv;
                    best_c[wave] = bc;
                }
                cb_sync();
                for (int w = 0; w < WAVES; ++w)
                    if (best_v[w] < bv || (best_v[w] == bv && best_c[w] < bc)) {
                        bv = best_v[w];
                        bc = best_c[w];
                    }
                for (int c = tid; c < n; c += CB_THREADS) at(z, c) = c == bc ? 1.0 : 0.0;
                nn = 1.0;
                cb_sync();
            }
            for (int pass = 0; pass < 3 && nn > 0.0; ++pass) {
                const double inv = 1.0 / sqrt(nn);
                for (int c = tid; c < n; c += CB_THREADS) at(z, c) *= inv;
                cb_sync();
                for (int r = wave; r < z; r += WAVES) {
                    double s = 0.0;
                    for (int c = lane; c < n; c += 64) s = fma(at(r, c), at(z, c), s);
                    s = wave_sum(s);
                    if (lane == 0) d[r] = s;
                }
                cb_sync();
                double part = 0.0;
                for (int c = tid; c < n; c += CB_THREADS) {
                    double s = 0.0;
                    for (int r = 0; r < z; ++r) s = fma(d[r], at(r, c), s);
                    const double v = at(z, c) - s;
                    at(z, c) = v;
                    part = fma(v, v, part);
                }
                nn = cb_block_sum(part, red4);
                // less than half the digits survive (remainder below sqrt(u) of a unit vector): x_z lies in the
                // span of its predecessors and what is left is rounding noise, which need not leave that span
                // (duplicate columns of A round identically in every vector) -- take e_c instead
                if (nn < SB_U) nn = 0.0;
            }
            if (nn > 0.0) break;
        }
        const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
        for (int c = tid; c < n; c += CB_THREADS) at(z, c) *= inv;
        cb_sync();
    }
}

// both factors of one member: the columns of U (m x k) and the rows of Vt (k x n)
void orthonormalise_factors(xrs_handle_t h, double* U, double* Vt, size_t m, size_t n) {
    const size_t k = std::min(m, n);
    XRS_REQUIRE(k <= size_t(CB_MAXK), "svd_batched: orthonormalise_factors needs min(m, n) <= 256");
    hipLaunchKernelGGL(k_orthonormalise, dim3(1), dim3(CB_THREADS), 0, h->stream, U, int(k), int(m), 1, int(k));
    check_launch("k_orthonormalise");
    hipLaunchKernelGGL(k_orthonormalise, dim3(1), dim3(CB_THREADS), 0, h->stream, Vt, int(k), int(n), int(n), 1);
    check_launch("k_orthonormalise");
}

template <int E>
void launch_svd_batched(xrs_handle_t h, const double* A, size_t batch, int m, int n, double* U, double* S, double* Vt, int* status_dev) {
    const int p = std::min(m, n);
    const int pairs = std::max(1, (p + 1) / 2);
    const int threads = std::min(SB_THREADS, ((pairs * SB_G + 63) / 64) * 64);
    const size_t bytes = svd_batched_lds_bytes(size_t(m), size_t(n));
    if (bytes > 64 * 1024) {
        XRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_svd_batched<E>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    int(SB_LDS)));
    }
    hipLaunchKernelGGL(k_svd_batched<E>, dim3(unsigned(batch)), dim3(unsigned(threads)), bytes, h->stream, A, m, n, SB_SWEEPS, U, S, Vt,
                       status_dev);
    check_launch("k_svd_batched");
}

}  // namespace

size_t svd_batched_lds_bytes(size_t m, size_t n) {
    const size_t p = std::min(m, n), q = std::max(m, n);
    if (p == 0 || p + q > size_t(SB_WIDTH)) return 0;
    return 8 * (p * size_t(sb_ld(int(p + q))) + p + 8) + 4 * (p + 2);
}

bool svd_batched_fits(size_t m, size_t n) {
    const size_t bytes = svd_batched_lds_bytes(m, n);
    return bytes != 0 && bytes <= SB_LDS;
}

void svd_batched(xrs_handle_t h, const double* A, size_t batch, size_t m, size_t n, double* U, double* S, double* Vt,
                 int* status_host) {
    XRS_REQUIRE(m > 0 && n > 0, "Dimension m and n must be larger than zero");
    XRS_REQUIRE(batch <= size_t(INT_MAX), "svd_batched: batch too large");
    if (batch == 0) return;
    const size_t k = std::min(m, n);
    std::vector<int> st(batch, -1);
    const bool inside = svd_batched_fits(m, n);
    if (inside) {
        DevBuf st_dev(h, batch * sizeof(int));
        {
            KernelTimer timer(h, XRS_KFAM_SVD, double(batch) * 3.5 * double(k) * k * (m + n) * 6.0, double(batch) * 16.0 * (m * n + k * k));
            const int wt = int(m + n);
            if (wt <= 32) launch_svd_batched<2>(h, A, batch, int(m), int(n), U, S, Vt, st_dev.as<int>());
            else if (wt <= 64) launch_svd_batched<4>(h, A, batch, int(m), int(n), U, S, Vt, st_dev.as<int>());
            else if (wt <= 128) launch_svd_batched<8>(h, A, batch, int(m), int(n), U, S, Vt, st_dev.as<int>());
            else if (wt <= 256) launch_svd_batched<16>(h, A, batch, int(m), int(n), U, S, Vt, st_dev.as<int>());
            else launch_svd_batched<32>(h, A, batch, int(m), int(n), U, S, Vt, st_dev.as<int>());
        }
        // the one host synchronisation of the batch
        XRS_HIP(hipMemcpyAsync(st.data(), st_dev.d(), batch * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        XRS_HIP(hipStreamSynchronize(h->stream));
    }
    for (size_t b = 0; b < batch; ++b) {
        if (st[b] >= 0) continue;
        st[b] = -1;
        svd(h, A + b * m * n, m, n, U + b * m * k, S + b * k, Vt + b * k * n);
        if (inside) orthonormalise_factors(h, U + b * m * k, Vt + b * k * n, m, n);
    }
    if (status_host)
        for (size_t b = 0; b < batch; ++b) status_host[b] = st[b];
}

}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_svd_batched(xrs_handle_t h, double* U, double* S, double* Vt, int* status, const double* A, size_t batch, size_t m, size_t n) {
    return guarded([&] {
        XRS_REQUIRE(h, "null argument");
        if (batch == 0) return;
        XRS_REQUIRE(U && S && Vt && A, "null argument");
        fence_readers(h);
        svd_batched(h, A, batch, m, n, U, S, Vt, status);
    });
}

int xrs_svd_batched_fits(size_t m, size_t n) { return svd_batched_fits(m, n) ? 1 : 0; }

}  // extern "C"
