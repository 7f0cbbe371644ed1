// Top-kk eigenpairs of a symmetric n x n matrix (n <= 256) for the certified truncating round: the
// reference computes the edge's singular vectors with dgesdd (tensor.cpp:1424-1489); where the round has
// certified the edge Gram P = B B^T to be well conditioned and the kept rank kk is fixed in advance
// (tt_trunc.hip round_truncate), the kept left singular vectors of B are the eigenvectors of P's kk
// largest eigenvalues. Three launches, LAPACK's dsytrd / dstebz / dstein / dormtr structure:
//   1. k_sytrd: Householder tridiagonalisation A = Q T Q^T in ONE workgroup, the matrix register-resident
//      (n <= 64: 1024 threads on a 32 x 32 grid, element (i, k) on thread (i mod 32, k mod 32): the
//      shrinking trailing block stays spread over every thread; 65..256: k_sytrd_l512<NR>, 512 threads
//      holding the lower block triangle of NR 32-row block rows, finished block rows / columns skipped by a
//      compile-time switch). Per column: the reflector from one wave, the symmetric matrix-vector product
//      with in-wave DPP / permlane reductions, the rank-2 update in registers -- LDS-only barriers.
//   2. k_stebz_stein: one wave per wanted eigenvalue (kk workgroups in parallel): Sturm-count
//      multisection on 64 points per round (~9 rounds to full precision; the counts as sign changes of the
//      three-term minor recurrence, one FMA per level on the chain), then inverse iteration with the
//      partially pivoted LU of T - (lambda + 64 u ||T||) I (dgttrf / dgttrs), three solves from a start vector
//      hashed from (row, eigenvalue index) (stein_start; the shift's offset keeps clusters independent), every
//      chain fed by operands read ahead in blocks (r04: 104 -> 73 us at order 128, the chains now
//      FP64-issue-bound, profiles/r04/stein_phases_r04z.txt).
//      Measured alternatives (profiles/r03/stein_variants_r03r.txt): a single twisted-factorisation solve
//      (orthogonality only 1e-12..1e-11 on flat spectra, T - lambda I not being a relatively robust
//      representation); 4 waves with 512 points per round (6 instead of 9 rounds, no gain with r03's chains).
//   3. k_ormtr: the eigenvectors back to A's coordinates, u = H_0 ... H_{n-2} z, one wave per vector
//      (64 lanes, 4 vectors per workgroup), the reflectors staged through LDS in chunks.
//   2b. k_cluster_orth: vectors of eigenvalue clusters (gaps <= 1e-3 ||T||, dstein's ORTOL) orthonormalised
//      by two modified Gram-Schmidt passes (dstein's reorthogonalisation within a cluster); a vector that
//      collapses against its predecessors sets status -3 (never a wrong vector with status 0).
// Measured dead end (round 4, profiles/r04/twostage_*_r04h.*): a two-stage tridiagonalisation (dense -> band
// 16 by MFMA panel updates, band -> tridiagonal by bulge chasing, Q2/Q1 back-transformation) ran 303 + 333
// + 186 us at n = 128 against this kernel's 330 us (cfg3 round(64): 8.25 vs 4.5 ms): in one workgroup every
// panel and bulge step is a chain of LDS / L2 round trips, where the register-resident column step is not.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "scratch_map.hpp"
#include "reduce_dev.hpp"
#include "smallla.hpp"

namespace xrs {

namespace {

constexpr int SY_MAX = 256;

// workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its global
// stores (__syncthreads' release fence would drain the per-column stores of the reflectors, d, e and tau
// to memory at every barrier of the column loop)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int NEWTON>
__device__ __forceinline__ double rcpn(double x) {   // 1/x: hardware estimate + NEWTON Newton steps
    double r = __builtin_amdgcn_rcp(x);
#pragma unroll
    for (int it = 0; it < NEWTON; ++it) r = fma(r, fma(-x, r, 1.0), r);
    return r;
}

__device__ __forceinline__ double rcp2(double x) {   // 1/x to ~1 ulp (hardware estimate + 2 Newton steps)
    double r = __builtin_amdgcn_rcp(x);
    double t = fma(-x, r, 1.0);
    r = fma(r, t, r);
    t = fma(-x, r, 1.0);
    return fma(r, t, r);
}

// LAPACK dsytd2 (lower) on the register grid (element (i, k) on thread (i mod GRID, k mod GRID)). V: row j = Householder vector v_j (v_j[i] = 0 for i <= j,
// v_j[j + 1] = 1); d (n), e (n - 1), tau (n - 1). A is read from its lower triangle.
// GRID x GRID threads (GRID = 32: 16 waves; GRID = 16: 4 waves, one per SIMD, NB x NB = 64 elements per
// thread at n = 128 -- fewer waves to wait for at every barrier and no SIMD shared between waves)
template <int GRID, int NB>
__global__ void __launch_bounds__(GRID * GRID) k_sytrd(const double* __restrict__ A, int lda, int n, double* __restrict__ d,
                                                double* __restrict__ e, double* __restrict__ tau, double* __restrict__ V,
                                                unsigned long long* __restrict__ stamps) {
    // diagnostics (stamps != null): threads 0 and 64 record s_memtime at 6 points of every column step
#define SYTRD_STAMP(p)                                                                                  \
    do {                                                                                                \
        if (stamps && (threadIdx.x == 0 || threadIdx.x == 64) && j < 64)                                 \
            stamps[(threadIdx.x == 0 ? 0 : 384) + 6 * j + (p)] = __builtin_amdgcn_s_memtime();           \
    } while (0)
    __shared__ double xs[SY_MAX], vs[SY_MAX], ps[SY_MAX];
    __shared__ double sh_tau;
    const int t = threadIdx.x, tr = t / GRID, tc = t % GRID, lane = t & 63, wave = t >> 6;
    constexpr int NP = GRID * NB;   // padded order
    double a[NB][NB];
#pragma unroll
    for (int ia = 0; ia < NB; ++ia)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
            const int i = tr + GRID * ia, k = tc + GRID * ib;
            a[ia][ib] = (i < n && k < n) ? (i >= k ? A[size_t(i) * lda + k] : A[size_t(k) * lda + i]) : 0.0;
        }
    // column j of the current matrix to LDS (xs) and its diagonal entry to d, by the column's owners
    auto publish_column = [&](int j) {
        if (tc == (j % GRID)) {
#pragma unroll
            for (int ia = 0; ia < NB; ++ia) {
                const int i = tr + GRID * ia;
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
                    if (ib == (j / GRID)) {
                        if (i > j && i < n) xs[i] = a[ia][ib];
                        if (i == j) d[j] = a[ia][ib];
                    }
            }
        }
    };
    publish_column(0);
    for (int j = 0; j + 2 < n; ++j) {
        SYTRD_STAMP(0);
        lds_barrier();
        SYTRD_STAMP(1);
        // (b) reflector (dlarfg): beta = -sign(alpha) ||(alpha, x)||, tau = (beta - alpha) / beta,
        //     v = (1, x / (alpha - beta))
        if (wave == 0) {
            constexpr int E = NP >= 64 ? NP / 64 : 1;   // entries per lane of the NP padded indices
            double x[E];
#pragma unroll
            for (int q = 0; q < E; ++q) x[q] = (lane + 64 * q < NP) ? xs[lane + 64 * q] : 0.0;
            const double alpha = xs[j + 1];
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int i = lane + 64 * q;
                if (i >= j + 2 && i < n) s = fma(x[q], x[q], s);
            }
            s = gsum<64>(s);
            double tv = 0.0, beta = alpha, scal = 0.0;
            if (s > 0.0) {
                beta = -copysign(sqrt(fma(alpha, alpha, s)), alpha);
                tv = (beta - alpha) * rcp2(beta);
                scal = rcp2(alpha - beta);
            }
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int i = lane + 64 * q;
                const double v = (i <= j || i >= n) ? 0.0 : (i == j + 1 ? 1.0 : x[q] * scal);
                if (i < NP) vs[i] = v;
                if (i < n) V[size_t(j) * n + i] = v;
            }
            if (lane == 0) {
                sh_tau = tv;
                e[j] = beta;
                tau[j] = tv;
            }
        }
        SYTRD_STAMP(2);
        lds_barrier();
        SYTRD_STAMP(3);
        const double tj = sh_tau;   // (tau = 0: p = w = 0, the update leaves A unchanged; no second latch)
        // (c) p = tau A v on the trailing block: row partials (NB independent chains), reduced over the 32
        //     column threads of a row level by level across the rows (ILP in the DPP chain)
        {
            double part[NB], vcol[NB];
#pragma unroll
            for (int ib = 0; ib < NB; ++ib) vcol[ib] = vs[tc + GRID * ib];
#pragma unroll
            for (int ia = 0; ia < NB; ++ia) {
                part[ia] = 0.0;
#pragma unroll
                for (int ib = 0; ib < NB; ++ib) part[ia] = fma(a[ia][ib], vcol[ib], part[ia]);
            }
#pragma unroll
            for (int ia = 0; ia < NB; ++ia) part[ia] += dpp<0x128>(part[ia]);
#pragma unroll
            for (int ia = 0; ia < NB; ++ia) part[ia] += dpp<0x124>(part[ia]);
#pragma unroll
            for (int ia = 0; ia < NB; ++ia) part[ia] += dpp<0x122>(part[ia]);
#pragma unroll
            for (int ia = 0; ia < NB; ++ia) part[ia] += dpp<0x121>(part[ia]);
            if constexpr (GRID == 32) {
#pragma unroll
                for (int ia = 0; ia < NB; ++ia) part[ia] = addx16(part[ia]);
            }
            if (tc == 0) {
#pragma unroll
                for (int ia = 0; ia < NB; ++ia) {
                    const int i = tr + GRID * ia;
                    ps[i] = (i > j && i < n) ? tj * part[ia] : 0.0;
                }
            }
        }
        for (int q = NP + t; q < SY_MAX; q += GRID * GRID) ps[q] = 0.0;
        SYTRD_STAMP(4);
        lds_barrier();
        SYTRD_STAMP(5);
        // (d) every wave forms K = -(tau / 2) (p . v) itself (no extra barrier), w = p + K v on the fly;
        //     the update's operands are read before the reduction so their LDS latency overlaps it
        double vr[NB], pr[NB], vc[NB], pc[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            vr[q] = vs[tr + GRID * q];
            pr[q] = ps[tr + GRID * q];
            vc[q] = vs[tc + GRID * q];
            pc[q] = ps[tc + GRID * q];
        }
        double sk = 0.0;
#pragma unroll
        for (int i = lane; i < NP; i += 64) sk = fma(ps[i], vs[i], sk);
        const double K = -0.5 * tj * gsum<64>(sk);
        // (e) A -= v w^T + w v^T (v, w vanish at indices <= j: finished rows and columns stay untouched), on
        //     the active blocks only: block rows / columns below (j + 1) / GRID are finished, so one
        //     compile-time loop nest per first active block (a switch, not per-block branches)
        auto update_from = [&](auto jb_c) {
            constexpr int JB = decltype(jb_c)::value;
#pragma unroll
            for (int ib = JB; ib < NB; ++ib) {
                const double wc = fma(K, vc[ib], pc[ib]);
#pragma unroll
                for (int ia = JB; ia < NB; ++ia) a[ia][ib] = fma(-vr[ia], wc, fma(-fma(K, vr[ia], pr[ia]), vc[ib], a[ia][ib]));
            }
        };
        switch ((j + 1) / GRID) {
            case 0: update_from(std::integral_constant<int, 0>{}); break;
            case 1: if constexpr (NB > 1) update_from(std::integral_constant<int, (NB > 1 ? 1 : 0)>{}); break;
            case 2: if constexpr (NB > 2) update_from(std::integral_constant<int, (NB > 2 ? 2 : 0)>{}); break;
            default: if constexpr (NB > 3) update_from(std::integral_constant<int, (NB > 3 ? 3 : 0)>{}); break;
        }
        publish_column(j + 1);
    }
#undef SYTRD_STAMP
    // the last 2 x 2 block: d[n-2], d[n-1], e[n-2] (tau = 0, H = I)
#pragma unroll
    for (int ia = 0; ia < NB; ++ia)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) {
            const int i = tr + GRID * ia, k = tc + GRID * ib;
            if (n >= 2 && i == n - 2 && k == n - 2) d[n - 2] = a[ia][ib];
            if (n >= 1 && i == n - 1 && k == n - 1) d[n - 1] = a[ia][ib];
            if (n >= 2 && i == n - 1 && k == n - 2) {
                e[n - 2] = a[ia][ib];
                tau[n - 2] = 0.0;
                for (int q = 0; q < n; ++q) V[size_t(n - 2) * n + q] = 0.0;
            }
        }
}

// Orders 129..256: the same column steps on 512 threads (8 waves, two per SIMD: 256 VGPRs each) holding
// the lower triangle by blocks. Thread (tr, tc) = (t / 16, t % 16) of a 32 x 16 grid owns the elements
// (tr + 32 ia, tc + 16 ib) of the blocks with ib <= 2 ia + 1 (the ones meeting the lower triangle:
// 72 doubles); the two diagonal-crossing blocks of a block row (its 32 x 32 diagonal square) hold both
// triangles. The symmetric product sums the rows of the stored entries (over the 16 column threads of a
// row: one DPP row) plus, for the mirrored upper triangle outside the squares, the columns of the strictly
// lower blocks (over the 4 rows of a wave by permlane16 / shuffle, then over the 8 waves through LDS). The column halves (ib < 8, ib >= 8) are
// processed one after the other to bound the live operand registers.
template <int NR>   // 32-row block rows: 8 (orders <= 256) or 4 (orders <= 128)
__global__ void __launch_bounds__(512) k_sytrd_l512(const double* __restrict__ A, int lda, int n, double* __restrict__ d,
                                                   double* __restrict__ e, double* __restrict__ tau, double* __restrict__ V,
                                                   unsigned long long* __restrict__ stamps) {
    constexpr int NW = 8, NP = 32 * NR;
    // diagnostics (stamps != null): threads 0 and 64 record s_memtime at 8 points of the first 64 column steps
    // (compiled for NR <= 4 only: at NR = 8 the stamp code alone spilled 216 B per lane)
#define L512_STAMP(p)                                                                                   \
    do {                                                                                                \
        if (NR <= 4 && stamps && (threadIdx.x == 0 || threadIdx.x == 64) && j < 64)                      \
            stamps[(threadIdx.x == 0 ? 0 : 512) + 8 * j + (p)] = __builtin_amdgcn_s_memtime();           \
    } while (0)
    constexpr int NL = NR * (NR + 1);   // block row ia holds column blocks 0 .. 2 ia + 1: offset ia (ia + 1)
    __shared__ double xs[SY_MAX], vs[SY_MAX], ps[SY_MAX], psr[SY_MAX], cbuf[NW][SY_MAX];
    __shared__ double sh_tau;
    const int t = threadIdx.x, tr = t >> 4, tc = t & 15, lane = t & 63, wave = t >> 6;
    // the 32 x 32 diagonal squares (blocks 2 ia, 2 ia + 1 of block row ia) hold BOTH triangles (the upper
    // entries are the mirrored values, kept by the same rank-2 update): no masks in the symmetric product or
    // the update; the product's row sums run over every stored entry, its column (mirror) sums over the
    // strictly lower blocks ib < 2 ia only
    double a[NL];
#pragma unroll
    for (int ia = 0; ia < NR; ++ia)
#pragma unroll
        for (int ib = 0; ib <= 2 * ia + 1; ++ib) {
            const int i = tr + 32 * ia, k = tc + 16 * ib;
            const bool in = i < n && k < n;
            const int r = i >= k ? i : k, c = i >= k ? k : i;   // (A is read from its lower triangle)
            const double x = A[size_t(in ? r : 0) * lda + (in ? c : 0)];
            a[ia * (ia + 1) + ib] = in ? x : 0.0;
        }
    // column jj of the current matrix to LDS (xs) and its diagonal entry to d, by the column's owners
#define L512_PUBLISH_CASE(IB)                                                             \
    case IB:                                                                              \
        _Pragma("unroll") for (int ia = (IB) / 2; ia < NR; ++ia) {                        \
            const int i = tr + 32 * ia;                                                   \
            const double av = a[ia * (ia + 1) + (IB)];                                    \
            if (i > pj && i < n) xs[i] = av;                                              \
            if (i == pj) d[pj] = av;                                                      \
        }                                                                                 \
        break;
#define L512_PUBLISH(jj)                                                                  \
    do {                                                                                  \
        const int pj = (jj);                                                              \
        if (tc == (pj & 15)) {                                                            \
            switch (pj >> 4) {                                                            \
                L512_PUBLISH_CASE(0) L512_PUBLISH_CASE(1) L512_PUBLISH_CASE(2)            \
                L512_PUBLISH_CASE(3) L512_PUBLISH_CASE(4) L512_PUBLISH_CASE(5)            \
                L512_PUBLISH_CASE(6) L512_PUBLISH_CASE(7) L512_PUBLISH_CASE(8)            \
                L512_PUBLISH_CASE(9) L512_PUBLISH_CASE(10) L512_PUBLISH_CASE(11)          \
                L512_PUBLISH_CASE(12) L512_PUBLISH_CASE(13) L512_PUBLISH_CASE(14)         \
                L512_PUBLISH_CASE(15)                                                     \
                default: break;                                                           \
            }                                                                             \
        }                                                                                 \
    } while (0)
    L512_PUBLISH(0);
    for (int j = 0; j + 2 < n; ++j) {
        L512_STAMP(0);
        lds_barrier();
        L512_STAMP(1);
        if (wave == 0) {   // reflector (dlarfg), as in k_sytrd
            constexpr int E = NP / 64;
            double x[E];
#pragma unroll
            for (int q = 0; q < E; ++q) x[q] = xs[lane + 64 * q];
            const double alpha = xs[j + 1];
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int i = lane + 64 * q;
                if (i >= j + 2 && i < n) s = fma(x[q], x[q], s);
            }
            s = gsum<64>(s);
            double tv = 0.0, beta = alpha, scal = 0.0;
            if (s > 0.0) {
                beta = -copysign(sqrt(fma(alpha, alpha, s)), alpha);
                tv = (beta - alpha) * rcp2(beta);
                scal = rcp2(alpha - beta);
            }
#pragma unroll
            for (int q = 0; q < E; ++q) {
                const int i = lane + 64 * q;
                const double v = (i <= j || i >= n) ? 0.0 : (i == j + 1 ? 1.0 : x[q] * scal);
                vs[i] = v;
                if (i < n) V[size_t(j) * n + i] = v;
            }
            if (lane == 0) {
                sh_tau = tv;
                e[j] = beta;
                tau[j] = tv;
            }
        }
        L512_STAMP(2);
        lds_barrier();
        L512_STAMP(3);
        // (no early exit for tau = 0: p = w = 0 then and the update leaves every entry unchanged; a second
        // loop latch would double the live matrix registers at the merge)
        const double tj = sh_tau;
        // symmetric product and update from block row IA0 on: rows and columns <= j are finished (v and p
        // vanish there, the update leaves them unchanged), so block rows ia < IA0 = (j + 1) / 32 and column
        // blocks ib < 2 IA0 are skipped -- one compile-time loop nest per IA0 (a switch, no per-block
        // branches). Their entries of psr / cbuf are not written; ps is 0 at indices <= j regardless.
        auto step_from = [&](auto ia0_c) {
            constexpr int IA0 = decltype(ia0_c)::value;
            // symmetric product: row sums of the stored entries, column sums of the strictly lower ones
            double rp[NR];
#pragma unroll
            for (int ia = IA0; ia < NR; ++ia) rp[ia] = 0.0;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                if (8 * hh + 7 < 2 * IA0 || 8 * hh >= 2 * NR) continue;   // (compile time) finished / absent half
                double cp[8], vk[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    cp[q] = 0.0;
                    vk[q] = vs[tc + 16 * (8 * hh + q)];
                }
                double vi_n = vs[tr + 32 * IA0];   // (the next block row's v_i read one block row ahead)
#pragma unroll
                for (int ia = IA0; ia < NR; ++ia) {
                    if constexpr (NR > 4) __builtin_amdgcn_sched_barrier(0);
                    const double vi = vi_n;
                    if (ia + 1 < NR) vi_n = vs[tr + 32 * (ia + 1)];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int ib = 8 * hh + q;
                        if (ib >= 2 * IA0 && ib <= 2 * ia + 1) {
                            const double av = a[ia * (ia + 1) + ib];
                            rp[ia] = fma(av, vk[q], rp[ia]);
                            if (ib < 2 * ia) cp[q] = fma(av, vi, cp[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    // (column blocks of the last square have no strictly lower block: cp = 0)
                    if (8 * hh + q < 2 * IA0 || 8 * hh + q >= 2 * NR - 2) continue;
                    cp[q] = addx32(addx16(cp[q]));
                }
                if (lane < 16) {
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (8 * hh + q >= 2 * IA0) cbuf[wave][tc + 16 * (8 * hh + q)] = cp[q];
                }
            }
#pragma unroll
            for (int ia = IA0; ia < NR; ++ia) {
                const double r = gsum<16>(rp[ia]);
                if (tc == 0) psr[tr + 32 * ia] = r;
            }
            L512_STAMP(4);
            lds_barrier();
            L512_STAMP(5);
            if (t < SY_MAX) {
                double c = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) c += cbuf[w][t];
                ps[t] = (t > j && t < n) ? tj * (psr[t] + c) : 0.0;
            }
            L512_STAMP(6);
            lds_barrier();
            L512_STAMP(7);
            // K = -(tau / 2) (p . v) in every wave, w = p + K v on the fly; A -= v w^T + w v^T on the kept entries
            double sk = 0.0;
#pragma unroll
            for (int q = 0; q < NP / 64; ++q) sk = fma(ps[lane + 64 * q], vs[lane + 64 * q], sk);
            const double K = -0.5 * tj * gsum<64>(sk);
            double vi[NR], wi[NR];
#pragma unroll
            for (int ia = IA0; ia < NR; ++ia) {
                vi[ia] = vs[tr + 32 * ia];
                wi[ia] = fma(K, vi[ia], ps[tr + 32 * ia]);
            }
            // one column block at a time at NR = 8 (hoisted operands spill there), its operands read one
            // block ahead; NR <= 4 leaves the scheduling to the compiler
            double vk_n = vs[tc + 32 * IA0], pk_n = ps[tc + 32 * IA0];
#pragma unroll
            for (int ib = 2 * IA0; ib < 2 * NR; ++ib) {
                if constexpr (NR > 4) __builtin_amdgcn_sched_barrier(0);
                const double vk = vk_n, pk = pk_n;
                if (ib + 1 < 2 * NR) {
                    vk_n = vs[tc + 16 * (ib + 1)];
                    pk_n = ps[tc + 16 * (ib + 1)];
                }
                const double wk = fma(K, vk, pk);
#pragma unroll
                for (int ia = (ib / 2 > IA0 ? ib / 2 : IA0); ia < NR; ++ia) {
                    const int ix = ia * (ia + 1) + ib;
                    a[ix] = fma(-vi[ia], wk, fma(-wi[ia], vk, a[ix]));
                }
            }
        };
        switch ((j + 1) >> 5) {
            case 0: step_from(std::integral_constant<int, 0>{}); break;
            case 1: step_from(std::integral_constant<int, 1>{}); break;
            case 2: step_from(std::integral_constant<int, 2>{}); break;
            case 3: step_from(std::integral_constant<int, (NR > 3 ? 3 : NR - 1)>{}); break;
            case 4: step_from(std::integral_constant<int, (NR > 4 ? 4 : NR - 1)>{}); break;
            case 5: step_from(std::integral_constant<int, (NR > 5 ? 5 : NR - 1)>{}); break;
            case 6: step_from(std::integral_constant<int, (NR > 6 ? 6 : NR - 1)>{}); break;
            default: step_from(std::integral_constant<int, NR - 1>{}); break;
        }
        L512_PUBLISH(j + 1);
    }
#undef L512_PUBLISH
#undef L512_PUBLISH_CASE
#undef L512_STAMP
    // the last 2 x 2 block: d[n-2], d[n-1], e[n-2] (tau = 0, H = I)
#pragma unroll
    for (int ia = 0; ia < NR; ++ia)
#pragma unroll
        for (int ib = 0; ib <= 2 * ia + 1; ++ib) {
            const int i = tr + 32 * ia, k = tc + 16 * ib;
            const double av = a[ia * (ia + 1) + ib];
            if (i == n - 2 && k == n - 2) d[n - 2] = av;
            if (i == n - 1 && k == n - 1) d[n - 1] = av;
            if (i == n - 1 && k == n - 2) {
                e[n - 2] = av;
                tau[n - 2] = 0.0;
                for (int q = 0; q < n; ++q) V[size_t(n - 2) * n + q] = 0.0;
            }
        }
}

// Entry i of the inverse iteration's start vector for eigenvalue q: uniform in (-1, 1) (dstein's dlarnv
// distribution), never 0, from a bijective 32-bit mix (murmur3's finaliser) of (i, q) -- no two of the SY_MAX^2
// entries share their bits' source, so the vectors of a cluster start independent in every coordinate subset.
// (The first formula was 1 + ((37 i + 11 q) mod 17) / 17, of period 17 in i and in q: the members q and q + 17
// of a cluster started identically and the 17 distinct vectors agreed on coordinates i = i' (mod 17): clusters of
// 18 and more, c I of order >= 18 and diagonals with repeated entries came back with zero or noise rows and
// status 0, tests/test_syev_gpu.py::test_sym_eig_top_spectra.) Formed once per entry by the whole workgroup, off
// the chains.
__device__ __forceinline__ double stein_start(int i, int q) {
    unsigned h = unsigned(i) | (unsigned(q) << 16);
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return (double(h >> 8) + 0.5) * (1.0 / 8388608.0) - 1.0;
}

// one 64-lane workgroup per wanted eigenvalue: block q -> the q-th largest (ascending index n - 1 - q).
// Zt (kk x ldz): row q = the eigenvector of T (normalised); lam[q]. status[0] <- -1 if a multisection
// did not reach full precision.
constexpr int SW_WAVES = 4;   // waves of the multisection (k_stebz_stein)
template <int NEWTON, int ITERS = 3>
__global__ void __launch_bounds__(64 * SW_WAVES) k_stebz_stein(const double* __restrict__ d, const double* __restrict__ e, int n,
                                                     double* __restrict__ lam, double* __restrict__ Zt, int ldz, int* __restrict__ status,
                                                     unsigned long long* __restrict__ stamps) {
    // diagnostics (stamps != null): workgroup 0 records s_memtime at its phase boundaries
#define STEIN_STAMP(p) \
    do { if (stamps && blockIdx.x == 0 && threadIdx.x == 0) stamps[p] = __builtin_amdgcn_s_memtime(); } while (0)
    STEIN_STAMP(0);
    __shared__ double sd[SY_MAX], se[SY_MAX], se2[SY_MAX], sds[SY_MAX], se2s[SY_MAX];
    __shared__ double ld[SY_MAX], ldl[SY_MAX], ldu[SY_MAX], ldu2[SY_MAX], lb[SY_MAX];
    __shared__ int lpiv[SY_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x, m = n - 1 - q;
    double gl = 1e300, gu = -1e300, emax2 = 0.0, amax = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double di = d[i], ei = i + 1 < n ? e[i] : 0.0, em = i > 0 ? e[i - 1] : 0.0;
        sd[i] = di;
        se[i] = ei;
        se2[i] = ei * ei;
        const double r = fabs(ei) + fabs(em);
        gl = fmin(gl, di - r);
        gu = fmax(gu, di + r);
        emax2 = fmax(emax2, ei * ei);
        amax = fmax(amax, fabs(di) + r);
    }
    gl = wave_fmin(gl);
    gu = wave_fmax(gu);
    emax2 = wave_fmax(emax2);
    amax = wave_fmax(amax);
    // the multisection's three-term recurrence runs on T scaled by a power of two (exact: the counts are
    // those of T) so that |d - x| and e^2 stay O(1) and 4 levels cannot overflow between rescalings
    const double tsc = ldexp(1.0, -ilogb(fmax(amax, 1e-300)));
    for (int i = lane; i < n; i += 64) {
        const double es = se[i] * tsc;   // (scaled first: e^2 of an O(1e-200) T underflows)
        sds[i] = sd[i] * tsc;
        se2s[i] = es * es;
    }
    __syncthreads();
    STEIN_STAMP(1);
    const double pivmin = 1e-290 * fmax(1.0, emax2);
    const double span = fmax(gu - gl, 1e-300);
    double lo = gl - 2.2e-16 * span - pivmin, hi = gu + 2.2e-16 * span + pivmin;
    // multisection: thread t counts the eigenvalues below lo + (hi - lo) (t + 1) / (64 SW_WAVES + 1); the
    // waves (one per SIMD: the chains are FP64-issue-bound) merge their brackets through LDS every round
    __shared__ double rlo[2][SW_WAVES], rhi[2][SW_WAVES];
    int rounds = 0;
    bool done = false;
    for (; rounds < 16 && !done; ++rounds) {
        const double x = lo + (hi - lo) * double(tid + 1) * (1.0 / (64.0 * SW_WAVES + 1.0));
        // Sturm count as sign changes of the leading minors p_i = (d_i - x) p_{i-1} - e_{i-1}^2 p_{i-2}
        // (the pivots q_i = p_i / p_{i-1} of the q-form without its division: one FMA per level on the
        // dependent chain instead of a reciprocal, two Newton steps and an FMA; the count is off the chain).
        // The q-form's |q_i| < pivmin -> -pivmin guards its next division; here a tiny p_i only makes the
        // next minor -e^2 p_{i-1}, and an exact zero (x an eigenvalue of a leading block) counted as
        // non-negative moves x to either end of the bracket, which still contains the eigenvalue.
        // p_{i-1}, p_{i-2} are rescaled by a power of two every 4 levels (|p_i| grows at most 4x per level
        // on the scaled T).
        const double xs = x * tsc, pivs = pivmin * tsc;
        double pm2 = 1.0, pm1 = sds[0] - xs;
        if (fabs(pm1) < pivs) pm1 = -pivs;
        int c = pm1 < 0.0;
        int i = 1;
        for (; i + 4 <= n; i += 4) {
            double dx[4], e2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                dx[u] = sds[i + u] - xs;
                e2[u] = se2s[i + u - 1];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double pv = fma(dx[u], pm1, -e2[u] * pm2);
                c += (pv < 0.0) != (pm1 < 0.0);
                pm2 = pm1;
                pm1 = pv;
            }
            const int ex = __builtin_amdgcn_frexp_exp(pm1);
            pm1 = ldexp(pm1, -ex);
            pm2 = ldexp(pm2, -ex);
        }
        for (; i < n; ++i) {
            const double pv = fma(sds[i] - xs, pm1, -se2s[i - 1] * pm2);
            c += (pv < 0.0) != (pm1 < 0.0);
            pm2 = pm1;
            pm1 = pv;
        }
        double nlo = c <= m ? x : -1e300, nhi = c >= m + 1 ? x : 1e300;
        nlo = wave_fmax(nlo);
        nhi = wave_fmin(nhi);
        if (lane == 0) {
            rlo[rounds & 1][wave] = nlo;
            rhi[rounds & 1][wave] = nhi;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < SW_WAVES; ++w) {
            nlo = fmax(nlo, rlo[rounds & 1][w]);
            nhi = fmin(nhi, rhi[rounds & 1][w]);
        }
        if (nlo > lo) lo = nlo;
        if (nhi < hi) hi = nhi;
        // absolute accuracy u ||T|| (dstebz's default abstol): all a backward-stable reduction delivers
        done = (hi - lo) <= 2.2204460492503131e-16 * (2.0 * fmax(fabs(lo), fabs(hi)) + 4.0 * span) + 2.0 * pivmin;
    }
    STEIN_STAMP(2);
    const double lmb = 0.5 * (lo + hi);
    __shared__ double ild[SY_MAX];   // inverse pivots of U
    if (tid == 0) {
        lam[q] = lmb;
        if (!done) atomicMin(status, -1);
        // inverse iteration: T - lambda I = P L U (dgttrf, row interchanges where the subdiagonal entry is
        // larger), tiny pivots replaced by u ||T|| (dlagtf's perturbation). The running diagonal and
        // superdiagonal entries are carried in registers (no LDS store -> load per level on the dependent
        // chain); the original entries of the next row are independent of it.
        // The shift is moved off the eigenvalue by 64 u ||T||: the members of a (nearly) multiple eigenvalue get
        // (nearly) the same shift, and the copies of that eigenvalue in T lie a few u ||T|| apart; a shift within
        // 0.01 u ||T|| of one of them weights its vector 1e6 times above the others after three solves, every
        // member comes back as that one vector and k_cluster_orth normalises what is left of it (measured: exact
        // multiplicities 18..64 at 1e-12..1e-10 in orthogonality and residual). 64 u ||T|| away the copies are
        // weighted within a small factor of each other and the members stay as independent as their start
        // vectors. Separated eigenvalues (gap > 1e-3 ||T||) still converge in one solve, (64 u ||T|| / gap) per
        // solve; for members ~64 u ||T|| apart the residual is bounded by the shift's distance, 1.4e-14 ||T||.
        const double lms = lmb + 64.0 * 2.2204460492503131e-16 * fmax(amax, 1e-300);
        double dcur = sd[0] - lms, ucur = n > 1 ? se[0] : 0.0;
        auto lu_level = [&](int i, double l, double dn, double un) {
            if (fabs(dcur) >= fabs(l)) {
                const double f = dcur != 0.0 ? l * rcpn<NEWTON>(dcur) : 0.0;
                ld[i] = dcur;
                ldl[i] = f;
                ldu[i] = ucur;
                ldu2[i] = 0.0;
                lpiv[i] = i;
                dcur = dn - f * ucur;
                ucur = un;
            } else {
                const double f = dcur * rcpn<NEWTON>(l);
                ld[i] = l;
                ldl[i] = f;
                ldu[i] = dn;
                ldu2[i] = un;
                lpiv[i] = i + 1;
                dcur = ucur - f * dn;
                ucur = -f * un;
            }
        };
        int i = 0;
        for (; i + 9 < n; i += 8) {   // the block's original entries read ahead of its chain
            double l8[8], d8[8], u8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                l8[u] = se[i + u];
                d8[u] = sd[i + u + 1] - lms;
                u8[u] = se[i + u + 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) lu_level(i + u, l8[u], d8[u], u8[u]);
        }
        for (; i + 1 < n; ++i) lu_level(i, se[i], sd[i + 1] - lms, i + 2 < n ? se[i + 1] : 0.0);
        ld[n - 1] = dcur;
        ldl[n - 1] = 0.0;
        ldu[n - 1] = 0.0;
        ldu2[n - 1] = 0.0;
        lpiv[n - 1] = n - 1;
    }
    __syncthreads();
    STEIN_STAMP(3);
    {
        const double tiny = 2.2204460492503131e-16 * fmax(amax, 1e-300);
        for (int i = tid; i < n; i += 64 * SW_WAVES) {
            double p = ld[i];
            if (fabs(p) < tiny) p = copysign(tiny, p == 0.0 ? 1.0 : p);
            ild[i] = rcp2(p);
            lb[i] = stein_start(i, q);
        }
    }
    __syncthreads();
    STEIN_STAMP(4);
    for (int it = 0; it < ITERS; ++it) {
        if (tid == 0) {   // dgttrs: forward with the interchanges, then back substitution (running values in
                           // registers, each block's 8 levels of LU operands read ahead of its dependent chain)
            // forward: cur' = a_i cur + b_i with (a, b) = (-f, nxt) (no interchange) or (1, -f nxt) (rows i,
            // i+1 swapped) formed off the chain; backward: x_i = alpha_i x_{i+1} + (beta_i x_{i+2} + gamma_i)
            // -- one FMA per level on each dependent chain
            double cur = lb[0];
            int i = 0;
            for (; i + 8 < n; i += 8) {
                double nx[8], fl[8];
                int pv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    nx[u] = lb[i + u + 1];
                    fl[u] = ldl[i + u];
                    pv[u] = lpiv[i + u];
                }
                double ca[8], cb[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool sw = pv[u] != i + u;
                    ca[u] = sw ? 1.0 : -fl[u];
                    cb[u] = sw ? -fl[u] * nx[u] : nx[u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    lb[i + u] = (pv[u] != i + u) ? nx[u] : cur;
                    cur = fma(ca[u], cur, cb[u]);
                }
            }
            for (; i + 1 < n; ++i) {
                const double nxt = lb[i + 1], f = ldl[i];
                if (lpiv[i] == i) {
                    lb[i] = cur;
                    cur = fma(-f, cur, nxt);
                } else {
                    lb[i] = nxt;
                    cur = fma(-f, nxt, cur);
                }
            }
            double x1 = cur * ild[n - 1], x2 = 0.0;
            lb[n - 1] = x1;
            i = n - 2;
            for (; i >= 7; i -= 8) {
                double al[8], be[8], ga[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double iv = ild[i - u];
                    al[u] = -iv * ldu[i - u];
                    be[u] = -iv * ldu2[i - u];
                    ga[u] = iv * lb[i - u];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double x0 = fma(al[u], x1, fma(be[u], x2, ga[u]));
                    lb[i - u] = x0;
                    x2 = x1;
                    x1 = x0;
                }
            }
            for (; i >= 0; --i) {
                const double x0 = (lb[i] - ldu[i] * x1 - ldu2[i] * x2) * ild[i];
                lb[i] = x0;
                x2 = x1;
                x1 = x0;
            }
        }
        __syncthreads();
        STEIN_STAMP(5 + 2 * it);
        // normalise (scaled 2-norm over the wave)
        double mx = 0.0;
        for (int i = lane; i < n; i += 64) mx = fmax(mx, fabs(lb[i]));
        mx = wave_fmax(mx);
        const double inv_mx = mx > 0.0 ? 1.0 / mx : 1.0;
        double ss = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double v = lb[i] * inv_mx;
            ss = fma(v, v, ss);
        }
        ss = gsum<64>(ss);
        const double sc = inv_mx / sqrt(ss);
        __syncthreads();
        if (wave == 0)   // (every wave formed the same scale)
            for (int i = lane; i < n; i += 64) lb[i] *= sc;
        __syncthreads();
        STEIN_STAMP(6 + 2 * it);
    }
    for (int i = tid; i < n; i += 64 * SW_WAVES) Zt[size_t(q) * ldz + i] = lb[i];
    STEIN_STAMP(11);
#undef STEIN_STAMP
}


// u = H_0 H_1 ... H_{n-2} z for every row z of Zt (in place): one wave per vector (entry i on lane i mod
// 64, ZE = n / 64 per lane), 4 vectors per 256-thread workgroup, so the dependent chain per reflector is
// two FMAs, a 64-lane reduction without the LDS crossbar (DPP, permlane16 / permlane32 swaps) and one
// FMA; the reflectors pass through LDS in chunks of 16384 / n rows, staged by the whole workgroup with
// coalesced loads. (The first version, 16 lanes per vector and 16 vectors per workgroup, ran a 16-deep
// FMA chain per reflector on only kk / 16 workgroups: 150 us at n = 256, kk = 128.)
// (blockIdx.y == 1: the second set V2 / tau2 / Zt2 -- the bidiagonal SVD's left and right vectors in one launch)
template <int ZE>
__global__ void __launch_bounds__(256) k_ormtr(const double* __restrict__ V, const double* __restrict__ tau, int n, int kk,
                                               double* __restrict__ Zt, int ldz, const double* __restrict__ V2,
                                               const double* __restrict__ tau2, double* __restrict__ Zt2) {
    if (blockIdx.y) {
        V = V2;
        tau = tau2;
        Zt = Zt2;
    }
    constexpr int CHUNK_ELEMS = 16384;
    __shared__ double sv[CHUNK_ELEMS], st[SY_MAX];
    for (int e = threadIdx.x; e < n; e += 256) st[e] = e + 1 < n ? tau[e] : 0.0;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = q < kk;
    double z[ZE];
#pragma unroll
    for (int s = 0; s < ZE; ++s) {
        const int i = lane + 64 * s;
        z[s] = (live && i < n) ? Zt[size_t(q) * ldz + i] : 0.0;
    }
    const int rows = CHUNK_ELEMS / n;
    for (int hi = n - 2; hi >= 0; hi -= rows) {
        const int lo = hi - rows + 1 > 0 ? hi - rows + 1 : 0;
        __syncthreads();
        for (int e = threadIdx.x; e < (hi - lo + 1) * n; e += 256) sv[e] = V[size_t(lo) * n + e];
        __syncthreads();
        for (int j = hi; j >= lo; --j) {   // (tau_j = 0: f = 0, z unchanged)
            const double* v = sv + size_t(j - lo) * n;
            double vv[ZE];
            double d0 = 0.0, d1 = 0.0;
#pragma unroll
            for (int s = 0; s < ZE; ++s) {
                const int i = lane + 64 * s;
                vv[s] = i < n ? v[i] : 0.0;
                if (s & 1) d1 = fma(vv[s], z[s], d1);
                else d0 = fma(vv[s], z[s], d0);
            }
            const double f = st[j] * gsum<64>(d0 + d1);
#pragma unroll
            for (int s = 0; s < ZE; ++s) z[s] = fma(-f, vv[s], z[s]);
        }
    }
    if (live) {
#pragma unroll
        for (int s = 0; s < ZE; ++s) {
            const int i = lane + 64 * s;
            if (i < n) Zt[size_t(q) * ldz + i] = z[s];
        }
    }
}

// Clusters of close eigenvalues (|lam_i - lam_{i+1}| <= 1e-3 ||T||, dstein's ORTOL): inverse iteration from
// different start vectors lands in the cluster's invariant subspace, but not orthogonally -- the vectors of each
// cluster are orthonormalised by two passes of modified Gram-Schmidt (in order of decreasing eigenvalue, as
// dstein reorthogonalises against the earlier vectors of a cluster). One workgroup; without clusters it only
// scans the eigenvalues.
// maxc: clusters larger than this are left alone and *status set to -2 (the bidiagonal SVD's fallback signal: its
// Jacobi route is cheaper than a long Gram-Schmidt chain).
// A vector that keeps less than kClusterCollapse of its unit norm after the first pass was numerically dependent on
// its predecessors: normalising the remainder multiplies inverse iteration's error outside the cluster's invariant
// subspace (up to u ||T|| / ortol = 1.1e-13) by more than 1e4, so the vector is not trusted and *status set to -3
// (the round and the bidiagonal SVD fall back on any negative status). Independent start vectors leave about
// 1 / sqrt(members) or more.
constexpr double kClusterCollapse = 1e-4;
__global__ void __launch_bounds__(256) k_cluster_orth(const double* __restrict__ lam, const double* __restrict__ d,
                                                      const double* __restrict__ e, int n, int kk, double* __restrict__ Zt, int ldz,
                                                      int maxc, int* __restrict__ status) {
    __shared__ double red[4];
    __shared__ double tnorm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a = 0.0;
    for (int i = tid; i < n; i += 256) a = fmax(a, fabs(d[i]) + (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < n ? fabs(e[i]) : 0.0));
    a = wave_fmax(a);
    wave_partials(a, red);
    if (tid == 0) tnorm = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    const double ortol = 1e-3 * tnorm;
    auto dot = [&](const double* x, const double* y) {
        double s = 0.0;
        for (int i = tid; i < n; i += 256) s = fma(x[i], y[i], s);
        s = gsum<64>(s);
        __syncthreads();
        if (lane == 0) red[wave] = s;
        __syncthreads();
        return sum_pairwise4(red);
    };
    int c0 = 0;
    while (c0 < kk) {
        int c1 = c0 + 1;
        while (c1 < kk && fabs(lam[c1 - 1] - lam[c1]) <= ortol) ++c1;
        if (c1 - c0 > maxc) {
            if (tid == 0) status[0] = -2;
            c0 = c1;
            continue;
        }
        for (int j = c0 + 1; j < c1; ++j) {   // cluster [c0, c1): orthonormalise vector j against c0 .. j-1
            double* zj = Zt + size_t(j) * ldz;
            for (int pass = 0; pass < 2; ++pass) {
                for (int i = c0; i < j; ++i) {
                    const double* zi = Zt + size_t(i) * ldz;
                    const double c = dot(zi, zj);
                    for (int k = tid; k < n; k += 256) zj[k] = fma(-c, zi[k], zj[k]);
                    __syncthreads();
                }
                const double nn = sqrt(dot(zj, zj));
                if (pass == 0 && !(nn >= kClusterCollapse) && tid == 0) status[0] = -3;
                const double inv = nn > 0.0 ? 1.0 / nn : 0.0;
                for (int k = tid; k < n; k += 256) zj[k] *= inv;
                __syncthreads();
            }
        }
        c0 = c1;
    }
}

__global__ void k_sqrt_lam(const double* __restrict__ lam, int kk, double* __restrict__ S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kk) S[i] = sqrt(fmax(lam[i], 0.0));
}

// ---- dense SVD through a bidiagonal (square n <= 128; svd_bidiag below) ------------------------------
constexpr int BD_MAX = 128, BD_LDA = BD_MAX + 1;   // LDS row stride 129 doubles: row-wise lanes conflict-free

// dlarfg from alpha and ss = ||x(1:)||^2: beta = -sign(alpha) sqrt(alpha^2 + ss), tau = (beta - alpha) / beta, v = x /
// (alpha - beta) with v_0 = 1; ss = 0 -> tau = 0, beta = alpha. Formed by every thread from the same operands, so
// bit-identical across the workgroup (no broadcast needed). k_gebrd_sq scales A to max |A| ~ 1 by a power of two
// first, so the unscaled sum of squares cannot overflow; squares below 2^-1022 of entries below 2^-511 max |A|
// are lost, which moves B by less than u ||A||.
__device__ __forceinline__ void bd_reflector(double alpha, double ss, double& beta, double& tau, double& scal) {
    if (ss == 0.0) {
        beta = alpha;
        tau = 0.0;
        scal = 0.0;
        return;
    }
    // (the reciprocals by the hardware estimate + 2 Newton steps: ~1 ulp, a 5-deep dependent chain where the IEEE
    // division's is ~10 -- at ~32 cycles per dependent FP64 operation the reflector is on every column's critical path)
    beta = -copysign(sqrt(fma(alpha, alpha, ss)), alpha);
    tau = (beta - alpha) * rcp2(beta);
    scal = rcp2(alpha - beta);
}

// Householder bidiagonalisation of a square A (n <= 128, row-major) in ONE workgroup (LAPACK dgebd2, m = n): per
// column j the left reflector H_j on column j (rows j..n-1), then the right reflector G_j on row j (columns
// j+1..n-1); A = (H_0 ... H_{n-1}) B (G_0 ... G_{n-2})^T, B upper bidiagonal (d_j, e_j).
// 512 threads (two waves per SIMD), the matrix register-resident: element (r, c) on the thread with r mod 16 =
// lane mod 16 and c mod 32 = 4 wave + lane / 16 -- 8 rows x 4 columns per thread. The left product w_c =
// sum_r v_r a_rc is a sum over a 16-lane DPP row (no LDS, no barrier); the right product w_r = sum_c a_rc v_c
// sums the wave's four DPP rows (permlane16 / permlane32 swaps) and then the 8 waves through LDS. H_j is formed
// by the DPP row that holds column j, G_j by every thread from row j's entries and partial squares staged in
// LDS; the reflector vectors go straight to Vl / Vr, so the registers of finished rows and columns are left as
// they are (every later product meets them with a zero v or a masked w). Row and column blocks of 16 / 32
// that lie wholly in the finished part are skipped (wave-uniform branches). Four LDS-only barriers per column.
// Per column ~9.3k cycles at n = 128 (XRS_STAMPS=bd; 490 us): latency-bound -- one DPP stage of a double sum
// (two v_mov_b32_dpp + v_add_f64) costs ~90 cycles, the H_j owners' two 16-lane sums ~720, the reflector ~320,
// and every column runs four such chains back to back. Measured before: A staged in LDS with 8 row groups x 128
// columns per product, 10k cycles per column (542 us; its __syncthreads also drained the per-column global
// stores); 1024 threads with 4 x 4 elements each, 10.5k cycles (the reductions, masks and the G_j reflector
// replicated over 16 waves).
// Outputs: the Golub-Kahan tridiagonal of B (diagonal tgd = 0 (2n), off-diagonal tge = d_0, e_0, d_1, e_1, ...
// (2n - 1)), whose top n eigenvalues are B's singular values with eigenvectors (v_0, u_0, v_1, u_1, ...) / sqrt 2;
// the reflectors in k_ormtr's row format (Vl row j: v with v_j = 1, zeros before; Vr row j: v with v_{j+1} = 1,
// zeros up to j) and their tau (tl, tr: n - 1 used, the length-1 ones are 0); status[0] = 0 (for k_stebz_stein).
// A is scaled to max |A| ~ 1 by a power of two first (exact; d and e are scaled back), so the reflectors' sums of
// squares cannot overflow.
__global__ void __launch_bounds__(512) k_gebrd_sq(const double* __restrict__ A, int n, double* __restrict__ tgd,
                                                  double* __restrict__ tge, double* __restrict__ Vl, double* __restrict__ tl,
                                                  double* __restrict__ Vr, double* __restrict__ tr, int* __restrict__ status,
                                                  unsigned long long* __restrict__ stamps) {
#define BD_STAMP(p) \
    do { if (stamps && threadIdx.x == 0) stamps[p] = __builtin_amdgcn_s_memtime(); } while (0)
    BD_STAMP(0);
    __shared__ double vbuf[BD_MAX], xbuf[BD_MAX], wbuf[BD_MAX], sqp[32], red[8];
    __shared__ double rp[32][BD_MAX + 16];   // right-product partials per column residue (row stride: sub
                                             // offsets land 32 banks apart -- conflict-free half waves)
    __shared__ double obuf[4][BD_MAX];   // d, e, tau_l, tau_r (stored at the end)
    __shared__ double stau;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rho = lane & 15, sub = lane >> 4, gam = 4 * wave + sub;
    if (tid == 0) status[0] = 0;
    double x[8][4];   // x[i][k] = a(rho + 16 i, gam + 32 k)
    double am = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = rho + 16 * i, c = gam + 32 * k;
            x[i][k] = (r < n && c < n) ? A[size_t(r) * n + c] : 0.0;
            am = fmax(am, fabs(x[i][k]));
        }
    am = wave_fmax(am);
    if (lane == 0) red[wave] = am;
    for (int i = tid; i < 2 * n; i += 512) tgd[i] = 0.0;
    lds_barrier();
    am = red[0];
#pragma unroll
    for (int w = 1; w < 8; ++w) am = fmax(am, red[w]);
    const int ex = am > 0.0 ? ilogb(am) : 0;
    // (ldexp on the entries themselves: 2^-ex is not representable for a subnormal max |A|, ex < -1023)
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) x[i][k] = ldexp(x[i][k], -ex);
    BD_STAMP(1);
    for (int j = 0; j < n; ++j) {
        BD_STAMP(4 + 4 * j);
        const int jk = j >> 5, ji = j >> 4;
        // ---- H_j: the DPP row holding column j (gam == j mod 32); v straight to Vl row j
        if (gam == (j & 31)) {
            double y[8];
#define BD_COL(K) for (int i = 0; i < 8; ++i) y[i] = x[i][K]
            switch (jk) {   // (uniform: a scalar branch, not selects over all 32 registers)
                case 0: BD_COL(0); break;
                case 1: BD_COL(1); break;
                case 2: BD_COL(2); break;
                default: BD_COL(3); break;
            }
#undef BD_COL
            double ss = 0.0, al = 0.0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = rho + 16 * i;
                ss = (r > j) ? fma(y[i], y[i], ss) : ss;
                al = (r == j) ? y[i] : al;
            }
            ss = gsum<16>(ss);
            al = gsum<16>(al);
            double beta, tau, sc;
            bd_reflector(al, ss, beta, tau, sc);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = rho + 16 * i;
                y[i] = r > j ? y[i] * sc : (r == j ? 1.0 : 0.0);
                vbuf[r] = y[i];
            }
            if (rho == 0) {
                obuf[0][j] = ldexp(beta, ex);
                obuf[2][j] = tau;
                stau = tau;
            }
        }
        lds_barrier();
        if (gam == (j & 31)) {   // Vl row j, after the barrier (off the other waves' wait)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = rho + 16 * i;
                if (r < n) Vl[size_t(j) * n + r] = vbuf[r];
            }
        }
        BD_STAMP(5 + 4 * j);
        const double taul = stau;
        if (taul != 0.0) {   // (uniform)
            double v[8], w[4];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (16 * i + 15 >= j) ? vbuf[rho + 16 * i] : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double p = 0.0;
                if (32 * k + 31 > j)
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (16 * i + 15 >= j) p = fma(v[i], x[i][k], p);
                w[k] = p;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (32 * k + 31 > j) w[k] = (gam + 32 * k > j) ? gsum<16>(w[k]) * taul : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (32 * k + 31 > j)
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (16 * i + 15 >= j) x[i][k] = fma(-v[i], w[k], x[i][k]);
        }
        if (j + 1 >= n) break;
        // ---- G_j: row j's entries and partial squares (columns >= j + 2) into LDS
        if (rho == (j & 15)) {
            double yr[4];
#define BD_ROW(I) for (int k = 0; k < 4; ++k) yr[k] = x[I][k]
            switch (ji) {   // (uniform)
                case 0: BD_ROW(0); break;
                case 1: BD_ROW(1); break;
                case 2: BD_ROW(2); break;
                case 3: BD_ROW(3); break;
                case 4: BD_ROW(4); break;
                case 5: BD_ROW(5); break;
                case 6: BD_ROW(6); break;
                default: BD_ROW(7); break;
            }
#undef BD_ROW
            double sp = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = gam + 32 * k;
                xbuf[c] = yr[k];
                sp = (c >= j + 2) ? fma(yr[k], yr[k], sp) : sp;
            }
            sqp[gam] = sp;
        }
        lds_barrier();
        BD_STAMP(6 + 4 * j);
        double t4[4] = {0.0, 0.0, 0.0, 0.0};   // (four interleaved chains)
#pragma unroll
        for (int g = 0; g < 32; g += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) t4[u] += sqp[g + u];
        double betr, taur, scr;
        bd_reflector(xbuf[j + 1], (t4[0] + t4[1]) + (t4[2] + t4[3]), betr, taur, scr);
        if (stamps && tid == 0 && j < 96) stamps[600 + 4 * j] = __builtin_amdgcn_s_memtime() + (unsigned long long)(scr * 0.0);
        double vc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = gam + 32 * k;
            vc[k] = c >= j + 2 ? xbuf[c] * scr : (c == j + 1 ? 1.0 : 0.0);
        }
        if (tid == 0) {
            obuf[1][j] = ldexp(betr, ex);
            obuf[3][j] = taur;
        }
        if (taur != 0.0) {   // (uniform)
            double q[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                double p = 0.0;
                if (16 * i + 15 > j)
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (32 * k + 31 > j) p = fma(x[i][k], vc[k], p);
                q[i] = p;
            }
            // (every lane's partials to LDS: 32 per row, summed below -- the permlane16 / permlane32 sums of the
            // wave's four DPP rows first cost ~2k cycles per column, their dependent chains on the critical path)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (16 * i + 15 > j) rp[gam][rho + 16 * i] = q[i];
            if (stamps && tid == 0 && j < 96) stamps[601 + 4 * j] = __builtin_amdgcn_s_memtime();
            lds_barrier();
            BD_STAMP(7 + 4 * j);
            if (rho == 0) {   // Vr row j (the wave's four DPP rows x 4 columns: 32 threads, all 128 columns)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (gam + 32 * k < n) Vr[size_t(j) * n + gam + 32 * k] = vc[k];
            }
            if (tid < BD_MAX && tid > j) {
                double t4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int g = 0; g < 32; g += 4)
#pragma unroll
                    for (int u = 0; u < 4; ++u) t4[u] += rp[g + u][tid];
                wbuf[tid] = ((t4[0] + t4[1]) + (t4[2] + t4[3])) * taur;
            } else if (tid < BD_MAX) {
                wbuf[tid] = 0.0;
            }
            lds_barrier();
            if (stamps && tid == 0 && j < 96) stamps[602 + 4 * j] = __builtin_amdgcn_s_memtime();
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (16 * i + 15 > j) {
                    const double wr = wbuf[rho + 16 * i];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (32 * k + 31 > j) x[i][k] = fma(-wr, vc[k], x[i][k]);
                }
        } else if (rho == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (gam + 32 * k < n) Vr[size_t(j) * n + gam + 32 * k] = vc[k];
        }
    }
    if (tid == 0) {
        obuf[2][n - 1] = 0.0;
        obuf[3][n - 1] = 0.0;
        obuf[3][n - 2] = 0.0;
    }
    lds_barrier();
    BD_STAMP(2);
    for (int i = tid; i < n; i += 512) {
        tge[2 * i] = obuf[0][i];
        if (i + 1 < n) tge[2 * i + 1] = obuf[1][i];
        tl[i] = obuf[2][i];
        tr[i] = obuf[3][i];
        Vr[size_t(n - 1) * n + i] = 0.0;
    }
    BD_STAMP(3);
#undef BD_STAMP
}

// Golub-Kahan eigenvectors -> singular vectors of B: row q of Z (2n) = (v_0, u_0, v_1, u_1, ...); Ub / Vb row q =
// its u / v half, each normalised (one wave per vector). S[q] = max(lam[q], 0), made non-increasing (the
// multisection's midpoints of equal singular values may differ in the last bits).
__global__ void __launch_bounds__(256) k_gk_split(const double* __restrict__ Z, const double* __restrict__ lam, int n,
                                                  double* __restrict__ Ub, double* __restrict__ Vb, double* __restrict__ S) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double prev = 1e308;
        for (int i = 0; i < n; ++i) {
            const double s = fmin(fmax(lam[i], 0.0), prev);
            S[i] = s;
            prev = s;
        }
    }
    if (q >= n) return;
    const double* z = Z + size_t(q) * 2 * n;
    double su = 0.0, sv = 0.0;
    for (int k = lane; k < n; k += 64) {
        const double v = z[2 * k], u = z[2 * k + 1];
        su = fma(u, u, su);
        sv = fma(v, v, sv);
    }
    su = gsum<64>(su);
    sv = gsum<64>(sv);
    const double iu = su > 0.0 ? 1.0 / sqrt(su) : 0.0, iv = sv > 0.0 ? 1.0 / sqrt(sv) : 0.0;
    for (int k = lane; k < n; k += 64) {
        Vb[size_t(q) * n + k] = z[2 * k] * iv;
        Ub[size_t(q) * n + k] = z[2 * k + 1] * iu;
    }
}

// First-order CholeskyQR step on the rows of X (nearly orthonormal): G = X X^T = I + E -> Li = I - Elow with Elow =
// strict_lower(E) + diag(E) / 2, so that Li X is orthonormal to O(||E||^2) (blockIdx.y: the U / V half)
__global__ void k_first_order_bd(const double* __restrict__ G, int n, double* __restrict__ Li) {
    const size_t off = size_t(blockIdx.y) * n * n;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * n; e += gridDim.x * blockDim.x) {
        const int i = e / n, k = e % n;
        const double g = G[off + e];
        Li[off + e] = i > k ? -g : (i == k ? 1.0 - 0.5 * (g - 1.0) : 0.0);
    }
}

__global__ void k_scale_rows_bd(const double* __restrict__ X, const double* __restrict__ S, int n, double* __restrict__ Y) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * n; e += gridDim.x * blockDim.x) Y[e] = S[e / n] * X[e];
}

// out[0] = ||(P - A) s||_F^2, out[1] = ||A s||_F^2 with s = 2^-ilogb(max |A|) (no overflow / underflow at any
// scale of A), out[2] / out[3] = max |G1 - I| / |G2 - I| (NaN -> inf)
__global__ void __launch_bounds__(1024) k_svd_check(const double* __restrict__ P, const double* __restrict__ A,
                                                    const double* __restrict__ G1, const double* __restrict__ G2, int n,
                                                    double* __restrict__ out) {
    __shared__ double red[4][16];
    __shared__ double samax;
    const int w = threadIdx.x >> 6;
    double am = 0.0;
    for (int e = threadIdx.x; e < n * n; e += 1024) am = fmax(am, fabs(A[e]));
    am = wave_fmax(am);
    wave_partials(am, red[0]);
    if (threadIdx.x == 0) {
        double v = 0.0;
        for (int i = 0; i < 16; ++i) v = fmax(v, red[0][i]);
        samax = v;
    }
    __syncthreads();
    const int sex = samax > 0.0 ? -ilogb(samax) : 0;   // (applied by ldexp: 2^sex overflows for a subnormal max |A|)
    double r2 = 0.0, a2 = 0.0, m1 = 0.0, m2 = 0.0;
    for (int e = threadIdx.x; e < n * n; e += 1024) {
        const double d = ldexp(P[e] - A[e], sex), as = ldexp(A[e], sex), id = (e / n == e % n) ? 1.0 : 0.0;
        r2 = fma(d, d, r2);
        a2 = fma(as, as, a2);
        const double g1 = fabs(G1[e] - id), g2 = fabs(G2[e] - id);
        m1 = (g1 > m1 || g1 != g1) ? (g1 != g1 ? INFINITY : g1) : m1;
        m2 = (g2 > m2 || g2 != g2) ? (g2 != g2 ? INFINITY : g2) : m2;
    }
    r2 = gsum<64>(r2);
    a2 = gsum<64>(a2);
    m1 = wave_fmax(m1);
    m2 = wave_fmax(m2);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = r2;
        red[1][w] = a2;
        red[2][w] = m1;
        red[3][w] = m2;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double v = 0.0;
        for (int i = 0; i < 16; ++i) v = threadIdx.x < 2 ? v + red[threadIdx.x][i] : fmax(v, red[threadIdx.x][i]);
        out[threadIdx.x] = (v != v) ? INFINITY : v;
    }
}

}  // namespace

// Order limit 256 (XRS_SYEV_MAX lowers it): the 512-thread lower-block kernel runs an order-256 edge in
// 1.31 ms against 2.8 ms of Jacobi sweeps ((x + y).round(128): 22.5 -> 13.8 ms, profiles/r03/sum128_l512_r03s.txt).
// Its first version spilled (the tau = 0 early exit gave the column loop a second latch, and the register
// copies at the merge doubled the live matrix): 3.6 ms; the spilling 1024-thread variant measured 5.8 ms.
bool sym_eig_top_fits(int n, int kk) {
    static const int nmax = std::getenv("XRS_SYEV_MAX") ? std::atoi(std::getenv("XRS_SYEV_MAX")) : 256;
    return n >= 2 && n <= std::min(nmax, SY_MAX) && kk >= 1 && kk <= n;
}

// Householder tridiagonalisation alone (d, e of T; xrs_sym_tridiag). Enqueued only.
void sym_tridiag(xrs_handle_t h, const double* A, int lda, int n, double* d, double* e) {
    XRS_REQUIRE(n >= 2 && n <= SY_MAX, "sym_tridiag: need 2 <= n <= 256");
    DevBuf tbuf(h, size_t(n) * 8), V(h, size_t(n) * n * 8);
    if (n <= 64) hipLaunchKernelGGL((k_sytrd<32, 2>), dim3(1), dim3(1024), 0, h->stream, A, lda, n, d, e, tbuf.d(), V.d(), nullptr);
    else if (n <= 128) hipLaunchKernelGGL(k_sytrd_l512<4>, dim3(1), dim3(512), 0, h->stream, A, lda, n, d, e, tbuf.d(), V.d(), nullptr);
    else hipLaunchKernelGGL(k_sytrd_l512<8>, dim3(1), dim3(512), 0, h->stream, A, lda, n, d, e, tbuf.d(), V.d(), nullptr);
    check_launch("k_sytrd");
}

void sym_eig_top(xrs_handle_t h, const double* A, int lda, int n, int kk, double* lam, double* S, double* Ut, int ldu, int* status) {
XRS_REQUIRE(n >= 2 && n <= SY_MAX && kk >= 1 && kk <= n, "sym_eig_top: need 2 <= n <= 256 and 1 <= kk <= n");
    DevBuf dbuf(h, size_t(n) * 8), ebuf(h, size_t(n) * 8), tbuf(h, size_t(n) * 8), V(h, size_t(n) * n * 8), lbuf(h, size_t(kk) * 8);
    double* lm = lam ? lam : lbuf.d();
    KernelTimer timer(h, XRS_KFAM_SVD, 4.0 / 3.0 * double(n) * n * n + 4.0 * double(n) * n * kk, 8.0 * double(n) * n * 2);
    static const bool want_stamps = stamps_enabled("syev");
    DevBuf sb(h, want_stamps ? 2048 * 8 : 0);
    unsigned long long* stp = want_stamps ? sb.as<unsigned long long>() : nullptr;
    if (stp) XRS_HIP(hipMemsetAsync(stp, 0, 2048 * 8, h->stream));
    // the 1024-thread grid up to 64 (r04 A/B, profiles/r04/sytrd_l512_ab_r04t.txt: order-64 edges 2.20 vs
    // 2.38 ms per cfg3-shaped round(32) with the 512-thread kernel), the 512-thread lower-block grid with
    // finished-block skipping above (order 128: 4.11 vs 4.58 ms per cfg3 round(64) against the 1024-thread
    // grid; r03: the 1024-thread grid beat 256 threads with 64 elements each, 5.1 vs 5.6 ms)
    if (n <= 64) {
        hipLaunchKernelGGL((k_sytrd<32, 2>), dim3(1), dim3(1024), 0, h->stream, A, lda, n, dbuf.d(), ebuf.d(), tbuf.d(), V.d(), stp);
    } else if (n <= 128) {
        hipLaunchKernelGGL(k_sytrd_l512<4>, dim3(1), dim3(512), 0, h->stream, A, lda, n, dbuf.d(), ebuf.d(), tbuf.d(), V.d(),
                           stp ? stp + 1024 : nullptr);
    } else {
        hipLaunchKernelGGL(k_sytrd_l512<8>, dim3(1), dim3(512), 0, h->stream, A, lda, n, dbuf.d(), ebuf.d(), tbuf.d(), V.d(),
                           stp ? stp + 1024 : nullptr);
    }
    check_launch("k_sytrd");
    // the chains' reciprocals: 2 Newton steps after the hardware estimate (one step measured 4.40 vs 4.47 ms
    // per cfg3 round(64) but multiplies the kept sigma's relative error by ~20)
    hipLaunchKernelGGL(k_stebz_stein<2>, dim3(kk), dim3(64 * SW_WAVES), 0, h->stream, dbuf.d(), ebuf.d(), n, lm, Ut, ldu, status,
                       stp ? stp + 768 : nullptr);
    check_launch("k_stebz_stein");
    hipLaunchKernelGGL(k_cluster_orth, dim3(1), dim3(256), 0, h->stream, lm, dbuf.d(), ebuf.d(), n, kk, Ut, ldu, kk, status);
    check_launch("k_cluster_orth");
    // (a blocked form -- 16 reflectors' dots together, their recurrence through the block's reflector Gram --
    // measured slower: 162 vs 108 us at order 256, 55 vs 38 us at 128, plus 22-28 us for the Grams; r04ah)
    if (n <= 64) hipLaunchKernelGGL((k_ormtr<1>), dim3((kk + 3) / 4), dim3(256), 0, h->stream, V.d(), tbuf.d(), n, kk, Ut, ldu, V.d(), tbuf.d(), Ut);
    else if (n <= 128) hipLaunchKernelGGL((k_ormtr<2>), dim3((kk + 3) / 4), dim3(256), 0, h->stream, V.d(), tbuf.d(), n, kk, Ut, ldu, V.d(), tbuf.d(), Ut);
    else hipLaunchKernelGGL((k_ormtr<4>), dim3((kk + 3) / 4), dim3(256), 0, h->stream, V.d(), tbuf.d(), n, kk, Ut, ldu, V.d(), tbuf.d(), Ut);
    check_launch("k_ormtr");
    if (stp && n > 64) {   // k_sytrd_l512 column-step phases (cycles, mean over the first 63 steps)
        std::vector<unsigned long long> hl(1024);
        XRS_HIP(hipMemcpyAsync(hl.data(), stp + 1024, 1024 * 8, hipMemcpyDeviceToHost, h->stream));
        XRS_HIP(hipStreamSynchronize(h->stream));
        for (int w = 0; w < 2; ++w) {
            double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int steps = 0;
            for (int j = 0; j + 1 < std::min(n - 2, 64); ++j) {
                const unsigned long long* a = hl.data() + 512 * w + 8 * j;
                if (!a[0] || !a[8]) continue;
                for (int p = 0; p < 7; ++p) ph[p] += double(a[p + 1] - a[p]);
                ph[7] += double(a[8] - a[7]);
                ++steps;
            }
            std::fprintf(stderr, "k_sytrd_l512 n=%d thread %d: mean cycles per step over %d: barrier1 %.0f reflector %.0f barrier2 %.0f symv %.0f "
                         "barrier3 %.0f combine %.0f barrier4 %.0f update %.0f\n", n, w ? 64 : 0, steps, ph[0] / steps, ph[1] / steps,
                         ph[2] / steps, ph[3] / steps, ph[4] / steps, ph[5] / steps, ph[6] / steps, ph[7] / steps);
        }
    }
    if (stp) {   // k_stebz_stein phases of workgroup 0 (cycles)
        std::vector<unsigned long long> hs(12);
        XRS_HIP(hipMemcpyAsync(hs.data(), stp + 768, 12 * 8, hipMemcpyDeviceToHost, h->stream));
        XRS_HIP(hipStreamSynchronize(h->stream));
        std::fprintf(stderr, "k_stebz_stein n=%d: prologue %llu multisection %llu LU %llu pivots %llu solve/normalise %llu/%llu %llu/%llu %llu/%llu store %llu\n", n,
                     hs[1] - hs[0], hs[2] - hs[1], hs[3] - hs[2], hs[4] - hs[3], hs[5] - hs[4], hs[6] - hs[5], hs[7] - hs[6],
                     hs[8] - hs[7], hs[9] - hs[8], hs[10] - hs[9], hs[11] - hs[10]);
    }
    if (stp) {   // per-phase cycles of the first steps: (b)-wait, reflector, wait, symv, wait, update (+ column)
        std::vector<unsigned long long> hst(768);
        XRS_HIP(hipMemcpyAsync(hst.data(), stp, 768 * 8, hipMemcpyDeviceToHost, h->stream));
        XRS_HIP(hipStreamSynchronize(h->stream));
        for (int w = 0; w < 2; ++w) {
            double ph[6] = {0, 0, 0, 0, 0, 0};
            int steps = 0;
            for (int j = 0; j + 1 < std::min(n - 2, 64); ++j) {
                const unsigned long long* a = hst.data() + 384 * w + 6 * j;
                const unsigned long long nxt = a[6];
                if (!a[0] || !nxt) continue;
                ph[0] += double(a[1] - a[0]); ph[1] += double(a[2] - a[1]); ph[2] += double(a[3] - a[2]);
                ph[3] += double(a[4] - a[3]); ph[4] += double(a[5] - a[4]); ph[5] += double(nxt - a[5]);
                ++steps;
            }
            std::fprintf(stderr, "k_sytrd n=%d thread %d: mean cycles per step over %d: barrier1 %.0f reflector %.0f barrier2 %.0f symv %.0f barrier3 %.0f update %.0f\n",
                         n, w ? 64 : 0, steps, ph[0] / steps, ph[1] / steps, ph[2] / steps, ph[3] / steps, ph[4] / steps, ph[5] / steps);
        }
    }
    if (S) {
        hipLaunchKernelGGL(k_sqrt_lam, dim3((kk + 255) / 256), dim3(256), 0, h->stream, lm, kk, S);
        check_launch("k_sqrt_lam");
    }
}

// Square SVD (dgesdd's role, n <= 128) without Jacobi sweeps: B = bidiagonal of A (k_gebrd_sq), its singular
// triplets as the top n eigenpairs of the Golub-Kahan tridiagonal of order 2n (the multisection + inverse
// iteration of sym_eig_top; clusters up to 24 vectors orthonormalised), the u / v halves back-transformed by the
// reflectors (k_ormtr, both sets in one launch) and re-orthonormalised by one first-order CholeskyQR step on their
// rows (inverse iteration leaves each half's error toward the -sigma partners at u ||A|| / sigma, so the
// correction changes U S Vt by O(u ||A||)). The result is certified a posteriori: ||U S Vt - A||_F <= 6e-15
// ||A||_F and max |U^T U - I|, |Vt Vt^T - I| <= 6e-15 (dgesdd measured 1e-15..3e-15 on these shapes) -- else
// false and the caller recomputes with Jacobi: spectra with clusters beyond 24 (graded over many decades, flat,
// rank-deficient), whose vectors inverse iteration cannot separate cheaply. Synchronises (the check).
// n = 128 (profiles/r06/svd_bidiag_*): 0.84 ms against 1.6 ms of Jacobi; k_gebrd_sq 490 us of it, k_stebz_stein
// 150 us, the rest 30-40 us launches.
int svd_bidiag_mode() {
    static const int mode = std::getenv("XRS_SVD_BIDIAG") ? std::atoi(std::getenv("XRS_SVD_BIDIAG")) : 1;
    return mode;
}

bool svd_bidiag(xrs_handle_t h, const double* A, int n, double* U, double* S, double* Vt, double* diag) {
    XRS_REQUIRE(n >= 2 && n <= BD_MAX, "svd_bidiag: need 2 <= n <= 128");
    const size_t nn = size_t(n) * n;
    // (Ub, Vb adjacent: the halves' first-order steps run as one batch; W holds the Grams, then Li)
    DevBuf tg(h, size_t(4 * n) * 8), Vl(h, nn * 8), Vr(h, nn * 8), taus(h, size_t(2 * n) * 8), lam(h, size_t(n) * 8),
        Z(h, nn * 2 * 8), UVb(h, nn * 2 * 8), W(h, nn * 2 * 8), Ut(h, nn * 8), st(h, 64), chk(h, 64);
    double *tgd = tg.d(), *tge = tg.d() + 2 * n, *tl = taus.d(), *tr = taus.d() + n, *Ub = UVb.d(), *Vb = UVb.d() + nn;
    {
        KernelTimer timer(h, XRS_KFAM_SVD, 8.0 / 3.0 * double(nn) * n + 8.0 * double(nn) * n, 8.0 * double(nn) * 4);
        static const bool want_stamps = stamps_enabled("bd");
        DevBuf sb(h, want_stamps ? 1024 * 8 : 0);
        unsigned long long* stp = want_stamps ? sb.as<unsigned long long>() : nullptr;
        if (stp) XRS_HIP(hipMemsetAsync(stp, 0, 1024 * 8, h->stream));
        hipLaunchKernelGGL(k_gebrd_sq, dim3(1), dim3(512), 0, h->stream, A, n, tgd, tge, Vl.d(), tl, Vr.d(), tr, st.as<int>(), stp);
        check_launch("k_gebrd_sq");
        if (stp) {   // k_gebrd_sq phases (cycles): prologue, per column (H partial, H update + squares, G phase), epilogue
            std::vector<unsigned long long> hs(1024);
            XRS_HIP(hipMemcpyAsync(hs.data(), stp, 1024 * 8, hipMemcpyDeviceToHost, h->stream));
            XRS_HIP(hipStreamSynchronize(h->stream));
            double ph[3] = {0, 0, 0};
            int steps = 0;
            for (int j = 0; j + 1 < n - 1; ++j) {
                const unsigned long long* q = hs.data() + 4 + 4 * j;
                if (!q[0] || !q[1] || !q[2] || !q[4]) continue;
                ph[0] += double(q[1] - q[0]);
                ph[1] += double(q[2] - q[1]);
                ph[2] += double(q[4] - q[2]);
                ++steps;
            }
            {
                double gp[5] = {0, 0, 0, 0, 0};
                int cnt = 0;
                for (int j = 0; j < std::min(n - 2, 95); ++j) {
                    const unsigned long long* q = hs.data() + 600 + 4 * j;
                    const unsigned long long g0 = hs[6 + 4 * j], b3 = hs[7 + 4 * j], nx = hs[8 + 4 * j];
                    if (!q[0] || !q[1] || !q[2] || !g0 || !b3 || !nx) continue;
                    gp[0] += double(q[0] - g0);   // ss + reflector
                    gp[1] += double(q[1] - q[0]);   // vc, right product, partials
                    gp[2] += double(b3 - q[1]);     // barrier 3
                    gp[3] += double(q[2] - b3);     // wsum + barrier 4
                    gp[4] += double(nx - q[2]);     // right update
                    ++cnt;
                }
                std::fprintf(stderr, "k_gebrd_sq n=%d G_j thread 0: reflector %.0f right product %.0f barrier3 %.0f wsum+barrier4 %.0f update %.0f (over %d)\n",
                             n, gp[0] / cnt, gp[1] / cnt, gp[2] / cnt, gp[3] / cnt, gp[4] / cnt, cnt);
            }
            std::fprintf(stderr, "k_gebrd_sq n=%d: total %llu prologue %llu epilogue %llu; mean per column over %d: H_j %.0f left product + row j %.0f G_j %.0f; "
                         "column 0: %llu %llu %llu\n", n, hs[3] - hs[0], hs[1] - hs[0], hs[3] - hs[2], steps, ph[0] / steps, ph[1] / steps,
                         ph[2] / steps, hs[5] - hs[4], hs[6] - hs[5], hs[8] - hs[6]);
        }
        // (two inverse-iteration solves instead of three measured 0.842 vs 0.862 ms at n = 128: not worth the margin)
        hipLaunchKernelGGL((k_stebz_stein<2, 3>), dim3(n), dim3(64 * SW_WAVES), 0, h->stream, tgd, tge, 2 * n, lam.d(), Z.d(),
                           2 * n, st.as<int>(), nullptr);
        check_launch("k_stebz_stein");
        hipLaunchKernelGGL(k_cluster_orth, dim3(1), dim3(256), 0, h->stream, lam.d(), tgd, tge, 2 * n, n, Z.d(), 2 * n, 24,
                           st.as<int>());
        check_launch("k_cluster_orth");
        hipLaunchKernelGGL(k_gk_split, dim3((n + 3) / 4), dim3(256), 0, h->stream, Z.d(), lam.d(), n, Ub, Vb, S);
        check_launch("k_gk_split");
        if (n <= 64)
            hipLaunchKernelGGL((k_ormtr<1>), dim3((n + 3) / 4, 2), dim3(256), 0, h->stream, Vl.d(), tl, n, n, Ub, n, Vr.d(), tr, Vb);
        else
            hipLaunchKernelGGL((k_ormtr<2>), dim3((n + 3) / 4, 2), dim3(256), 0, h->stream, Vl.d(), tl, n, n, Ub, n, Vr.d(), tr, Vb);
        check_launch("k_ormtr");
    }
    // the halves' rows orthonormalised by one first-order CholeskyQR step (their Grams are I + O(u ||T|| / gap)
    // outside the clusters; a half that needs more fails the check below)
    {
        double* Gp[2] = {W.d(), W.d() + nn};
        const double* Xp[2] = {Ub, Vb};
        gemm_batched(h, 2, Gp, size_t(n), size_t(n), 1.0, Xp, size_t(n), false, size_t(n), Xp, size_t(n), true, true);
        hipLaunchKernelGGL(k_first_order_bd, dim3((unsigned(nn) + 255) / 256, 2), dim3(256), 0, h->stream, W.d(), n, W.d());
        check_launch("k_first_order_bd");
        double* Qp[2] = {Ut.d(), Vt};
        const double* Lp[2] = {W.d(), W.d() + nn};
        gemm_batched(h, 2, Qp, size_t(n), size_t(n), 1.0, Lp, size_t(n), false, size_t(n), Xp, size_t(n), false, false, kTriA);
    }
    transpose(h, U, Ut.d(), size_t(n), size_t(n));
    // a posteriori check (Ub / Vb / W / Z reused as scratch)
    hipLaunchKernelGGL(k_scale_rows_bd, dim3((nn + 255) / 256), dim3(256), 0, h->stream, Vt, S, n, Ub);
    check_launch("k_scale_rows_bd");
    gemm(h, Vb, size_t(n), size_t(n), 1.0, U, size_t(n), false, size_t(n), Ub, size_t(n), false);   // U S Vt
    {
        double* Gp[2] = {Z.d(), Z.d() + nn};
        const double* Xp[2] = {Ut.d(), Vt};
        gemm_batched(h, 2, Gp, size_t(n), size_t(n), 1.0, Xp, size_t(n), false, size_t(n), Xp, size_t(n), true, true);   // U^T U, Vt Vt^T
    }
    hipLaunchKernelGGL(k_svd_check, dim3(1), dim3(1024), 0, h->stream, Vb, A, Z.d(), Z.d() + nn, n, chk.d());
    check_launch("k_svd_check");
    double* hc = scratch::host<double>(h, scratch::kHostSvdCheck, 5);
    XRS_HIP(hipMemcpyAsync(hc, chk.d(), 32, hipMemcpyDeviceToHost, h->stream));
    XRS_HIP(hipMemcpyAsync(hc + 4, st.d(), 4, hipMemcpyDeviceToHost, h->stream));
    XRS_HIP(hipStreamSynchronize(h->stream));
    int hs = 0;
    std::memcpy(&hs, hc + 4, 4);
    const double res = std::sqrt(hc[0]), anorm = std::sqrt(hc[1]);
    if (diag) {
        diag[0] = anorm > 0.0 ? res / anorm : res;
        diag[1] = hc[2];
        diag[2] = hc[3];
        diag[3] = hs;
    }
    return hs == 0 && res <= 6e-15 * anorm && hc[2] <= 6e-15 && hc[3] <= 6e-15;
}

}  // namespace xrs
