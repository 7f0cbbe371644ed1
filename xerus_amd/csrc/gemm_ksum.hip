// Summed fp64 GEMM: C (M x N, row-major, ldc = N) = alpha * sum_j A_j (M x K_j, lda_j) * B_j (K_j x N, ldb_j), the
// operands of every term j living in their own allocations (the sketch Z = sum_j V(X_j) W_j and the last core of the
// randomized rounding of a TT sum, tt_rand.hip). No concatenated operand is ever formed.
//
// Kernel (k_gemm_ksum): 256 threads = 4 waves as 2 x 2, block tile (32 T) x (32 T), T = 1 or 2, each wave a
// (16 T) x (16 T) sub-tile of 16x16 v_mfma_f64_16x16x4_f64 tiles with the lane layouts of gemm.hip:
//   A operand: lane l holds A[row l&15][k l>>4]; B operand: B[k l>>4][col l&15]; C/D: col = l&15, row = (l>>4) + 4*reg.
// Operands are staged k-major through LDS ([k][m] and [k][n]) with the odd row stride S = 32 T + 17 doubles: the
// transposed ds_write_b64 of the k-contiguous A rows hits 16 distinct bank pairs per 16-lane group, and the k / k+1
// fragment rows of a ds_read_b64 overlap in one bank pair. The next K-step is loaded into registers while the
// current one computes (one barrier per step, LDS ping-pong).
// The segment loop is the outer K loop: the concatenated K is measured in 16-wide chunks per segment (segment j has
// ceil(K_j / 16) of them, a K_j = 0 segment none), a workgroup walks its range of chunks and re-bases the A and B
// pointers at each segment boundary. Rows at or past M, columns at or past N and k at or past K_j are exact zeros
// that are never read from memory.
// The segment table {A, B, K, lda, ldb} travels by value, kKsumTable entries per launch; larger counts take further
// launches. The tile grid of the shapes this serves (M ~ 1100, N <= ~270) cannot fill 256 CUs, so the chunks of a
// launch are cut into slices (grid.y) that write partial slabs into pool scratch; k_ksum_combine sums all slabs of
// all launches in slice order and applies alpha. No atomics, no tickets; the slice count depends on the shape
// arguments only, so the result is the same bits on every run. One launch with one slice writes C directly.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "gemm_ksum.hpp"
#include "runtime.hpp"

namespace xrs {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

struct KsumTable {
    const double* A[kKsumTable];
    const double* B[kKsumTable];
    unsigned long long lda[kKsumTable];
    unsigned long long ldb[kKsumTable];
    unsigned K[kKsumTable];
    unsigned chunk0[kKsumTable + 1];   // first chunk of segment j in the launch's concatenated K; [nseg] = total
    int nseg;
};

// grid (tiles_m * tiles_n, slices). out: C (scale = alpha) or the first slab of this launch (scale = 1)
template <int T>
__global__ void __launch_bounds__(256) k_gemm_ksum(const KsumTable tab, double* __restrict__ out, int M, int N, int tiles_m,
                                                   unsigned cps, double scale, int to_slab) {
    constexpr int BM = 32 * T, BN = 32 * T, S = 32 * T + 17;
    constexpr int PER = BM * 16 / 256;   // staged doubles per thread and operand
    __shared__ double As[2][16 * S];
    __shared__ double Bs[2][16 * S];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int wm = (wave >> 1) * (16 * T), wn = (wave & 1) * (16 * T);
    const int m0 = (int(blockIdx.x) % tiles_m) * BM, n0 = (int(blockIdx.x) / tiles_m) * BN;
    const unsigned total = tab.chunk0[tab.nseg];
    const unsigned c_lo = blockIdx.y * cps;
    const unsigned c_hi = c_lo + cps < total ? c_lo + cps : total;

    // this thread's staging coordinates: A elements (m, k) with k fastest (a row's 16 doubles are 128 contiguous
    // bytes), B elements (k, n) with n fastest
    int am[PER], ak[PER], bk[PER], bn[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int idx = tid + e * 256;
        ak[e] = idx & 15;
        am[e] = idx >> 4;
        bn[e] = idx % BN;
        bk[e] = idx / BN;
    }

    d4 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};

    int seg = 0;   // segment of the chunk loaded last (chunks are loaded in ascending order)
    double ra[PER], rb[PER];
    auto load = [&](unsigned c) {
        while (c >= tab.chunk0[seg + 1]) ++seg;
        const double* __restrict__ A = tab.A[seg];
        const double* __restrict__ B = tab.B[seg];
        const unsigned long long lda = tab.lda[seg], ldb = tab.ldb[seg];
        const unsigned K = tab.K[seg], k0 = (c - tab.chunk0[seg]) * 16u;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int gm = m0 + am[e];
            const unsigned gk = k0 + unsigned(ak[e]);
            ra[e] = (gm < M && gk < K) ? A[(unsigned long long)gm * lda + gk] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            const int gn = n0 + bn[e];
            const unsigned gk = k0 + unsigned(bk[e]);
            rb[e] = (gn < N && gk < K) ? B[(unsigned long long)gk * ldb + gn] : 0.0;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int e = 0; e < PER; ++e) As[buf][ak[e] * S + am[e]] = ra[e];
#pragma unroll
        for (int e = 0; e < PER; ++e) Bs[buf][bk[e] * S + bn[e]] = rb[e];
    };

    if (c_lo < c_hi) {
        load(c_lo);
        stage(0);
    }
    __syncthreads();
    int buf = 0;
    for (unsigned c = c_lo; c < c_hi; ++c) {
        const bool more = c + 1 < c_hi;
        if (more) load(c + 1);   // in flight under the MFMAs below
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            double a[T], b[T];
#pragma unroll
            for (int i = 0; i < T; ++i) a[i] = As[buf][(4 * kk + lk) * S + wm + 16 * i + lr];
#pragma unroll
            for (int j = 0; j < T; ++j) b[j] = Bs[buf][(4 * kk + lk) * S + wn + 16 * j + lr];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) stage(buf ^ 1);   // (its readers finished before the last barrier)
        __syncthreads();
        buf ^= 1;
    }

    double* dst = out + (to_slab ? (unsigned long long)blockIdx.y * (unsigned long long)M * (unsigned long long)N : 0ull);
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int col = n0 + wn + 16 * j + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm + 16 * i + lk + 4 * r;
                if (row < M && col < N) dst[(unsigned long long)row * N + col] = scale * acc[i][j][r];
            }
        }
}

// C[e] = alpha * (part[0][e] + part[1][e] + ..), the slabs in slice order (none: C = 0)
__global__ void __launch_bounds__(256) k_ksum_combine(double* __restrict__ C, const double* __restrict__ part,
                                                      unsigned long long elems, unsigned nslabs, double alpha) {
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < elems;
         e += (unsigned long long)gridDim.x * 256) {
        if (nslabs == 0) {
            C[e] = 0.0;
            continue;
        }
        double t = part[e];
        for (unsigned p = 1; p < nslabs; ++p) t += part[(unsigned long long)p * elems + e];
        C[e] = alpha * t;
    }
}

}  // namespace

void gemm_ksum(xrs_handle_t h, double* C, size_t M, size_t N, double alpha, size_t count, const double* const* A,
               const size_t* lda, const size_t* K, const double* const* B, const size_t* ldb) {
    if (const char* wrong = ksum_check(C, M, N, count, A, lda, K, B, ldb)) XRS_REQUIRE(false, wrong);
    const KsumPlan plan = ksum_plan(M, N, count, K);
    const bool direct = plan.slabs == 1;
    const size_t MN = M * N;
    DevBuf ksum_slabs;   // [slab][M][N]
    if (!direct && plan.slabs > 0) ksum_slabs = DevBuf(h, plan.slabs * MN * 8);

    for (const KsumLaunch& l : plan.launches) {
        KsumTable tab{};
        unsigned chunk = 0;
        int nseg = 0;
        for (size_t s = 0; s < l.count; ++s) {
            const size_t j = l.first + s;
            if (K[j] == 0) continue;
            tab.A[nseg] = A[j];
            tab.B[nseg] = B[j];
            tab.lda[nseg] = lda[j];
            tab.ldb[nseg] = ldb[j];
            tab.K[nseg] = unsigned(K[j]);
            tab.chunk0[nseg] = chunk;
            chunk += unsigned((K[j] + kKsumChunk - 1) / kKsumChunk);
            ++nseg;
        }
        tab.chunk0[nseg] = chunk;
        tab.nseg = nseg;
        double* out = direct ? C : ksum_slabs.d() + l.slab0 * MN;
        const dim3 grid{unsigned(plan.tiles_m * plan.tiles_n), unsigned(l.slices), 1};
        double kl = 0.0;
        for (int s = 0; s < nseg; ++s) kl += double(tab.K[s]);
        KernelTimer timer(h, XRS_KFAM_GEMM, 2.0 * double(M) * double(N) * kl, 8.0 * (double(M) + double(N)) * kl);
        if (plan.tile == 32)
            hipLaunchKernelGGL((k_gemm_ksum<1>), grid, dim3(256), 0, h->stream, tab, out, int(M), int(N), int(plan.tiles_m),
                               unsigned(l.chunks_per_slice), direct ? alpha : 1.0, direct ? 0 : 1);
        else
            hipLaunchKernelGGL((k_gemm_ksum<2>), grid, dim3(256), 0, h->stream, tab, out, int(M), int(N), int(plan.tiles_m),
                               unsigned(l.chunks_per_slice), direct ? alpha : 1.0, direct ? 0 : 1);
        check_launch("k_gemm_ksum");
    }
    if (!direct) {
        KernelTimer timer(h, XRS_KFAM_SPLITK, double(plan.slabs) * double(MN), 8.0 * double(plan.slabs + 1) * double(MN));
        const unsigned blocks = unsigned(std::min<size_t>((MN + 255) / 256, size_t(1) << 16));
        hipLaunchKernelGGL(k_ksum_combine, dim3(blocks), dim3(256), 0, h->stream, C, ksum_slabs.d(), (unsigned long long)MN,
                           unsigned(plan.slabs), alpha);
        check_launch("k_ksum_combine");
    }
}

}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_gemm_ksum(xrs_handle_t h, double* C, size_t M, size_t N, double alpha, size_t count, const double* const* A,
                  const size_t* lda, const size_t* K, const double* const* B, const size_t* ldb) {
    return guarded([&] {
        XRS_REQUIRE(h, "null handle");
        if (const char* wrong = ksum_check(C, M, N, count, A, lda, K, B, ldb)) XRS_REQUIRE(false, wrong);
        fence_readers(h);
        gemm_ksum(h, C, M, N, alpha, count, A, lda, K, B, ldb);
    });
}

}  // extern "C"
