// Gaussian sketches Y = G A of the randomized TT-SVD (host/random_svd.cpp; reference algorithm:
// include/xerus/algorithms/randomSVD.h:31-98, whose g = Tensor::random(...) and contract(a, g, b) these replace).
// G = G(seed, stream) is the counter-based matrix of philox.hpp; DESIGN §3.9.
//
//   xrs_philox_words      the raw words W(i, q) (diagnostic of the bit-exact test)
//   xrs_gaussian_matrix   the leading s x m block of G in HBM (one thread per word block, 32 B each)
//   xrs_sketch_gaussian   Y (s x n) = G[0:s, 0:m] A (m x n):
//     route 1, fused (k_sketch_fused): G never exists in memory. On v_mfma_f64_16x16x4_f64 the A operand is one
//       fp64 per lane (row l & 15, k l >> 4), so a lane generates the word block W(row, q0 + (l >> 4)) and feeds
//       its four normals to four consecutive MFMA K-steps: step j contracts the columns c = 4 (q0 + (l >> 4)) + j
//       of G, and the B operand of that step is the caller's A[c][col l & 15] -- per 16-lane group one 128-byte row
//       segment. A wave keeps the accumulators of all RB = ceil(s / 16) row blocks and of CB column blocks, so a
//       loaded tile of A is used RB times and a generated normal CB times. The contracted dimension m is split:
//       a workgroup (4 waves) owns a slab of m, its waves take the slab's 16-row chunks round robin and are summed
//       in wave order through LDS; with more than one slab the workgroups write partial products that
//       k_sketch_combine sums in slab order. No atomics: the result is the same bits every run.
//     route 2, materialised: xrs_gaussian_matrix into pool scratch, then the GEMM.
#include <algorithm>
#include <cstdint>

#include "elementwise.hpp"
#include "philox.hpp"
#include "runtime.hpp"

namespace xrs {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMaxRowBlocks = 5;                      // fused envelope: s <= 80
constexpr size_t kFusedMaxS = 16 * kMaxRowBlocks;
constexpr uint64_t kSlabQuantum = 64;                 // 4 waves x one 16-row chunk
constexpr uint64_t kMinSlab = 256;
constexpr uint64_t kTargetGroups = 1024;              // 4 workgroups per CU of a 256-CU device
constexpr uint64_t kMaxSlabs = 4096;

// ------------------------------------------------------------------------------------------ words, matrix
__global__ void __launch_bounds__(256) k_philox_words(uint32_t* __restrict__ out, uint64_t s, uint64_t qn, uint64_t seed,
                                                      uint32_t stream) {
    const uint64_t total = s * qn;
    for (uint64_t idx = uint64_t(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += uint64_t(gridDim.x) * 256) {
        const uint64_t i = idx / qn, q = idx - i * qn;
        const philox::Words x = philox::words(seed, stream, uint32_t(i), q);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[4 * idx + j] = x.w[j];
    }
}

__global__ void __launch_bounds__(256) k_gaussian_matrix(double* __restrict__ G, uint64_t s, uint64_t m, uint64_t qn,
                                                         uint64_t seed, uint32_t stream) {
    const uint64_t total = s * qn;
    for (uint64_t idx = uint64_t(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += uint64_t(gridDim.x) * 256) {
        const uint64_t i = idx / qn, q = idx - i * qn;
        double g[4];
        philox::gauss4(seed, stream, uint32_t(i), q, g);
        double* row = G + i * m;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < m) row[4 * q + j] = g[j];
    }
}

unsigned grid_for(uint64_t total) { return unsigned(std::min<uint64_t>((total + 255) / 256, uint64_t(1) << 20)); }

// ------------------------------------------------------------------------------------------ fused product
// grid (column groups of 16 CB, slabs). out: Y when there is one slab, else the partial products [slab][s][n].
template <int RB, int CB>
__global__ void __launch_bounds__(256) k_sketch_fused(const double* __restrict__ A, double* __restrict__ out, uint32_t s,
                                                      uint64_t m, uint32_t n, uint64_t slab, uint64_t seed, uint32_t stream) {
    __shared__ double red[RB * CB * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const uint64_t k_lo = uint64_t(blockIdx.y) * slab;
    const uint64_t k_hi = k_lo + slab < m ? k_lo + slab : m;
    const uint32_t col0 = blockIdx.x * (16 * CB);

    bool colok[CB];
    const double* acol[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const uint32_t col = col0 + cb * 16 + lr;
        colok[cb] = col < n;
        acol[cb] = A + (colok[cb] ? col : 0);
    }

    d4 acc[RB][CB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) acc[rb][cb] = d4{0.0, 0.0, 0.0, 0.0};

    // the rows of A this lane contracts in the chunk at k0: c = k0 + 4 lk + j, j = 0..3; a masked element is an exact
    // zero that is never read from memory (rows at or past m, columns at or past n)
    auto load = [&](uint64_t k0, double (&b)[CB][4]) {
        const uint64_t c0 = k0 + 4 * lk;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) b[cb][j] = (colok[cb] && c0 + j < k_hi) ? acol[cb][(c0 + j) * n] : 0.0;
    };

    double bcur[CB][4], bnext[CB][4];
    uint64_t k0 = k_lo + 16 * uint64_t(wave);
    if (k0 < k_hi) load(k0, bcur);
    for (; k0 < k_hi; k0 += 64) {
        load(k0 + 64, bnext);   // in flight under the generation below (past the slab: all masked, no access)
        double g[RB][4];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) philox::gauss4(seed, stream, uint32_t(rb * 16 + lr), (k0 >> 2) + lk, g[rb]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
                    acc[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(g[rb][j], bcur[cb][j], acc[rb][cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) bcur[cb][j] = bnext[cb][j];
    }

    // waves 1..3 into wave 0, in wave order
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[((rb * CB + cb) * 4 + r) * 64 + lane] = acc[rb][cb][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[rb][cb][r] += red[((rb * CB + cb) * 4 + r) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    double* dst = out + (gridDim.y > 1 ? uint64_t(blockIdx.y) * s * n : 0);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t row = rb * 16 + lk + 4 * r;   // D: col l & 15, row (l >> 4) + 4 reg
                if (row < s && colok[cb]) dst[uint64_t(row) * n + col0 + cb * 16 + lr] = acc[rb][cb][r];
            }
}

// Y[e] = sum over the slabs p = 0, 1, .. of part[p][e] in a fixed order: 16 elements per workgroup, thread (ty, tx)
// sums the slabs ty, ty + 16, .. of element tx in ascending order, thread (0, tx) then the 16 sums in ty order
__global__ void __launch_bounds__(256) k_sketch_combine(double* __restrict__ Y, const double* __restrict__ part, uint64_t elems,
                                                        uint32_t nslabs) {
    __shared__ double sums[16][16];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const uint64_t e = uint64_t(blockIdx.x) * 16 + tx;
    double v = 0.0;
    if (e < elems)
        for (uint32_t p = ty; p < nslabs; p += 16) v += part[uint64_t(p) * elems + e];
    sums[ty][tx] = v;
    __syncthreads();
    if (ty == 0 && e < elems) {
        double t = sums[0][tx];
#pragma unroll
        for (int k = 1; k < 16; ++k) t += sums[k][tx];
        Y[e] = t;
    }
}

int fused_col_blocks(size_t s, size_t n) {
    const int rb = int((s + 15) / 16);
    int cb = n <= 16 ? 1 : n <= 32 ? 2 : 4;
    if (rb >= 4 && cb > 2) cb = 2;   // 20 accumulator tiles would leave one wave per SIMD
    return cb;
}

template <int RB, int CB>
void launch_fused(xrs_handle_t h, dim3 grid, const double* A, double* out, size_t s, size_t m, size_t n, uint64_t slab,
                  uint64_t seed, uint32_t stream) {
    hipLaunchKernelGGL((k_sketch_fused<RB, CB>), grid, dim3(256), 0, h->stream, A, out, uint32_t(s), uint64_t(m), uint32_t(n),
                       slab, seed, stream);
}

template <int RB>
void launch_fused_cb(xrs_handle_t h, int cb, dim3 grid, const double* A, double* out, size_t s, size_t m, size_t n,
                     uint64_t slab, uint64_t seed, uint32_t stream) {
    if (cb == 1) launch_fused<RB, 1>(h, grid, A, out, s, m, n, slab, seed, stream);
    else if (cb == 2) launch_fused<RB, 2>(h, grid, A, out, s, m, n, slab, seed, stream);
    else if constexpr (RB < 4) launch_fused<RB, 4>(h, grid, A, out, s, m, n, slab, seed, stream);
}

void sketch_fused(xrs_handle_t h, double* Y, size_t s, const double* A, size_t m, size_t n, uint64_t seed, uint32_t stream) {
    const int rb = int((s + 15) / 16), cb = fused_col_blocks(s, n);
    const uint64_t groups = (n + 16 * size_t(cb) - 1) / (16 * size_t(cb));
    uint64_t nslabs = std::max<uint64_t>(1, kTargetGroups / groups);
    nslabs = std::min({nslabs, (uint64_t(m) + kMinSlab - 1) / kMinSlab, kMaxSlabs});
    uint64_t slab = (uint64_t(m) + nslabs - 1) / nslabs;
    slab = (slab + kSlabQuantum - 1) / kSlabQuantum * kSlabQuantum;
    nslabs = (uint64_t(m) + slab - 1) / slab;
    DevBuf part;
    if (nslabs > 1) part = DevBuf(h, nslabs * s * n * 8);
    double* out = nslabs > 1 ? part.d() : Y;
    const dim3 grid{unsigned(groups), unsigned(nslabs), 1};
    {
        KernelTimer timer(h, XRS_KFAM_GEMM, 2.0 * double(s) * double(m) * double(n), 8.0 * double(m) * double(n));
        switch (rb) {
            case 1: launch_fused_cb<1>(h, cb, grid, A, out, s, m, n, slab, seed, stream); break;
            case 2: launch_fused_cb<2>(h, cb, grid, A, out, s, m, n, slab, seed, stream); break;
            case 3: launch_fused_cb<3>(h, cb, grid, A, out, s, m, n, slab, seed, stream); break;
            case 4: launch_fused_cb<4>(h, cb, grid, A, out, s, m, n, slab, seed, stream); break;
            default: launch_fused_cb<5>(h, cb, grid, A, out, s, m, n, slab, seed, stream); break;
        }
        check_launch("k_sketch_fused");
    }
    if (nslabs > 1) {
        const uint64_t elems = uint64_t(s) * n;
        KernelTimer timer(h, XRS_KFAM_SPLITK, double(nslabs) * double(elems), 8.0 * double(nslabs) * double(elems));
        hipLaunchKernelGGL(k_sketch_combine, dim3(unsigned((elems + 15) / 16)), dim3(256), 0, h->stream, Y, part.d(), elems,
                           uint32_t(nslabs));
        check_launch("k_sketch_combine");
    }
}

void gaussian_matrix(xrs_handle_t h, double* G, size_t s, size_t m, uint64_t seed, uint32_t stream) {
    const uint64_t qn = (uint64_t(m) + 3) / 4;
    KernelTimer timer(h, XRS_KFAM_ELEMWISE, 0.0, 8.0 * double(s) * double(m));
    hipLaunchKernelGGL(k_gaussian_matrix, dim3(grid_for(uint64_t(s) * qn)), dim3(256), 0, h->stream, G, uint64_t(s), uint64_t(m),
                       qn, seed, stream);
    check_launch("k_gaussian_matrix");
}

constexpr size_t kRowLimit = size_t(1) << 32;   // rows of G are 32-bit counter words

// route 0. Measured (tools/random_ttsvd_probe.py): at s = 16, 40, 72 and n = 16 .. 1024 the fused route
// takes 0.08 - 0.80 of the materialised one's time, the ratio growing with s and n but below 1 everywhere, so the rule
// is the envelope: fused wherever the kernel holds s.
int auto_route(size_t s) { return s <= kFusedMaxS ? XRS_SKETCH_FUSED : XRS_SKETCH_MATERIALISED; }

}  // namespace
}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_philox_words(xrs_handle_t h, uint32_t* out, size_t s, size_t q, uint64_t seed, uint32_t stream) {
    return guarded([&] {
        XRS_REQUIRE(h, "null handle");
        XRS_REQUIRE(s > 0 && q > 0, "s and q must be positive");
        XRS_REQUIRE(s <= kRowLimit, "rows of G must be below 2^32");
        XRS_REQUIRE(q <= (size_t(1) << 58) / s, "too many word blocks");
        XRS_REQUIRE(out, "null output");
        fence_readers(h);
        hipLaunchKernelGGL(k_philox_words, dim3(grid_for(uint64_t(s) * q)), dim3(256), 0, h->stream, out, uint64_t(s), uint64_t(q),
                           seed, stream);
        check_launch("k_philox_words");
    });
}

int xrs_gaussian_matrix(xrs_handle_t h, double* G, size_t s, size_t m, uint64_t seed, uint32_t stream) {
    return guarded([&] {
        XRS_REQUIRE(h, "null handle");
        XRS_REQUIRE(s > 0 && m > 0, "s and m must be positive");
        XRS_REQUIRE(s <= kRowLimit, "rows of G must be below 2^32");
        XRS_REQUIRE(m <= (size_t(1) << 58) / s, "matrix too large");
        XRS_REQUIRE(G, "null output");
        fence_readers(h);
        gaussian_matrix(h, G, s, m, seed, stream);
    });
}

int xrs_sketch_gaussian(xrs_handle_t h, double* Y, size_t s, const double* A, size_t m, size_t n, uint64_t seed, uint32_t stream,
                        int route) {
    return guarded([&] {
        XRS_REQUIRE(h, "null handle");
        XRS_REQUIRE(s > 0 && m > 0 && n > 0, "s, m and n must be positive");
        XRS_REQUIRE(s <= kRowLimit, "rows of G must be below 2^32");
        XRS_REQUIRE(m < (size_t(1) << 40) && n < (size_t(1) << 31) && s < (size_t(1) << 30), "sketch dimension too large");
        XRS_REQUIRE(Y && A, "null argument");
        XRS_REQUIRE(Y != A, "Y must not alias A");
        XRS_REQUIRE(route >= 0 && route <= 2, "route must be 0 (auto), 1 (fused) or 2 (materialised)");
        XRS_REQUIRE(route != XRS_SKETCH_FUSED || s <= kFusedMaxS, "the fused route takes at most 80 sketch rows");
        if (route == 0) route = auto_route(s);
        fence_readers(h);
        if (route == XRS_SKETCH_FUSED) {
            sketch_fused(h, Y, s, A, m, n, seed, stream);
        } else {
            DevBuf G(h, s * m * 8);
            gaussian_matrix(h, G.d(), s, m, seed, stream);
            gemm(h, Y, s, n, 1.0, G.d(), m, false, m, A, n, false);
        }
        h->last_sketch_route = route;
    });
}

int xrs_sketch_last_route(xrs_handle_t h) { return h ? h->last_sketch_route : 0; }

}  // extern "C"
