// The entrywise square X o X of a TT in the symmetric basis, and the argmax of a rank-one TT: the two kernels
// of find_largest_entry (reference: src/xerus/algorithms/largestEntry.cpp:6-54; host/largest_entry.cpp).
//
//   xrs_tt_entrywise_square   Z_k[i] = X_k[i] (x) X_k[i] commutes with the swap of the two factors and the
//                             boundary ranks are 1, so the chain lives in Sym^2(R^r) on every edge. In the
//                             orthonormal basis u_aa = e_a (x) e_a, u_ab = (e_a (x) e_b + e_b (x) e_a) / sqrt 2
//                             (a < b) the cores C_k[i] = S_k^T Z_k[i] S_{k+1} represent X o X exactly with edge
//                             rank s(r) = r (r + 1) / 2 instead of r^2. Pair index
//                             p(a, b) = a r - a (a - 1) / 2 + (b - a), 0 <= a <= b < r.
//   xrs_tt_rank_one_argmax    per core of a rank-one TT the first index of largest modulus.
//
// Both are one launch for all cores (descriptor table by value, as k_tangent_block): the cores of the
// algorithm are small and d is 10-60, so a launch per core would be launch-bound. The square writes every
// output element once (8 B per element, the HBM bound); the input cores are s(r)/r^2 ~ half as large per
// side and stay cache-resident.
#include <cstdint>
#include <vector>

#include "reduce_dev.hpp"
#include "runtime.hpp"
#include "scratch_map.hpp"

namespace xrs {
namespace {

constexpr int kSegMax = 64;   // cores per launch (arguments by value: 40 B per core)
constexpr double kSqrt2 = 1.4142135623730951;

// first pair index of row a: off(a) = a r - a (a - 1) / 2 = a (2 r - a + 1) / 2
__host__ __device__ __forceinline__ uint64_t pair_row_start(uint32_t a, uint32_t r) {
    return (uint64_t(a) * (2ull * r + 1 - a)) >> 1;
}

// p -> (a, b) with p = p(a, b): a is the largest row with off(a) <= p, the root of a^2 - (2 r + 1) a + 2 p = 0.
// The single-precision root is an estimate only; the integer loops make it exact (r < 65536: s(r) < 2^31).
__host__ __device__ __forceinline__ void pair_decode(uint32_t p, uint32_t r, uint32_t& a, uint32_t& b) {
    const uint64_t t = 2ull * r + 1;
    const uint64_t disc = t * t - 8ull * p;   // >= 9 for p < s(r)
    const float root = sqrtf(float(disc));
    float est = (float(t) - root) * 0.5f;
    est = est < 0.0f ? 0.0f : est;
    uint32_t q = uint32_t(est);
    q = q < r ? q : r - 1;
    while (q + 1 < r && pair_row_start(q + 1, r) <= p) ++q;
    while (q > 0 && pair_row_start(q, r) > p) --q;
    a = q;
    b = q + uint32_t(p - pair_row_start(q, r));
}

struct SquareArgs {
    const double* A[kSegMax];
    double* C[kSegMax];
    uint32_t ra[kSegMax], ext[kSegMax], rb[kSegMax];   // input ranks (left, right) and external size of the core
    uint32_t sa[kSegMax], sb[kSegMax];                 // s(ra), s(rb)
    uint32_t block0[kSegMax + 1];                      // first workgroup of each core
    int nseg;
    double alpha;                                      // multiplied into segment 0
};

// one thread per output element C[p(a,b), i, p(a',b')], the right pair index fastest (coalesced stores);
// a workgroup belongs to one core
__global__ void __launch_bounds__(256) k_entrywise_square(const SquareArgs g) {
    int s = 0;
    while (s + 1 < g.nseg && blockIdx.x >= g.block0[s + 1]) ++s;
    const uint32_t ext = g.ext[s], rb = g.rb[s], sb = g.sb[s], ra = g.ra[s];
    const uint64_t total = uint64_t(g.sa[s]) * ext * sb;
    const uint64_t idx = uint64_t(blockIdx.x - g.block0[s]) * 256 + threadIdx.x;
    if (idx >= total) return;
    const uint32_t q = uint32_t(idx % sb);
    const uint64_t t = idx / sb;
    const uint32_t i = uint32_t(t % ext), p = uint32_t(t / ext);
    uint32_t a, b, a2, b2;
    pair_decode(p, ra, a, b);
    pair_decode(q, rb, a2, b2);
    const double* __restrict__ A = g.A[s];
    const double* rowa = A + (size_t(a) * ext + i) * rb;
    const double* rowb = A + (size_t(b) * ext + i) * rb;
    const double x = rowa[a2];
    double v;
    if (a == b) {
        v = (a2 == b2) ? x * x : kSqrt2 * (x * rowa[b2]);
    } else if (a2 == b2) {
        v = kSqrt2 * (x * rowb[a2]);
    } else {
        v = fma(x, rowb[b2], rowa[b2] * rowb[a2]);
    }
    if (s == 0) v *= g.alpha;
    g.C[s][idx] = v;
}

struct ArgmaxArgs {
    const double* x[kSegMax];
    uint32_t len[kSegMax];
    unsigned long long* pos;   // one index per core of this launch
};

// one workgroup per core: the first index of largest |x|; NaN never wins (an all-NaN core gives 0)
__global__ void __launch_bounds__(256) k_rank_one_argmax(const ArgmaxArgs g) {
    __shared__ double sv[4];
    __shared__ uint32_t si[4];
    const int s = blockIdx.x;
    const double* __restrict__ x = g.x[s];
    const uint32_t len = g.len[s];
    constexpr uint32_t kNone = 0xffffffffu;
    double best = -1.0;
    uint32_t at = kNone;
    for (uint32_t i = threadIdx.x; i < len; i += 256) {   // ascending i: the strict > keeps the first
        const double v = fabs(x[i]);
        if (v > best) {
            best = v;
            at = i;
        }
    }
    wave_arg_best(best, at, [](double a, double b) { return a > b; });
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = best;
        si[threadIdx.x >> 6] = at;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < at)) {
                best = sv[w];
                at = si[w];
            }
        g.pos[s] = at == kNone ? 0ull : (unsigned long long)at;
    }
}

size_t sym_rank(size_t r) { return r * (r + 1) / 2; }

}  // namespace
}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_tt_entrywise_square(xrs_handle_t h, size_t d, const size_t* ext, const size_t* r, const double* const* A, double alpha,
                            double** out, size_t* r_out) {
    return guarded([&] {
        XRS_REQUIRE(h && ext && r && A && out && r_out, "null argument");
        XRS_REQUIRE(d >= 1, "TT must have at least one component");
        XRS_REQUIRE(r[0] == 1 && r[d] == 1, "boundary ranks must be 1");
        for (size_t k = 0; k < d; ++k) {
            XRS_REQUIRE(ext[k] > 0 && r[k + 1] > 0, "dimensions and ranks must be positive");
            XRS_REQUIRE(A[k], "null core");
            XRS_REQUIRE(r[k] < 65536 && r[k + 1] < 65536 && ext[k] < (1u << 31), "square rank or mode too large");
        }
        std::vector<size_t> total(d);
        for (size_t k = 0; k < d; ++k) {
            const unsigned __int128 t = (unsigned __int128)(sym_rank(r[k]) * ext[k]) * sym_rank(r[k + 1]);   // (< 2^62) x (< 2^31)
            XRS_REQUIRE(t < ((unsigned __int128)1 << 39), "square core too large");
            total[k] = size_t(t);
        }
        std::vector<double*> made(d, nullptr);
        try {
            for (size_t k = 0; k < d; ++k) made[k] = static_cast<double*>(h->pool->alloc(total[k] * 8));
            for (size_t k0 = 0; k0 < d; k0 += kSegMax) {
                const size_t cnt = std::min<size_t>(kSegMax, d - k0);
                SquareArgs g{};
                size_t blocks = 0, elems = 0;
                for (size_t s = 0; s < cnt; ++s) {
                    const size_t k = k0 + s;
                    g.A[s] = A[k];
                    g.C[s] = made[k];
                    g.ra[s] = uint32_t(r[k]);
                    g.rb[s] = uint32_t(r[k + 1]);
                    g.ext[s] = uint32_t(ext[k]);
                    g.sa[s] = uint32_t(sym_rank(r[k]));
                    g.sb[s] = uint32_t(sym_rank(r[k + 1]));
                    g.block0[s] = uint32_t(blocks);
                    blocks += (total[k] + 255) / 256;
                    elems += total[k];
                    XRS_REQUIRE(blocks < (size_t(1) << 31), "too many output elements for one launch");
                }
                g.block0[cnt] = uint32_t(blocks);
                g.nseg = int(cnt);
                g.alpha = k0 == 0 ? alpha : 1.0;
                KernelTimer timer(h, XRS_KFAM_ELEMWISE, 3.0 * double(elems), 8.0 * double(elems));
                hipLaunchKernelGGL(k_entrywise_square, dim3(unsigned(blocks)), dim3(256), 0, h->stream, g);
                check_launch("k_entrywise_square");
            }
        } catch (...) {
            for (double* q : made)
                if (q) h->pool->release(q);
            throw;
        }
        for (size_t k = 0; k < d; ++k) out[k] = made[k];
        for (size_t k = 0; k <= d; ++k) r_out[k] = sym_rank(r[k]);
    });
}

int xrs_tt_rank_one_argmax(xrs_handle_t h, size_t d, const size_t* ext, const double* const* cores, size_t* pos) {
    return guarded([&] {
        XRS_REQUIRE(h && ext && cores && pos, "null argument");
        XRS_REQUIRE(d >= 1, "TT must have at least one component");
        for (size_t k = 0; k < d; ++k) {
            XRS_REQUIRE(ext[k] > 0 && ext[k] < (1u << 31), "dimensions must be positive and below 2^31");
            XRS_REQUIRE(cores[k], "null core");
        }
        static_assert(sizeof(unsigned long long) == sizeof(size_t), "positions travel as 64-bit words");
        unsigned long long* hp = scratch::host<unsigned long long>(h, scratch::kHostLocal, d);
        DevBuf res(h, d * 8);
        for (size_t k0 = 0; k0 < d; k0 += kSegMax) {
            const size_t cnt = std::min<size_t>(kSegMax, d - k0);
            ArgmaxArgs g{};
            for (size_t s = 0; s < cnt; ++s) {
                g.x[s] = cores[k0 + s];
                g.len[s] = uint32_t(ext[k0 + s]);
            }
            g.pos = res.as<unsigned long long>() + k0;
            hipLaunchKernelGGL(k_rank_one_argmax, dim3(unsigned(cnt)), dim3(256), 0, h->stream, g);
            check_launch("k_rank_one_argmax");
        }
        XRS_HIP(hipMemcpyAsync(hp, res.p, d * 8, hipMemcpyDeviceToHost, h->stream));
        host_wait(h);
        for (size_t k = 0; k < d; ++k) pos[k] = size_t(hp[k]);
    });
}

}  // extern "C"
