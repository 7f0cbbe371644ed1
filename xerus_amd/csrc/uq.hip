// UQ-ADF per-sample kernels (reference src/xerus/algorithms/uqAdf.cpp:110-282; declarations in uq.hpp). The
// reference walks the N samples one by one under OpenMP; here one launch covers all samples of a core position.
//   - congruence Lout_j = M_j^T L_j M_j, M_j = sum_t P[j, t] X[:, t, :]: the hot kernel. M_j and T_j = L_j M_j are
//     formed in LDS and never reach HBM, so a sample costs the read of L_j (a^2) and the write of Lout_j (b^2);
//     the component X and the basis row stay cache-resident. Two kernels:
//       k_congruence_mfma: one workgroup (4 waves) per sample, M_j and T_j zero-padded to multiples of 16 in LDS,
//         both products on 16 x 16 v_mfma_f64_16x16x4_f64 tiles (A operand: lane l holds A[row l & 15][k l >> 4],
//         B operand B[k l >> 4][col l & 15], D: col l & 15, row (l >> 4) + 4 reg);
//       k_congruence_fma: 1, 2 or 4 samples per workgroup (256 / samples threads each), FMA; shapes whose M_j
//         does not fit the LDS go through column panels of M_j (the row panel of the second product is formed
//         again per panel pair: more flops, still no HBM intermediate).
//     Both compute the entries on or below the diagonal and write each to (p, q) and (q, p).
//   - symmetric matrix-vector product and quadratic form: one thread per entry (j, c); the sum over samples is
//     a fixed-order LDS tree per block, then one block over the block partials.
// L_j is read as L_j[d][c] for the entry (c, d) (coalesced over c): the stacks are exactly symmetric.
#include "uq.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "reduce_dev.hpp"
#include "scratch_map.hpp"

namespace xrs {
namespace uq {

namespace {

constexpr int kThreads = 256;
constexpr int kModesPerLaunch = 32;
constexpr size_t kFmaLds = 64 * 1024;     // static limit of a launch without an attribute
constexpr size_t kMfmaLds = 160 * 1024;   // LDS of a gfx950 compute unit
constexpr int kPartialBlocks = 1024;

typedef double d4 __attribute__((ext_vector_type(4)));

unsigned grid_of(size_t n) { return unsigned(std::min<size_t>(std::max<size_t>((n + kThreads - 1) / kThreads, 1), 65535)); }

struct BasisArgs {
    unsigned n[kModesPerLaunch];
    size_t off[kModesPerLaunch];
};

__global__ void __launch_bounds__(kThreads) k_basis(size_t N, int modes, const double* __restrict__ xi, size_t ld, BasisArgs args,
                                                    double* __restrict__ Pbase) {
    for (size_t e = size_t(blockIdx.x) * kThreads + threadIdx.x; e < N * size_t(modes); e += size_t(gridDim.x) * kThreads) {
        const size_t j = e / size_t(modes);
        const int m = int(e - j * size_t(modes));
        const unsigned n = args.n[m];
        double* p = Pbase + args.off[m] + j * n;
        const double v = xi[j * ld + m];
        double pm = 1.0, pc = v;
        if (n > 0) p[0] = 1.0;
        if (n > 1) p[1] = v;
        for (unsigned i = 1; i + 1 < n; ++i) {
            const double pn = v * pc - double(i) * pm;
            p[i + 1] = pn;
            pm = pc;
            pc = pn;
        }
    }
}

// entry (c, q) of M_j
__device__ __forceinline__ double m_entry(const double* __restrict__ X, const double* __restrict__ pj, int c, int q, int n, int b) {
    double s = 0.0;
    const double* x = X + size_t(c) * n * b + q;
    for (int t = 0; t < n; ++t) s = fma(pj[t], x[size_t(t) * b], s);
    return s;
}

// ---- FMA kernel. Dynamic LDS per sample slot: Mc (a x W), Tt (W x a, T transposed), Mr (a x W, only with panels).
__global__ void __launch_bounds__(kThreads) k_congruence_fma(size_t N, const double* __restrict__ Lprev, const double* __restrict__ X,
                                                             const double* __restrict__ P, int a, int n, int b, int W, int spb,
                                                             double* __restrict__ Lout) {
    extern __shared__ double lds[];
    const int G = kThreads / spb;                 // threads of a sample slot
    const int slot = int(threadIdx.x) / G, g = int(threadIdx.x) - slot * G;
    const bool panels = W < b;
    const size_t per = size_t(a) * W * (panels ? 3 : 2);
    double* Mc = lds + slot * per;
    double* Tt = Mc + size_t(a) * W;
    double* Mr = panels ? Tt + size_t(a) * W : Mc;
    // every slot runs the same number of rounds (the barriers are workgroup-wide); a slot past N idles
    for (size_t j0 = size_t(blockIdx.x) * spb; j0 < N; j0 += size_t(gridDim.x) * spb) {
        const size_t j = j0 + slot;
        const bool live = j < N;
        const double* pj = P + (live ? j : 0) * n;
        const double* Lj = Lprev ? Lprev + (live ? j : 0) * size_t(a) * a : nullptr;
        double* Oj = Lout + (live ? j : 0) * size_t(b) * b;
        for (int cb = 0; cb < b; cb += W) {
            const int wc = min(W, b - cb);
            __syncthreads();
            if (live)
                for (int e = g; e < a * wc; e += G) {
                    const int c = e / wc, q = e - c * wc;
                    Mc[c * W + q] = m_entry(X, pj, c, cb + q, n, b);
                }
            __syncthreads();
            if (live)
                for (int e = g; e < a * wc; e += G) {   // T[c][q] = sum_d L[d][c] Mc[d][q], c fastest
                    const int q = e / a, c = e - q * a;
                    double s;
                    if (Lj) {
                        s = 0.0;
                        for (int d = 0; d < a; ++d) s = fma(Lj[size_t(d) * a + c], Mc[d * W + q], s);
                    } else {
                        s = Mc[c * W + q];
                    }
                    Tt[q * a + c] = s;
                }
            for (int rb = cb; rb < b; rb += W) {
                const int wr = min(W, b - rb);
                if (panels) {
                    __syncthreads();   // the previous row panel has been consumed
                    if (live)
                        for (int e = g; e < a * wr; e += G) {
                            const int c = e / wr, p = e - c * wr;
                            Mr[c * W + p] = m_entry(X, pj, c, rb + p, n, b);
                        }
                }
                __syncthreads();
                if (live)
                    for (int e = g; e < wr * wc; e += G) {   // out[rb + p][cb + q], p fastest
                        const int q = e / wr, p = e - q * wr;
                        const int gp = rb + p, gq = cb + q;
                        if (gp < gq) continue;
                        double s = 0.0;
                        for (int c = 0; c < a; ++c) s = fma(Mr[c * W + p], Tt[q * a + c], s);
                        Oj[size_t(gp) * b + gq] = s;
                        Oj[size_t(gq) * b + gp] = s;
                    }
            }
        }
    }
}

// ---- MFMA kernel. Dynamic LDS: Ms (ap x bp), Ts (ap x bp; aliases Ms when L is the identity). The fragments
// of L_j come straight from global memory, four K-steps' loads ahead of their MFMAs, the first eight K-steps' even
// ahead of the formation of M_j. The kernel is a chain of round trips per sample (X from L2, L_j from HBM, LDS),
// so what it gains comes from loads that go out together: see the variants measured in DESIGN.md section 3.7.
__global__ void __launch_bounds__(kThreads) k_congruence_mfma(size_t N, const double* __restrict__ Lprev, const double* __restrict__ X,
                                                              const double* __restrict__ P, int a, int n, int b, int ap, int bp,
                                                              double* __restrict__ Lout) {
    extern __shared__ double lds[];
    double* Ms = lds;
    double* Ts = Lprev ? lds + size_t(ap) * bp : lds;
    const int tid = int(threadIdx.x), wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int ta = ap >> 4, tb = bp >> 4;
    for (size_t j = blockIdx.x; j < N; j += gridDim.x) {
        const double* pj = P + j * n;
        const double* Lj = Lprev ? Lprev + j * size_t(a) * a : nullptr;
        double* Oj = Lout + j * size_t(b) * b;
        __syncthreads();   // the previous sample's products have read Ms / Ts
        // the first fragments of L_j this wave needs (its first tile, K-steps 0..7) are requested before M_j is
        // formed: the HBM round trip overlaps the formation instead of following it
        const bool pre_on = Lj && wave < ta * tb;
        double pre[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = 4 * u + lk, row = (wave / tb) * 16 + lr;
            pre[u] = (pre_on && row < a && k < a) ? Lj[size_t(k) * a + row] : 0.0;
        }
        // M_j, four entries per thread at a time, their loads of X unconditional (an entry of the padding reads
        // X[0, t, 0] and stores zero) so that they go out together
        for (int e0 = tid; e0 < ap * bp; e0 += 4 * kThreads) {
            const double* x[4];
            double s[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + u * kThreads;
                const int c = e / bp, q = e - c * bp;
                in[u] = e < ap * bp && c < a && q < b;
                x[u] = in[u] ? X + size_t(c) * n * b + q : X;
                s[u] = 0.0;
            }
#pragma unroll 2
            for (int t = 0; t < n; ++t) {
                const double pt = pj[t];
#pragma unroll
                for (int u = 0; u < 4; ++u) s[u] = fma(pt, x[u][size_t(t) * b], s[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * kThreads < ap * bp) Ms[e0 + u * kThreads] = in[u] ? s[u] : 0.0;
        }
        __syncthreads();
        if (Lj) {   // T = L M: tile (ti, tj), rows of L through its transpose (L[k][row]); ap is a multiple of 16
            for (int tile = wave; tile < ta * tb; tile += kThreads / 64) {
                const int ti = tile / tb, tj = tile - ti * tb;
                const int row = ti * 16 + lr;
                d4 acc = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < ap; k0 += 16) {
                    double av[4], bv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = k0 + 4 * u + lk;
                        bv[u] = Ms[k * bp + tj * 16 + lr];
                    }
                    if (tile == wave && k0 == 0) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) av[u] = pre[u];
                    } else if (tile == wave && k0 == 16) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) av[u] = pre[4 + u];
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int k = k0 + 4 * u + lk;
                            av[u] = (row < a && k < a) ? Lj[size_t(k) * a + row] : 0.0;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) Ts[(ti * 16 + lk + 4 * r) * bp + tj * 16 + lr] = acc[r];
            }
            __syncthreads();
        }
        // out = M^T T: tiles (pi, qi) with pi >= qi
        for (int tile = wave; tile < tb * tb; tile += kThreads / 64) {
            const int pi = tile / tb, qi = tile - pi * tb;
            if (pi < qi) continue;
            d4 acc = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < ap; k0 += 16) {
                double av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 4 * u + lk;
                    av[u] = Ms[k * bp + pi * 16 + lr];
                    bv[u] = Ts[k * bp + qi * 16 + lr];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc, 0, 0, 0);
            }
            const int q = qi * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = pi * 16 + lk + 4 * r;
                if (p < b && q < b && p >= q) {
                    Oj[size_t(p) * b + q] = acc[r];
                    Oj[size_t(q) * b + p] = acc[r];
                }
            }
        }
    }
}

// (L_j v_j)[c]
__device__ __forceinline__ double symv_entry(const double* __restrict__ L, const double* __restrict__ V, size_t j, size_t c, size_t a) {
    const double* v = V + j * a;
    if (!L) return v[c];
    const double* Lj = L + j * a * a;
    double s = 0.0;
    for (size_t d = 0; d < a; ++d) s = fma(Lj[d * a + c], v[d], s);
    return s;
}

__global__ void __launch_bounds__(kThreads) k_symv(size_t N, const double* __restrict__ L, const double* __restrict__ V, size_t a,
                                                   double* __restrict__ Y) {
    for (size_t e = size_t(blockIdx.x) * kThreads + threadIdx.x; e < N * a; e += size_t(gridDim.x) * kThreads) {
        const size_t j = e / a;
        Y[e] = symv_entry(L, V, j, e - j * a, a);
    }
}

__global__ void __launch_bounds__(kThreads) k_quadform_partial(size_t N, const double* __restrict__ L, const double* __restrict__ V, size_t a,
                                                               double* __restrict__ partial) {
    double s = 0.0;
    for (size_t e = size_t(blockIdx.x) * kThreads + threadIdx.x; e < N * a; e += size_t(gridDim.x) * kThreads) {
        const size_t j = e / a;
        s = fma(V[e], symv_entry(L, V, j, e - j * a, a), s);
    }
    s = block_sum_tree<kThreads>(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kThreads) k_sum_partials(int count, const double* __restrict__ partial, double* __restrict__ out) {
    double s = 0.0;
    for (int i = int(threadIdx.x); i < count; i += kThreads) s += partial[i];
    s = block_sum_tree<kThreads>(s);
    if (threadIdx.x == 0) out[0] = s;
}

__global__ void __launch_bounds__(kThreads) k_khatri_rao(size_t N, const double* __restrict__ P, size_t n, const double* __restrict__ R,
                                                         size_t b, double* __restrict__ W) {
    const size_t w = n * b;
    for (size_t e = size_t(blockIdx.x) * kThreads + threadIdx.x; e < N * w; e += size_t(gridDim.x) * kThreads) {
        const size_t j = e / w, tq = e - j * w, t = tq / b, q = tq - t * b;
        W[e] = P[j * n + t] * R[j * b + q];
    }
}

// one workgroup per column
__global__ void __launch_bounds__(kThreads) k_column_mean(size_t N, const double* __restrict__ S, size_t n, double* __restrict__ out) {
    const size_t c = blockIdx.x;
    double s = 0.0;
    for (size_t j = threadIdx.x; j < N; j += kThreads) s += S[j * n + c];
    s = block_sum_tree<kThreads>(s);
    if (threadIdx.x == 0) out[c] = s / double(N);
}

size_t round16(size_t v) { return (v + 15) / 16 * 16; }

bool mfma_fits(bool with_l, size_t a, size_t b) { return a >= 16 && b >= 16 && round16(a) * round16(b) * 8 * (with_l ? 2 : 1) <= kMfmaLds; }

}  // namespace

void basis(xrs_handle_t h, size_t N, size_t modes, const double* xi, size_t ld, const size_t* n, const size_t* off, double* Pbase) {
    if (N == 0) return;
    for (size_t m0 = 0; m0 < modes; m0 += kModesPerLaunch) {
        const int cnt = int(std::min<size_t>(kModesPerLaunch, modes - m0));
        BasisArgs args{};
        for (int m = 0; m < cnt; ++m) {
            XRS_REQUIRE(n[m0 + m] < (size_t(1) << 31), "uq: basis too large");
            args.n[m] = unsigned(n[m0 + m]);
            args.off[m] = off[m0 + m];
        }
        hipLaunchKernelGGL(k_basis, dim3(grid_of(N * size_t(cnt))), dim3(kThreads), 0, h->stream, N, cnt, xi + m0, ld, args, Pbase);
        check_launch("k_basis");
    }
}

void stack_congruence(xrs_handle_t h, size_t N, const double* Lprev, const double* X, const double* P, size_t a, size_t n, size_t b,
                      double* Lout, Path path) {
    XRS_REQUIRE(a >= 1 && b >= 1 && a <= kMaxRank && b <= kMaxRank, "uq: ranks must lie in 1..256");
    XRS_REQUIRE(n >= 1 && n < (size_t(1) << 20), "uq: mode dimension out of range");
    if (N == 0) return;
    const bool fits = mfma_fits(Lprev != nullptr, a, b);
    if (path == Path::Auto) {   // diagnostic A/B: XRS_UQ_CONGRUENCE=fma / mfma forces a kernel where the shape allows it
        const char* env = std::getenv("XRS_UQ_CONGRUENCE");
        if (env && std::strcmp(env, "fma") == 0) path = Path::Fma;
        if (env && std::strcmp(env, "mfma") == 0 && fits) path = Path::Mfma;
    }
    XRS_REQUIRE(path != Path::Mfma || fits, "uq: the MFMA congruence needs both ranks >= 16 and M_j within the LDS");
    if (path == Path::Mfma || (path == Path::Auto && fits)) {
        const size_t ap = round16(a), bp = round16(b);
        const size_t bytes = ap * bp * 8 * (Lprev ? 2 : 1);
        if (bytes > 64 * 1024) {
            XRS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_congruence_mfma), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        int(kMfmaLds)));
        }
        const unsigned grid = unsigned(std::min<size_t>(N, 8192));
        hipLaunchKernelGGL(k_congruence_mfma, dim3(grid), dim3(kThreads), bytes, h->stream, N, Lprev, X, P, int(a), int(n), int(b), int(ap),
                           int(bp), Lout);
        check_launch("k_congruence_mfma");
        return;
    }
    // FMA: whole M_j per sample slot when it fits (4, 2 or 1 slots), else column panels of one sample
    int spb = 0;
    size_t W = b;
    for (int s : {4, 2, 1}) {
        if (size_t(s) * 2 * a * b * 8 <= kFmaLds) {
            spb = s;
            break;
        }
    }
    if (spb == 0) {
        spb = 1;
        W = kFmaLds / (3 * a * 8);   // >= 10 at a = 256
        XRS_REQUIRE(W >= 1, "uq: rank too large");
        W = std::min(W, b);
    }
    const size_t bytes = size_t(spb) * a * W * 8 * (W < b ? 3 : 2);
    const unsigned grid = unsigned(std::min<size_t>((N + spb - 1) / spb, 8192));
    hipLaunchKernelGGL(k_congruence_fma, dim3(grid), dim3(kThreads), bytes, h->stream, N, Lprev, X, P, int(a), int(n), int(b), int(W), spb,
                       Lout);
    check_launch("k_congruence_fma");
}

void stack_symv(xrs_handle_t h, size_t N, const double* L, const double* V, size_t a, double* Y) {
    XRS_REQUIRE(a >= 1 && a <= kMaxRank, "uq: rank must lie in 1..256");
    if (N == 0) return;
    hipLaunchKernelGGL(k_symv, dim3(grid_of(N * a)), dim3(kThreads), 0, h->stream, N, L, V, a, Y);
    check_launch("k_symv");
}

void quadform(xrs_handle_t h, size_t N, const double* L, const double* V, size_t a, double* out_dev) {
    XRS_REQUIRE(a >= 1 && a <= kMaxRank, "uq: rank must lie in 1..256");
    const int nb = int(std::min<size_t>(kPartialBlocks, std::max<size_t>(1, (N * a + kThreads - 1) / kThreads)));
    DevBuf partial(h, size_t(nb) * 8);
    hipLaunchKernelGGL(k_quadform_partial, dim3(nb), dim3(kThreads), 0, h->stream, N, L, V, a, partial.d());
    check_launch("k_quadform_partial");
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kThreads), 0, h->stream, nb, partial.d(), out_dev);
    check_launch("k_sum_partials");
}

double quadform_to_host(xrs_handle_t h, size_t N, const double* L, const double* V, size_t a) {
    double* out = scratch::dev<double>(h, scratch::kDevResult);
    quadform(h, N, L, V, a, out);
    double* host = scratch::host<double>(h, scratch::kHostResult);
    XRS_HIP(hipMemcpyAsync(host, out, 8, hipMemcpyDeviceToHost, h->stream));
    host_wait(h);
    return host[0];
}

void khatri_rao_rows(xrs_handle_t h, size_t N, const double* P, size_t n, const double* R, size_t b, double* W) {
    if (N * n * b == 0) return;
    hipLaunchKernelGGL(k_khatri_rao, dim3(grid_of(N * n * b)), dim3(kThreads), 0, h->stream, N, P, n, R, b, W);
    check_launch("k_khatri_rao");
}

void column_mean(xrs_handle_t h, size_t N, const double* S, size_t n, double* out) {
    XRS_REQUIRE(N >= 1 && n >= 1 && n < (size_t(1) << 31), "uq: empty mean");
    hipLaunchKernelGGL(k_column_mean, dim3(unsigned(n)), dim3(kThreads), 0, h->stream, N, S, n, out);
    check_launch("k_column_mean");
}

}  // namespace uq
}  // namespace xrs

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int xrs_uq_basis(xrs_handle_t h, double* P, const double* xi, size_t N, size_t n) {
    return xrs::guarded([&] {
        XRS_REQUIRE(h, "null handle");
        XRS_REQUIRE(N == 0 || n == 0 || (P && xi), "null P / xi");
        if (n == 0) return;
        xrs::fence_readers(h);
        const size_t off = 0;
        xrs::uq::basis(h, N, 1, xi, 1, &n, &off, P);
    });
}

extern "C" int xrs_uq_stack_congruence(xrs_handle_t h, double* Lout, const double* Lprev, const double* X, const double* P, size_t N,
                                       size_t a, size_t n, size_t b) {
    return xrs::guarded([&] {
        XRS_REQUIRE(h, "null handle");
        XRS_REQUIRE(N == 0 || (Lout && X && P), "null Lout / X / P");
        XRS_REQUIRE(Lout != Lprev || N == 0, "Lout must not alias Lprev");
        xrs::fence_readers(h);
        xrs::uq::stack_congruence(h, N, Lprev, X, P, a, n, b, Lout);
    });
}

extern "C" int xrs_uq_quadform(xrs_handle_t h, double* result, const double* L, const double* V, size_t N, size_t a) {
    return xrs::guarded([&] {
        XRS_REQUIRE(h && result, "null handle / result");
        XRS_REQUIRE(N == 0 || V, "null V");
        *result = xrs::uq::quadform_to_host(h, N, L, V, a);
    });
}
