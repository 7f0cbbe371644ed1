// Tangent vectors of the fixed-rank TT manifold (reference: src/xerus/algorithms/retractions.cpp).
//
//   xrs_tt_tangent_project   the components V_k of the projection of Z onto the tangent space at U
//                            (retractions.cpp:82-130)
//   xrs_tt_tangent_to_tt     the rank-2r block TT of a tangent vector (retractions.cpp:186-260)
//   xrs_tt_tangent_dot       sum_k <UU_k A_k, B_k> (retractions.cpp:167-179)
//
// Projection pipeline (U right-orthogonal with the core at 0, a_k = ru[k], b_k = rz[k]):
//   left chains   UV_{k+1} = sum_i U_k[:,i,:]^T UV_k Z_k[:,i,:]   and   UU_{k+1} (U in both places): two GEMMs per
//                 step each, the two chains on two side streams;
//   right chain   Y_k = Z_k R_{k+1}^T (b_k n_k x a_{k+1}),  R_k = U_k Y_k^T (a_k x b_k): the only other sequential
//                 part, on the main stream beside the left chains;
//   solves        all d-1 systems UU_k W_k = UV_k in ONE batched Cholesky launch behind the UU chain, one
//                 certificate launch (below), one batched triangular inversion; W_k = L^-T (L^-1 UV_k) as
//                 batched GEMMs;
//   per core      V_k = W_k Y_k, then for k >= 1 the gauge step V_k -= (V_k U_k^T) U_k: independent over k,
//                 same-shape products in one batched launch, the subtraction of all cores in one launch.
// Certificate: an edge is certified when its Cholesky factorisation ran through and no squared pivot is
// <= EPSILON * max diag(UU_k) -- the cut of the reference's pseudo-inverse (singular values <= EPSILON sigma_max
// dropped, tensor.cpp:1568-1574) applied to the pivots. The words of all edges are read back once, after
// everything is enqueued; an uncertified edge recomputes W_k = UU_k^+ UV_k through the SVD pseudo-inverse
// (svd_solve) and repeats its per-core products. No component data crosses to the host.
#include <cstdint>
#include <vector>

#include "reduce_dev.hpp"
#include "runtime.hpp"
#include "tt_common.hpp"

namespace xrs {
namespace {

constexpr double kEpsilon = 8.0 * 2.220446049250313e-16;   // xerus::EPSILON (basic.h)
constexpr int kSegMax = 48;                                 // cores / segments per launch (arguments by value)

typedef double d2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// sum over the 256 threads of a workgroup (red: 4 doubles of LDS); every thread returns the sum
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = block_sum_all<Order::pairwise4>(v, red);
    __syncthreads();
    return v;
}

__global__ void k_tangent_one(double* __restrict__ p) {
    if (threadIdx.x == 0 && blockIdx.x == 0) p[0] = 1.0;
}

// ---- certificate of the batched Cholesky: one workgroup per edge
struct CertArgs {
    const double* UU[kSegMax];
    const double* L[kSegMax];
    int n[kSegMax];
    const int* status;   // potrf statuses of these edges
    int* cert;           // 0 certified, 1 not
};

__global__ void __launch_bounds__(256) k_tangent_cert(const CertArgs a, double eps) {
    __shared__ double smx[4], smn[4];
    const int e = blockIdx.x, n = a.n[e];
    const double* __restrict__ G = a.UU[e];
    const double* __restrict__ L = a.L[e];
    double mx = 0.0, mn = 1.0e300;
    bool nan = false;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double g = G[size_t(i) * n + i], l = L[size_t(i) * n + i];
        const double p2 = l * l;
        nan = nan || g != g || p2 != p2;
        mx = g > mx ? g : mx;
        mn = p2 < mn ? p2 : mn;
    }
    if (nan) mn = -1.0;
    mx = wave_max_gt(mx);
    mn = wave_min_lt(mn);
    if ((threadIdx.x & 63) == 0) {
        smx[threadIdx.x >> 6] = mx;
        smn[threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            mx = smx[w] > mx ? smx[w] : mx;
            mn = smn[w] < mn ? smn[w] : mn;
        }
        a.cert[e] = (a.status[e] != 0 || !(mn > eps * mx)) ? 1 : 0;
    }
}

// ---- y_s -= x_s for up to kSegMax segments in one launch (the gauge step of all cores)
struct SubArgs {
    double* y[kSegMax];
    const double* x[kSegMax];
    size_t len[kSegMax];
};

__global__ void __launch_bounds__(256) k_tangent_sub(const SubArgs a) {
    const int s = blockIdx.y;
    double* __restrict__ y = a.y[s];
    const double* __restrict__ x = a.x[s];
    const size_t len = a.len[s];
    const size_t stride = size_t(gridDim.x) * 256, t0 = size_t(blockIdx.x) * 256 + threadIdx.x;
    if (aligned16(y) && aligned16(x)) {
        const size_t n2 = len / 2;
        d2* __restrict__ y2 = reinterpret_cast<d2*>(y);
        const d2* __restrict__ x2 = reinterpret_cast<const d2*>(x);
        for (size_t i = t0; i < n2; i += stride) y2[i] = y2[i] - x2[i];
        if ((len & 1) && t0 == 0) y[len - 1] -= x[len - 1];
    } else {
        for (size_t i = t0; i < len; i += stride) y[i] -= x[i];
    }
}

// ---- the block TT of a tangent vector: every output core in one launch.
// An output core is `rows` rows of `nh` halves of `hl` contiguous doubles each; a half is a copy of a row of
// U or V, the sum of both (first core with add_base), or zero:
//   first    (1, n, 2 rb):      row (i)     = [U(i,:) | V(i,:) (+ U(i,:))]
//   interior (2 ra, n, 2 rb):   row (a', i) = [U(a',i,:) | V(a',i,:)] for a' < ra, [0 | U(a'-ra,i,:)] below
//   last     (2 ra, n, 1):      two rows of ra n doubles: V, then U
//   single   (1, n, 1), d = 1:  V (+ U)
// 16-byte accesses where hl is even (rb even) and the buffers are 16-byte aligned, else 8-byte ones.
enum BlockKind : int { kFirst = 0, kInterior = 1, kLast = 2, kSingle = 3 };
struct BlockArgs {
    const double* U[kSegMax];
    const double* V[kSegMax];
    double* out[kSegMax];
    unsigned ra[kSegMax], n[kSegMax], rb[kSegMax];
    int kind[kSegMax];
    int add_base;
};

template <class T>
__device__ __forceinline__ void block_core(const double* __restrict__ U, const double* __restrict__ V,
                                           double* __restrict__ out, unsigned rows, unsigned nh, unsigned hl, int kind,
                                           unsigned upper_rows, bool add_base) {
    constexpr unsigned W = sizeof(T) / sizeof(double);
    const unsigned upr = hl / W;                 // units per half
    const unsigned total = rows * nh * upr;      // < 2^32 (checked by the launcher)
    const T* __restrict__ Ut = reinterpret_cast<const T*>(U);
    const T* __restrict__ Vt = reinterpret_cast<const T*>(V);
    T* __restrict__ Ot = reinterpret_cast<T*>(out);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const unsigned u = i % upr, rh = i / upr;
        const unsigned q = nh == 2 ? (rh & 1u) : 0u, j = nh == 2 ? (rh >> 1) : rh;
        T v;
        if (kind == kFirst) {
            const size_t s = size_t(j) * upr + u;
            v = q == 0 ? Ut[s] : (add_base ? Ut[s] + Vt[s] : Vt[s]);
        } else if (kind == kInterior) {
            if (j < upper_rows) {
                const size_t s = size_t(j) * upr + u;
                v = q == 0 ? Ut[s] : Vt[s];
            } else {
                v = q == 0 ? T(0.0) : Ut[size_t(j - upper_rows) * upr + u];
            }
        } else if (kind == kLast) {
            v = j == 0 ? Vt[u] : Ut[u];
        } else {
            v = add_base ? Ut[u] + Vt[u] : Vt[u];
        }
        Ot[i] = v;   // (j * nh + q) * upr + u == i
    }
}

__global__ void __launch_bounds__(256) k_tangent_block(const BlockArgs a) {
    const int k = blockIdx.y;
    const double* U = a.U[k];
    const double* V = a.V[k];
    double* out = a.out[k];
    const unsigned ra = a.ra[k], n = a.n[k], rb = a.rb[k];
    const int kind = a.kind[k];
    unsigned rows, nh, hl;
    if (kind == kFirst) { rows = n; nh = 2; hl = rb; }
    else if (kind == kInterior) { rows = 2 * ra * n; nh = 2; hl = rb; }
    else if (kind == kLast) { rows = 2; nh = 1; hl = ra * n; }
    else { rows = 1; nh = 1; hl = n; }
    const bool vec = (hl & 1u) == 0 && aligned16(U) && aligned16(V) && aligned16(out);
    if (vec) block_core<d2>(U, V, out, rows, nh, hl, kind, ra * n, a.add_base != 0);
    else block_core<double>(U, V, out, rows, nh, hl, kind, ra * n, a.add_base != 0);
}

// ---- sum_s <x_s, y_s> over up to kSegMax segments in one launch: every workgroup sums its chunks, stores
// its partial and draws a ticket; the last one adds the partials in workgroup order (deterministic).
constexpr unsigned kDotChunk = 4096;   // doubles per chunk (a multiple of 2: chunk starts keep the alignment)
struct DotArgs {
    const double* x[kSegMax];
    const double* y[kSegMax];
    size_t len[kSegMax];
    unsigned chunk0[kSegMax + 1];   // first chunk of segment s; chunk0[nseg] = all chunks
    int nseg;
    double* partial;                // gridDim.x doubles
    unsigned* ticket;               // zero on entry, zero on exit
    double* out;
};

__global__ void __launch_bounds__(256) k_tangent_dot(const DotArgs a) {
    __shared__ double red[4];
    __shared__ int last;
    const unsigned chunks = a.chunk0[a.nseg];
    double s = 0.0;
    for (unsigned c = blockIdx.x; c < chunks; c += gridDim.x) {
        int seg = 0;
        while (c >= a.chunk0[seg + 1]) ++seg;
        const size_t start = size_t(c - a.chunk0[seg]) * kDotChunk;
        const size_t rest = a.len[seg] - start;
        const unsigned cnt = rest < kDotChunk ? unsigned(rest) : kDotChunk;
        const double* __restrict__ x = a.x[seg] + start;
        const double* __restrict__ y = a.y[seg] + start;
        if (aligned16(x) && aligned16(y)) {
            const d2* __restrict__ x2 = reinterpret_cast<const d2*>(x);
            const d2* __restrict__ y2 = reinterpret_cast<const d2*>(y);
            for (unsigned i = threadIdx.x; i < cnt / 2; i += 256) {
                const d2 p = x2[i], q = y2[i];
                s = fma(p.x, q.x, s);
                s = fma(p.y, q.y, s);
            }
            if ((cnt & 1u) && threadIdx.x == 0) s = fma(x[cnt - 1], y[cnt - 1], s);
        } else {
            for (unsigned i = threadIdx.x; i < cnt; i += 256) s = fma(x[i], y[i], s);
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        // the partial goes out as an agent-scope store ahead of the releasing ticket draw; the last drawer's
        // acquire orders its workgroup's agent-scope loads of every partial behind all the draws
        __hip_atomic_store(&a.partial[blockIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    double v = 0.0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += 256)
        v += __hip_atomic_load(&a.partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = block_sum(v, red);
    if (threadIdx.x == 0) {
        a.out[0] = v;
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------ drivers
void check_shapes(size_t d, const size_t* n, const size_t* r, const char* what) {
    XRS_REQUIRE(d >= 1 && n != nullptr && r != nullptr, std::string(what) + ": empty TT");
    XRS_REQUIRE(r[0] == 1 && r[d] == 1, std::string(what) + ": boundary ranks must be 1");
    for (size_t k = 0; k < d; ++k) {
        XRS_REQUIRE(n[k] >= 1 && r[k] >= 1, std::string(what) + ": zero dimension or rank");
        XRS_REQUIRE(double(r[k]) * double(n[k]) * double(r[k + 1]) < 1.0e9, std::string(what) + ": core too large");
    }
}

void check_ptrs(size_t d, const double* const* P, const char* what) {
    XRS_REQUIRE(P != nullptr, std::string(what) + ": null core table");
    for (size_t k = 0; k < d; ++k) XRS_REQUIRE(P[k] != nullptr, std::string(what) + ": null core");
}

void sub_many(xrs_handle_t h, const std::vector<double*>& y, const std::vector<const double*>& x, const std::vector<size_t>& len) {
    for (size_t s0 = 0; s0 < y.size(); s0 += kSegMax) {
        const size_t cnt = std::min<size_t>(kSegMax, y.size() - s0);
        SubArgs a{};
        size_t mx = 1;
        for (size_t s = 0; s < cnt; ++s) {
            a.y[s] = y[s0 + s];
            a.x[s] = x[s0 + s];
            a.len[s] = len[s0 + s];
            mx = std::max(mx, len[s0 + s]);
        }
        const unsigned bx = unsigned(std::min<size_t>((mx / 2 + 255) / 256 + 1, 1024));
        hipLaunchKernelGGL(k_tangent_sub, dim3(bx, unsigned(cnt)), dim3(256), 0, h->stream, a);
        check_launch("k_tangent_sub");
    }
}

void project(xrs_handle_t h, size_t d, const size_t* n, const size_t* ru, const double* const* U, const size_t* rz,
             const double* const* Z, double** Vout, double** UUout, size_t* fallback_edges) {
    check_shapes(d, n, ru, "tangent_project (base)");
    check_shapes(d, n, rz, "tangent_project (direction)");
    check_ptrs(d, U, "tangent_project (base)");
    check_ptrs(d, Z, "tangent_project (direction)");
    XRS_REQUIRE(Vout != nullptr && UUout != nullptr, "tangent_project: null output table");
    for (size_t k = 0; k < d; ++k) XRS_REQUIRE(ru[k] <= size_t(kSmallMax), "tangent_project: base rank above 512");
    auto csize = [&](size_t k) { return ru[k] * n[k] * ru[k + 1]; };

    // everything shared between the streams is allocated before the fork and released after the join
    std::vector<DevBuf> V(d), UU(d);
    for (size_t k = 0; k < d; ++k) {
        V[k] = DevBuf(h, csize(k) * 8);
        UU[k] = DevBuf(h, ru[k] * ru[k] * 8);
    }
    hipLaunchKernelGGL(k_tangent_one, dim3(1), dim3(64), 0, h->stream, UU[0].d());
    check_launch("k_tangent_one");
    size_t nfallback = 0;
    if (d == 1) {
        XRS_HIP(hipMemcpyAsync(V[0].d(), Z[0], n[0] * 8, hipMemcpyDeviceToDevice, h->stream));
    } else {
        const size_t E = d - 1;   // edges 1 .. d-1
        std::vector<DevBuf> UV(d), Rm(d), Y(d), L(d), Di(d), Zi(d), W1(d), W(d), Gk(d), P(d);
        size_t tuv = 1, tuu = 1;
        for (size_t k = 1; k < d; ++k) {
            const size_t a = ru[k], b = rz[k];
            UV[k] = DevBuf(h, a * b * 8);
            Rm[k] = DevBuf(h, a * b * 8);
            L[k] = DevBuf(h, a * a * 8);
            Di[k] = DevBuf(h, dinv_elems(int(a)) * 8);
            Zi[k] = DevBuf(h, a * a * 8);
            W1[k] = DevBuf(h, a * b * 8);
            W[k] = DevBuf(h, a * b * 8);
            Gk[k] = DevBuf(h, a * a * 8);
            P[k] = DevBuf(h, csize(k) * 8);
            if (k + 1 < d) {
                Y[k] = DevBuf(h, b * n[k] * ru[k + 1] * 8);
                tuv = std::max(tuv, b * n[k] * ru[k + 1]);
                tuu = std::max(tuu, a * n[k] * ru[k + 1]);
            }
        }
        DevBuf Tuv(h, tuv * 8), Tuu(h, tuu * 8), words(h, 2 * E * sizeof(int));
        int* status = words.as<int>();
        int* cert = status + E;
        // Y_k = Z_k R_{k+1}^T: Y_0 is V_0 itself (UU_0 = UV_0 = 1, no gauge step), Y_{d-1} = Z_{d-1} (R_d = 1)
        auto Yk = [&](size_t k) -> const double* { return k == 0 ? V[0].d() : (k + 1 == d ? Z[k] : Y[k].d()); };
        {
            // one step of each chain (UV_{k+1}, UU_{k+1} from core k; Y_k, R_k from core k)
            auto uv_step = [&](size_t k) {
                const size_t a = ru[k], b = rz[k], nk = n[k], a2 = ru[k + 1], b2 = rz[k + 1];
                const double* T = U[0];
                if (k > 0) {
                    gemm(h, Tuv.d(), b, nk * a2, 1.0, UV[k].d(), b, true, a, U[k], nk * a2, false);   // UV_k^T U_k
                    T = Tuv.d();
                }
                gemm(h, UV[k + 1].d(), a2, b2, 1.0, T, a2, true, b * nk, Z[k], b2, false);
            };
            auto uu_step = [&](size_t k) {
                const size_t a = ru[k], nk = n[k], a2 = ru[k + 1];
                const double* T = U[0];
                if (k > 0) {
                    gemm(h, Tuu.d(), a, nk * a2, 1.0, UU[k].d(), a, true, a, U[k], nk * a2, false);
                    T = Tuu.d();
                }
                gemm_sym(h, UU[k + 1].d(), a2, 1.0, T, a2, true, a * nk, U[k], a2, false);
            };
            auto right_step = [&](size_t k) {
                const size_t a = ru[k], b = rz[k], nk = n[k], a2 = ru[k + 1], b2 = rz[k + 1];
                if (k + 1 < d)   // Y_k (b nk x a2) = Z_k (b nk x b2) R_{k+1}^T (R: a2 x b2)
                    gemm(h, k == 0 ? V[0].d() : Y[k].d(), b * nk, a2, 1.0, Z[k], b2, false, b2, Rm[k + 1].d(), b2, true);
                if (k > 0) gemm(h, Rm[k].d(), a, b, 1.0, U[k], nk * a2, false, nk * a2, Yk(k), nk * a2, true);   // U_k Y_k^T
            };
            // the three chains on three streams, their launches interleaved step by step: a chain enqueued
            // whole ahead of the next one would have finished before the next one's first launch arrives
            // (see gram_chains in tt.hip)
            StreamFork fork(h, 2);
            for (size_t s = 0; s + 1 < d; ++s) {
                fork.side(0);
                uv_step(s);
                fork.side(1);
                uu_step(s);
                fork.main();
                right_step(d - 1 - s);
            }
            fork.side(1);   // every factorisation, behind the UU chain
            // (not through chol_enqueue: 257..512 goes to the 32-block kernel here, with k_tangent_cert in between)
            for (size_t e0 = 0; e0 < E; e0 += kSegMax) {
                const int cnt = int(std::min<size_t>(kSegMax, E - e0));
                PotrfBatch pb{};
                TrinvBatch tb{};
                CertArgs ca{};
                for (int i = 0; i < cnt; ++i) {
                    const size_t k = e0 + size_t(i) + 1;
                    pb.src[i] = UU[k].d();
                    pb.G[i] = L[k].d();
                    pb.Dinv[i] = Di[k].d();
                    pb.shift[i] = 0.0;
                    pb.n[i] = int(ru[k]);
                    tb.L[i] = L[k].d();
                    tb.Dinv[i] = Di[k].d();
                    tb.X[i] = Zi[k].d();
                    tb.n[i] = int(ru[k]);
                    ca.UU[i] = UU[k].d();
                    ca.L[i] = L[k].d();
                    ca.n[i] = int(ru[k]);
                }
                pb.status = status + e0;
                ca.status = status + e0;
                ca.cert = cert + e0;
                potrf_batched(h, pb, cnt);
                hipLaunchKernelGGL(k_tangent_cert, dim3(unsigned(cnt)), dim3(256), 0, h->stream, ca, kEpsilon);
                check_launch("k_tangent_cert");
                trinv_batched(h, tb, cnt);
            }
            fork.main();
            right_step(0);
            fork.join();
        }
        // W_k = UU_k^{-1} UV_k = L^-T (L^-1 UV_k)
        std::vector<ttd::GemmJob> jobs;
        for (size_t k = 1; k < d; ++k) {
            const size_t a = ru[k], b = rz[k];
            jobs.push_back(ttd::GemmJob{a, b, a, a, b, false, false, Zi[k].d(), UV[k].d(), W1[k].d()});
        }
        ttd::gemm_grouped(h, jobs);
        jobs.clear();
        for (size_t k = 1; k < d; ++k) {
            const size_t a = ru[k], b = rz[k];
            jobs.push_back(ttd::GemmJob{a, b, a, a, b, true, false, Zi[k].d(), W1[k].d(), W[k].d()});
        }
        ttd::gemm_grouped(h, jobs);
        // V_k = W_k Y_k, V_k -= (V_k U_k^T) U_k for the cores in `ks`
        auto finish = [&](const std::vector<size_t>& ks) {
            std::vector<ttd::GemmJob> j1, j2, j3;
            std::vector<double*> ys;
            std::vector<const double*> xs;
            std::vector<size_t> lens;
            for (size_t k : ks) {
                const size_t a = ru[k], b = rz[k], c = n[k] * ru[k + 1];
                j1.push_back(ttd::GemmJob{a, c, b, b, c, false, false, W[k].d(), Yk(k), V[k].d()});
                j2.push_back(ttd::GemmJob{a, a, c, c, c, false, true, V[k].d(), U[k], Gk[k].d()});
                j3.push_back(ttd::GemmJob{a, c, a, a, c, false, false, Gk[k].d(), U[k], P[k].d()});
                ys.push_back(V[k].d());
                xs.push_back(P[k].d());
                lens.push_back(a * c);
            }
            ttd::gemm_grouped(h, j1);
            ttd::gemm_grouped(h, j2);
            ttd::gemm_grouped(h, j3);
            sub_many(h, ys, xs, lens);
        };
        std::vector<size_t> all;
        for (size_t k = 1; k < d; ++k) all.push_back(k);
        finish(all);
        // the one read-back: the certificate words of every edge
        std::vector<int> hc(E, 0);
        std::vector<size_t> failed;
        for (size_t e0 = 0; e0 < E; e0 += 1024) {   // (read_status stages through the pinned scratch)
            const int cnt = int(std::min<size_t>(1024, E - e0));
            read_status(h, cert + e0, cnt, hc.data() + e0);
        }
        for (size_t e = 0; e < E; ++e)
            if (hc[e] != 0) failed.push_back(e + 1);
        for (size_t k : failed) svd_solve(h, W[k].d(), UU[k].d(), ru[k], ru[k], UV[k].d(), rz[k]);
        if (!failed.empty()) finish(failed);
        nfallback = failed.size();
    }
    for (size_t k = 0; k < d; ++k) {
        Vout[k] = V[k].d();
        V[k].p = nullptr;
        UUout[k] = UU[k].d();
        UU[k].p = nullptr;
    }
    if (fallback_edges) *fallback_edges = nfallback;
}

void to_tt(xrs_handle_t h, size_t d, const size_t* n, const size_t* r, const double* const* U, const double* const* V,
           bool add_base, double** out) {
    check_shapes(d, n, r, "tangent_to_tt");
    check_ptrs(d, U, "tangent_to_tt (base)");
    check_ptrs(d, V, "tangent_to_tt (components)");
    XRS_REQUIRE(out != nullptr, "tangent_to_tt: null output table");
    auto osize = [&](size_t k) { return (k == 0 ? 1 : 2 * r[k]) * n[k] * (k + 1 == d ? 1 : 2 * r[k + 1]); };
    for (size_t k = 0; k < d; ++k) XRS_REQUIRE(osize(k) < (size_t(1) << 31), "tangent_to_tt: core too large");
    std::vector<DevBuf> O(d);
    for (size_t k = 0; k < d; ++k) O[k] = DevBuf(h, osize(k) * 8);
    for (size_t k0 = 0; k0 < d; k0 += kSegMax) {
        const size_t cnt = std::min<size_t>(kSegMax, d - k0);
        BlockArgs a{};
        size_t mx = 1;
        for (size_t s = 0; s < cnt; ++s) {
            const size_t k = k0 + s;
            a.U[s] = U[k];
            a.V[s] = V[k];
            a.out[s] = O[k].d();
            a.ra[s] = unsigned(r[k]);
            a.n[s] = unsigned(n[k]);
            a.rb[s] = unsigned(r[k + 1]);
            a.kind[s] = d == 1 ? kSingle : (k == 0 ? kFirst : (k + 1 == d ? kLast : kInterior));
            mx = std::max(mx, osize(k));
        }
        a.add_base = add_base ? 1 : 0;
        const unsigned bx = unsigned(std::min<size_t>((mx / 2 + 255) / 256 + 1, 2048));
        hipLaunchKernelGGL(k_tangent_block, dim3(bx, unsigned(cnt)), dim3(256), 0, h->stream, a);
        check_launch("k_tangent_block");
    }
    for (size_t k = 0; k < d; ++k) {
        out[k] = O[k].d();
        O[k].p = nullptr;
    }
}

double tangent_dot(xrs_handle_t h, size_t d, const size_t* n, const size_t* r, const double* const* UU,
                   const double* const* A, const double* const* B) {
    check_shapes(d, n, r, "tangent_dot");
    check_ptrs(d, UU, "tangent_dot (Grams)");
    check_ptrs(d, A, "tangent_dot (first vector)");
    check_ptrs(d, B, "tangent_dot (second vector)");
    // the weighted components UU_k A_k (k >= 1; UU_0 = 1), same shapes batched
    std::vector<DevBuf> P(d);
    std::vector<ttd::GemmJob> jobs;
    for (size_t k = 1; k < d; ++k) {
        const size_t a = r[k], c = n[k] * r[k + 1];
        P[k] = DevBuf(h, a * c * 8);
        jobs.push_back(ttd::GemmJob{a, c, a, a, c, false, false, UU[k], A[k], P[k].d()});
    }
    ttd::gemm_grouped(h, jobs);
    const size_t launches = (d + kSegMax - 1) / kSegMax;
    XRS_REQUIRE(launches <= 64, "tangent_dot: order too large");
    constexpr unsigned kBlocksMax = 1024;
    DevBuf partial(h, kBlocksMax * 8), res(h, launches * 8), ticket(h, 16);
    XRS_HIP(hipMemsetAsync(ticket.p, 0, 16, h->stream));
    for (size_t l = 0; l < launches; ++l) {
        const size_t k0 = l * kSegMax, cnt = std::min<size_t>(kSegMax, d - k0);
        DotArgs a{};
        unsigned chunks = 0;
        for (size_t s = 0; s < cnt; ++s) {
            const size_t k = k0 + s;
            a.x[s] = k == 0 ? A[0] : P[k].d();
            a.y[s] = B[k];
            a.len[s] = r[k] * n[k] * r[k + 1];
            a.chunk0[s] = chunks;
            chunks += unsigned((a.len[s] + kDotChunk - 1) / kDotChunk);
        }
        a.chunk0[cnt] = chunks;
        a.nseg = int(cnt);
        a.partial = partial.d();
        a.ticket = ticket.as<unsigned>();
        a.out = res.d() + l;
        hipLaunchKernelGGL(k_tangent_dot, dim3(std::min(chunks, kBlocksMax)), dim3(256), 0, h->stream, a);
        check_launch("k_tangent_dot");
    }
    double* hs = scratch::host<double>(h, scratch::kHostLocal, launches);
    XRS_HIP(hipMemcpyAsync(hs, res.d(), launches * 8, hipMemcpyDeviceToHost, h->stream));
    host_wait(h);
    double sum = 0.0;
    for (size_t l = 0; l < launches; ++l) sum += hs[l];
    return sum;
}

}  // namespace

namespace tt {
void tangent_project(xrs_handle_t h, size_t d, const size_t* n, const size_t* ru, const double* const* U, const size_t* rz,
                     const double* const* Z, double** V, double** UU, size_t* fallback_edges) {
    project(h, d, n, ru, U, rz, Z, V, UU, fallback_edges);
}
void tangent_to_tt(xrs_handle_t h, size_t d, const size_t* n, const size_t* r, const double* const* U, const double* const* V,
                   bool add_base, double** out) {
    to_tt(h, d, n, r, U, V, add_base, out);
}
double tangent_dot(xrs_handle_t h, size_t d, const size_t* n, const size_t* r, const double* const* UU, const double* const* A,
                   const double* const* B) {
    return xrs::tangent_dot(h, d, n, r, UU, A, B);
}
}  // namespace tt
}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_tt_tangent_project(xrs_handle_t h, size_t d, const size_t* n, const size_t* ru, const double* const* U,
                           const size_t* rz, const double* const* Z, double** V, double** UU, size_t* fallback_edges) {
    return guarded([&] {
        XRS_REQUIRE(h != nullptr, "null handle");
        project(h, d, n, ru, U, rz, Z, V, UU, fallback_edges);
    });
}

int xrs_tt_tangent_to_tt(xrs_handle_t h, size_t d, const size_t* n, const size_t* r, const double* const* U,
                         const double* const* V, int add_base, double** out) {
    return guarded([&] {
        XRS_REQUIRE(h != nullptr, "null handle");
        to_tt(h, d, n, r, U, V, add_base != 0, out);
    });
}

int xrs_tt_tangent_dot(xrs_handle_t h, double* result, size_t d, const size_t* n, const size_t* r,
                       const double* const* UU, const double* const* A, const double* const* B) {
    return guarded([&] {
        XRS_REQUIRE(h != nullptr && result != nullptr, "null handle or result");
        *result = tangent_dot(h, d, n, r, UU, A, B);
    });
}

}  // extern "C"
