// Batched Cholesky front end of the TT rounds (chol_batch.hpp): dispatch of a job list over the three size
// classes -- n <= 256 (register-resident batched kernels, smallla.hip), 257..512 (2 x 2 blocks of those,
// below) and above (solve.hip chol_full, the one blocked Cholesky) -- with the kernels' argument tables chunked here.
#include <algorithm>

#include "reduce_dev.hpp"
#include "tt_common.hpp"

namespace xrs {

namespace {

using ttd::GemmJob;
using ttd::gemm_grouped;

static_assert(kCholLaunchJobs == kPotrfBatchMax);
constexpr int kBigMax = 64;   // entries of the 2 x 2-block kernels' argument tables
struct BigJob {
    const double* src;
    double shift_rel;
    int n;
    double* L;   // factor jobs: full L and Z = L^{-1} (n x n); certificates: both null
    double* Z;
};

// ---- Cholesky for 256 < n <= 512 from the n <= 256 kernels (2 x 2 blocks, n1 = 256, n2 = n - 256):
//   W = A + shift*I (shift = shift_rel tr A), L11 = chol(W11), Z11 = L11^{-1}, L21 = W21 Z11^T,
//   L22 = chol(W22 - L21 L21^T); factor jobs also get L = [L11 0; L21 L22] and
//   Z = L^{-1} = [Z11 0; -Z22 L21 Z11, Z22]. Every step is one batched launch over all jobs, so the
//   latency is two 256-Cholesky + two 256-inverses instead of one 512-column sequential sweep
//   (k_potrf32_batched + k_trinv_batched<32>: 1.1 ms per cfg5 pass).
struct BigArgs {
    const double* src[kBigMax];
    double* w11[kBigMax];
    double* w21[kBigMax];
    double* w22[kBigMax];
    double shift[kBigMax];
    int n[kBigMax];
};

__global__ void __launch_bounds__(256) k_split_shift(const BigArgs a) {
    const int j = blockIdx.y, n = a.n[j], n1 = 256, n2 = n - 256;
    const double* A = a.src[j];
    __shared__ double red[4];
    block_trace<256>(A, n, red);
    const double shift = a.shift[j] * sum_chain4(red);
    const size_t total = size_t(n) * n;
    for (size_t e = size_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += size_t(gridDim.x) * 256) {
        const int r = int(e / n), c = int(e - size_t(r) * n);
        const double v = A[e] + (r == c ? shift : 0.0);
        if (r < n1 && c < n1) a.w11[j][size_t(r) * n1 + c] = v;
        else if (r >= n1 && c < n1) a.w21[j][size_t(r - n1) * n1 + c] = v;
        else if (r >= n1 && c >= n1) a.w22[j][size_t(r - n1) * n2 + (c - n1)] = v;
    }
}

struct SubArgs {
    double* y[kBigMax];
    const double* x[kBigMax];
    int count[kBigMax];
};

__global__ void __launch_bounds__(256) k_sub_batched(const SubArgs a) {   // y -= x
    const int j = blockIdx.y;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < a.count[j]; e += gridDim.x * 256) a.y[j][e] -= a.x[j][e];
}

struct AssembleArgs {
    double* out[kBigMax];   // n x n
    const double* b11[kBigMax];
    const double* b21[kBigMax];
    const double* b22[kBigMax];
    int n[kBigMax];
};

__global__ void __launch_bounds__(256) k_assemble_lower(const AssembleArgs a) {   // [B11 0; B21 B22]
    const int j = blockIdx.y, n = a.n[j], n1 = 256, n2 = n - 256;
    const size_t total = size_t(n) * n;
    for (size_t e = size_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += size_t(gridDim.x) * 256) {
        const int r = int(e / n), c = int(e - size_t(r) * n);
        double v = 0.0;
        if (r < n1) v = c < n1 ? a.b11[j][size_t(r) * n1 + c] : 0.0;
        else v = c < n1 ? a.b21[j][size_t(r - n1) * n1 + c] : a.b22[j][size_t(r - n1) * n2 + (c - n1)];
        a.out[j][e] = v;
    }
}


// Enqueues every job; statuses (2 per job: the two diagonal factorisations) go to status[0 .. 2*jobs).
void factor_big(xrs_handle_t h, const std::vector<BigJob>& jobs, int* status, std::vector<DevBuf>& keep) {
    const int nj = int(jobs.size());
    XRS_REQUIRE(nj <= kBigMax, "factor_big: too many jobs");
    constexpr int n1 = 256;
    BigArgs ba{};
    std::vector<double*> w11(nj), w21(nj), w22(nj), d11(nj), d22(nj), z11(nj), pp(nj);
    auto buf = [&](size_t elems) { keep.emplace_back(h, std::max<size_t>(elems, 1) * 8); return keep.back().d(); };
    size_t maxn2 = 0;
    for (int j = 0; j < nj; ++j) {
        const int n = jobs[j].n, n2 = n - n1;
        XRS_REQUIRE(n > n1 && n <= 2 * n1, "factor_big: n out of range");
        w11[j] = buf(size_t(n1) * n1);
        w21[j] = buf(size_t(n2) * n1);
        w22[j] = buf(size_t(n2) * n2);
        d11[j] = buf(dinv_elems(n1));
        d22[j] = buf(dinv_elems(n2));
        z11[j] = buf(size_t(n1) * n1);
        pp[j] = buf(size_t(n2) * n2);
        ba.src[j] = jobs[j].src;
        ba.w11[j] = w11[j];
        ba.w21[j] = w21[j];
        ba.w22[j] = w22[j];
        ba.shift[j] = jobs[j].shift_rel;
        ba.n[j] = n;
        maxn2 = std::max(maxn2, size_t(n2));
    }
    hipLaunchKernelGGL(k_split_shift, dim3(256, nj), dim3(256), 0, h->stream, ba);
    check_launch("k_split_shift");
    auto chol = [&](const std::vector<double*>& W, const std::vector<double*>& D, int first_slot, bool upper_half) {
        for (int b0 = 0; b0 < nj; b0 += kPotrfBatchMax) {
            PotrfBatch pb{};
            const int c = std::min(kPotrfBatchMax, nj - b0);
            for (int i = 0; i < c; ++i) {
                pb.src[i] = nullptr;
                pb.G[i] = W[b0 + i];
                pb.Dinv[i] = D[b0 + i];
                pb.shift[i] = 0.0;
                pb.n[i] = upper_half ? n1 : jobs[b0 + i].n - n1;
            }
            pb.status = status + first_slot + b0;
            potrf_batched(h, pb, c);
        }
    };
    auto inverse = [&](const std::vector<double*>& L, const std::vector<double*>& D, const std::vector<double*>& X,
                       bool upper_half, const std::vector<int>& which) {
        TrinvBatch tb{};
        int c = 0;
        for (int j : which) {
            tb.L[c] = L[j];
            tb.Dinv[c] = D[j];
            tb.X[c] = X[j];
            tb.n[c] = upper_half ? n1 : jobs[j].n - n1;
            ++c;
        }
        if (c) trinv_batched(h, tb, c);
    };
    std::vector<int> all(nj), fac;
    for (int j = 0; j < nj; ++j) {
        all[j] = j;
        if (jobs[j].L) fac.push_back(j);
    }
    chol(w11, d11, 0, true);                     // L11 in w11
    inverse(w11, d11, z11, true, all);           // Z11
    std::vector<GemmJob> g1, g2;
    for (int j = 0; j < nj; ++j) {
        const size_t n2 = size_t(jobs[j].n - n1);
        g1.push_back({n2, size_t(n1), size_t(n1), size_t(n1), size_t(n1), false, true, w21[j], z11[j], w21[j] == nullptr ? nullptr : buf(n2 * n1)});
    }
    // L21 = W21 Z11^T into fresh buffers (GEMM outputs must not alias inputs)
    std::vector<double*> l21(nj);
    for (int j = 0; j < nj; ++j) l21[j] = g1[j].C;
    gemm_grouped(h, g1);
    for (int j = 0; j < nj; ++j) {
        const size_t n2 = size_t(jobs[j].n - n1);
        g2.push_back({n2, n2, size_t(n1), size_t(n1), size_t(n1), false, true, l21[j], l21[j], pp[j], true});
    }
    gemm_grouped(h, g2);                         // P = L21 L21^T (symmetric)
    SubArgs sa{};
    for (int j = 0; j < nj; ++j) {
        sa.y[j] = w22[j];
        sa.x[j] = pp[j];
        sa.count[j] = (jobs[j].n - n1) * (jobs[j].n - n1);
    }
    hipLaunchKernelGGL(k_sub_batched, dim3(64, nj), dim3(256), 0, h->stream, sa);
    check_launch("k_sub_batched");
    chol(w22, d22, nj, false);                   // L22 in w22
    if (fac.empty()) return;
    std::vector<double*> z22(nj, nullptr), tt(nj, nullptr), z21(nj, nullptr);
    for (int j : fac) {
        const size_t n2 = size_t(jobs[j].n - n1);
        z22[j] = buf(n2 * n2);
        tt[j] = buf(n2 * n1);
        z21[j] = buf(n2 * n1);
    }
    inverse(w22, d22, z22, false, fac);          // Z22
    std::vector<GemmJob> g3, g4;
    for (int j : fac) {
        const size_t n2 = size_t(jobs[j].n - n1);
        g3.push_back({n2, size_t(n1), size_t(n1), size_t(n1), size_t(n1), false, false, l21[j], z11[j], tt[j]});
    }
    gemm_grouped(h, g3);                         // T = L21 Z11
    for (int j : fac) {
        const size_t n2 = size_t(jobs[j].n - n1);
        GemmJob g{n2, size_t(n1), n2, n2, size_t(n1), false, false, z22[j], tt[j], z21[j]};
        g.alpha = -1.0;
        g4.push_back(g);
    }
    gemm_grouped(h, g4);                         // Z21 = -Z22 T
    AssembleArgs al{}, az{};
    int c = 0;
    for (int j : fac) {
        al.out[c] = jobs[j].L; al.b11[c] = w11[j]; al.b21[c] = l21[j]; al.b22[c] = w22[j]; al.n[c] = jobs[j].n;
        az.out[c] = jobs[j].Z; az.b11[c] = z11[j]; az.b21[c] = z21[j]; az.b22[c] = z22[j]; az.n[c] = jobs[j].n;
        ++c;
    }
    hipLaunchKernelGGL(k_assemble_lower, dim3(256, c), dim3(256), 0, h->stream, al);
    check_launch("k_assemble_lower");
    hipLaunchKernelGGL(k_assemble_lower, dim3(256, c), dim3(256), 0, h->stream, az);
    check_launch("k_assemble_lower");
}

}  // namespace

int chol_status_count(const std::vector<CholJob>& jobs) {
    int c = 0;
    for (const CholJob& j : jobs) c += j.n > 512 ? chol_full_blocks(size_t(j.n)) : (j.n > 256 ? 2 : 1);
    return c;
}

// Status layout: one word per n <= 256 job in job order, then two per 257..512 job, then the blocks of the
// larger ones.
void chol_enqueue_factors(xrs_handle_t h, const std::vector<CholJob>& jobs, int* status, std::vector<DevBuf>& keep,
                          CholInverses& later) {
    std::vector<const CholJob*> small, huge;
    std::vector<BigJob> big;
    size_t dsz = 0;
    for (const CholJob& j : jobs) {
        XRS_REQUIRE(j.A != nullptr && j.n >= 1, "chol_enqueue: empty job");
        if (j.n > 512) {
            huge.push_back(&j);
        } else if (j.n > 256) {
            double* Z = j.Z;   // (the 2 x 2 blocks always build L^{-1} beside L)
            if (j.L && !Z) {
                keep.emplace_back(h, size_t(j.n) * j.n * 8);
                Z = keep.back().d();
            }
            big.push_back({j.A, j.shift, j.n, j.L, Z});
        } else {
            small.push_back(&j);
            dsz += dinv_elems(j.n);
        }
    }
    const int ns = int(small.size());
    int slot = ns + 2 * int(big.size());
    for (const CholJob* j : huge) {
        chol_full(h, j->A, size_t(j->n), j->shift, j->L, j->Z, status + slot);
        slot += chol_full_blocks(size_t(j->n));
    }
    for (size_t b0 = 0; b0 < big.size(); b0 += kBigMax) {
        const std::vector<BigJob> part(big.begin() + long(b0), big.begin() + long(std::min(big.size(), b0 + kBigMax)));
        factor_big(h, part, status + ns + 2 * b0, keep);
    }
    if (ns == 0) return;
    keep.emplace_back(h, dsz * 8);   // the diagonal-block inverses of every n <= 256 job: one slab per call
    double* dinv = keep.back().d();
    std::vector<CholInverses::Item>& inv = later.items;   // the factor jobs that ask for Z
    for (int b0 = 0; b0 < ns; b0 += kPotrfBatchMax) {
        PotrfBatch pb{};
        const int c = std::min(kPotrfBatchMax, ns - b0);
        for (int i = 0; i < c; ++i) {
            const CholJob& j = *small[size_t(b0 + i)];
            pb.src[i] = j.A;
            pb.G[i] = j.L;
            pb.Dinv[i] = dinv;
            pb.shift[i] = j.shift;
            pb.n[i] = j.n;
            if (j.L && j.Z) inv.push_back({j.L, dinv, j.Z, j.n});
            dinv += dinv_elems(j.n);
        }
        pb.status = status + b0;
        potrf_batched(h, pb, c);
    }
}

void chol_enqueue_inverses(xrs_handle_t h, const CholInverses& later) {
    const std::vector<CholInverses::Item>& inv = later.items;
    for (size_t b0 = 0; b0 < inv.size(); b0 += kTrinvBatchMax) {
        TrinvBatch tb{};
        const int c = int(std::min<size_t>(kTrinvBatchMax, inv.size() - b0));
        for (int i = 0; i < c; ++i) {
            const CholInverses::Item& v = inv[b0 + size_t(i)];
            tb.L[i] = v.L;
            tb.Dinv[i] = v.Dinv;
            tb.X[i] = v.X;
            tb.n[i] = v.n;
        }
        trinv_batched(h, tb, c);
    }
}

void chol_enqueue(xrs_handle_t h, const std::vector<CholJob>& jobs, int* status, std::vector<DevBuf>& keep) {
    CholInverses later;
    chol_enqueue_factors(h, jobs, status, keep, later);
    chol_enqueue_inverses(h, later);
}

namespace {

// 1 + first failing column of the whole matrix from the front end's words of every job (the layout above)
void decode_status(const std::vector<CholJob>& jobs, const std::vector<int>& raw, int* status) {
    int ns = 0, nb = 0;
    for (const CholJob& j : jobs) {
        ns += j.n <= 256;
        nb += j.n > 256 && j.n <= 512;
    }
    int is = 0, ib = 0, slot = ns + 2 * nb;
    for (size_t i = 0; i < jobs.size(); ++i) {
        const int n = jobs[i].n;
        if (n <= 256) {
            status[i] = raw[size_t(is++)];
        } else if (n <= 512) {
            const int b0 = ib / kBigMax * kBigMax, part = std::min(kBigMax, nb - b0);   // this job's chunk of factor_big
            const int w1 = raw[size_t(ns + 2 * b0 + (ib - b0))], w2 = raw[size_t(ns + 2 * b0 + part + (ib - b0))];
            status[i] = w1 ? w1 : (w2 ? 256 + w2 : 0);
            ++ib;
        } else {
            status[i] = 0;
            const int blocks = chol_full_blocks(size_t(n));
            for (int b = 0; b < blocks && !status[i]; ++b)
                if (raw[size_t(slot + b)]) status[i] = 256 * b + raw[size_t(slot + b)];
            slot += blocks;
        }
    }
}

}  // namespace

}  // namespace xrs

extern "C" int xrs_chol_batch(xrs_handle_t h, size_t count, const double* const* A, double* const* L, double* const* Z,
                              const int* n, const double* shift, int mode, int* status, int* raw, size_t raw_len) {
    using namespace xrs;
    return guarded([&] {
        XRS_REQUIRE(h && (count == 0 || (A && L && Z && n && shift && status)), "null argument");
        XRS_REQUIRE(mode >= 0 && mode <= 2, "xrs_chol_batch: mode is 0, 1 or 2");
        if (count == 0) return;
        std::vector<CholJob> jobs;
        for (size_t i = 0; i < count; ++i) {
            XRS_REQUIRE(A[i] != nullptr && n[i] >= 1, "xrs_chol_batch: empty job");
            XRS_REQUIRE(L[i] != nullptr || Z[i] == nullptr, "xrs_chol_batch: Z without L");
            XRS_REQUIRE(L[i] != A[i] && (Z[i] == nullptr || (Z[i] != A[i] && Z[i] != L[i])), "xrs_chol_batch: aliased job");
            jobs.push_back(CholJob{A[i], n[i], L[i], Z[i], shift[i]});
        }
        const int words = mode == 2 ? int(count) : chol_status_count(jobs);
        XRS_REQUIRE(raw == nullptr || raw_len == size_t(words), "xrs_chol_batch: raw_len is not the status word count");
        fence_readers(h);
        DevBuf st(h, size_t(words) * sizeof(int));
        // (every word is written by its job: a word a launch missed reads back as -1, not as a success)
        XRS_HIP(hipMemsetAsync(st.p, 0xFF, size_t(words) * sizeof(int), h->stream));
        std::vector<DevBuf> keep;
        if (mode == 0) {
            chol_enqueue(h, jobs, st.as<int>(), keep);
        } else if (mode == 1) {
            CholInverses later;
            chol_enqueue_factors(h, jobs, st.as<int>(), keep, later);
            chol_enqueue_inverses(h, later);
        } else {
            XRS_REQUIRE(count <= size_t(kPotrfBatchMax), "xrs_chol_batch: mode 2 holds at most 48 jobs");
            PotrfBatch pb{};
            TrinvBatch tb{};
            int nz = 0;
            for (size_t i = 0; i < count; ++i) {
                XRS_REQUIRE(n[i] <= kSmallMax, "xrs_chol_batch: mode 2 needs n <= 512");
                keep.emplace_back(h, dinv_elems(n[i]) * 8);
                pb.src[i] = A[i];
                pb.G[i] = L[i];
                pb.Dinv[i] = keep.back().d();
                pb.shift[i] = shift[i];
                pb.n[i] = n[i];
                if (Z[i]) {
                    tb.L[nz] = L[i];
                    tb.Dinv[nz] = keep.back().d();
                    tb.X[nz] = Z[i];
                    tb.n[nz] = n[i];
                    ++nz;
                }
            }
            pb.status = st.as<int>();
            potrf_batched(h, pb, int(count));
            trinv_batched(h, tb, nz);
        }
        std::vector<int> words_host(size_t(words), 0);
        read_status(h, st.as<int>(), words, words_host.data());
        if (mode == 2) std::copy(words_host.begin(), words_host.end(), status);
        else decode_status(jobs, words_host, status);
        if (raw) std::copy(words_host.begin(), words_host.end(), raw);
    });
}
