// Randomize-then-orthogonalize rounding of a TT sum (Al Daas, Ballard, Cazeaux, Hallman, Miedlar, Pasha, Reid, Saibaba:
// "Randomized algorithms for rounding in the tensor-train format", SISC 2023, Alg. 3.2 applied to a formal sum as in
// §3.3); include/xerus/algorithms/randomizedRounding.h states the recursion, DESIGN §3.12 the costs.
//
//   random TT   Omega_k (l_k, n_k, l_{k+1}), k = 1 .. d-1: as a row-major l_k x (n_k l_{k+1}) matrix the leading block of
//               G(seed, stream = k) (philox.hpp), materialised by xrs_gaussian_matrix.
//   pass 1      right to left, each term on its own: W_d = 1, T = Y_k x_3 W_{k+1}, W_k = T_(R_k x n l) H(Omega_k)^T.
//               Two plain GEMMs per term and core; terms of equal shape share a batched launch.
//   pass 2      left to right: X_0 = c_j Y_0; Z = sum_j V(X_k) W_{k+1} (xrs_gemm_ksum), Q = qr(Z) is output core k,
//               M = Q^T V(X_k), X_{k+1} = M x_1 Y_{k+1}; the last core is sum_j M Y_{d-1} (xrs_gemm_ksum again).
// The block-diagonal cores of the sum are never formed and nothing is factorised at rank sum R: the only
// factorisations are QRs of (l_k n_k) x l_{k+1} matrices. A term enters through term_sketch_jobs / term_project_jobs /
// term_advance_jobs below (its cores times small matrices), the places a second kind of term would replace.
#include <algorithm>
#include <limits>
#include <vector>

#include "elementwise.hpp"
#include "gemm_ksum.hpp"
#include "runtime.hpp"
#include "smallla.hpp"

namespace xrs {
namespace {

struct Term {
    const size_t* r;           // d + 1 ranks
    const double* const* Y;    // d cores
    double c;
};

bool same_shape(const GemmSpec& a, const GemmSpec& b) {
    return a.M == b.M && a.N == b.N && a.K == b.K && a.lda == b.lda && a.ldb == b.ldb && a.ta == b.ta && a.tb == b.tb;
}

// the jobs of one step over all terms: those of equal shape in one batched launch, the others one by one
void run_jobs(xrs_handle_t h, const std::vector<GemmSpec>& jobs) {
    std::vector<char> done(jobs.size(), 0);
    for (size_t i = 0; i < jobs.size(); ++i) {
        if (done[i]) continue;
        std::vector<const double*> A, B;
        std::vector<double*> C;
        for (size_t j = i; j < jobs.size(); ++j)
            if (!done[j] && same_shape(jobs[i], jobs[j])) {
                done[j] = 1;
                A.push_back(jobs[j].A);
                B.push_back(jobs[j].B);
                C.push_back(jobs[j].C);
            }
        const GemmSpec& g = jobs[i];
        if (C.size() == 1) gemm(h, g);
        else gemm_batched(h, int(C.size()), C.data(), g.M, g.N, 1.0, A.data(), g.lda, g.ta, g.K, B.data(), g.ldb, g.tb);
    }
}

// ---- the per-term steps (everything that reads a term's cores) -------------------------------------------------
// pass 1 at core k: T (R_k n_k x l_{k+1}) = Y_k W_{k+1}, then W_k (R_k x l_k) = T_(R_k x n_k l_{k+1}) Omega_k^T.
// At k = d - 1, W_d = 1 and T is the core itself.
void term_sketch_jobs(const Term& t, size_t k, size_t d, size_t nk, size_t l_k, size_t l_k1, const double* Wnext, double* T,
                      const double* Omega, double* W, std::vector<GemmSpec>& first, std::vector<GemmSpec>& second) {
    const size_t R = t.r[k], R1 = t.r[k + 1];
    const double* Tsrc = t.Y[k];
    if (k + 1 < d) {
        first.push_back(GemmSpec{t.Y[k], Wnext, T, R * nk, l_k1, R1, R1, l_k1, false, false});
        Tsrc = T;
    }
    second.push_back(GemmSpec{Tsrc, Omega, W, R, l_k, nk * l_k1, nk * l_k1, nk * l_k1, false, true});
}
// pass 2 at core k: M (l_{k+1} x R_{k+1}) = Q^T V(X_k)
GemmSpec term_project_job(const Term& t, size_t k, size_t rows, size_t l_k1, const double* Q, const double* X, double* M) {
    return GemmSpec{Q, X, M, l_k1, t.r[k + 1], rows, l_k1, t.r[k + 1], true, false};
}
// pass 2: X_{k+1} (l_{k+1} x n_{k+1} R_{k+2}) = M Y_{k+1}
GemmSpec term_advance_job(const Term& t, size_t k1, size_t nk1, size_t l_k1, const double* M, double* X) {
    return GemmSpec{M, t.Y[k1], X, l_k1, nk1 * t.r[k1 + 1], t.r[k1], t.r[k1], nk1 * t.r[k1 + 1], false, false};
}

size_t sat_mul(size_t a, size_t b) {
    constexpr size_t cap = std::numeric_limits<size_t>::max() / 2;
    return (a != 0 && b > cap / a) ? cap : a * b;
}

// l[0 .. d]: the capped sketch ranks (header of xrs_tt_round_randomized), l[0] = l[d] = 1
std::vector<size_t> capped_ranks(size_t d, const size_t* n, const std::vector<Term>& terms, const size_t* ell) {
    std::vector<size_t> l(d + 1, 1), right(d + 1, 1);
    for (size_t k = d; k-- > 0;) right[k] = sat_mul(right[k + 1], n[k]);
    size_t left = 1;
    for (size_t k = 1; k < d; ++k) {
        left = sat_mul(left, n[k - 1]);
        size_t sum = 0;
        for (const Term& t : terms) sum += t.r[k];   // (ranks below 2^16, terms below 2^31)
        l[k] = std::min({ell[k - 1], left, right[k], sum, sat_mul(l[k - 1], n[k - 1])});
    }
    return l;
}

void round_randomized(xrs_handle_t h, size_t d, const size_t* n, const std::vector<Term>& terms, const std::vector<size_t>& l,
                      uint64_t seed, std::vector<double*>& out) {
    const size_t s = terms.size();
    std::vector<const double*> A(s), B(s);
    std::vector<size_t> lda(s), K(s), ldb(s);

    if (d == 1) {   // sum_j c_j Y_0 as (n_0 x 1) (1 x 1) products
        std::vector<double> c(s);
        for (size_t j = 0; j < s; ++j) c[j] = terms[j].c;
        DevBuf rr_coef(h, s * 8);
        XRS_HIP(hipMemcpyAsync(rr_coef.p, c.data(), s * 8, hipMemcpyHostToDevice, h->stream));
        for (size_t j = 0; j < s; ++j) {
            A[j] = terms[j].Y[0];
            B[j] = rr_coef.d() + j;
            lda[j] = K[j] = ldb[j] = 1;
        }
        gemm_ksum(h, out[0], n[0], 1, 1.0, s, A.data(), lda.data(), K.data(), B.data(), ldb.data());
        host_wait(h);   // c leaves scope
        return;
    }

    // ---- pass 1: W[j][k], k = 1 .. d-1
    std::vector<std::vector<DevBuf>> rr_W(s);
    for (size_t j = 0; j < s; ++j) {
        rr_W[j].resize(d);
        for (size_t k = 1; k < d; ++k) rr_W[j][k] = DevBuf(h, terms[j].r[k] * l[k] * 8);
    }
    for (size_t k = d - 1; k >= 1; --k) {
        const size_t cols = n[k] * l[k + 1];
        DevBuf rr_omega(h, l[k] * cols * 8);
        {
            const int st = xrs_gaussian_matrix(h, rr_omega.d(), l[k], cols, seed, uint32_t(k));
            if (st != XRS_OK) throw Error{st, xrs_last_error()};
        }
        std::vector<DevBuf> rr_T(s);
        std::vector<GemmSpec> first, second;
        for (size_t j = 0; j < s; ++j) {
            if (k + 1 < d) rr_T[j] = DevBuf(h, terms[j].r[k] * cols * 8);
            term_sketch_jobs(terms[j], k, d, n[k], l[k], l[k + 1], k + 1 < d ? rr_W[j][k + 1].d() : nullptr, rr_T[j].d(),
                             rr_omega.d(), rr_W[j][k].d(), first, second);
        }
        run_jobs(h, first);
        run_jobs(h, second);
    }

    // ---- pass 2
    std::vector<DevBuf> rr_X(s), rr_M(s);
    for (size_t j = 0; j < s; ++j) {
        const size_t len = n[0] * terms[j].r[1];
        rr_X[j] = DevBuf(h, len * 8);
        XRS_HIP(hipMemcpyAsync(rr_X[j].p, terms[j].Y[0], len * 8, hipMemcpyDeviceToDevice, h->stream));
        if (terms[j].c != 1.0) scal(h, rr_X[j].d(), terms[j].c, len);
    }
    for (size_t k = 0; k + 1 < d; ++k) {
        const size_t rows = l[k] * n[k];
        // Z = sum_j V(X_k) W_{k+1}
        DevBuf rr_Z(h, rows * l[k + 1] * 8), rr_R(h, l[k + 1] * l[k + 1] * 8);
        for (size_t j = 0; j < s; ++j) {
            A[j] = rr_X[j].d();
            B[j] = rr_W[j][k + 1].d();
            lda[j] = K[j] = terms[j].r[k + 1];
            ldb[j] = l[k + 1];
        }
        gemm_ksum(h, rr_Z.d(), rows, l[k + 1], 1.0, s, A.data(), lda.data(), K.data(), B.data(), ldb.data());
        qr(h, rr_Z.d(), rows, l[k + 1], out[k], rr_R.d());   // rows >= l[k + 1] by the caps: Q is rows x l[k + 1]
        std::vector<GemmSpec> jobs;
        for (size_t j = 0; j < s; ++j) {
            rr_M[j] = DevBuf(h, l[k + 1] * terms[j].r[k + 1] * 8);
            jobs.push_back(term_project_job(terms[j], k, rows, l[k + 1], out[k], rr_X[j].d(), rr_M[j].d()));
        }
        run_jobs(h, jobs);
        if (k + 2 < d) {
            jobs.clear();
            std::vector<DevBuf> next(s);
            for (size_t j = 0; j < s; ++j) {
                next[j] = DevBuf(h, l[k + 1] * n[k + 1] * terms[j].r[k + 2] * 8);
                jobs.push_back(term_advance_job(terms[j], k + 1, n[k + 1], l[k + 1], rr_M[j].d(), next[j].d()));
            }
            run_jobs(h, jobs);
            for (size_t j = 0; j < s; ++j) rr_X[j] = std::move(next[j]);
        } else {   // the last core: sum_j M Y_{d-1}
            for (size_t j = 0; j < s; ++j) {
                A[j] = rr_M[j].d();
                B[j] = terms[j].Y[d - 1];
                lda[j] = K[j] = terms[j].r[d - 1];
                ldb[j] = n[d - 1];
            }
            gemm_ksum(h, out[d - 1], l[d - 1], n[d - 1], 1.0, s, A.data(), lda.data(), K.data(), B.data(), ldb.data());
        }
    }
}

}  // namespace
}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_tt_round_randomized(xrs_handle_t h, size_t d, const size_t* n, size_t count, const size_t* const* r,
                            const double* const* const* cores, const double* coef, const size_t* ell, uint64_t seed,
                            double** out, size_t* r_out) {
    return guarded([&] {
        XRS_REQUIRE(h && n && r && cores && coef && out && r_out, "null argument");
        XRS_REQUIRE(d >= 1, "TT must have at least one component");
        XRS_REQUIRE(d < (size_t(1) << 32), "the streams of the random TT are 32-bit words");
        XRS_REQUIRE(count >= 1, "at least one term is needed");
        XRS_REQUIRE(d == 1 || ell, "null sketch ranks");
        for (size_t k = 0; k < d; ++k) XRS_REQUIRE(n[k] > 0 && n[k] < (size_t(1) << 31), "dimensions must be positive and below 2^31");
        for (size_t k = 0; k + 1 < d; ++k) XRS_REQUIRE(ell[k] >= 1, "sketch ranks must be at least 1");
        std::vector<Term> terms(count);
        for (size_t j = 0; j < count; ++j) {
            XRS_REQUIRE(r[j] && cores[j], "null term");
            XRS_REQUIRE(r[j][0] == 1 && r[j][d] == 1, "boundary ranks must be 1");
            for (size_t k = 0; k < d; ++k) {
                XRS_REQUIRE(r[j][k + 1] > 0 && r[j][k + 1] < 65536, "ranks must be positive and below 65536");
                XRS_REQUIRE(cores[j][k], "null core");
            }
            terms[j] = Term{r[j], cores[j], coef[j]};
        }
        const std::vector<size_t> l = capped_ranks(d, n, terms, ell);
        for (size_t k = 0; k < d; ++k) {
            XRS_REQUIRE(l[k] < 65536 && l[k + 1] < 65536, "sketch rank too large");
            XRS_REQUIRE(l[k] * n[k] <= (size_t(1) << 39) / l[k + 1], "sketch core too large");
        }
        fence_readers(h);
        std::vector<double*> made(d, nullptr);
        try {
            for (size_t k = 0; k < d; ++k) made[k] = static_cast<double*>(h->pool->alloc(l[k] * n[k] * l[k + 1] * 8));
            round_randomized(h, d, n, terms, l, seed, made);
        } catch (...) {
            for (double* q : made)
                if (q) h->pool->release(q);
            throw;
        }
        for (size_t k = 0; k < d; ++k) out[k] = made[k];
        for (size_t k = 0; k <= d; ++k) r_out[k] = l[k];
    });
}

}  // extern "C"
