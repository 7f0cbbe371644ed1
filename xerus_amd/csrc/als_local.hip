// Matrix-free local problem of one-site ALS (reference src/xerus/algorithms/als.cpp:383-400 assembles the local
// operator as a dense (rl n rr)^2 tensor and hands it to a direct solver; at TT ranks beyond ~48 that tensor no
// longer fits). Here the operator is applied through its two environments and the operator core as a chain of
// fp64 MFMA GEMMs without a permutation on the hot path, and the local system is solved by conjugate gradients
// whose scalars, convergence flag and iteration counter stay in device memory: the host enqueues iterations and
// looks at the flag every `check_every` of them.
//
// Chains (row-major; Ahat[(p,j),(i,q)] = A(p,i,j,q) is the core with its two middle modes swapped, permuted once
// per LocalOp):
//   symmetric form                                            normal equations (A^T A)
//   1. T1[(a,p),(j,b')]  = L[(a,p),a'] x[a',(j,b')]           1. T1[(a,p,p'),(j,b')] = L x
//   2. per a:  T2_a[(i,q),b'] = Ahat^T T1_a[(p,j),b']         2. per (a,p): T2[(y,q'),b'] = Ahat^T T1_{a,p}[(p',j),b']
//   3. y[(a,i),b] = T2[(a,i),(q,b')] R[b,(q,b')]^T            3. per a: T3_a[(i,q),(q',b')] = A[(p,y),(i,q)]^T T2_a
//                                                             4. y = T3[(a,i),(q,q',b')] R[b,(q,q',b')]^T
//
// CG kernels: per iteration (i) partial sums of p.q, (ii) alpha, x += alpha p, r -= alpha q and partial sums of
// r.r, (iii) beta, p = r + beta p and the state words. Every block of (ii) and (iii) sums the previous launch's
// partials itself, in one fixed order, so all blocks hold the same scalar without a grid barrier and the result
// is bit-reproducible. A word of the state is never read by a launch that also writes it: (ii) reads rr and done
// and writes pq, rr_prev and skip; (iii) reads rr_prev, skip and the threshold and writes rr, done, status and the
// counter. Once done is set, (ii) and (iii) return at once (the freeze), so the iterations the host enqueues up to
// its next look change nothing and the result does not depend on how often it looks.
#include <cmath>

#include "als_local.hpp"
#include "als_reduce.hpp"
#include "elementwise.hpp"
#include "scratch_map.hpp"

namespace xrs {
namespace als_local {

namespace {

struct CgState {
    double rr, rr_prev, pq, bb, thresh;
    int done, skip, status, iters;
};
static_assert(sizeof(CgState) <= scratch::kDevCgState.len && sizeof(CgState) <= scratch::kHostCgState.len);
static_assert(2 * CMAXB * sizeof(double) <= scratch::kDevCgPartials.len);

// r = b - q (q = M x0), p = r; partial sums of r.r (first CMAXB) and b.b (second CMAXB)
__global__ void __launch_bounds__(CB) k_cg_init(double* __restrict__ r, double* __restrict__ p, const double* __restrict__ b,
                                                const double* __restrict__ q, size_t n, double* __restrict__ partial) {
    double arr = 0.0, abb = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) {
        const double bi = b[i], ri = bi - q[i];
        r[i] = ri;
        p[i] = ri;
        arr += ri * ri;
        abb += bi * bi;
    }
    const double srr = block_sum_all(arr), sbb = block_sum_all(abb);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = srr;
        partial[CMAXB + blockIdx.x] = sbb;
    }
}

__global__ void __launch_bounds__(CB) k_cg_init_state(const double* __restrict__ partial, int nb, double tol, CgState* __restrict__ st) {
    const double rr = sum_partials(partial, nb), bb = sum_partials(partial + CMAXB, nb);
    if (threadIdx.x == 0) {
        const double thresh = tol * tol * bb;
        st->rr = rr;
        st->rr_prev = rr;
        st->pq = 0.0;
        st->bb = bb;
        st->thresh = thresh;
        st->done = rr <= thresh ? 1 : 0;
        st->skip = 0;
        st->status = 0;
        st->iters = 0;
    }
}

// (i) partial sums of p.q
__global__ void __launch_bounds__(CB) k_cg_pq(const double* __restrict__ p, const double* __restrict__ q, size_t n,
                                              double* __restrict__ partial) {
    double acc = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) acc += p[i] * q[i];
    const double s = block_sum_all(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// (ii) alpha = rr / pq; x += alpha p; r -= alpha q; partial sums of r.r. Frozen (done) or broken down (pq <= 0 or
// not finite): nothing is touched but the skip word that tells (iii) so.
__global__ void __launch_bounds__(CB) k_cg_update(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                  const double* __restrict__ q, size_t n, const double* __restrict__ pq_partial,
                                                  double* __restrict__ rr_partial, int nb, CgState* __restrict__ st) {
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (st->done) {
        if (first) st->skip = 1;
        return;
    }
    const double pq = sum_partials(pq_partial, nb);
    const double rr = st->rr;
    if (!(pq > 0.0) || !isfinite(pq)) {
        if (first) {
            st->pq = pq;
            st->status = XRS_CG_BREAKDOWN;
            st->skip = 1;
        }
        return;
    }
    const double alpha = rr / pq;
    double acc = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        acc += ri * ri;
    }
    const double s = block_sum_all(acc);
    if (threadIdx.x == 0) rr_partial[blockIdx.x] = s;
    if (first) {
        st->pq = pq;
        st->rr_prev = rr;
        st->skip = 0;
    }
}

// (iii) rr' and beta = rr' / rr; p = r + beta p; block 0 writes the scalars, counts the iteration and sets done on
// convergence (or when (ii) skipped its update)
__global__ void __launch_bounds__(CB) k_cg_direction(const double* __restrict__ r, double* __restrict__ p, size_t n,
                                                     const double* __restrict__ rr_partial, int nb, CgState* __restrict__ st) {
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (st->skip) {
        if (first) st->done = 1;
        return;
    }
    const double rrn = sum_partials(rr_partial, nb);
    const double beta = rrn / st->rr_prev;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) p[i] = r[i] + beta * p[i];
    if (first) {
        st->rr = rrn;
        st->iters += 1;
        if (!isfinite(rrn)) {
            st->status = XRS_CG_BREAKDOWN;
            st->done = 1;
        } else if (rrn <= st->thresh) {
            st->done = 1;
        }
    }
}

CgState read_state(xrs_handle_t h, const CgState* dev) {
    CgState* host = scratch::host<CgState>(h, scratch::kHostCgState);
    XRS_HIP(hipMemcpyAsync(host, dev, sizeof(CgState), hipMemcpyDeviceToHost, h->stream));
    host_wait(h);
    return *host;
}

}  // namespace

LocalOp::LocalOp(xrs_handle_t h, size_t rl, size_t n, size_t rr, size_t pl, size_t pr, const double* L, const double* A,
                 const double* R, bool normal)
    : h_(h), rl_(rl), n_(n), rr_(rr), pl_(pl), pr_(pr), L_(L), R_(R), normal_(normal) {
    const size_t lim = size_t(1) << 30;
    XRS_REQUIRE(rl < lim && n < lim && rr < lim && pl < lim && pr < lim, "extent too large");
    const size_t envl = normal ? pl * pl : pl, envr = normal ? pr * pr : pr;
    XRS_REQUIRE(rl * envl < lim && n * rr < lim && n * pr < lim && pl * n < lim && envr * rr < lim && rl * n < lim,
                "local problem too large for one GEMM");
    XRS_REQUIRE(rl * envl < (size_t(1) << 40) / (n * rr) && rl * n * pr < (size_t(1) << 40) / (envr * rr),
                "local problem too large");
    Ahat_ = DevBuf(h, pl * n * n * pr * 8);
    const size_t dims[4] = {pl, n, n, pr}, shuffle[4] = {0, 2, 1, 3};
    permute(h, Ahat_.d(), A, 4, dims, shuffle);
    T1_ = DevBuf(h, rl * envl * n * rr * 8);
    const size_t batch2 = normal ? rl * pl : rl;
    T2_ = DevBuf(h, batch2 * n * pr * rr * 8);
    a2_.assign(batch2, Ahat_.d());
    b2_.resize(batch2);
    c2_.resize(batch2);
    for (size_t i = 0; i < batch2; ++i) {
        b2_[i] = T1_.d() + i * (pl * n * rr);
        c2_[i] = T2_.d() + i * (n * pr * rr);
    }
    if (normal) {
        T3_ = DevBuf(h, rl * n * pr * pr * rr * 8);
        a3_.assign(rl, A);
        b3_.resize(rl);
        c3_.resize(rl);
        for (size_t i = 0; i < rl; ++i) {
            b3_[i] = T2_.d() + i * (pl * n * pr * rr);
            c3_[i] = T3_.d() + i * (n * pr * pr * rr);
        }
    }
}

void LocalOp::apply(double* y, const double* x) {
    const size_t envl = normal_ ? pl_ * pl_ : pl_;
    gemm(h_, T1_.d(), rl_ * envl, n_ * rr_, 1.0, L_, rl_, false, rl_, x, n_ * rr_, false);
    gemm_batched(h_, int(a2_.size()), c2_.data(), n_ * pr_, rr_, 1.0, a2_.data(), n_ * pr_, true, pl_ * n_, b2_.data(), rr_, false);
    if (!normal_) {
        gemm(h_, y, rl_ * n_, rr_, 1.0, T2_.d(), pr_ * rr_, false, pr_ * rr_, R_, pr_ * rr_, true);
        return;
    }
    gemm_batched(h_, int(rl_), c3_.data(), n_ * pr_, pr_ * rr_, 1.0, a3_.data(), n_ * pr_, true, pl_ * n_, b3_.data(), pr_ * rr_,
                 false);
    const size_t k4 = pr_ * pr_ * rr_;
    gemm(h_, y, rl_ * n_, rr_, 1.0, T3_.d(), k4, false, k4, R_, k4, true);
}

CgResult cg(xrs_handle_t h, LocalOp& op, double* x, const double* b, double tol, size_t max_iter, size_t check_every) {
    const size_t n = op.size();
    const size_t cap = 4 * n + 50;
    if (max_iter == 0 || max_iter > cap) max_iter = cap;
    const int nb = blocks_for(n);
    CgState* st = scratch::dev<CgState>(h, scratch::kDevCgState);
    double* partial = scratch::dev<double>(h, scratch::kDevCgPartials, 2 * CMAXB);
    double* pq_partial = partial;
    double* rr_partial = partial + CMAXB;
    DevBuf rbuf(h, n * 8), pbuf(h, n * 8), qbuf(h, n * 8);
    double *r = rbuf.d(), *p = pbuf.d(), *q = qbuf.d();
    const double dn = double(n);

    op.apply(q, x);
    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, 5.0 * dn, 32.0 * dn);
        hipLaunchKernelGGL(k_cg_init, dim3(nb), dim3(CB), 0, h->stream, r, p, b, q, n, partial);
        check_launch("k_cg_init");
    }
    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, 2.0 * double(nb), 16.0 * double(nb));
        hipLaunchKernelGGL(k_cg_init_state, dim3(1), dim3(CB), 0, h->stream, partial, nb, tol, st);
        check_launch("k_cg_init_state");
    }
    CgState s = read_state(h, st);
    if (s.bb == 0.0) {
        XRS_HIP(hipMemsetAsync(x, 0, n * 8, h->stream));
        host_wait(h);
        return {0, 0.0, XRS_CG_CONVERGED};
    }
    for (size_t k = 0; k < max_iter && !s.done; ++k) {
        op.apply(q, p);
        {
            KernelTimer timer(h, XRS_KFAM_ELEMWISE, 2.0 * dn, 16.0 * dn);
            hipLaunchKernelGGL(k_cg_pq, dim3(nb), dim3(CB), 0, h->stream, p, q, n, pq_partial);
            check_launch("k_cg_pq");
        }
        {
            KernelTimer timer(h, XRS_KFAM_ELEMWISE, 6.0 * dn, 48.0 * dn);
            hipLaunchKernelGGL(k_cg_update, dim3(nb), dim3(CB), 0, h->stream, x, r, p, q, n, pq_partial, rr_partial, nb, st);
            check_launch("k_cg_update");
        }
        {
            KernelTimer timer(h, XRS_KFAM_ELEMWISE, 2.0 * dn, 24.0 * dn);
            hipLaunchKernelGGL(k_cg_direction, dim3(nb), dim3(CB), 0, h->stream, r, p, n, rr_partial, nb, st);
            check_launch("k_cg_direction");
        }
        if ((k + 1) % check_every == 0 || k + 1 == max_iter) s = read_state(h, st);
    }
    return {size_t(s.iters), std::sqrt(s.rr / s.bb), s.done ? s.status : XRS_CG_MAX_ITER};
}

}  // namespace als_local
}  // namespace xrs

using namespace xrs;

namespace {
void check_local_args(xrs_handle_t h, const double* x, const double* y, size_t rl, size_t n, size_t rr, size_t pl, size_t pr,
                      const double* L, const double* A, const double* R) {
    XRS_REQUIRE(h, "null handle");
    XRS_REQUIRE(rl > 0 && n > 0 && rr > 0 && pl > 0 && pr > 0, "extents must be positive");
    XRS_REQUIRE(x && y && L && A && R, "null argument");
}
}  // namespace

extern "C" {

int xrs_als_local_apply(xrs_handle_t h, double* y, const double* x, size_t rl, size_t n, size_t rr, size_t pl, size_t pr,
                        const double* L, const double* A, const double* R, int normal) {
    return guarded([&] {
        check_local_args(h, x, y, rl, n, rr, pl, pr, L, A, R);
        XRS_REQUIRE(y != x, "y must not alias x");
        fence_readers(h);
        als_local::LocalOp op(h, rl, n, rr, pl, pr, L, A, R, normal != 0);
        op.apply(y, x);
    });
}

int xrs_als_local_cg(xrs_handle_t h, double* x, const double* b, size_t rl, size_t n, size_t rr, size_t pl, size_t pr,
                     const double* L, const double* A, const double* R, int normal, double tol, size_t max_iter,
                     size_t check_every, size_t* iters, double* relres, int* status) {
    return guarded([&] {
        check_local_args(h, x, b, rl, n, rr, pl, pr, L, A, R);
        XRS_REQUIRE(iters && relres && status, "null result pointer");
        XRS_REQUIRE(x != b, "x must not alias b");
        XRS_REQUIRE(tol >= 0.0, "tol must be non-negative");   // (false for NaN)
        XRS_REQUIRE(check_every > 0, "check_every must be positive");
        fence_readers(h);
        als_local::LocalOp op(h, rl, n, rr, pl, pr, L, A, R, normal != 0);
        const als_local::CgResult res = als_local::cg(h, op, x, b, tol, max_iter, check_every);
        *iters = res.iters;
        *relres = res.relres;
        *status = res.status;
    });
}

}  // extern "C"
