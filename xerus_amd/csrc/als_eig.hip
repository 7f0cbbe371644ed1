// Lowest eigenpair of the local operator of a one-site sweep, matrix-free: LOBPCG with block size 1 and no
// preconditioner (Knyazev 2001) around the GEMM chain of als_local.hip (LocalOp, symmetric form). Like the CG there,
// the iteration keeps its scalars, its convergence flag and its counter in device memory; the host enqueues
// iterations and looks at the flag every `check_every` of them.
//
// Vectors (N = rl n rr): x (unit), ax = M x, p, ap = M p, r = ax - theta x, ar = M r. Per iteration, after the one
// operator application ar = M r:
//   (i)   k_eig_gram: per-block partial sums of the Gram pair of S = [x, r, p]: G = S^T S and H = S^T M S, six
//         unique entries each (x.ar serves as both H_xr and H_rx);
//   (ii)  k_eig_update: every block sums those partials itself in one fixed order (no grid barrier, no atomics,
//         bit-reproducible), solves the 3 x 3 pencil for its smallest pair (theta, c) in registers (geneig.hpp; 2 x 2
//         in the first iteration, where p is absent), and updates p' = c1 r + c2 p, ap' = c1 ar + c2 ap,
//         x' = c0 x + p', ax' = c0 ax + ap', r' = ax' - theta x' with partial sums of r'.r'. c has unit G-norm, so
//         x' is a unit vector by the measured Gram entries and its norm does not drift;
//   (iii) k_eig_state (one block): rr = r'.r', theta, the counter, and done once rr <= tol^2 ||M x0||^2.
// No word of the state is read by one thread of a launch and written by another: (i) reads done; (ii) reads done and
// the counter and writes skip, theta_next and (on breakdown) status; (iii) reads skip, theta_next, the threshold and
// the counter and writes theta, rr, done, status and the counter -- the counter is the one word a launch both reads
// and writes, incremented by the single thread of the single block that writes the state (as in the CG). Once done
// is set, (i) and (ii) return at once (the freeze), so the iterations the host enqueues up to its next look change
// nothing and the result does not depend on how often it looks. A breakdown of the small problem leaves every vector at the iterate before the failing step.
#include <cmath>

#include "als_eig.hpp"
#include "als_reduce.hpp"
#include "geneig.hpp"
#include "scratch_map.hpp"

namespace xrs {
namespace als_local {

namespace {

struct EigState {
    double theta, theta_next, rr, nax2, thresh;
    int done, skip, status, iters;
};
static_assert(sizeof(EigState) <= scratch::kDevEigState.len && sizeof(EigState) <= scratch::kHostEigState.len);

// partial sums (pool buffer of kSlots x CMAXB doubles): slots 0..5 G (xx xr xp rr rp pp), 6..11 H (x.ax x.ar x.ap
// r.ar r.ap p.ap), 12 r'.r' of the update. The initialisation uses 0 (x.x), 6 (x.ax), 11 (ax.ax) and 12.
constexpr int kSlots = 13, kSlotRR = 12, kSlotXX = 0, kSlotXAX = 6, kSlotAXAX = 11;

__global__ void __launch_bounds__(CB) k_eig_norm(const double* __restrict__ x, size_t n, double* __restrict__ partial) {
    double acc = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) acc += x[i] * x[i];
    const double s = block_sum_all(acc);
    if (threadIdx.x == 0) partial[kSlotXX * CMAXB + blockIdx.x] = s;
}

// x /= ||x|| (left alone when the norm is zero or not finite: the state kernel reports that)
__global__ void __launch_bounds__(CB) k_eig_scale(double* __restrict__ x, size_t n, const double* __restrict__ partial, int nb) {
    const double xx = sum_partials(partial + kSlotXX * CMAXB, nb);
    if (!(xx > 0.0) || !geneig_finite(xx)) return;
    const double s = 1.0 / sqrt(xx);
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) x[i] *= s;
}

__global__ void __launch_bounds__(CB) k_eig_rayleigh(const double* __restrict__ x, const double* __restrict__ ax, size_t n,
                                                     double* __restrict__ partial) {
    double axx = 0.0, aaa = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) {
        const double xi = x[i], ai = ax[i];
        axx += xi * ai;
        aaa += ai * ai;
    }
    const double sxx = block_sum_all(axx), saa = block_sum_all(aaa);
    if (threadIdx.x == 0) {
        partial[kSlotXAX * CMAXB + blockIdx.x] = sxx;
        partial[kSlotAXAX * CMAXB + blockIdx.x] = saa;
    }
}

// theta = x.ax; r = ax - theta x; p = ap = 0; partial sums of r.r
__global__ void __launch_bounds__(CB) k_eig_residual(const double* __restrict__ x, const double* __restrict__ ax, double* __restrict__ r,
                                                     double* __restrict__ p, double* __restrict__ ap, size_t n,
                                                     double* __restrict__ partial, int nb) {
    const double theta = sum_partials(partial + kSlotXAX * CMAXB, nb);
    double acc = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) {
        const double ri = ax[i] - theta * x[i];
        r[i] = ri;
        p[i] = 0.0;
        ap[i] = 0.0;
        acc += ri * ri;
    }
    const double s = block_sum_all(acc);
    if (threadIdx.x == 0) partial[kSlotRR * CMAXB + blockIdx.x] = s;
}

__global__ void __launch_bounds__(CB) k_eig_init_state(const double* __restrict__ partial, int nb, double tol, EigState* __restrict__ st) {
    const double xx = sum_partials(partial + kSlotXX * CMAXB, nb), theta = sum_partials(partial + kSlotXAX * CMAXB, nb);
    const double nax2 = sum_partials(partial + kSlotAXAX * CMAXB, nb), rr = sum_partials(partial + kSlotRR * CMAXB, nb);
    if (threadIdx.x == 0) {
        const bool ok = xx > 0.0 && geneig_finite(xx) && geneig_finite(theta) && geneig_finite(nax2) && geneig_finite(rr);
        const double thresh = tol * tol * nax2;
        st->theta = theta;
        st->theta_next = theta;
        st->rr = rr;
        st->nax2 = nax2;
        st->thresh = thresh;
        st->done = (!ok || rr <= thresh) ? 1 : 0;
        st->skip = 0;
        st->status = ok ? XRS_EIG_CONVERGED : XRS_EIG_BREAKDOWN;
        st->iters = 0;
    }
}

// (i) partial sums of the Gram pair
__global__ void __launch_bounds__(CB) k_eig_gram(const double* __restrict__ x, const double* __restrict__ r, const double* __restrict__ p,
                                                 const double* __restrict__ ax, const double* __restrict__ ar,
                                                 const double* __restrict__ ap, size_t n, double* __restrict__ partial,
                                                 const EigState* __restrict__ st) {
    if (st->done) return;
    double acc[12] = {};
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) {
        const double xi = x[i], ri = r[i], pi = p[i], axi = ax[i], ari = ar[i], api = ap[i];
        acc[0] += xi * xi;
        acc[1] += xi * ri;
        acc[2] += xi * pi;
        acc[3] += ri * ri;
        acc[4] += ri * pi;
        acc[5] += pi * pi;
        acc[6] += xi * axi;
        acc[7] += xi * ari;
        acc[8] += xi * api;
        acc[9] += ri * ari;
        acc[10] += ri * api;
        acc[11] += pi * api;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const double s = block_sum_all(acc[k]);
        if (threadIdx.x == 0) partial[k * CMAXB + blockIdx.x] = s;
    }
}

// (ii) the small problem and the fused update. Frozen (done) or broken down: nothing is touched but the skip word
// that tells (iii) so (and the status).
__global__ void __launch_bounds__(CB) k_eig_update(double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                   double* __restrict__ ax, const double* __restrict__ ar, double* __restrict__ ap,
                                                   size_t n, double* __restrict__ partial, int nb, EigState* __restrict__ st) {
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (st->done) {
        if (first) st->skip = 1;
        return;
    }
    double G[6], H[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        G[k] = sum_partials(partial + k * CMAXB, nb);
        H[k] = sum_partials(partial + (6 + k) * CMAXB, nb);
    }
    double theta = 0.0, c[3] = {0.0, 0.0, 0.0};
    int used;
    if (st->iters == 0) {   // p is absent: S = [x, r]
        const double G2[3] = {G[0], G[1], G[3]}, H2[3] = {H[0], H[1], H[3]};
        used = geneig_lowest(2, G2, H2, &theta, c);
    } else {
        used = geneig_lowest(3, G, H, &theta, c);
    }
    if (used == 0) {
        if (first) {
            st->status = XRS_EIG_BREAKDOWN;
            st->skip = 1;
        }
        return;
    }
    const double c0 = c[0], c1 = c[1], c2 = c[2];
    double acc = 0.0;
    const size_t stride = size_t(gridDim.x) * CB;
    for (size_t i = size_t(blockIdx.x) * CB + threadIdx.x; i < n; i += stride) {
        const double pn = c1 * r[i] + c2 * p[i];
        const double apn = c1 * ar[i] + c2 * ap[i];
        const double xn = c0 * x[i] + pn;
        const double axn = c0 * ax[i] + apn;
        const double rn = axn - theta * xn;
        p[i] = pn;
        ap[i] = apn;
        x[i] = xn;
        ax[i] = axn;
        r[i] = rn;
        acc += rn * rn;
    }
    const double s = block_sum_all(acc);
    if (threadIdx.x == 0) partial[kSlotRR * CMAXB + blockIdx.x] = s;
    if (first) {
        st->theta_next = theta;
        st->skip = 0;
    }
}

// (iii) one block: the state words
__global__ void __launch_bounds__(CB) k_eig_state(const double* __restrict__ partial, int nb, EigState* __restrict__ st) {
    if (st->skip) {
        if (threadIdx.x == 0) st->done = 1;
        return;
    }
    const double rr = sum_partials(partial + kSlotRR * CMAXB, nb);
    if (threadIdx.x == 0) {
        st->rr = rr;
        st->theta = st->theta_next;
        st->iters += 1;
        if (!geneig_finite(rr)) {
            st->status = XRS_EIG_BREAKDOWN;
            st->done = 1;
        } else if (rr <= st->thresh) {
            st->done = 1;
        }
    }
}

EigState read_state(xrs_handle_t h, const EigState* dev) {
    EigState* host = scratch::host<EigState>(h, scratch::kHostEigState);
    XRS_HIP(hipMemcpyAsync(host, dev, sizeof(EigState), hipMemcpyDeviceToHost, h->stream));
    host_wait(h);
    return *host;
}

}  // namespace

EigResult eig(xrs_handle_t h, LocalOp& op, double* x, double tol, size_t max_iter, size_t check_every) {
    const size_t n = op.size();
    const size_t cap = 4 * n + 50;
    if (max_iter == 0 || max_iter > cap) max_iter = cap;
    const int nb = blocks_for(n);
    EigState* st = scratch::dev<EigState>(h, scratch::kDevEigState);
    DevBuf pbuf(h, size_t(kSlots) * CMAXB * 8);
    double* partial = pbuf.d();
    DevBuf axb(h, n * 8), rb(h, n * 8), arb(h, n * 8), pb(h, n * 8), apb(h, n * 8);
    double *ax = axb.d(), *r = rb.d(), *ar = arb.d(), *p = pb.d(), *ap = apb.d();
    const double dn = double(n), dnb = double(nb);

    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, 2.0 * dn, 8.0 * dn);
        hipLaunchKernelGGL(k_eig_norm, dim3(nb), dim3(CB), 0, h->stream, x, n, partial);
        check_launch("k_eig_norm");
    }
    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, dn, 16.0 * dn);
        hipLaunchKernelGGL(k_eig_scale, dim3(nb), dim3(CB), 0, h->stream, x, n, partial, nb);
        check_launch("k_eig_scale");
    }
    op.apply(ax, x);
    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, 4.0 * dn, 16.0 * dn);
        hipLaunchKernelGGL(k_eig_rayleigh, dim3(nb), dim3(CB), 0, h->stream, x, ax, n, partial);
        check_launch("k_eig_rayleigh");
    }
    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, 4.0 * dn, 40.0 * dn);
        hipLaunchKernelGGL(k_eig_residual, dim3(nb), dim3(CB), 0, h->stream, x, ax, r, p, ap, n, partial, nb);
        check_launch("k_eig_residual");
    }
    {
        KernelTimer timer(h, XRS_KFAM_ELEMWISE, 4.0 * dnb, 32.0 * dnb);
        hipLaunchKernelGGL(k_eig_init_state, dim3(1), dim3(CB), 0, h->stream, partial, nb, tol, st);
        check_launch("k_eig_init_state");
    }
    EigState s = read_state(h, st);
    for (size_t k = 0; k < max_iter && !s.done; ++k) {
        op.apply(ar, r);
        {
            KernelTimer timer(h, XRS_KFAM_ELEMWISE, 24.0 * dn, 48.0 * dn);
            hipLaunchKernelGGL(k_eig_gram, dim3(nb), dim3(CB), 0, h->stream, x, r, p, ax, ar, ap, n, partial, st);
            check_launch("k_eig_gram");
        }
        {
            KernelTimer timer(h, XRS_KFAM_ELEMWISE, 12.0 * dn, 88.0 * dn);
            hipLaunchKernelGGL(k_eig_update, dim3(nb), dim3(CB), 0, h->stream, x, r, p, ax, ar, ap, n, partial, nb, st);
            check_launch("k_eig_update");
        }
        {
            KernelTimer timer(h, XRS_KFAM_ELEMWISE, dnb, 8.0 * dnb);
            hipLaunchKernelGGL(k_eig_state, dim3(1), dim3(CB), 0, h->stream, partial, nb, st);
            check_launch("k_eig_state");
        }
        if ((k + 1) % check_every == 0 || k + 1 == max_iter) s = read_state(h, st);
    }
    const double relres = s.nax2 > 0.0 ? std::sqrt(s.rr / s.nax2) : 0.0;
    return {s.theta, size_t(s.iters), relres, s.done ? s.status : XRS_EIG_MAX_ITER};
}

}  // namespace als_local
}  // namespace xrs

using namespace xrs;

extern "C" {

int xrs_als_local_eig(xrs_handle_t h, double* x, size_t rl, size_t n, size_t rr, size_t pl, size_t pr, const double* L,
                      const double* A, const double* R, double tol, size_t max_iter, size_t check_every, double* theta,
                      size_t* iters, double* relres, int* status) {
    return guarded([&] {
        XRS_REQUIRE(h, "null handle");
        XRS_REQUIRE(rl > 0 && n > 0 && rr > 0 && pl > 0 && pr > 0, "extents must be positive");
        XRS_REQUIRE(x && L && A && R, "null argument");
        XRS_REQUIRE(theta && iters && relres && status, "null result pointer");
        XRS_REQUIRE(tol >= 0.0 && std::isfinite(tol), "tol must be finite and non-negative");   // (false for NaN)
        XRS_REQUIRE(check_every > 0, "check_every must be positive");
        fence_readers(h);
        als_local::LocalOp op(h, rl, n, rr, pl, pr, L, A, R, false);
        const als_local::EigResult res = als_local::eig(h, op, x, tol, max_iter, check_every);
        *theta = res.theta;
        *iters = res.iters;
        *relres = res.relres;
        *status = res.status;
    });
}

int xrs_geneig_lowest(int k, const double* G, const double* H, double* theta, double* c) {
    if ((k != 2 && k != 3) || !G || !H || !theta || !c) return 0;
    double th = 0.0, co[3] = {0.0, 0.0, 0.0};
    const int used = geneig_lowest(k, G, H, &th, co);
    if (used == 0) return 0;
    *theta = th;
    for (int i = 0; i < k; ++i) c[i] = co[i];
    return used;
}

}  // extern "C"
