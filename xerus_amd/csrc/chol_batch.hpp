// Batched Cholesky front end of the TT rounds (chol_batch.hip): a list of small SPD Gram matrices of any
// mix of sizes goes to the kernel family of each size class, with the kernels' argument tables chunked here.
#pragma once
#include <vector>

#include "smallla.hpp"

namespace xrs {

// A + shift tr(A) I = L L^T of an n x n symmetric matrix A (any n; lower triangle read).
struct CholJob {
    const double* A;
    int n;
    double* L;            // factor (lower, out of place); null: a status-only certificate
    double* Z;            // L^{-1} (n x n); null: not wanted
    double shift = 0.0;   // relative diagonal shift, always the one given
    // the status-only factorisation chol(A - tau tr(A) I) that certifies lambda_min(A) >= ~tau tr(A)
    static CholJob certificate(const double* A, int n, double tau) { return {A, n, nullptr, nullptr, -tau}; }
};

constexpr int kCholLaunchJobs = 48;   // n <= 256 jobs that one launch of the register-resident kernel holds

// Status words the jobs write (1 for n <= 256, 2 for 257..512, chol_full_blocks(n) above).
int chol_status_count(const std::vector<CholJob>& jobs);

// Enqueues every job on the handle's stream, never synchronises. status[0 .. chol_status_count(jobs)) are all
// zero when every factorisation succeeded; the layout inside is the front end's own. `keep` receives the
// device temporaries, which must outlive the enqueued work.
// Order on the stream: the jobs above 512 one at a time (chol_full), the 257..512 ones as 2 x 2 blocks of the
// n <= 256 kernels (one batched launch per step over all of them), then the n <= 256 ones: one
// register-resident launch per kCholLaunchJobs jobs, and one inverse launch per 64 factor jobs that ask for Z.
// L and Z of a job with n <= 256 have exact zeros above the diagonal (the register-resident kernels' outputs:
// GEMMs may skip their zero blocks, kTriA / kTriB); above 256 they are assembled from blocks, zeros included,
// but the callers claim nothing about them.
void chol_enqueue(xrs_handle_t h, const std::vector<CholJob>& jobs, int* status, std::vector<DevBuf>& keep);

// The same in two calls, for a caller that runs the explicit inverses on another lane than the factorisations
// (tt.hip chain_pass): chol_enqueue_factors enqueues everything but the inverse launches of the n <= 256 jobs
// and lists those in `later`; chol_enqueue_inverses enqueues them on the handle's (then current) stream, which
// the caller has ordered behind the factorisations. The inverses read L and the diagonal-block slab in `keep`:
// both outlive them. Jobs above 256 get their Z in the first call, as part of their blocked factorisation.
struct CholInverses {
    struct Item {
        const double* L;
        const double* Dinv;
        double* X;
        int n;
    };
    std::vector<Item> items;
};
void chol_enqueue_factors(xrs_handle_t h, const std::vector<CholJob>& jobs, int* status, std::vector<DevBuf>& keep,
                          CholInverses& later);
void chol_enqueue_inverses(xrs_handle_t h, const CholInverses& later);

}  // namespace xrs
