// Matrix-free local problem of one-site ALS (als_local.hip): the local operator applied through the two
// environments and the operator core, and a conjugate-gradient solve whose state stays on the device.
#pragma once
#include <vector>

#include "runtime.hpp"

namespace xrs {
namespace als_local {

// The local operator M of xrs_als_local_apply as a planned GEMM chain: the permuted core, the temporaries and the
// batch pointer tables are set up once and reused by every product of a solve.
class LocalOp {
   public:
    LocalOp(xrs_handle_t h, size_t rl, size_t n, size_t rr, size_t pl, size_t pr, const double* L, const double* A,
            const double* R, bool normal);
    size_t size() const { return rl_ * n_ * rr_; }
    // y = M x: three (normal: four) GEMMs, enqueued only. y must not alias x.
    void apply(double* y, const double* x);

   private:
    xrs_handle_t h_;
    size_t rl_, n_, rr_, pl_, pr_;
    const double *L_, *R_;
    bool normal_;
    DevBuf Ahat_, T1_, T2_, T3_;
    std::vector<const double*> a2_, b2_, a3_, b3_;
    std::vector<double*> c2_, c3_;
};

struct CgResult {
    size_t iters;
    double relres;
    int status;
};
// CG on M x = b from the start in x (xrs_als_local_cg); synchronises
CgResult cg(xrs_handle_t h, LocalOp& op, double* x, const double* b, double tol, size_t max_iter, size_t check_every);

}  // namespace als_local
}  // namespace xrs
