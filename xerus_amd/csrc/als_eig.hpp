// Lowest eigenpair of the symmetric local operator of a one-site sweep (als_eig.hip): LOBPCG with block size 1
// around als_local::LocalOp, its state on the device.
#pragma once
#include "als_local.hpp"

namespace xrs {
namespace als_local {

struct EigResult {
    double theta;
    size_t iters;
    double relres;
    int status;
};
// the smallest algebraic eigenvalue of M (symmetric form) from the start in x (xrs_als_local_eig); synchronises
EigResult eig(xrs_handle_t h, LocalOp& op, double* x, double tol, size_t max_iter, size_t check_every);

}  // namespace als_local
}  // namespace xrs
