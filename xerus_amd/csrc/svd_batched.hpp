// Batched thin SVD of many small same-shape matrices (svd_batched.hip): one workgroup per matrix, one launch
// and one host synchronisation for the whole batch.
#pragma once
#include <cstddef>

#include "runtime.hpp"

namespace xrs {

// The batched kernel's envelope. With p = min(m, n), q = max(m, n) a workgroup keeps p rows of p + q doubles
// (the data and the accumulated rotations) in LDS, at a row stride ld = the next value >= p + q that is
// 16 mod 32, so it needs
//     8 (p ld + p + 8) + 4 (p + 2)  <=  160 KiB          and          p + q <= 512
// (the second bound is the widest register tiling, 32 doubles per lane of a 16-lane group). 64 x 64 (73 KiB)
// and 32 x 448 (124 KiB) fit; 128 x 128 (272 KiB) does not.
bool svd_batched_fits(size_t m, size_t n);
size_t svd_batched_lds_bytes(size_t m, size_t n);   // of one workgroup (0 outside p + q <= 512)

// Thin SVDs A_b = U_b diag(S_b) Vt_b of `batch` m x n matrices stored back to back (device: A batch*m*n,
// U batch*m*k, S batch*k, Vt batch*k*n, k = min(m, n); S_b descending). Inside the envelope: one launch, the
// statuses read back with one host synchronisation, then every member whose status is -1 (not converged,
// numerically rank-deficient or zero) is recomputed by svd(). Outside: svd() per member, all statuses -1.
// Inside the envelope a recomputed member's factors are then re-orthonormalised (Gram-Schmidt in the order of
// S): svd() leaves zero or non-orthogonal vectors for singular values that are zero or of rounding size.
// status_host (batch ints, may be null): the kernel's sweeps (>= 0), or -1 for a recomputed member.
void svd_batched(xrs_handle_t h, const double* A, size_t batch, size_t m, size_t n, double* U, double* S, double* Vt,
                 int* status_host);

}  // namespace xrs
