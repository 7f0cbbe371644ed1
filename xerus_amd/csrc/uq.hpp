// UQ-ADF per-sample kernels (uq.hip; reference src/xerus/algorithms/uqAdf.cpp:110-282). A sample j carries,
// per core position, its basis row P[j, :] (n), vector stacks (N x r row-major, the rank-one mode of adf.hpp)
// and the symmetric matrix stack L_j (N x r x r row-major). With M_j = sum_t P[j, t] X[:, t, :] (a x b) for a
// component X (a x n x b), everything here is one launch over all N samples, enqueued on h->stream; every
// reduction runs in a fixed order (bit-reproducible).
#pragma once
#include <cstddef>

#include "runtime.hpp"

namespace xrs {
namespace uq {

constexpr size_t kMaxRank = 256;   // larger ranks are refused

// Basis matrices of several modes in one launch: for mode m < modes, P_m[j, i] = He_i(xi[j * ld + m]) for
// i < n[m], He the probabilists' Hermite polynomials (He_0 = 1, He_1 = v, He_{i+1} = v He_i - i He_{i-1};
// uqAdf.cpp:40-52). P_m = Pbase + off[m], N x n[m] row-major. n / off are host arrays.
void basis(xrs_handle_t h, size_t N, size_t modes, const double* xi, size_t ld, const size_t* n, const size_t* off, double* Pbase);

// Which kernel stack_congruence uses: the choice by shape, or one of the two forced (A/B measurements).
enum class Path { Auto, Fma, Mfma };
// Lout[j] (b x b) = M_j^T L_j M_j, L_j (a x a) symmetric, or the identity when Lprev is null
// (calc_left_stack, uqAdf.cpp:128-135). M_j and L_j M_j live in LDS only. One triangle is computed and
// mirrored: Lout[j] is exactly symmetric. Lprev is read through its transpose, i.e. must be symmetric.
//   Mfma: one workgroup per sample, 16 x 16 v_mfma_f64_16x16x4_f64 tiles, ragged edges zero-padded in LDS
//         (both ranks >= 16 and M_j, L_j M_j within the LDS);
//   Fma:  several samples per workgroup for small ranks; column panels of M_j for shapes beyond the LDS.
void stack_congruence(xrs_handle_t h, size_t N, const double* Lprev, const double* X, const double* P, size_t a, size_t n, size_t b,
                      double* Lout, Path path = Path::Auto);

// Y (N x a): y_j = L_j v_j (L symmetric, read through its transpose; null: Y = V). Y must not alias V.
void stack_symv(xrs_handle_t h, size_t N, const double* L, const double* V, size_t a, double* Y);
// out_dev[0] = sum_j v_j^T L_j v_j (L null: sum_j v_j^T v_j): block partials in a grid fixed by the shape, then
// one block over the partials. Enqueued only.
void quadform(xrs_handle_t h, size_t N, const double* L, const double* V, size_t a, double* out_dev);
// the same, read back (one host wait)
double quadform_to_host(xrs_handle_t h, size_t N, const double* L, const double* V, size_t a);
// W (N x n*b): W[j, t*b + q] = P[j, t] R[j, q], the rows of the delta product E^T W (uqAdf.cpp:176-180, :199)
void khatri_rao_rows(xrs_handle_t h, size_t N, const double* P, size_t n, const double* R, size_t b, double* W);
// out (n): the mean over the N rows of S (N x n), fixed order
void column_mean(xrs_handle_t h, size_t N, const double* S, size_t n, double* out);

}  // namespace uq
}  // namespace xrs
