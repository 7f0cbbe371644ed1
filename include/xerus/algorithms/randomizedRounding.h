// Randomized rounding of TT sums: sum_rounded(terms, c, ranks, p) approximates sum_j c_j Y^(j) by a TT of the given
// ranks without ever forming the sum. Randomize-then-orthogonalize of Al Daas, Ballard, Cazeaux, Hallman, Miedlar,
// Pasha, Reid, Saibaba, "Randomized algorithms for rounding in the tensor-train format" (SISC 2023), Alg. 3.2 on a
// formal sum (§3.3). The reference library has no counterpart: its only route is operator+ followed by round, whose
// block-diagonal cores of rank sum R are orthogonalised and truncated at that rank (cost ~ d n (sum R)^3).
//
// With cores Y^(j)_k (R^(j)_k, n_k, R^(j)_{k+1}), sketch ranks l_k = ranks[k-1] + oversampling[k-1] (l_0 = l_d = 1),
// H(.) the horizontal (r x n r') and V(.) the vertical (r n x r') unfolding:
//   random TT   Omega_k (l_k, n_k, l_{k+1}), k = 1 .. d-1, Gaussian;
//   pass 1      right to left, each term on its own: W^(j)_d = 1, W^(j)_k = H(Y^(j)_k x_3 W^(j)_{k+1}) H(Omega_k)^T;
//   pass 2      left to right, X^(j)_0 = c_j Y^(j)_0:  Z = sum_j V(X^(j)_k) W^(j)_{k+1},  Q = qr(Z) is core k,
//               M^(j) = Q^T V(X^(j)_k),  X^(j)_{k+1} = M^(j) x_1 Y^(j)_{k+1};  the last core is sum_j M^(j) Y^(j)_{d-1};
//   then round(ranks). Cost O(s d n R^2 l) for s terms of rank R; the only factorisations are QRs of (l n) x l matrices.
//
// MI355X realisation: xrs_tt_round_randomized (tt_rand.hip). The sums over j are one kernel, xrs_gemm_ksum
// (gemm_ksum.hip), that contracts operands living in different allocations; the per-term products of equal shape
// share batched launches; the QR is xrs_qr (CholeskyQR2 on the certified path). DESIGN §3.12.
//
// Deviations from the paper's text:
//   - l_k is capped, left to right, by the product of the modes on either side of edge k, by sum_j R^(j)_k and by
//     l_{k-1} n_{k-1}: more sketch columns than Z has rows or the sum has rank add nothing;
//   - Omega is not normalised (the paper scales its cores by 1 / sqrt of their size): the scaling cancels in Q;
//   - the normals come from the device generator: Omega_k as an l_k x (n_k l_{k+1}) matrix is the leading block of
//     G(seed, stream = k) (philox.hpp), not of misc::randomEngine's normal stream. One 64-bit word is drawn from
//     misc::randomEngine per call and is the seed, so seeding the engine makes a call reproducible and two calls in
//     a row differ. |G| <= 6.66 (Box-Muller on 32-bit uniforms);
//   - the closing deterministic round(ranks) is part of the call (the paper returns the rank-l sketch result).
// Where l_k exceeds the exact rank of the k-th unfolding of the sum, Z is rank deficient by construction and xrs_qr
// takes its verified Householder route: correct, and slow, as for randomTTSVD.
#pragma once
#include <vector>

#include "../ttNetwork.h"

namespace xerus {

/// sum_j _coefficients[j] _terms[j] rounded to _ranks. All terms have the same dimensions; _coefficients has one
/// entry per term; _ranks (>= 1) and _oversampling have degree - 1 entries each. The result is what round(_ranks)
/// leaves of the sketch result: canonicalized, core at 0.
TTTensor sum_rounded(const std::vector<TTTensor>& _terms, const std::vector<value_t>& _coefficients,
                     const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling);
/// the same on the TT view of the operators (degree / 2 cores of mode size n_k m_k)
TTOperator sum_rounded(const std::vector<TTOperator>& _terms, const std::vector<value_t>& _coefficients,
                       const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling);

/// sum_rounded of the one term _x with coefficient 1: a randomized round(_ranks)
TTTensor round_randomized(const TTTensor& _x, const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling);
TTOperator round_randomized(const TTOperator& _x, const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling);

}  // namespace xerus
