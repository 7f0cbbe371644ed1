// find_largest_entry (reference include/xerus/algorithms/largestEntry.h, src/xerus/algorithms/largestEntry.cpp:6-54):
// the position of the entry of largest modulus of a TT without forming the dense tensor, by power iteration in
// the TT format -- X <- X o X, soft_threshold, round(1) for the running estimate, normalise -- until every rank is 1.
//
// MI355X realisation: X o X is formed in the symmetric basis (entrywise_square below, xrs_tt_entrywise_square:
// edge rank r (r + 1) / 2 instead of the r^2 of entrywise_product(X, X), whose surplus directions are exactly
// rank deficient and would have to be found and cut by the rank-revealing QC that follows); the positions of a
// rank-one TT are read by one launch and one copy (xrs_tt_rank_one_argmax); single entries of a TT are read
// through TTTensor::operator[] (the device evaluation stack of the measurement sets).
#pragma once
#include "../ttNetwork.h"

namespace xerus {

/// The row-major position (over _T.dimensions) of the entry of largest modulus, as the reference's loop
/// (largestEntry.cpp:10-36) with its constants and its termination test sum(ranks) >= degree. _accuracy is the
/// assumed ratio |second largest| / |largest|, _lowerBound a lower bound of the largest modulus. _T is not modified.
/// Deviation (iteration guard): the reference loops forever when the iteration cannot reach rank one; here a
/// generic_error is thrown after 1000 iterations, or as soon as a norm read by the loop is zero or not finite
/// (the input's norm is read once before the first round for the same reason). A degree-0 TT gives 0.
/// Cost: every iteration takes the ranks r to r (r + 1) / 2 before its threshold; where the threshold cuts
/// nothing (a small gap on a large tensor) the second square is already out of reach.
size_t find_largest_entry(const TTTensor& _T, const double _accuracy, const value_t _lowerBound = 0.0);

/// The same for an operator, on its TT view with modes n_k m_k. Deviation (position): the result is the row-major
/// position in the operator's own order (i_0 .. i_{d-1}, j_0 .. j_{d-1}), so that Tensor(_T)[position] is the entry.
/// The reference's operator branch (largestEntry.cpp:38-52) composes an interleaved position but reads
/// _T[position] in the other order, and applies the degree-2d termination test to d - 1 ranks; neither
/// inconsistency is reproduced.
size_t find_largest_entry(const TTOperator& _T, const double _accuracy, const value_t _lowerBound = 0.0);

}  // namespace xerus
