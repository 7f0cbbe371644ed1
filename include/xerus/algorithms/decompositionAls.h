// decomposition_als (reference include/xerus/algorithms/decompositionAls.h:30, src/xerus/algorithms/
// decompositionAls.cpp:36-65): fits a TT of fixed ranks to a dense tensor by alternating exact local solves.
// With the core at pos and every other component orthogonal, the minimiser of ||x - b|| over component pos is the
// projection  (left interface)^T b (right interface)^T;  a sweep visits 0 .. d-1 and then d-2 .. 1.
//
// MI355X realisation: the two interfaces are built as matrices by GEMMs over the orthogonal cores and applied to
// b by two more (the reference contracts the chopped networks through its indexed layer: the same tensor).
#pragma once
#include "../ttNetwork.h"

namespace xerus {

/// Sweeps until the residual ||x - b|| is below EPSILON, its relative decrease over a sweep below _eps, or
/// _maxIterations sweeps are done. _x keeps its ranks; it ends canonicalized with the core at 1 (d >= 3).
void decomposition_als(TTTensor& _x, const Tensor& _b, const double _eps = EPSILON, const size_t _maxIterations = 1000);

}  // namespace xerus
