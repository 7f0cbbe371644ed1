// randomTTSVD (reference include/xerus/algorithms/randomSVD.h:31-98, whose body is commented out upstream but
// complete): a TT approximation of a dense tensor from Gaussian sketches instead of one full SVD per mode.
// For j = d .. 2, with b the remaining (n_1 .. n_{j-1}) x (n_j r_j) matrix:
//     a = G_j b  (s_j = ranks[j-2] + oversampling[j-2] rows),   (R, Q) = rq(a),   b <- b Q^T,   component j-1 = Q;
// then component 0 = b and round(ranks). Q spans (a random s_j-dimensional part of) the row space of b, so no
// SVD of a large unfolding is ever formed; the closing round works on cores of rank s_j.
//
// MI355X realisation: G_j is never stored. xrs_sketch_gaussian generates it inside the product (philox.hpp,
// sketch.hip) -- at j = d the sketch matrix would be s_d / n_d times larger than the tensor itself.
// The RQ is xrs_rq (CholeskyQR on the certified path), b Q^T one GEMM.
//
// Deviations from the reference's text:
//   - s_j is capped at M_j = n_1 .. n_{j-1}: more sketch rows than b has rows add nothing and make a rank
//     deficient by construction;
//   - the sketch is always dense (the tensors here are; the reference's sparse branch has no counterpart);
//   - the normals come from the device generator G(seed, stream = j), not from misc::randomEngine's normal
//     stream: one 64-bit word is drawn from misc::randomEngine per call and is the seed, so seeding the engine
//     makes a call reproducible and two calls in a row differ. |G| <= 6.66 (Box-Muller on 32-bit uniforms).
// Where _x has exact TT rank below s_j the sketch is rank deficient and xrs_rq takes its one-workgroup Householder
// route: correct, and slow (DESIGN §3.9 has the measurement).
#pragma once
#include <vector>

#include "../ttNetwork.h"

namespace xerus {

/// _ranks and _oversampling: degree - 1 entries each, ranks >= 1. The result is what round(_ranks) leaves:
/// canonicalized, core at 0, ranks capped by _ranks and by the maximal TT ranks of the dimensions. Degree 1 gives
/// the tensor as the one core, degree 0 what the TT-SVD constructor gives.
TTTensor randomTTSVD(const Tensor& _x, const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling);

}  // namespace xerus
