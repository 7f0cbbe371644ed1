// Geometric (Riemannian) conjugate gradients on TT tensors (reference include/xerus/algorithms/cg.h:33-138,
// src/xerus/algorithms/cg.cpp:38-126): projected gradients as TTTangentVectors, line search along a retraction
// of type I, transported directions, Fletcher-Reeves update.
// As with ALSVariant, the PerformanceData argument of the reference is not carried.
#pragma once
#include "../ttNetwork.h"
#include "retractions.h"
#include "steepestDescent.h"

namespace xerus {

/// Wrapper class for all geometric CG variants (only for TTTensors)
class GeometricCGVariant {
   protected:
    double solve(const TTOperator* _Ap, TTTensor& _x, const TTTensor& _b, size_t _numSteps, value_t _convergenceEpsilon) const;

   public:
    size_t numSteps;               ///< maximum number of steps to perform. set to 0 for infinite
    value_t convergenceEpsilon;    ///< change in the residual at which the algorithm assumes it is converged
    bool assumeSymmetricPositiveDefiniteOperator;   ///< calculates the gradient as b-Ax instead of A^T(b-Ax)

    TTRetractionI retraction;            ///< the retraction from point + tangent vector to a new point on the manifold
    TTVectorTransport vectorTransport;   ///< the vector transport from the old tangent space to the new one

    /// fully defining constructor
    GeometricCGVariant(size_t _numSteps, value_t _convergenceEpsilon, bool _symPosOp, TTRetractionI _retraction,
                       TTVectorTransport _vectorTransport)
        : numSteps(_numSteps), convergenceEpsilon(_convergenceEpsilon), assumeSymmetricPositiveDefiniteOperator(_symPosOp),
          retraction(_retraction), vectorTransport(_vectorTransport) {}

    /// definition using only the retraction: an operator() with a convergenceEpsilon or numSteps must be used
    GeometricCGVariant(TTRetractionI _retraction, TTVectorTransport _vectorTransport)
        : numSteps(0), convergenceEpsilon(0.0), assumeSymmetricPositiveDefiniteOperator(false), retraction(_retraction),
          vectorTransport(_vectorTransport) {}

    /// solve A x = b (least squares); returns the residual |Ax-b| of the final x
    double operator()(const TTOperator& _A, TTTensor& _x, const TTTensor& _b, value_t _convergenceEpsilon) const {
        return solve(&_A, _x, _b, numSteps, _convergenceEpsilon);
    }
    double operator()(const TTOperator& _A, TTTensor& _x, const TTTensor& _b, size_t _numSteps) const {
        return solve(&_A, _x, _b, _numSteps, convergenceEpsilon);
    }
    double operator()(const TTOperator& _A, TTTensor& _x, const TTTensor& _b) const {
        return solve(&_A, _x, _b, numSteps, convergenceEpsilon);
    }
    /// minimise ||x - b||; returns the residual |x-b| of the final x
    double operator()(TTTensor& _x, const TTTensor& _b, value_t _convergenceEpsilon) const {
        return solve(nullptr, _x, _b, numSteps, _convergenceEpsilon);
    }
    double operator()(TTTensor& _x, const TTTensor& _b, size_t _numSteps) const {
        return solve(nullptr, _x, _b, _numSteps, convergenceEpsilon);
    }
    double operator()(TTTensor& _x, const TTTensor& _b) const { return solve(nullptr, _x, _b, numSteps, convergenceEpsilon); }
};

/// default variant of the geometric CG (cg.cpp:126)
extern const GeometricCGVariant GeometricCG;

}  // namespace xerus
