// Riemannian steepest descent on TT tensors (reference include/xerus/algorithms/steepestDescent.h:34-138,
// src/xerus/algorithms/steepestDescent.cpp:37-178): minimises ||A x - b|| or ||x - b|| by gradient steps
// followed by a retraction onto the manifold of the ranks of x, with step doubling and backtracking.
// As with ALSVariant, the PerformanceData argument of the reference is not carried.
#pragma once
#include <functional>

#include "../ttNetwork.h"
#include "retractions.h"

namespace xerus {

/// line search of the geometric CG (steepestDescent.cpp:37-80): shrinks _alpha by _changeInAlpha while the
/// residual improves, then Armijo backtracking with the constant 1e-4
void line_search(TTTensor& _x, value_t& _alpha, const TTTangentVector& _direction, value_t _derivative, value_t& _residual,
                 std::function<void(TTTensor&, const TTTangentVector&)> _retraction, std::function<value_t()> _calculate_residual,
                 value_t _changeInAlpha = 0.5);

/// Wrapper class for all steepest descent variants (only for TTTensors)
class SteepestDescentVariant {
   protected:
    double solve(const TTOperator* _Ap, TTTensor& _x, const TTTensor& _b, size_t _numSteps, value_t _convergenceEpsilon) const;

   public:
    size_t numSteps;               ///< maximum number of steps to perform. set to 0 for infinite
    value_t convergenceEpsilon;    ///< change in the residual at which the algorithm assumes it is converged
    bool assumeSymmetricPositiveDefiniteOperator;   ///< calculates the gradient as b-Ax instead of A^T(b-Ax)
    TTOperator* preconditioner;

    TTRetractionII retraction;     ///< the retraction from point + change to a new point on the manifold

    /// fully defining constructor
    SteepestDescentVariant(size_t _numSteps, value_t _convergenceEpsilon, bool _symPosOp, TTRetractionII _retraction)
        : numSteps(_numSteps), convergenceEpsilon(_convergenceEpsilon), assumeSymmetricPositiveDefiniteOperator(_symPosOp),
          preconditioner(nullptr), retraction(_retraction) {}

    /// definition using only the retraction: an operator() with a convergenceEpsilon or numSteps must be used
    SteepestDescentVariant(TTRetractionII _retraction)
        : numSteps(0), convergenceEpsilon(0.0), assumeSymmetricPositiveDefiniteOperator(false), preconditioner(nullptr),
          retraction(_retraction) {}

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

/// default variant of the steepest descent algorithm (steepestDescent.cpp:178)
extern const SteepestDescentVariant SteepestDescent;

}  // namespace xerus
