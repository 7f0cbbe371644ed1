// Lowest eigenpair of a symmetric TTOperator by a single-site alternating sweep (not in the reference): the
// smallest algebraic eigenvalue lambda and a unit TT eigenvector x of fixed ranks, i.e. the minimiser of the Rayleigh
// quotient <x, A x> / <x, x> over the TT manifold of x's ranks (the ground state of a Hamiltonian, the smallest mode
// of a discretised operator).
//
// The sweep is ALS's: the core moves site by site with keepRank, the environments <x, A x> are cached as stacks,
// and at each site the lowest eigenpair of the local operator replaces the component. The local operator is never
// assembled: it is applied through the two environments and the operator core (the GEMM chain of
// xrs_als_local_apply) inside a LOBPCG iteration that stays on the device (xrs_als_local_eig), started from the
// current component -- so every local step starts inside its own search space and lambda never increases.
#pragma once
#include "../ttNetwork.h"

namespace xerus {

class ALSEigenVariant {
   public:
    size_t numHalfSweeps;             ///< 0: no limit
    value_t convergenceEpsilon;       ///< stop when lambda changed by less than this over one or two half sweeps
    bool preserveCorePosition;        ///< move the core back to where a canonicalized x had it
    /// The local eigenpair is found to this relative residual ||M x - theta x|| <= tol ||M x0|| (x0 the component
    /// the local step starts from), not to rounding.
    value_t localTolerance = 1e-10;
    size_t localMaxIterations = 0;    ///< 0: the cap 4 N + 50, N the size of the component

    ALSEigenVariant(size_t _numHalfSweeps, value_t _convergenceEpsilon, bool _preserveCorePosition)
        : numHalfSweeps(_numHalfSweeps), convergenceEpsilon(_convergenceEpsilon), preserveCorePosition(_preserveCorePosition) {}

    /// _A must be symmetric (not checked; for the largest eigenvalue pass -_A). _x: in the start (any non-zero TT
    /// tensor of the wanted ranks), out the unit eigenvector approximation of the same ranks. Returns the Rayleigh
    /// quotient lambda = <x, A x> of the returned x.
    double operator()(const TTOperator& _A, TTTensor& _x, value_t _convergenceEpsilon) const {
        return solve(_A, _x, numHalfSweeps, _convergenceEpsilon);
    }
    double operator()(const TTOperator& _A, TTTensor& _x, size_t _numHalfSweeps) const {
        return solve(_A, _x, _numHalfSweeps, convergenceEpsilon);
    }
    double operator()(const TTOperator& _A, TTTensor& _x) const { return solve(_A, _x, numHalfSweeps, convergenceEpsilon); }

    double solve(const TTOperator& _A, TTTensor& _x, size_t _numHalfSweeps, value_t _convergenceEpsilon) const;
};

/// numHalfSweeps 0, convergenceEpsilon 1e-6, preserveCorePosition true (the defaults of ALS)
extern const ALSEigenVariant ALS_EIGEN;

}  // namespace xerus
