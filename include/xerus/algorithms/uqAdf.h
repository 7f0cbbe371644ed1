// UQ-ADF (reference include/xerus/algorithms/uqAdf.h, src/xerus/algorithms/uqAdf.cpp:40-477): reconstructs a
// TT surrogate x(space, xi_1 .. xi_{d-1}) of a parametric problem from N sampled solutions. Mode 0 is the
// physical one; every further mode is expanded in the probabilists' Hermite polynomials of one random variable.
// One component at a time takes a projected-gradient step, the others kept orthogonal (move_core with keepRank).
//
// MI355X realisation: the reference's loops over the samples (OpenMP, uqAdf.cpp:117-262) are device launches
// over all N samples. Per core position a sample carries a vector stack (N x r, the rank-one stacks of ADF), an
// r x r matrix stack (N x r x r) and a quadratic form; the random variables, the basis matrices and the
// solutions are uploaded once, and the host reads back only the scalars of a step.
#pragma once
#include <utility>
#include <vector>

#include "../tensor.h"
#include "../ttNetwork.h"

namespace xerus {

class UQMeasurementSet {
   public:
    std::vector<std::vector<double>> randomVectors;
    std::vector<Tensor> solutions;

    std::vector<std::vector<double>> initialRandomVectors;
    std::vector<Tensor> initialSolutions;

    UQMeasurementSet() = default;
    UQMeasurementSet(const UQMeasurementSet& _other) = default;

    void add(const std::vector<double>& _rndvec, const Tensor& _solution);
    void add_initial(const std::vector<double>& _rndvec, const Tensor& _solution);
};

/// the basis values He_0(v) .. He_{polyDegree-1}(v): He_0 = 1, He_1 = v, He_{i+1} = v He_i - i He_{i-1}
/// (the reference's boost hermite(i, v / sqrt 2) / 2^(i/2), uqAdf.cpp:40-52)
Tensor randVar_to_position(const double _v, const size_t _polyDegree);

/// fits _x to the samples (uqAdf.cpp:327-331): at most 1000 iterations, stops when the relative residual fell
/// by less than 1 % over the last ten
void uq_adf(TTTensor& _x, const std::vector<std::vector<double>>& _randomVariables, const std::vector<Tensor>& _solutions);

/// extension (the reference hard-codes 1000 iterations): at most _maxIterations (0: no limit); _residualHistory,
/// when given, receives the relative residual computed at core 0 of every iteration
void uq_adf(TTTensor& _x, const std::vector<std::vector<double>>& _randomVariables, const std::vector<Tensor>& _solutions,
            const size_t _maxIterations, std::vector<double>* _residualHistory);

/// with initial measurements: starts from their mean and linear terms, rounded at 0.00025 (uqAdf.cpp:338-405);
/// without: from _guess
TTTensor uq_adf(const UQMeasurementSet& _measurments, const TTTensor& _guess);

/// the same with the iteration limit and residual history of the extended overload above
TTTensor uq_adf(const UQMeasurementSet& _measurments, const TTTensor& _guess, const size_t _maxIterations,
                std::vector<double>* _residualHistory);

/// _N samples of _x at standard normal random vectors (0.3 x for the first _numSpecial stochastic modes) from a
/// default-seeded std::mt19937_64 (uqAdf.cpp:425-448); all samples are evaluated in one batched device pass
std::pair<std::vector<std::vector<double>>, std::vector<Tensor>> uq_mc(const TTTensor& _x, const size_t _N, const size_t _numSpecial);

/// the mean of those samples (uqAdf.cpp:451-477), reduced on the device in a fixed order
Tensor uq_avg(const TTTensor& _x, const size_t _N, const size_t _numSpecial);

}  // namespace xerus
