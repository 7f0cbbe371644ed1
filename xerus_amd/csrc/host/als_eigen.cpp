// ALS_EIGEN: the lowest eigenpair of a symmetric TTOperator by a single-site sweep (algorithms/alsEigen.h). The loop
// is ALSVariant::solve's (als.cpp) with the local linear system replaced by the local eigenproblem: core to site 0,
// x normalised, the right stack of symmetric-form environments built once, then per site xrs_als_local_eig
// (als_eig.hip: matrix-free LOBPCG on opLeft.back(), the operator core and opRight.back(), started from the
// current component), a core move with keepRank and one environment update. The component is the orthogonality
// centre, so its norm is ||x|| and the local Rayleigh quotient is <x, A x>: lambda is the theta of the half
// sweep's last site. Boundary components of full rank are not folded away (they are ordinary local problems here).
#include <cmath>
#include <cstdio>

#include "xerus_amd.h"   // (before xerus.h: gpu::handle() returns the C-ABI's handle type)
#include "xerus.h"
#include "xerus/algorithms/alsEigen.h"

namespace xerus {

namespace {

// the lowest eigenpair of the local operator at _pos replaces the component; returns theta
double solve_local(const ALSEigenVariant& _variant, const TTOperator& _A, TTTensor& _x, size_t _pos, Tensor _L, Tensor _R) {
    Tensor Ak = _A.get_component(_pos);
    Tensor xk = _x.get_component(_pos);
    const size_t rl = xk.dimensions[0], n = xk.dimensions[1], rr = xk.dimensions[2];
    const size_t pl = Ak.dimensions[0], pr = Ak.dimensions[3];
    // the tensors' lazy factors are applied into copies first (copy-on-write: no copy where the factor is 1)
    const auto applied = [](Tensor& _t) {
        _t.apply_factor();
        return _t.device_data();
    };
    const double* Ld = applied(_L);
    const double* Ad = applied(Ak);
    const double* Rd = applied(_R);
    double* xd = xk.device_data_applied();
    double theta = 0.0, relres = 0.0;
    size_t iters = 0;
    int status = 0;
    const int st = xrs_als_local_eig(gpu::handle(), xd, rl, n, rr, pl, pr, Ld, Ad, Rd, _variant.localTolerance,
                                     _variant.localMaxIterations, 16, &theta, &iters, &relres, &status);
    if (st != XRS_OK) throw misc::generic_error(xrs_last_error());
    if (status == XRS_EIG_BREAKDOWN) {
        throw misc::generic_error() << "ALS_EIGEN: the local eigenproblem at site " << _pos << " broke down after " << iters
                                    << " iterations (a zero start, or an operator or tensor with entries that are not finite)";
    }
    if (status == XRS_EIG_MAX_ITER) {
        std::fprintf(stderr, "[xerus_amd warning] ALS_EIGEN: LOBPCG at site %zu stopped after %zu iterations at relative residual %.3e (tolerance %.3e)\n",
                     _pos, iters, relres, double(_variant.localTolerance));
    }
    _x.set_component(_pos, std::move(xk));
    return theta;
}

}  // namespace

double ALSEigenVariant::solve(const TTOperator& _A, TTTensor& _x, size_t _numHalfSweeps, value_t _convergenceEpsilon) const {
    _x.require_correct_format();
    _A.require_correct_format();
    XERUS_REQUIRE(_x.degree() > 0, "ALS_EIGEN: x must have at least one mode");
    XERUS_REQUIRE(_A.dimensions.size() == _x.dimensions.size() * 2,
                  "ALS_EIGEN: degree mismatch: A has " << _A.dimensions.size() << " modes, x has " << _x.dimensions.size());
    for (size_t i = 0; i < _x.dimensions.size(); ++i) {
        XERUS_REQUIRE(_A.dimensions[i] == _x.dimensions[i] && _A.dimensions[i + _A.degree() / 2] == _x.dimensions[i],
                      "ALS_EIGEN: dimension mismatch at mode " << i << ": A is " << _A.dimensions[i] << " x "
                                                               << _A.dimensions[i + _A.degree() / 2] << ", x has " << _x.dimensions[i]);
    }
    const size_t d = _x.degree();
    const bool canonicalizeAtTheEnd = _x.canonicalized;
    const size_t corePosAtTheEnd = _x.corePosition;

    _x.move_core(0, true);
    const value_t norm = frob_norm(_x.get_component(0));
    if (norm > 0.0 && std::isfinite(norm)) _x /= norm;   // (else the first local problem reports the breakdown)

    std::vector<Tensor> opLeft(1, Tensor::ones({1, 1, 1})), opRight(1, Tensor::ones({1, 1, 1}));
    for (size_t i = d - 1; i > 0; --i) opRight.push_back(internal::als_env_step_right(opRight.back(), _x.get_component(i), _A.get_component(i)));

    size_t pos = 0, halfSweepCount = 0;
    bool increasing = true;
    value_t lastEnergy2 = 1e102, lastEnergy = 1e101, energy = 1e100;
    while (true) {
        const value_t theta = solve_local(*this, _A, _x, pos, opLeft.back(), opRight.back());
        if (d == 1 || (increasing ? pos == d - 1 : pos == 0)) {
            halfSweepCount += 1;
            lastEnergy2 = lastEnergy;
            lastEnergy = energy;
            energy = theta;
            if (d == 1 || halfSweepCount == _numHalfSweeps || std::abs(lastEnergy - energy) < _convergenceEpsilon ||
                std::abs(lastEnergy2 - energy) < _convergenceEpsilon) {
                if (canonicalizeAtTheEnd && preserveCorePosition) _x.move_core(corePosAtTheEnd, true);
                return energy;
            }
            increasing = !increasing;
        }
        if (increasing) {
            _x.move_core(pos + 1, true);
            opRight.pop_back();
            opLeft.push_back(internal::als_env_step_left(opLeft.back(), _x.get_component(pos), _A.get_component(pos)));
            ++pos;
        } else {
            _x.move_core(pos - 1, true);
            opLeft.pop_back();
            opRight.push_back(internal::als_env_step_right(opRight.back(), _x.get_component(pos), _A.get_component(pos)));
            --pos;
        }
    }
}

const ALSEigenVariant ALS_EIGEN(0, 1e-6, true);

}  // namespace xerus
