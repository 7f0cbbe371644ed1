// Riemannian optimisation on the manifold of fixed TT rank: tangent vectors, retractions, the projective
// vector transport, steepest descent and geometric CG (reference src/xerus/algorithms/retractions.cpp:30-288,
// steepestDescent.cpp:37-178, cg.cpp:38-126). The tangent-space projection, the rank-2r block TT and the
// inner product of tangent vectors are the tangent drivers of tangent.hip; everything else composes the
// TTTensor operations (sums, round, move_core, operator application) that already run on the GPU.
#include <cmath>

#include "../tt_internal.hpp"
#include "xerus.h"

namespace xerus {

namespace {

template <class F>
auto guard(F&& f) -> decltype(f()) {
    try {
        return f();
    } catch (const xrs::Error& e) {
        throw misc::generic_error(e.msg);
    }
}

// read-only device view of the cores of a TT (or of a component list): tensors with a pending scalar factor
// are replaced by private factor-applied copies that live as long as the view
struct CoreView {
    std::vector<Tensor> applied;
    std::vector<const double*> ptr;
    explicit CoreView(const std::vector<Tensor>& _cores) : ptr(_cores.size()) {
        applied.reserve(_cores.size());
        for (size_t k = 0; k < _cores.size(); ++k) {
            if (_cores[k].has_factor()) {
                applied.push_back(_cores[k]);
                applied.back().apply_factor();
                ptr[k] = applied.back().device_data();
            } else {
                ptr[k] = _cores[k].device_data();
            }
        }
    }
};

std::vector<size_t> ranks_with_ends(const TTTensor& _tt) {
    std::vector<size_t> r(_tt.degree() + 1, 1);
    for (size_t k = 0; k + 1 < _tt.degree(); ++k) r[k + 1] = _tt.get_component(k).dimensions[2];
    return r;
}

void require_components_fit(const TTTensor& _base, const std::vector<Tensor>& _components) {
    XERUS_REQUIRE(_components.size() == _base.degree(), "illegal base tensor for this tangent vector (the number of components does not coincide)");
    for (size_t k = 0; k < _components.size(); ++k)
        XERUS_REQUIRE(_base.get_component(k).dimensions == _components[k].dimensions,
                      "illegal base tensor for this tangent vector (ranks or external dimension do not coincide)");
}

}  // namespace

// ------------------------------------------------------------------------------------------ TTTangentVector
void TTTangentVector::set_base(const TTTensor& _newBase) {
    XERUS_REQUIRE(_newBase.dimensions == baseL.dimensions, "");
    baseL = _newBase;
    baseL.move_core(0, true);
    leftGrams.reset();
}

TTTangentVector::TTTangentVector(const TTTensor& _base, const TTTensor& _direction) {
    XERUS_REQUIRE(_base.canonicalized && _base.corePosition == 0,
                  "projection onto tangent plane is only implemented for core position 0 at the moment");
    XERUS_REQUIRE(_base.dimensions == _direction.dimensions, "");
    XERUS_REQUIRE(_base.degree() >= 1, "tangent vectors need a TT of degree 1 or more");
    _base.require_correct_format();
    _direction.require_correct_format();

    baseL = _base;
    baseL.move_core(0, true);

    const size_t d = baseL.degree();
    const std::vector<size_t> ru = ranks_with_ends(baseL), rz = ranks_with_ends(_direction);
    const CoreView U(baseL.components), Z(_direction.components);
    std::vector<double*> V(d, nullptr), UU(d, nullptr);
    guard([&] {
        xrs::tt::tangent_project(gpu::handle(), d, baseL.dimensions.data(), ru.data(), U.ptr.data(), rz.data(), Z.ptr.data(), V.data(),
                                 UU.data(), &fallbackEdges);
    });
    auto grams = std::make_shared<std::vector<Tensor>>();
    for (size_t k = 0; k < d; ++k) {
        components.push_back(Tensor::adopt_device({ru[k], baseL.dimensions[k], ru[k + 1]}, V[k]));
        grams->push_back(Tensor::adopt_device({ru[k], ru[k]}, UU[k]));
    }
    leftGrams = std::move(grams);
}

// UU_{k+1} = sum_i U_k[:,i,:]^T UU_k U_k[:,i,:] (retractions.cpp:99, :175), recomputed after set_base
const std::vector<Tensor>& TTTangentVector::left_grams() const {
    if (leftGrams) return *leftGrams;
    auto grams = std::make_shared<std::vector<Tensor>>();
    grams->push_back(Tensor::ones({1, 1}));
    for (size_t k = 0; k + 1 < baseL.degree(); ++k) {
        const Tensor& Uk = baseL.get_component(k);
        const Tensor T = contract(grams->back(), true, Uk, false, 1);   // (a', i, c) = sum_a UU(a, a') U(a, i, c)
        grams->push_back(contract(Uk, true, T, false, 2));              // (c', c) = sum_{a', i} U(a', i, c') T(a', i, c)
    }
    leftGrams = std::move(grams);
    return *leftGrams;
}

TTTangentVector& TTTangentVector::operator+=(const TTTangentVector& _rhs) {
    XERUS_REQUIRE(components.size() == _rhs.components.size(), "");
    for (size_t i = 0; i < components.size(); ++i) components[i] += _rhs.components[i];
    return *this;
}

TTTangentVector& TTTangentVector::operator-=(const TTTangentVector& _rhs) {
    XERUS_REQUIRE(components.size() == _rhs.components.size(), "");
    for (size_t i = 0; i < components.size(); ++i) components[i] -= _rhs.components[i];
    return *this;
}

TTTangentVector& TTTangentVector::operator*=(value_t _alpha) {
    for (auto& c : components) c *= _alpha;
    return *this;
}

TTTangentVector TTTangentVector::operator*(value_t _alpha) const {
    TTTangentVector result(*this);
    result *= _alpha;
    return result;
}

TTTangentVector operator*(value_t _alpha, const TTTangentVector& _rhs) {
    TTTangentVector result(_rhs);
    result *= _alpha;
    return result;
}

value_t TTTangentVector::scalar_product(const TTTangentVector& _other) const {
    XERUS_REQUIRE(components.size() == _other.components.size(), "");
    require_components_fit(baseL, components);
    require_components_fit(baseL, _other.components);
    const size_t d = baseL.degree();
    const std::vector<size_t> r = ranks_with_ends(baseL);
    const CoreView G(left_grams()), A(components), B(_other.components);
    return guard([&] {
        return xrs::tt::tangent_dot(gpu::handle(), d, baseL.dimensions.data(), r.data(), G.ptr.data(), A.ptr.data(), B.ptr.data());
    });
}

value_t TTTangentVector::frob_norm() const { return std::sqrt(scalar_product(*this)); }

// the rank-2r TT (retractions.cpp:186-260): every core written by one kernel, then move_core(0)
TTTensor TTTangentVector::block_tt(bool _addBase) const {
    require_components_fit(baseL, components);
    const size_t d = baseL.degree();
    const std::vector<size_t> r = ranks_with_ends(baseL);
    const CoreView U(baseL.components), V(components);
    std::vector<double*> out(d, nullptr);
    guard([&] {
        xrs::tt::tangent_to_tt(gpu::handle(), d, baseL.dimensions.data(), r.data(), U.ptr.data(), V.ptr.data(), _addBase, out.data());
    });
    TTTensor result(baseL.dimensions);
    for (size_t k = 0; k < d; ++k)
        result.components[k] =
            Tensor::adopt_device({k == 0 ? 1 : 2 * r[k], baseL.dimensions[k], k + 1 == d ? 1 : 2 * r[k + 1]}, out[k]);
    if (d == 1) {
        result.assume_core_position(0);
    } else {
        result.canonicalized = false;
        result.move_core(0);
    }
    return result;
}

TTTangentVector::operator TTTensor() const { return block_tt(false); }

TTTensor TTTangentVector::added_to_base() const { return block_tt(true); }

// ------------------------------------------------------------------------------------------ retractions
void HOSVDRetraction::operator()(TTTensor& _U, const TTTensor& _change) const {
    _U = _U + _change;
    if (roundByVector) _U.round(rankVector);
    else _U.round(rank);
}

void HOSVDRetraction::operator()(TTTensor& _U, const TTTangentVector& _change) const {
    _U = _change.added_to_base();
    if (roundByVector) _U.round(rankVector);
    else _U.round(rank);
}

void HOSVDRetractionII(TTTensor& _U, const TTTensor& _change) {
    const std::vector<size_t> oldRank = _U.ranks();
    _U = _U + _change;
    _U.round(oldRank);
}

void HOSVDRetractionI(TTTensor& _U, const TTTangentVector& _change) {
    const std::vector<size_t> oldRank = _U.ranks();
    _U = _change.added_to_base();
    _U.round(oldRank);
}

void ALSRetractionII(TTTensor& _U, const TTTensor& _change) {
    static const ALSVariant roundingALS(1, 2, ALSVariant::lapack_solver, false);
    const TTTensor target = _U + _change;
    roundingALS(_U, target);
}

void ALSRetractionI(TTTensor& _U, const TTTangentVector& _change) {
    static const ALSVariant roundingALS(1, 2, ALSVariant::lapack_solver, false);
    const TTTensor target = _change.added_to_base();
    roundingALS(_U, target);
}

void SubmanifoldRetractionII(TTTensor& _U, const TTTensor& _change) {
    const TTTangentVector W(_U, _change);
    SubmanifoldRetractionI(_U, W);
}

void SubmanifoldRetractionI(TTTensor& _U, const TTTangentVector& _change) {
    XERUS_REQUIRE(_change.components.size() == _U.degree(), "");
    for (size_t i = 0; i < _U.degree(); ++i) _U.set_component(i, _U.get_component(i) + _change.components[i]);
    _U.move_core(0, true);
}

void ProjectiveVectorTransport(const TTTensor& _newBase, TTTangentVector& _tangentVector) {
    XERUS_REQUIRE(_newBase.canonicalized && _newBase.corePosition == 0, "Tangent vectors only implemented for core position 0 atm");
    _tangentVector = TTTangentVector(_newBase, TTTensor(_tangentVector));
}

// ------------------------------------------------------------------------------------------ steepest descent
void line_search(TTTensor& _x, value_t& _alpha, const TTTangentVector& _direction, value_t _derivative, value_t& _residual,
                 std::function<void(TTTensor&, const TTTangentVector&)> _retraction, std::function<value_t()> _calculate_residual,
                 value_t _changeInAlpha) {
    const value_t dirNorm = _direction.frob_norm();
    value_t currAlpha = _alpha / _changeInAlpha;
    const TTTensor oldX(_x);
    _retraction(_x, currAlpha / dirNorm * _direction);
    value_t bestResidual = _calculate_residual();
    value_t bestAlpha = currAlpha;
    TTTensor bestX = _x;

    do {
        currAlpha *= _changeInAlpha;
        _x = oldX;
        _retraction(_x, currAlpha / dirNorm * _direction);
        const value_t newResidual = _calculate_residual();
        if (newResidual < bestResidual) {
            bestResidual = newResidual;
            bestAlpha = currAlpha;
            bestX = _x;
        } else {
            break;
        }
    } while (true);

    _x = std::move(bestX);
    _alpha = bestAlpha;

    // armijo backtracking
    const value_t min_decrease = 1e-4;
    while (_alpha > 1e-16 && bestResidual > _residual - min_decrease * _alpha / dirNorm * _derivative) {
        _alpha *= _changeInAlpha;
        _x = oldX;
        _retraction(_x, _alpha / dirNorm * _direction);
        bestResidual = _calculate_residual();
    }

    _residual = bestResidual;
}

double SteepestDescentVariant::solve(const TTOperator* _Ap, TTTensor& _x, const TTTensor& _b, size_t _numSteps,
                                     value_t _convergenceEpsilon) const {
    const Index i, j;
    size_t stepCount = 0;
    TTTensor residual;
    value_t lastResidual = 1e100;
    value_t currResidual = 1e100;

    auto updateResidual = [&]() {
        if (_Ap != nullptr) {
            TTTensor Ax;
            Ax(i & 0) = (*_Ap)(i / 2, j / 2) * _x(j & 0);
            residual = _b - Ax;
        } else {
            residual = _b - _x;
        }
        currResidual = frob_norm(residual);
    };
    updateResidual();

    TTTensor y;
    value_t alpha = 1;
    while ((_numSteps == 0 || stepCount < _numSteps) && currResidual > _convergenceEpsilon &&
           std::abs(lastResidual - currResidual) > _convergenceEpsilon &&
           std::abs(1 - currResidual / lastResidual) > _convergenceEpsilon) {
        stepCount += 1;

        if (_Ap != nullptr) {
            if (assumeSymmetricPositiveDefiniteOperator) {
                y = residual;   // search direction: y = b-Ax
            } else {
                TTTensor g;     // search direction: y = A^T(b-Ax)
                g(i & 0) = (*_Ap)(j / 2, i / 2) * residual(j & 0);
                y = std::move(g);
            }
            if (preconditioner != nullptr) {
                TTTensor py;
                py(j & 0) = (*preconditioner)(j / 2, i / 2) * y(i & 0);
                y = std::move(py);
            }
        } else {
            y = residual;
        }

        const TTTensor oldX(_x);
        alpha *= 2;
        retraction(_x, y * alpha);
        lastResidual = currResidual;
        updateResidual();
        // armijo backtracking
        while (alpha > 1e-30 && lastResidual < currResidual) {
            alpha /= 2;
            _x = oldX;
            retraction(_x, y * alpha);
            updateResidual();
        }
    }

    return currResidual;
}

const SteepestDescentVariant SteepestDescent(0, 1e-8, false, SubmanifoldRetractionII);

// ------------------------------------------------------------------------------------------ geometric CG
double GeometricCGVariant::solve(const TTOperator* _Ap, TTTensor& _x, const TTTensor& _b, size_t _numSteps,
                                 value_t _convergenceEpsilon) const {
    const Index i, j;
    size_t stepCount = 0;
    TTTensor residual;
    TTTangentVector gradient;
    value_t gradientNorm = 1.0;
    value_t lastResidual = 1e100;
    value_t currResidual = 1e100;
    const value_t normB = frob_norm(_b);

    auto calculateResidual = [&]() -> value_t {
        if (_Ap != nullptr) {
            TTTensor Ax;
            Ax(i & 0) = (*_Ap)(i / 2, j / 2) * _x(j & 0);
            residual = _b - Ax;
        } else {
            residual = _b - _x;
        }
        return frob_norm(residual);
    };
    auto updateGradient = [&]() {
        if (assumeSymmetricPositiveDefiniteOperator || (_Ap == nullptr)) {
            gradient = TTTangentVector(_x, residual);
        } else {
            TTTensor grad;
            grad(i & 0) = (*_Ap)(j / 2, i / 2) * residual(j & 0);   // grad = A^T * (b - Ax)
            gradient = TTTangentVector(_x, grad);
        }
        gradientNorm = gradient.frob_norm();
    };

    currResidual = calculateResidual();

    updateGradient();
    TTTangentVector direction = gradient;
    value_t alpha = 1;
    while ((_numSteps == 0 || stepCount < _numSteps) && currResidual / normB > _convergenceEpsilon &&
           std::abs(lastResidual - currResidual) / normB > _convergenceEpsilon &&
           std::abs(1 - currResidual / lastResidual) / normB > _convergenceEpsilon) {
        stepCount += 1;

        // check the derivative along the current direction
        value_t derivative = gradient.scalar_product(direction) / direction.frob_norm();

        // if movement in the given direction would increase the residual rather than decrease it, perform one
        // steepest descent step instead
        if (derivative <= 0) {
            direction = gradient;
            derivative = gradient.frob_norm();
            alpha = 1;
        }

        line_search(_x, alpha, direction, derivative, currResidual, retraction, calculateResidual, 0.8);

        TTTangentVector oldDirection(direction);
        vectorTransport(_x, oldDirection);
        const value_t oldGradNorm = gradientNorm;
        updateGradient();

        const double beta = gradientNorm / oldGradNorm;   // Fletcher-Reeves update
        direction = gradient;
        direction += oldDirection * beta;
    }

    return currResidual;
}

const GeometricCGVariant GeometricCG(0, 1e-8, false, SubmanifoldRetractionI, ProjectiveVectorTransport);

}  // namespace xerus
