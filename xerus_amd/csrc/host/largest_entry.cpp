// find_largest_entry (reference src/xerus/algorithms/largestEntry.cpp:6-54) and what it stands on here:
// TTTensor::operator[] (the reference's TTNetwork reads entries through TensorNetwork::operator[]), the
// symmetric-basis square entrywise_square (xrs_tt_entrywise_square, hadamard.hip) in place of the reference's
// entrywise_product(X, X), and the positions of a rank-one TT in one launch (xrs_tt_rank_one_argmax).
// soft_threshold, round, frob_norm are the existing TT drivers.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "measurement_device.hpp"

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

// the row-major position of the entry of largest modulus of a TT of ranks 1 (largestEntry.cpp:38-53): per
// component the first index of largest |.|
size_t rank_one_position(const TTTensor& _T) {
    const size_t d = _T.degree();
    if (d == 0) return 0;
    std::vector<Tensor> applied;   // private copies of the components that carry a factor
    applied.reserve(d);
    std::vector<const double*> cores(d);
    for (size_t k = 0; k < d; ++k) {
        const Tensor& c = _T.get_component(k);
        if (c.has_factor()) {
            applied.push_back(c);
            cores[k] = applied.back().device_data_applied();
        } else {
            cores[k] = c.device_data();
        }
    }
    std::vector<size_t> pos(d);
    guard([&] {
        const int st = xrs_tt_rank_one_argmax(gpu::handle(), d, _T.dimensions.data(), cores.data(), pos.data());
        if (st != XRS_OK) throw xrs::Error{st, xrs_last_error()};
    });
    size_t position = 0;
    for (size_t k = 0; k < d; ++k) position = position * _T.dimensions[k] + pos[k];
    return position;
}

size_t rank_sum(const TTTensor& _T) {
    const std::vector<size_t> r = _T.ranks();
    return std::accumulate(r.begin(), r.end(), size_t(0));
}

}  // namespace

// ------------------------------------------------------------------------------------------ operator[]
value_t TTTensor::operator[](const std::vector<size_t>& _positions) const {
    require_correct_format();
    XERUS_REQUIRE(_positions.size() == degree(), "Wrong number of given positions: " << _positions.size() << " for degree " << degree());
    if (degree() == 0) return components[0][0];
    for (size_t k = 0; k < degree(); ++k)
        XERUS_REQUIRE(_positions[k] < dimensions[k], "Position " << _positions[k] << " of mode " << k << " exceeds dimension " << dimensions[k]);
    SinglePointMeasurementSet set;
    set.add(_positions, 0.0);
    return guard([&] {
        const internal::DeviceMeasurements dm(set, dimensions);
        return internal::evaluate_tt(*this, dm)[0];
    });
}

value_t TTTensor::operator[](const size_t _position) const {
    return (*this)[Tensor::position_to_multiIndex(_position, dimensions)];
}

// ------------------------------------------------------------------------------------------ entrywise_square
TTTensor entrywise_square(const TTTensor& _A) {
    _A.require_correct_format();
    const size_t d = _A.degree();
    if (d == 0) {
        TTTensor result(_A);
        result *= _A.components[0][0];
        return result;
    }
    std::vector<size_t> r(d + 1, 1), rs(d + 1, 1);
    std::vector<const double*> pa(d);
    value_t alpha = 1.0;
    for (size_t k = 0; k < d; ++k) {
        r[k + 1] = _A.components[k].dimensions[2];
        pa[k] = _A.components[k].device_data();
        alpha *= _A.components[k].factor * _A.components[k].factor;
    }
    std::vector<double*> out(d, nullptr);
    guard([&] {
        const int st = xrs_tt_entrywise_square(gpu::handle(), d, _A.dimensions.data(), r.data(), pa.data(), alpha, out.data(), rs.data());
        if (st != XRS_OK) throw xrs::Error{st, xrs_last_error()};
    });
    TTTensor result(_A.dimensions);
    for (size_t k = 0; k < d; ++k) result.components[k] = Tensor::adopt_device({rs[k], _A.dimensions[k], rs[k + 1]}, out[k]);
    result.canonicalized = false;
    if (_A.canonicalized) result.move_core(_A.corePosition);
    return result;
}

TTOperator entrywise_square(const TTOperator& _A) {
    TTOperator A(_A);
    const std::vector<size_t> dims = _A.dimensions;
    return TTOperator::from_tt(entrywise_square(std::move(A).to_tt()), dims);
}

// ------------------------------------------------------------------------------------------ find_largest_entry
size_t find_largest_entry(const TTTensor& _T, const double _accuracy, const value_t _lowerBound) {
    _T.require_correct_format();
    const size_t d = _T.degree();
    if (d == 0) return 0;   // (the reference's loop would not end: no rank to reduce)

    // There is actual work to be done (largestEntry.cpp:10)
    if (rank_sum(_T) >= d) {
        const double alpha = _accuracy;
        const auto usable = [](double _norm) { return std::isfinite(_norm) && _norm > 0.0; };
        XERUS_REQUIRE(usable(_T.frob_norm()), "find_largest_entry: the norm of the tensor is zero or not finite");

        TTTensor X = _T;
        X.round(size_t(1));
        double Xn = std::max(_T[find_largest_entry(X, 0.0, 0.0)], _lowerBound);
        double tau = (1 - alpha) * alpha * Xn * Xn / (2.0 * double(d - 1));

        X = _T;
        size_t iterations = 0;
        while (rank_sum(X) >= d) {
            XERUS_REQUIRE(iterations++ < 1000, "find_largest_entry: no rank-one iterate after 1000 iterations");
            X = entrywise_square(X);   // (the reference: entrywise_product(X, X), :20)

            X.soft_threshold(tau, true);

            TTTensor Y = X;
            Y.round(size_t(1));
            const size_t yMaxPos = find_largest_entry(Y, 0.0, 0.0);

            Xn = std::max(X[yMaxPos], (1 - (1 - alpha) * alpha / 2.0) * Xn * Xn);

            const double fNorm = X.frob_norm();
            XERUS_REQUIRE(usable(fNorm), "find_largest_entry: the norm of the iterate is zero or not finite (" << fNorm << ")");
            Xn /= fNorm;
            X /= fNorm;
            tau = (1 - alpha) * alpha * Xn * Xn / (2.0 * double(d - 1));
        }
        return rank_one_position(X);
    }
    // We are already rank one (:37-53)
    return rank_one_position(_T);
}

size_t find_largest_entry(const TTOperator& _T, const double _accuracy, const value_t _lowerBound) {
    _T.require_correct_format();
    const size_t d = _T.degree() / 2;
    TTOperator copy(_T);
    size_t merged = find_largest_entry(std::move(copy).to_tt(), _accuracy, _lowerBound);
    // merged position over the modes (n_k m_k) -> (i_0 .. i_{d-1}, j_0 .. j_{d-1}) row-major
    std::vector<size_t> idx(2 * d);
    for (size_t k = d; k-- > 0;) {
        const size_t nk = _T.dimensions[k], mk = _T.dimensions[d + k];
        const size_t c = merged % (nk * mk);
        merged /= nk * mk;
        idx[k] = c / mk;
        idx[d + k] = c % mk;
    }
    size_t position = 0;
    for (size_t k = 0; k < 2 * d; ++k) position = position * _T.dimensions[k] + idx[k];
    return position;
}

}  // namespace xerus
