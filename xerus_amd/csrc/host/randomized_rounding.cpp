// sum_rounded / round_randomized (include/xerus/algorithms/randomizedRounding.h): the arguments are checked, the
// component factors folded into the coefficients, and the two passes run on the device (xrs_tt_round_randomized,
// tt_rand.hip); the cores it returns are adopted and round(ranks) closes the call.
#include <algorithm>

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

}  // namespace

TTTensor sum_rounded(const std::vector<TTTensor>& _terms, const std::vector<value_t>& _coefficients,
                     const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling) {
    XERUS_REQUIRE(!_terms.empty(), "sum_rounded needs at least one term");
    XERUS_REQUIRE(_coefficients.size() == _terms.size(),
                  "We need " << _terms.size() << " coefficients but " << _coefficients.size() << " where given");
    const size_t d = _terms[0].degree();
    const size_t numRanks = d == 0 ? 0 : d - 1;
    XERUS_REQUIRE(_ranks.size() == numRanks, "We need " << numRanks << " ranks but " << _ranks.size() << " where given");
    XERUS_REQUIRE(_oversampling.size() == numRanks,
                  "We need " << numRanks << " oversampling parameters but " << _oversampling.size() << " where given");
    XERUS_REQUIRE(std::find(_ranks.begin(), _ranks.end(), size_t(0)) == _ranks.end(), "Ranks must be strictly positive.");
    for (const TTTensor& t : _terms) {
        t.require_correct_format();
        XERUS_REQUIRE(t.dimensions == _terms[0].dimensions, "The dimensions of the terms must coincide");
    }
    if (d == 0) {
        TTTensor result(_terms[0]);
        value_t sum = 0.0;
        for (size_t j = 0; j < _terms.size(); ++j) sum += _coefficients[j] * _terms[j].components[0][0];
        result.components[0][0] = sum;
        return result;
    }

    const size_t s = _terms.size();
    std::vector<size_t> ell(numRanks);
    for (size_t k = 0; k < numRanks; ++k) {
        ell[k] = _ranks[k] + _oversampling[k];
        XERUS_REQUIRE(ell[k] >= _ranks[k], "rank plus oversampling overflows");
    }
    std::vector<std::vector<size_t>> r(s, std::vector<size_t>(d + 1, 1));
    std::vector<std::vector<const double*>> cores(s, std::vector<const double*>(d));
    std::vector<value_t> coef(_coefficients);
    std::vector<const size_t*> rp(s);
    std::vector<const double* const*> cp(s);
    for (size_t j = 0; j < s; ++j) {
        for (size_t k = 0; k < d; ++k) {
            const Tensor& c = _terms[j].components[k];
            r[j][k + 1] = c.dimensions[2];
            cores[j][k] = c.device_data();
            coef[j] *= c.factor;
        }
        rp[j] = r[j].data();
        cp[j] = cores[j].data();
    }

    const uint64_t seed = misc::randomEngine();   // one word per call: xe.seed(k) makes the call reproducible
    std::vector<double*> out(d, nullptr);
    std::vector<size_t> rs(d + 1, 1);
    TTTensor result(_terms[0].dimensions);
    guard([&] {
        xrs_handle_t h = gpu::handle();
        const int st = xrs_tt_round_randomized(h, d, result.dimensions.data(), s, rp.data(), cp.data(), coef.data(), ell.data(), seed,
                                               out.data(), rs.data());
        if (st != XRS_OK) throw xrs::Error{st, xrs_last_error()};
        if (d == 1) return;
        // the closing round, told that cores 0 .. d-2 are Q factors: one truncating sweep from d - 1 down to 0 (through
        // TTTensor::round the core would be moved back to d - 1 afterwards)
        try {
            xrs::tt::round(h, d, result.dimensions.data(), rs.data(), out.data(), true, d - 1, _ranks.data(), EPSILON);
        } catch (...) {
            for (double* p : out)
                if (p) h->pool->release(p);
            throw;
        }
    });
    for (size_t k = 0; k < d; ++k) result.components[k] = Tensor::adopt_device({rs[k], result.dimensions[k], rs[k + 1]}, out[k]);
    result.assume_core_position(0);
    return result;
}

TTOperator sum_rounded(const std::vector<TTOperator>& _terms, const std::vector<value_t>& _coefficients,
                       const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling) {
    XERUS_REQUIRE(!_terms.empty(), "sum_rounded needs at least one term");
    const std::vector<size_t> dims = _terms[0].dimensions;
    std::vector<TTTensor> views;
    views.reserve(_terms.size());
    for (const TTOperator& t : _terms) {
        XERUS_REQUIRE(t.dimensions == dims, "The dimensions of the terms must coincide");
        TTOperator copy(t);
        views.push_back(std::move(copy).to_tt());
    }
    return TTOperator::from_tt(sum_rounded(views, _coefficients, _ranks, _oversampling), dims);
}

TTTensor round_randomized(const TTTensor& _x, const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling) {
    return sum_rounded(std::vector<TTTensor>{_x}, {1.0}, _ranks, _oversampling);
}

TTOperator round_randomized(const TTOperator& _x, const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling) {
    return sum_rounded(std::vector<TTOperator>{_x}, {1.0}, _ranks, _oversampling);
}

}  // namespace xerus
