// decomposition_als (reference src/xerus/algorithms/decompositionAls.cpp:36-65). The reference's local step
//     x.component(pos)(rU, iX, rL) = split.first(iU&1, rU) * split.second(rL, iL&1) * b(iU^pos, iX, iL&(pos+1))
// contracts the two chopped networks with b; here the same two interfaces are built as matrices by running GEMMs
// over the orthogonal cores (left: (n_0 .. n_{pos-1}) x r_pos, right: r_{pos+1} x (n_{pos+1} .. n_{d-1})) and
// applied to b by two more GEMMs. Host code over existing kernels.
#include <cmath>

#include "xerus.h"

namespace xerus {

namespace {

// component pos <- (left interface)^T b (right interface)^T, the core at pos
void project_component(TTTensor& _x, const Tensor& _b, const size_t _pos) {
    const size_t d = _x.degree();
    _x.move_core(_pos);
    Tensor t = _b;
    if (_pos > 0) {
        Tensor left = _x.get_component(0);   // (1, n_0, r_1) -> (n_0, r_1)
        left.reinterpret_dimensions({left.dimensions[1], left.dimensions[2]});
        for (size_t k = 1; k < _pos; ++k) contract(left, left, false, _x.get_component(k), false, 1);
        contract(t, left, true, t, false, _pos);   // (r_pos, n_pos .. n_{d-1})
    } else {
        Tensor::DimensionTuple dims{1};
        dims.insert(dims.end(), t.dimensions.begin(), t.dimensions.end());
        t.reinterpret_dimensions(dims);
    }
    if (_pos + 1 < d) {
        Tensor right = _x.get_component(d - 1);   // (r_{d-1}, n_{d-1}, 1) -> (r_{d-1}, n_{d-1})
        right.reinterpret_dimensions({right.dimensions[0], right.dimensions[1]});
        for (size_t k = d - 1; k-- > _pos + 1;) contract(right, _x.get_component(k), false, right, false, 1);
        contract(t, t, false, right, true, d - 1 - _pos);   // (r_pos, n_pos, r_{pos+1})
    } else {
        Tensor::DimensionTuple dims = t.dimensions;
        dims.push_back(1);
        t.reinterpret_dimensions(dims);
    }
    _x.set_component(_pos, std::move(t));
}

}  // namespace

void decomposition_als(TTTensor& _x, const Tensor& _b, const double _eps, const size_t _maxIterations) {
    _x.require_correct_format();
    XERUS_REQUIRE(_x.dimensions == _b.dimensions, "The dimensions of the TT and of the tensor to decompose must coincide.");
    const size_t d = _x.degree();
    if (d == 0) {
        _x.components[0] = _b;
        return;
    }

    double lastResidual = frob_norm(Tensor(_x) - _b);

    for (size_t iteration = 0; iteration < _maxIterations; ++iteration) {
        // Move right
        for (size_t pos = 0; pos < d; ++pos) project_component(_x, _b, pos);
        // Move left
        for (size_t pos = d - 1; pos-- > 1;) project_component(_x, _b, pos);

        const double residual = frob_norm(Tensor(_x) - _b);
        if (residual < EPSILON || (lastResidual - residual) / residual < _eps) return;
        lastResidual = residual;
    }
}

}  // namespace xerus
