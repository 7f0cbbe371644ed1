// randomTTSVD (reference include/xerus/algorithms/randomSVD.h:31-98): Gaussian sketch, RQ and projection per mode,
// right to left, then one round. The sketch a = G b is xrs_sketch_gaussian (sketch.hip: G is generated inside the
// product), the RQ is calculate_rq (xrs_rq), b Q^T is one GEMM (contract with the right side transposed).
// Deviations (cap of s_j, dense only, device normals) are stated in the header.
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

TTTensor randomTTSVD(const Tensor& _x, const std::vector<size_t>& _ranks, const std::vector<size_t>& _oversampling) {
    const size_t d = _x.degree();
    const size_t numRanks = d == 0 ? 0 : d - 1;
    XERUS_REQUIRE(_ranks.size() == numRanks, "We need " << numRanks << " ranks but " << _ranks.size() << " where given");
    XERUS_REQUIRE(_oversampling.size() == numRanks,
                  "We need " << numRanks << " oversampling parameters but " << _oversampling.size() << " where given");
    XERUS_REQUIRE(std::find(_ranks.begin(), _ranks.end(), size_t(0)) == _ranks.end(), "Ranks must be strictly positive.");
    if (d == 0) {
        TTTensor u(size_t(0));
        u.components[0] = _x;
        return u;
    }
    TTTensor u(_x.dimensions);
    Tensor b = _x;
    if (d == 1) {
        b.reinterpret_dimensions({1, _x.dimensions[0], 1});
        u.set_component(0, std::move(b));
        u.assume_core_position(0);
        return u;
    }

    const uint64_t seed = misc::randomEngine();   // one word per call: xe.seed(k) makes the call reproducible

    for (size_t j = d; j >= 2; --j) {
        // b: (n_1 .. n_{j-1}) x (n_j [x r_j]); sketch its first j - 1 modes
        size_t M = 1;
        for (size_t k = 0; k + 1 < j; ++k) M *= b.dimensions[k];
        const size_t N = b.size / M;
        const size_t wanted = _ranks[j - 2] + _oversampling[j - 2];
        XERUS_REQUIRE(wanted >= _ranks[j - 2], "rank plus oversampling overflows");
        const size_t s = std::min(wanted, M);

        Tensor::DimensionTuple outDims{s};
        outDims.insert(outDims.end(), b.dimensions.begin() + long(j - 1), b.dimensions.end());
        Tensor a(outDims, Tensor::Representation::Dense, Tensor::Initialisation::None);
        const double* bd = b.device_data();
        double* ad = a.device_data_for_write();
        guard([&] {
            const int st = xrs_sketch_gaussian(gpu::handle(), ad, s, bd, M, N, seed, uint32_t(j), 0);
            if (st != XRS_OK) throw xrs::Error{st, xrs_last_error()};
        });
        a.factor = b.factor;

        Tensor R, Q;
        calculate_rq(R, Q, a, 1);

        if (j == d) {
            contract(b, b, false, Q, true, 1);
            Tensor::DimensionTuple qd = Q.dimensions;
            qd.push_back(1);
            Q.reinterpret_dimensions(qd);
        } else {
            contract(b, b, false, Q, true, 2);
        }
        u.set_component(j - 1, std::move(Q));
    }

    Tensor::DimensionTuple bdms{1};
    bdms.insert(bdms.end(), b.dimensions.begin(), b.dimensions.end());
    b.reinterpret_dimensions(bdms);
    u.set_component(0, std::move(b));

    u.round(_ranks);
    return u;
}

}  // namespace xerus
