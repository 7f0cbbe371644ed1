// UQ-ADF (reference src/xerus/algorithms/uqAdf.cpp:40-477) on the GPU. The algorithm, step by step, is the
// reference's InternalSolver::solve (:285-322): per iteration move_core(0, keepRank), the right stacks for
// k = d-1 .. 1, then per core position the residual and the stopping rule (k = 0), delta, ||A(delta)||, the
// update x_k -= ||delta||^2 / ||A delta||^2 delta, move_core(k + 1, keepRank) and the left stacks.
// The loops over the N samples are device launches (uq.hip, adf.hip, gemm.hip). With M_j = sum_t P_k[j, t] X_k[:, t, :]:
//   right stack   R_k[j] = M_j R_{k+1}[j]                      N x r_k        (adf::stack_backward, vec = P_k)
//   leftOught_k[j] = leftOught_{k-1}[j] M_j                    N x r_{k+1}    (adf::stack_forward)
//   leftIs_k[j]   = M_j^T leftIs_{k-1}[j] M_j                  N x r_{k+1}^2  (uq::stack_congruence)
//   delta         = E^T W, e_j = leftIs_{k-1}[j] M_j R_{k+1}[j] - leftOught_{k-1}[j], W the Khatri-Rao rows
//                   P_k[j, t] R_{k+1}[j, b]                                   (uq::stack_symv, xrs::gemm)
//   ||A delta||^2 = sum_j g_j^T leftIs_{k-1}[j] g_j, g_j = M_j(delta) R_{k+1}[j]   (uq::quadform)
// and the core-0 products are GEMMs against R_1. leftIs / leftOught of position k are read at position k + 1
// only and rebuilt every sweep: two rolling buffers each instead of the reference's d. The host reads back
// ||delta||, ||A delta|| per step and the residual per iteration.
#include <cmath>
#include <random>

#include "../adf.hpp"
#include "../elementwise.hpp"
#include "../uq.hpp"
#include "xerus.h"
#include "xerus/algorithms/uqAdf.h"

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

void upload(xrs_handle_t h, double* dst, const double* src, size_t count) {
    if (count) XRS_HIP(hipMemcpyAsync(dst, src, count * 8, hipMemcpyHostToDevice, h->stream));
}

// Random variables (N x d-1) and the basis matrices P_k (N x n_k, k >= 1) on the device
struct DeviceBasis {
    size_t N, d;
    std::vector<size_t> n, off;   // per stochastic mode m = k - 1
    std::vector<double> hxi;      // staging, alive until the upload has run
    xrs::DevBuf xi, P;

    DeviceBasis(xrs_handle_t h, const std::vector<size_t>& dims, const std::vector<std::vector<double>>& rv) : N(rv.size()), d(dims.size()) {
        const size_t m = d - 1;
        hxi.resize(N * m);
        for (size_t j = 0; j < N; ++j) {
            XERUS_REQUIRE(rv[j].size() == m, "UQ: random vector " << j << " has " << rv[j].size() << " entries, expected " << m);
            for (size_t i = 0; i < m; ++i) hxi[j * m + i] = rv[j][i];
        }
        size_t total = 0;
        for (size_t k = 1; k < d; ++k) {
            n.push_back(dims[k]);
            off.push_back(total);
            total += N * dims[k];
        }
        xi = xrs::DevBuf(h, std::max<size_t>(N * m, 1) * 8);
        P = xrs::DevBuf(h, std::max<size_t>(total, 1) * 8);
        upload(h, xi.d(), hxi.data(), N * m);
        xrs::uq::basis(h, N, m, xi.d(), m, n.data(), off.data(), P.d());
    }
    const double* of(size_t k) const { return P.d() + off[k - 1]; }
};

struct Dims {
    size_t a, n, b;
};
Dims dims_of(const TTTensor& x, size_t k) {
    const Tensor& C = x.get_component(k);
    return {C.dimensions[0], C.dimensions[1], C.dimensions[2]};
}

// p_j = M_j^{(1)} .. M_j^{(d-1)} for every sample (N x r_1): the sample loop of uq_mc (:436-441)
xrs::DevBuf right_product(xrs_handle_t h, const TTTensor& x, const DeviceBasis& B, const double* ones) {
    xrs::DevBuf cur;
    for (size_t k = x.degree() - 1; k > 0; --k) {
        const Dims c = dims_of(x, k);
        Tensor comp = x.get_component(k);
        xrs::DevBuf out(h, B.N * c.a * 8);
        xrs::adf::stack_backward(h, B.N, comp.device_data_applied(), xrs::adf::Mode{nullptr, B.of(k)}, cur.p ? cur.d() : ones, c.a, c.n, c.b,
                                 out.d());
        cur = std::move(out);
    }
    return cur;
}

class UqSolver {
   public:
    UqSolver(TTTensor& _x, const std::vector<std::vector<double>>& _rv, const std::vector<Tensor>& _sol, size_t _maxIterations,
             std::vector<double>* _history)
        : x(_x), N(_rv.size()), d(_x.degree()), maxIterations(_maxIterations), history(_history), h(gpu::handle()) {
        XERUS_REQUIRE(_rv.size() == _sol.size(), "UQ: " << _rv.size() << " random vectors but " << _sol.size() << " solutions");
        XERUS_REQUIRE(d >= 2, "UQ-ADF needs a TT of degree >= 2");
        XERUS_REQUIRE(N >= 1, "UQ-ADF needs at least one sample");
        _x.require_correct_format();
        n0 = _x.dimensions[0];
        for (size_t k = 0; k + 1 < d; ++k) XERUS_REQUIRE(_x.rank(k) <= xrs::uq::kMaxRank, "UQ-ADF supports ranks up to 256");
        basis.reset(new DeviceBasis(h, _x.dimensions, _rv));
        S = xrs::DevBuf(h, N * n0 * 8);
        for (size_t j = 0; j < N; ++j) {
            XERUS_REQUIRE(_sol[j].size == n0, "UQ: solution " << j << " has size " << _sol[j].size << ", expected " << n0);
            XRS_HIP(hipMemcpyAsync(S.d() + j * n0, _sol[j].device_data(), n0 * 8, hipMemcpyDeviceToDevice, h->stream));
            if (_sol[j].has_factor()) xrs::scal(h, S.d() + j * n0, _sol[j].factor, n0);
        }
        solutionsNorm = xrs::reduce_to_host(h, 0, S.d(), nullptr, N * n0);   // calc_solutions_norm (:85-92)
        const std::vector<double> one(N, 1.0);
        ones = xrs::DevBuf(h, N * 8);
        upload(h, ones.d(), one.data(), N);
        XRS_HIP(hipStreamSynchronize(h->stream));   // `one` and the staging of the basis leave scope
        R.resize(d + 1);
    }

    void solve() {   // :285-322
        std::vector<double> residuals(10, 1000.0);
        for (size_t iteration = 0; maxIterations == 0 || iteration < maxIterations; ++iteration) {
            x.move_core(0, true);
            for (size_t k = d - 1; k > 0; --k) calc_right_stack(k);
            for (size_t k = 0; k < d; ++k) {
                Tensor delta;
                double normA;
                if (k == 0) {
                    const double res = core0_residual_and_delta(delta, normA) / solutionsNorm;
                    residuals.push_back(res);
                    if (history) history->push_back(res);
                    if (residuals.back() / residuals[residuals.size() - 10] > 0.99) return;
                } else {
                    delta = calculate_delta(k);
                    normA = calculate_norm_A_projGrad(delta, k);
                }
                const double nd = xrs::reduce_to_host(h, 0, delta.device_data(), nullptr, delta.size);
                const double PyR = nd * nd;
                xrs::axpy(h, x.component(k).device_data_applied(), -(PyR / (normA * normA)), delta.device_data(), delta.size);   // :313
                if (k + 1 < d) {
                    x.move_core(k + 1, true);
                    calc_left_stack(k);
                }
            }
        }
    }

   private:
    TTTensor& x;
    const size_t N, d, maxIterations;
    std::vector<double>* history;
    xrs_handle_t h;
    size_t n0 = 0;
    double solutionsNorm = 0.0;
    std::unique_ptr<DeviceBasis> basis;
    xrs::DevBuf S, ones;
    std::vector<xrs::DevBuf> R;            // R[k] (N x r_k), k = 1 .. d-1
    xrs::DevBuf leftIs[2], leftOught[2];   // position k lives in slot k & 1; leftIs of position 0 is the identity

    xrs::adf::Mode mode(size_t k) const { return xrs::adf::Mode{nullptr, basis->of(k)}; }
    const double* right_of(size_t k) const { return k + 1 < d ? R[k + 1].d() : ones.d(); }   // R_{k+1}, ones at the end
    const double* is_of(size_t k) const { return k >= 1 ? leftIs[k & 1].d() : nullptr; }     // null: the identity

    void calc_right_stack(size_t k) {   // :143-161
        const Dims c = dims_of(x, k);
        xrs::DevBuf out(h, N * c.a * 8);
        xrs::adf::stack_backward(h, N, x.component(k).device_data_applied(), mode(k), right_of(k), c.a, c.n, c.b, out.d());
        R[k] = std::move(out);
    }

    void calc_left_stack(size_t k) {   // :110-140
        const Dims c = dims_of(x, k);
        xrs::DevBuf ought(h, N * c.b * 8);
        const double* X = x.component(k).device_data_applied();
        if (k == 0) {   // leftOught_0 = S X_0
            xrs::gemm(h, ought.d(), N, c.b, 1.0, S.d(), n0, false, n0, X, c.b, false);
        } else {
            xrs::DevBuf is(h, N * c.b * c.b * 8);
            xrs::uq::stack_congruence(h, N, is_of(k - 1), X, basis->of(k), c.a, c.n, c.b, is.d());
            xrs::adf::stack_forward(h, N, leftOught[(k - 1) & 1].d(), X, mode(k), c.a, c.n, c.b, ought.d());
            leftIs[k & 1] = std::move(is);
        }
        leftOught[k & 1] = std::move(ought);
    }

    // k = 0 (:204-217, :227-233, :268-282): D = R_1 X_0^T - S, delta = D^T R_1, ||A delta|| = ||R_1 delta^T||_F;
    // returns ||D||_F
    double core0_residual_and_delta(Tensor& delta, double& normA) {
        const Dims c = dims_of(x, 0);
        const double* X = x.component(0).device_data_applied();
        xrs::DevBuf D(h, N * n0 * 8);
        xrs::gemm(h, D.d(), N, n0, 1.0, R[1].d(), c.b, false, c.b, X, c.b, true);
        xrs::axpy(h, D.d(), -1.0, S.d(), N * n0);
        const double res = xrs::reduce_to_host(h, 0, D.d(), nullptr, N * n0);
        delta = Tensor({1, n0, c.b}, Tensor::Representation::Dense, Tensor::Initialisation::None);
        xrs::gemm(h, delta.device_data_for_write(), n0, c.b, 1.0, D.d(), n0, true, N, R[1].d(), c.b, false);
        xrs::gemm(h, D.d(), N, n0, 1.0, R[1].d(), c.b, false, c.b, delta.device_data(), c.b, true);
        normA = xrs::reduce_to_host(h, 0, D.d(), nullptr, N * n0);
        return res;
    }

    Tensor calculate_delta(size_t k) {   // :164-203, k >= 1
        const Dims c = dims_of(x, k);
        xrs::DevBuf E(h, N * c.a * 8);
        xrs::adf::stack_backward(h, N, x.component(k).device_data_applied(), mode(k), right_of(k), c.a, c.n, c.b, E.d());
        if (k > 1) {   // leftIs of position 0 is the identity
            xrs::DevBuf Y(h, N * c.a * 8);
            xrs::uq::stack_symv(h, N, is_of(k - 1), E.d(), c.a, Y.d());
            E = std::move(Y);
        }
        xrs::axpy(h, E.d(), -1.0, leftOught[(k - 1) & 1].d(), N * c.a);
        xrs::DevBuf W(h, N * c.n * c.b * 8);
        xrs::uq::khatri_rao_rows(h, N, basis->of(k), c.n, right_of(k), c.b, W.d());
        Tensor delta({c.a, c.n, c.b}, Tensor::Representation::Dense, Tensor::Initialisation::None);
        xrs::gemm(h, delta.device_data_for_write(), c.a, c.n * c.b, 1.0, E.d(), c.a, true, N, W.d(), c.n * c.b, false);
        return delta;
    }

    double calculate_norm_A_projGrad(const Tensor& delta, size_t k) {   // :223-265, k >= 1
        const Dims c = dims_of(x, k);
        xrs::DevBuf G(h, N * c.a * 8);
        xrs::adf::stack_backward(h, N, delta.device_data(), mode(k), right_of(k), c.a, c.n, c.b, G.d());
        return std::sqrt(xrs::uq::quadform_to_host(h, N, k > 1 ? is_of(k - 1) : nullptr, G.d(), c.a));
    }
};

}  // namespace

Tensor randVar_to_position(const double _v, const size_t _polyDegree) {
    std::unique_ptr<value_t[]> p(new value_t[std::max<size_t>(_polyDegree, 1)]);
    for (size_t i = 0; i < _polyDegree; ++i) p[i] = i == 0 ? 1.0 : i == 1 ? _v : _v * p[i - 1] - double(i - 1) * p[i - 2];
    return Tensor({_polyDegree}, std::move(p));
}

void uq_adf(TTTensor& _x, const std::vector<std::vector<double>>& _randomVariables, const std::vector<Tensor>& _solutions,
            const size_t _maxIterations, std::vector<double>* _residualHistory) {
    guard([&] {
        UqSolver solver(_x, _randomVariables, _solutions, _maxIterations, _residualHistory);
        solver.solve();
    });
}

void uq_adf(TTTensor& _x, const std::vector<std::vector<double>>& _randomVariables, const std::vector<Tensor>& _solutions) {
    uq_adf(_x, _randomVariables, _solutions, 1000, nullptr);
}

TTTensor uq_adf(const UQMeasurementSet& _measurments, const TTTensor& _guess) { return uq_adf(_measurments, _guess, 1000, nullptr); }

TTTensor uq_adf(const UQMeasurementSet& _measurments, const TTTensor& _guess, const size_t _maxIterations,
                std::vector<double>* _residualHistory) {
    XERUS_REQUIRE(_measurments.randomVectors.size() == _measurments.solutions.size(), "Invalid measurments");
    XERUS_REQUIRE(_measurments.initialRandomVectors.size() == _measurments.initialSolutions.size(), "Invalid initial measurments");
    const size_t numInitial = _measurments.initialRandomVectors.size();
    if (numInitial == 0) {
        TTTensor x = _guess;
        uq_adf(x, _measurments.randomVectors, _measurments.solutions, _maxIterations, _residualHistory);
        return x;
    }
    // :338-405
    TTTensor x(_guess.dimensions);
    TTTensor newX(x.dimensions);
    std::vector<std::vector<double>> randomVectors = _measurments.randomVectors;
    std::vector<Tensor> solutions = _measurments.solutions;
    XERUS_REQUIRE(!solutions.empty(), "UQ: the mean needs at least one solution");
    XERUS_REQUIRE(numInitial == _measurments.initialRandomVectors[0].size(), "Sizes don't match.");
    XERUS_REQUIRE(numInitial + 1 == x.degree(), "Sizes don't match.");

    Tensor mean({x.dimensions[0]});   // over `solutions` only: the initial ones are merged after it (:396-398)
    for (const Tensor& sol : solutions) {
        XERUS_REQUIRE(sol.size == x.dimensions[0], "UQ: a solution's size is not the first dimension");
        Tensor s = sol;
        s.reinterpret_dimensions({x.dimensions[0]});
        mean += s;
    }
    mean /= double(solutions.size());

    TTTensor baseTerm(x.dimensions);
    mean.reinterpret_dimensions({1, x.dimensions[0], 1});
    baseTerm.set_component(0, mean);
    for (size_t k = 0; k < numInitial; ++k) baseTerm.set_component(k + 1, Tensor::dirac({1, x.dimensions[k + 1], 1}, 0));
    baseTerm.assume_core_position(0);
    newX += baseTerm;
    mean.reinterpret_dimensions({x.dimensions[0]});

    for (size_t m = 0; m < numInitial; ++m) {   // linear terms
        XERUS_REQUIRE(_measurments.initialRandomVectors[m].size() == numInitial, "Sizes don't match.");
        XERUS_REQUIRE(_measurments.initialRandomVectors[m][m] > 0.0, "Invalid initial randVec");
        XERUS_REQUIRE(_measurments.initialSolutions[m].size == x.dimensions[0], "UQ: an initial solution's size is not the first dimension");
        TTTensor linearTerm(x.dimensions);
        Tensor init = _measurments.initialSolutions[m];
        init.reinterpret_dimensions({x.dimensions[0]});
        Tensor tmp = init - mean;
        tmp.reinterpret_dimensions({1, x.dimensions[0], 1});
        linearTerm.set_component(0, tmp);
        for (size_t k = 0; k < numInitial; ++k) {
            if (k == m) {
                linearTerm.set_component(k + 1, Tensor::dirac({1, x.dimensions[k + 1], 1}, 0));
            } else {
                XERUS_REQUIRE(_measurments.initialRandomVectors[m][k] == 0.0, "Invalid initial randVec");
                XERUS_REQUIRE(x.dimensions[k + 1] >= 2, "UQ: a linear term needs a basis of at least two polynomials");
                linearTerm.set_component(k + 1, Tensor::dirac({1, x.dimensions[k + 1], 1}, 1));
            }
        }
        linearTerm.assume_core_position(0);
        newX += linearTerm;
    }
    // the merged vectors are built as in the reference (:397-398) -- and, as there, the solver gets the unmerged ones (:404)
    randomVectors.insert(randomVectors.end(), _measurments.initialRandomVectors.begin(), _measurments.initialRandomVectors.end());
    solutions.insert(solutions.end(), _measurments.initialSolutions.begin(), _measurments.initialSolutions.end());

    x = newX;
    x.round(0.00025);
    uq_adf(x, _measurments.randomVectors, _measurments.solutions, _maxIterations, _residualHistory);
    return x;
}

void UQMeasurementSet::add(const std::vector<double>& _rndvec, const Tensor& _solution) {
    randomVectors.push_back(_rndvec);
    solutions.push_back(_solution);
}

void UQMeasurementSet::add_initial(const std::vector<double>& _rndvec, const Tensor& _solution) {
    initialRandomVectors.push_back(_rndvec);
    initialSolutions.push_back(_solution);
}

namespace {

// the reference's serial draws (:434-438): sample-major, k from d-1 down to 1, 0.3 x for k <= numSpecial
std::vector<std::vector<double>> draw_random_variables(size_t d, size_t N, size_t numSpecial) {
    std::mt19937_64 rnd;
    std::normal_distribution<double> dist(0.0, 1.0);
    std::vector<std::vector<double>> rv(N, std::vector<double>(d - 1));
    for (size_t i = 0; i < N; ++i)
        for (size_t k = d - 1; k > 0; --k) rv[i][k - 1] = (k <= numSpecial ? 0.3 : 1.0) * dist(rnd);
    return rv;
}

// all N solutions (N x n_0) in one device pass: the basis, the right products, one GEMM against component 0
xrs::DevBuf evaluate_samples(xrs_handle_t h, const TTTensor& x, const std::vector<std::vector<double>>& rv) {
    const size_t N = rv.size(), n0 = x.dimensions[0];
    DeviceBasis B(h, x.dimensions, rv);
    const std::vector<double> one(N, 1.0);
    xrs::DevBuf ones(h, N * 8);
    upload(h, ones.d(), one.data(), N);
    xrs::DevBuf p = right_product(h, x, B, ones.d());
    Tensor c0 = x.get_component(0);
    const size_t r1 = c0.dimensions[2];
    xrs::DevBuf out(h, N * n0 * 8);
    xrs::gemm(h, out.d(), N, n0, 1.0, p.d(), r1, false, r1, c0.device_data_applied(), r1, true);
    XRS_HIP(hipStreamSynchronize(h->stream));   // the staging vectors leave scope
    return out;
}

}  // namespace

std::pair<std::vector<std::vector<double>>, std::vector<Tensor>> uq_mc(const TTTensor& _x, const size_t _N, const size_t _numSpecial) {
    XERUS_REQUIRE(_x.degree() >= 2, "uq_mc needs a TT of degree >= 2");
    _x.require_correct_format();
    return guard([&] {
        std::vector<std::vector<double>> rv = draw_random_variables(_x.degree(), _N, _numSpecial);
        std::vector<Tensor> solutions;
        solutions.reserve(_N);
        if (_N > 0) {
            xrs_handle_t h = gpu::handle();
            const size_t n0 = _x.dimensions[0];
            xrs::DevBuf all = evaluate_samples(h, _x, rv);
            std::vector<double> host(_N * n0);
            XRS_HIP(hipMemcpyAsync(host.data(), all.d(), _N * n0 * 8, hipMemcpyDeviceToHost, h->stream));
            XRS_HIP(hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < _N; ++i) {
                std::unique_ptr<value_t[]> data(new value_t[n0]);
                std::copy(host.begin() + i * n0, host.begin() + (i + 1) * n0, data.get());
                solutions.emplace_back(Tensor::DimensionTuple{n0}, std::move(data));
            }
        }
        return std::make_pair(std::move(rv), std::move(solutions));
    });
}

Tensor uq_avg(const TTTensor& _x, const size_t _N, const size_t _numSpecial) {
    XERUS_REQUIRE(_x.degree() >= 2, "uq_avg needs a TT of degree >= 2");
    XERUS_REQUIRE(_N >= 1, "uq_avg needs at least one sample");
    _x.require_correct_format();
    return guard([&] {
        xrs_handle_t h = gpu::handle();
        const size_t n0 = _x.dimensions[0];
        const std::vector<std::vector<double>> rv = draw_random_variables(_x.degree(), _N, _numSpecial);
        xrs::DevBuf all = evaluate_samples(h, _x, rv);
        Tensor avg({n0}, Tensor::Representation::Dense, Tensor::Initialisation::None);
        xrs::uq::column_mean(h, _N, all.d(), n0, avg.device_data_for_write());
        return avg;
    });
}

}  // namespace xerus
