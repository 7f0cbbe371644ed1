// CholeskyQR, once: the Gram, the shifted factorisation, the application of the inverse factor and the product of
// the factors that orthogonalize / orthogonalize_big (linalg.hip), qr_solve_big (solve.hip) and the general round's
// scqr3 (tt_trunc.hip) are built from. Tall X (m x n, m >= n) = Q R, wide X (m x n, m <= n) = L Q.
// Everything here only enqueues on h->stream: no allocation (the callers own the workspaces and their allocation
// order), no synchronisation; the status words stay the callers' (per pass: potrf 1, chol_full chol_full_blocks(N)).
#pragma once
#include <cmath>
#include <functional>

#include "smallla.hpp"

namespace xrs::cholqr {

constexpr double kU = 1.1102230246251565e-16;    // unit roundoff 2^-53
constexpr double kEps = 2.220446049250313e-16;   // std::numeric_limits<double>::epsilon()

// Shifts of the first factorisation, relative to trace(G) = ||X||_F^2; M the long dimension (sharded: the global
// one, the shift must be the same on every rank), N the Gram order.
// Certifying, applied downwards: if chol(G - tau tr(G) I) succeeds, sigma_min(X) >= cert_ratio(tau) ||X||_F.
inline double certify_shift(size_t M, size_t N) { return 4.0 * double(M + 2 * N) * kU; }
inline double cert_ratio(double shift) { return std::sqrt(0.5 * shift); }
// Robust, applied upwards: shifted CholeskyQR3 (Fukaya et al. 2020), valid for kappa(X) < 1/u.
inline double robust_shift(size_t M, size_t N) { return 11.0 * (double(M) * N + double(N) * (N + 1)) * kU; }

struct Shape {
    size_t m, n;
    bool wide;
    size_t N() const { return wide ? m : n; }   // Gram order
    size_t M() const { return wide ? n : m; }   // long dimension
};

// out (N x N) = X X^T (wide) / X^T X (tall). sym: gemm_sym, else the plain gemm. Known asymmetry: orthogonalize
// (N <= 512) uses the plain gemm, the other three callers gemm_sym; the two differ in bits and in time, so each
// caller keeps its own.
inline void gram(xrs_handle_t h, const Shape& s, double* out, const double* X, bool sym) {
    if (sym) gemm_sym(h, out, s.N(), 1.0, X, s.n, !s.wide, s.M(), X, s.n, s.wide);
    else gemm(h, out, s.N(), s.N(), 1.0, X, s.n, !s.wide, s.M(), X, s.n, s.wide);
}

// One pass's factorisation: the caller's workspace before factorize(), the lower factor of order N after it.
// Z null: potrf factors the Gram G in place, with its diagonal-block inverses Dinv for trsm and the optional trace
// output info. Z given: chol_full factors G into L (optional) and the explicit inverse Z = L^{-1}, applied by a GEMM.
struct Factor {
    double* G = nullptr;
    int* status = nullptr;
    double* Dinv = nullptr;
    double* info = nullptr;
    double* L = nullptr;
    double* Z = nullptr;
    const double* lower() const { return Z ? L : G; }
};
inline void factorize(xrs_handle_t h, size_t N, const Factor& f, double shift) {
    if (f.Z) chol_full(h, f.G, N, shift, f.L, f.Z, f.status);
    else potrf(h, f.G, int(N), shift, f.Dinv, f.status, f.info);
}
// out = X L^{-T} (tall) / L^{-1} X (wide)
inline void apply_inverse(xrs_handle_t h, const Shape& s, const Factor& f, const double* X, double* out) {
    const size_t N = s.N();
    if (!f.Z) trsm(h, s.wide, f.G, f.Dinv, int(N), X, s.n, out, s.n, int(s.M()));
    else if (s.wide) gemm(h, out, N, s.n, 1.0, f.Z, N, false, N, X, s.n, false);
    else gemm(h, out, s.m, N, 1.0, X, s.n, false, N, f.Z, N, true);
}
// RL = L0 L1 [L2] (wide: the L of X = L Q) / [L2^T] L1^T L0^T (tall: the R of X = Q R) of count = 2 or 3 factors;
// tmp (N x N) for count 3. The factors' upper triangles are zero.
inline void factor_product(xrs_handle_t h, const Shape& s, const Factor* f, int count, double* tmp, double* RL) {
    const size_t N = s.N();
    const double *a = f[0].lower(), *b = f[1].lower(), *c = count == 3 ? f[2].lower() : nullptr;
    if (s.wide) {
        gemm(h, c ? tmp : RL, N, N, 1.0, a, N, false, N, b, N, false);
        if (c) gemm(h, RL, N, N, 1.0, tmp, N, false, N, c, N, false);
    } else if (!c) {
        gemm(h, RL, N, N, 1.0, b, N, true, N, a, N, true);
    } else {
        gemm(h, tmp, N, N, 1.0, c, N, true, N, b, N, true);
        gemm(h, RL, N, N, 1.0, tmp, N, false, N, a, N, true);
    }
}

struct Steps {   // the callers' optional steps inside a pass, enqueued in place
    std::function<void(double* G)> on_gram;                     // on the Gram, before it is factored
    std::function<void(int pass, const Factor& f)> on_factor;   // between the factorisation and its use
};
// One pass: G = Gram(X), [on_gram], chol(G + shift tr(G) I), [on_factor], out = X L^{-T} / L^{-1} X
inline void pass(xrs_handle_t h, const Shape& s, const Factor& f, double shift, bool sym, const double* X, double* out,
                 const Steps& steps = {}, int index = 0) {
    gram(h, s, f.G, X, sym);
    if (steps.on_gram) steps.on_gram(f.G);
    factorize(h, s.N(), f, shift);
    if (steps.on_factor) steps.on_factor(index, f);
    apply_inverse(h, s, f, X, out);
}
// Shifted CholeskyQR3: three passes X -> out[0] -> out[1] -> out[2] = Q, the first one shifted (robust_shift);
// the triangular factor is factor_product(f, 3).
inline void scqr3(xrs_handle_t h, const Shape& s, double shift, bool sym, const Factor* f, const double* X,
                  double* const* out, const Steps& steps = {}) {
    for (int p = 0; p < 3; ++p) {
        pass(h, s, f[p], p == 0 ? shift : 0.0, sym, X, out[p], steps, p);
        X = out[p];
    }
}

}  // namespace xrs::cholqr
