// Tangent vectors of the manifold of fixed TT rank, retractions and the projective vector transport
// (reference include/xerus/algorithms/retractions.h:32-93, src/xerus/algorithms/retractions.cpp:30-288).
//
// The projection onto the tangent space, the rank-2r block TT of a tangent vector and the inner product
// run through the tangent drivers of xerus_amd (xrs_tt_tangent_project / _to_tt / _dot): the components
// stay in HBM, the environments never leave the device.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "../ttNetwork.h"

namespace xerus {

/// class to compactly represent tangent vectors of the manifold of constant TT-rank
class TTTangentVector {
   public:
    TTTensor baseL;

    /// @note components will not be changed. use a vector transport to update them accordingly
    void set_base(const TTTensor& _newBase);

    std::vector<Tensor> components;
    /// edges of the projecting constructor whose Gram UU_k failed the Cholesky certificate and went through
    /// the SVD pseudo-inverse (diagnostics; 0 for a base of full rank)
    size_t fallbackEdges = 0;

    TTTangentVector() {}
    /// creates a tangent vector by projecting @a _direction onto the tangent plane located at @a _base
    TTTangentVector(const TTTensor& _base, const TTTensor& _direction);
    TTTangentVector& operator+=(const TTTangentVector& _rhs);
    TTTangentVector& operator-=(const TTTangentVector& _rhs);
    TTTangentVector& operator*=(value_t _alpha);
    TTTangentVector operator*(value_t _alpha) const;
    value_t scalar_product(const TTTangentVector& _other) const;
    value_t frob_norm() const;

    explicit operator TTTensor() const;
    TTTensor added_to_base() const;

   private:
    /// the left Grams UU_k of baseL (UU_0 = 1), shared between copies and between vectors created over the same
    /// base object state; dropped by set_base and recomputed on demand
    mutable std::shared_ptr<const std::vector<Tensor>> leftGrams;
    const std::vector<Tensor>& left_grams() const;
    TTTensor block_tt(bool _addBase) const;
};

TTTangentVector operator*(value_t _alpha, const TTTangentVector& _rhs);

/// retraction that performs a HOSVD to project back onto the Manifold
struct HOSVDRetraction {
    bool roundByVector;
    size_t rank;
    std::vector<size_t> rankVector;
    void operator()(TTTensor& _U, const TTTensor& _change) const;
    void operator()(TTTensor& _U, const TTTangentVector& _change) const;
    HOSVDRetraction(size_t _rank) : roundByVector(false), rank(_rank) {}
    HOSVDRetraction(const std::vector<size_t>& _rank) : roundByVector(true), rank(~0ul), rankVector(_rank) {}
};

using TTRetractionI = std::function<void(TTTensor&, const TTTangentVector&)>;
using TTRetractionII = std::function<void(TTTensor&, const TTTensor&)>;
using TTVectorTransport = std::function<void(const TTTensor&, TTTangentVector&)>;

/// retraction that performs a HOSVD to project back onto the Manifold (keeps the ranks of @a _U)
void HOSVDRetractionI(TTTensor& _U, const TTTangentVector& _change);
void HOSVDRetractionII(TTTensor& _U, const TTTensor& _change);

/// retraction that performs an ALS half-sweep to project back onto the Manifold. Retains the ranks of @a _U
void ALSRetractionII(TTTensor& _U, const TTTensor& _change);
void ALSRetractionI(TTTensor& _U, const TTTangentVector& _change);

/// retraction that performs componentwise addition of U_i and W_i, the i-th component of the tangent vector
void SubmanifoldRetractionII(TTTensor& _U, const TTTensor& _change);
void SubmanifoldRetractionI(TTTensor& _U, const TTTangentVector& _change);

/// simple vector transport by projecting onto the new tangent plane
void ProjectiveVectorTransport(const TTTensor& _newBase, TTTangentVector& _tangentVector);

}  // namespace xerus
