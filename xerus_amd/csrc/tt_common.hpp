// Internal interface of the TT drivers (tt.hip: move_core, certified chain round, <x,y>; tt_trunc.hip:
// the certified truncating round). Not part of the C-ABI. Shared by the three device-resident rounds:
//   Sweep                 owner of a round's temporaries and candidate cores (released unless committed)
//   orth_enqueue          the orthogonality check of a core vector, enqueued up to its pinned copy
//   worst_dev, first_bad  the host-side judges of that copy and of the factorisation statuses
//   gram_chains, gemm_grouped, k_dev_identity_many
#pragma once
#include <algorithm>
#include <vector>

#include "chol_batch.hpp"
#include "scratch_map.hpp"
#include "smallla.hpp"

namespace xrs {
// start a gated asynchronous inner product of the handle behind its current stream point (tt.hip)
void open_dot_gate(xrs_handle_t h);

namespace ttd {

struct TT {
    xrs_handle_t h;
    size_t d;
    const size_t* n;
    size_t* r;      // d + 1 ranks, r[0] = r[d] = 1
    double** core;

    size_t rows_left(size_t k) const { return r[k] * n[k]; }      // (r_k n_k) x r_{k+1}
    size_t cols_right(size_t k) const { return n[k] * r[k + 1]; }  // r_k x (n_k r_{k+1})
    size_t size(size_t k) const { return r[k] * n[k] * r[k + 1]; }

    double* alloc(size_t elems) { return static_cast<double*>(h->pool->alloc(std::max<size_t>(elems, 1) * 8)); }
    void release(double* p) {
        if (!p) return;
        fence_readers(h);   // an in-flight async inner product may still read the block
        h->pool->release(p);
    }
    void replace(size_t k, double* p) { release(core[k]); core[k] = p; }

    // Mode-sharded TT (xrs_tt_*_sharded): n[] are this rank's slice counts and every sum over the
    // mode index is completed by an all-reduce across ranks; null for a whole TT on one device.
    // shard_mode without a hook: a single rank (the local sums are the global ones, no synchronisation)
    bool shard_mode = false;
    xrs_allreduce_fn ar = nullptr;
    void* ar_ctx = nullptr;
    // the ranks' layout (xrs_tt_round_sharded_ex): world > 0 when known; each rank holds a contiguous block
    // of every mode, blocks in rank order. Unknown (0): cores whose unfolding spans the ranks' blocks
    // (tall right edges, structural-excess QC steps) cannot be gathered and the round reports uncertified
    int world = 0;
    int rank = 0;
    // shard_layout's result, computed once per TT (its all-reduce and host wait are paid once per round even
    // when the certified truncation falls through to the general round)
    bool layout_cached = false;
    std::vector<size_t> layout_ng, layout_off;
    bool layout_known = false;
    bool sharded() const { return shard_mode; }
    // round(): the norm of every core is on its way to the handle's pinned scratch (probe_core_ranges)
    bool range_probed = false;
    bool range_hit = false;      // a device-resident round gave up on it (core_range_exceeded behind its host wait)
    void reduce(double* buf, size_t count) const {
        if (!ar) return;
        // the built-in RCCL hook is stream-ordered; any other hook sees a synchronised stream
        if (ar != &xrs_comm_allreduce) XRS_HIP(hipStreamSynchronize(h->stream));
        const int rc = ar(ar_ctx, buf, count);
        XRS_REQUIRE(rc == 0, "all-reduce callback failed");
    }
};

// Everything a device-resident round has enqueued and not yet judged. `keep`: temporaries that must outlive
// the enqueued work. `owned`: the candidate cores, pool blocks that become the TT's cores through commit();
// whatever is still owned when the round leaves, by a return or a throw, goes back to the pool.
struct Sweep {
    TT& t;
    std::vector<DevBuf> keep;
    std::vector<double*> owned;
    explicit Sweep(TT& tt) : t(tt) {}
    Sweep(const Sweep&) = delete;
    Sweep& operator=(const Sweep&) = delete;
    ~Sweep() {
        for (double* p : owned) {
            try {
                t.release(p);
            } catch (...) {   // (fence_readers: the block stays out of the pool rather than under a reader)
            }
        }
    }
    double* buf(size_t elems) {
        keep.emplace_back(t.h, std::max<size_t>(elems, 1) * 8);
        return keep.back().d();
    }
    double* core(size_t elems) {
        double* p = t.alloc(elems);
        owned.push_back(p);
        return p;
    }
    void drop(double* p) {   // a core block that is no longer needed
        auto it = std::find(owned.begin(), owned.end(), p);
        if (it != owned.end()) {
            owned.erase(it);
            t.release(p);
        }
    }
    // the candidates C (all owned) become the TT's cores, with the internal ranks r[1..d-1] when given
    void commit(const std::vector<double*>& C, const size_t* r = nullptr) {
        fence_readers(t.h);   // the one step of replace() that can throw, before any ownership moves
        for (size_t k = 0; k < t.d; ++k) t.replace(k, C[k]);
        owned.clear();
        for (size_t k = 1; r && k < t.d; ++k) t.r[k] = r[k];
    }
};

// Mode layout of a sharded TT (tt_trunc.hip): global mode sizes ng, this rank's first slice off per mode;
// known = false when the ranks' order is unknown (world 0) -- then off is meaningless.
struct ShardLayout {
    std::vector<size_t> ng, off;
    bool known = true;
};
ShardLayout shard_layout(TT& t);
void gather_core(TT& t, const double* local, size_t a, size_t nl, size_t ng, size_t b, size_t off, double* full);
void slice_core(TT& t, const double* full, size_t a, size_t ng, size_t b, size_t off, size_t nl, double* local);
void transfer_right_sharded(TT& t, size_t k, const ShardLayout& lay);
void remove_left_excess(TT& t, const ShardLayout& lay);

// reduce_to_maximal_ranks (ttNetwork.cpp:370-402) of the internal ranks; true if any rank exceeds it
std::vector<size_t> maximal_ranks(const TT& t);
bool exceeds_maximal_ranks(const TT& t);

// Range control of round() (tt.hip). The Gram chains multiply the squares of all cores, and a sweep gathers the
// scale of every core it has passed in one, so a TT whose cores' exponents add up to 2^+-300 is far outside
// them although each core, and the tensor, is representable. probe_core_ranges enqueues the norm of every
// core and its copy to pinned host memory, without a synchronisation; core_range_exceeded reads it after the
// caller's next host wait: true when the exponents of the cores' scales (norm over the root of the unfolding
// rank: 0 for the orthonormal cores of a canonical TT) summed over some run of neighbouring cores exceed 200
// in magnitude -- the device-resident rounds then give up (range_hit) before their iterative kernels see
// inf / NaN, and round() repeats itself on cores brought to scale ~ 1 by exact powers of two, whose product
// it gives back to core 0.
void probe_core_ranges(TT& t);
bool core_range_exceeded(const TT& t);

// relative downward shift of the certifying Cholesky factorisations (see tt.hip, round_chain)
constexpr double kGramShift = 1e-11;
constexpr double kOrthTol = 1e-13;   // max |C_k C_k^T - I| accepted for the right-canonical cores

// Gram chains (k = 1..d-1): left G_{k+1} = M_k^T (G_k M_k), right H_k = M_k (I (x) H_{k+1}) M_k^T
void left_gram_step(TT& t, std::vector<double*>& G, double* T, size_t k, bool do_reduce = true);
void right_gram_step(TT& t, std::vector<double*>& H, double* T, size_t k, bool do_reduce = true);
void gram_chains(TT& t, std::vector<double*>& G, std::vector<double*>& H, std::vector<DevBuf>& store, bool left = true);

struct DevIdArgs {
    const double* G[64];
    int n[64];
    double* out;
};
// max |G_i - I| of a batch of square matrices; out[i * gridDim.y + slice]
__global__ void k_dev_identity_many(const DevIdArgs args);

// The orthogonality check of the cores C with ranks r (d + 1): max |C_k C_k^T - I| of the right unfoldings of
// cores 1..d-1 (`rows`) or max |C_k^T C_k - I| of the left unfoldings of cores 0..d-2, kOrthSlices values per
// core. Enqueues the Grams (one buffer, pushed onto `keep`; sharded: completed by ONE all-reduce), the
// deviations and their copy to the pinned `host`; returns the number of values, valid after the next host wait.
// With `aux` (an open fork of an unsharded TT; `on_main[k]`: core k was written on the main lane) only the
// same-shape group of Grams with the most flops stays on the main lane; the others go to the fork's side lane
// behind the cores' writers there, and the fork is joined before the deviations. Either way the fork is joined
// when the call returns.
constexpr int kOrthSlices = 16;
int orth_enqueue(TT& t, std::vector<DevBuf>& keep, const std::vector<double*>& C, const size_t* r, bool rows, double* host,
                 StreamFork* aux = nullptr, const std::vector<bool>* on_main = nullptr);
// NaN-propagating maximum of the check's values
inline double worst_dev(const double* v, int count) {
    double worst = 0.0;
    for (int i = 0; i < count; ++i) worst = (v[i] > worst || v[i] != v[i]) ? v[i] : worst;
    return worst;
}
// first non-zero status word, -1 when every factorisation succeeded
inline int first_bad(const int* status, int count) {
    for (int i = 0; i < count; ++i)
        if (status[i] != 0) return i;
    return -1;
}

// Independent GEMMs; the ones of identical shape go out as one batched launch.
struct GemmJob {
    size_t M, N, K, lda, ldb;
    bool ta, tb;
    const double* A;
    const double* B;
    double* C;
    bool sym = false;   // result known symmetric (M == N): lower tiles only, mirrored
    double alpha = 1.0;
    int tri = 0;        // triangular operands (kTriA / kTriB, gemm): zero K-blocks skipped
};
void gemm_grouped(xrs_handle_t h, const std::vector<GemmJob>& jobs);
// in_largest[i]: job i belongs to the same-shape group (gemm_grouped's grouping) with the most flops, the
// first such group on a tie. That group fills the chip; the others are a handful of workgroups each.
std::vector<bool> largest_group(const std::vector<GemmJob>& jobs);

// largest rank of the certified chain / truncating rounds (blocked Cholesky above 512, the 1024-column
// register tiling of the block Jacobi SVD)
constexpr size_t kHugeMax = 1024;

// the reference's two-sweep algorithm pieces (sequential, host-synchronising)
void transfer_right(TT& t, size_t k, bool rank_reduce);   // transfer_core(k -> k+1): QC (or QR) + R * next
void orth_right(TT& t, size_t k);
size_t svd_cut(const std::vector<double>& s, size_t max_rank, double eps);
// round_edge (tensorNetwork.cpp:678-818) of the edge k-1 | k, core moving to k-1; soft > 0 replaces the
// kept singular values by max(0, sigma - soft) (round_edge's _softThreshold, :766 / :788)
void truncate_edge(TT& t, size_t k, size_t max_rank, double eps, double soft = 0.0);
// TTNetwork::soft_threshold (ttNetwork.cpp:688-713): canonicalize_right, then round_edge(maxRank = inf,
// eps = 0, soft = taus[i]) over the edges right to left, taus[0] at the last edge (the reference's order)
void soft_threshold(TT& t, bool canonicalized, size_t core_pos, const double* taus);

// one right chain pass restoring right-orthonormality of nearly orthonormal cores (tt.hip)
bool reorthonormalize(TT& t);

// certified truncating round (tt_trunc.hip): left-canonical chain pass + device-resident right-to-left
// truncation sweep with one host synchronisation; false (cores untouched) when a certificate fails
bool round_truncate(TT& t, const size_t* max_ranks, double eps);

// general truncating round (tt_trunc.hip): any spectrum, maxRank and eps cuts, shifted CholeskyQR3 +
// Jacobi SVD per edge, enqueued with device-side rank cuts and one synchronisation; false (cores
// untouched) when a certificate fails (possible QC rank drop, breakdown, non-orthonormal result)
bool round_general(TT& t, const size_t* max_ranks, double eps);

}  // namespace ttd
}  // namespace xrs
