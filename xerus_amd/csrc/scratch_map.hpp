// Map of the handle's two 64 KiB scratch areas: the pinned host one (host_scratch: read-backs of scalars,
// statuses, norms) and the device one (dev_scratch: reduction partials and results). Every user takes its
// region through host<T>() / dev<T>() below, which check the amount it is about to use against the region.
#pragma once
#include <string>

#include "runtime.hpp"

namespace xrs {
namespace scratch {

constexpr size_t kBytes = size_t(1) << 16;   // size of each area (runtime.cpp)

struct Region {
    size_t off, len;   // bytes
    const char* owner;
};

template <size_t N>
constexpr bool disjoint_within(const Region (&r)[N], size_t lo, size_t hi) {
    for (size_t i = 0; i < N; ++i) {
        if (r[i].len == 0 || r[i].off < lo || r[i].off + r[i].len > hi) return false;
        for (size_t j = 0; j < i; ++j)
            if (r[i].off < r[j].off + r[j].len && r[j].off < r[i].off + r[i].len) return false;
    }
    return true;
}

// ---- pinned host area ------------------------------------------------------------------------------------
// kHostLocal is call-local: a routine copies into it, waits and reads before it returns, and starts no other
// user of it in between, so its users need no separation from each other (slots inside it: below). The other
// regions stay live across calls -- a copy is enqueued into them by one routine and read behind a later host
// wait, with other routines' read-backs in between -- and so are disjoint from it and from each other.
constexpr Region kHostLocal{0, 16384, "call-local read-backs (read_status, reductions, <x,y>, chain_check, ...)"};
constexpr Region kHostTruncDev{16384, 16384, "truncating rounds: (d - 1) x 16 orthonormality deviations"};
constexpr Region kHostDotOnes{32768, 16, "dot_two_ended: the unit boundary environments (upload source)"};
constexpr Region kHostRangeAmax{32784, 8, "range_controlled: max |A|, read behind the factorisation's own wait"};
constexpr Region kHostShardLayout{32800, 16320, "shard_layout: world x d mode-size table (<= 2040 doubles)"};
constexpr Region kHostChainStatus{49152, 3072, "chain_pass: factorisation statuses (<= 64 edges x 3 jobs x 4 words)"};
constexpr Region kHostTruncStatus{53248, 4096, "round_truncate: the 1024 status words of a sweep"};
constexpr Region kHostRangeProbe{57600, 7680, "probe_core_ranges: one norm per core (<= 960)"};
constexpr Region kHostMap[] = {kHostLocal,       kHostTruncDev,    kHostDotOnes,     kHostRangeAmax,
                               kHostShardLayout, kHostChainStatus, kHostTruncStatus, kHostRangeProbe};
static_assert(disjoint_within(kHostMap, 0, kBytes), "pinned scratch regions overlap or leave the allocation");
// round_general starts after the chain and the truncating round have read their statuses, and takes both
// regions (and the gap between them) as its own 2048 status words
constexpr Region kHostGeneralStatus{kHostChainStatus.off, 8192, "round_general: 2048 status words"};
static_assert(kHostGeneralStatus.off + kHostGeneralStatus.len == kHostTruncStatus.off + kHostTruncStatus.len);

// slots inside kHostLocal. The first five are used side by side within one factorisation and are disjoint;
// the last two belong to routines that use nothing else of the area while they wait.
constexpr Region kHostResult{0, 64, "a scalar result or up to 16 status words"};
constexpr Region kHostOrthEmax{64, 64, "orthogonalize: the 8 partial maxima of its first-order pass"};
constexpr Region kHostIdentityDev{256, 8, "max_abs_dev_identity"};
constexpr Region kHostAmax{384, 8, "range_exponent: max |A|"};
constexpr Region kHostCgState{128, 64, "als_local_cg: the iteration's state words (CgState)"};
constexpr Region kHostEigState{192, 64, "als_local_eig: the iteration's state words (EigState)"};
constexpr Region kHostLocalSlots[] = {kHostResult, kHostOrthEmax, kHostCgState, kHostEigState, kHostIdentityDev, kHostAmax};
static_assert(disjoint_within(kHostLocalSlots, kHostLocal.off, kHostLocal.off + kHostLocal.len));
constexpr Region kHostChainDev{512, 8192, "chain_check: (d - 1) x 16 orthonormality deviations"};
constexpr Region kHostSvdCheck{640, 40, "svd_bidiag: residuals (4 doubles) and the multisection status"};
static_assert(kHostChainDev.off + kHostChainDev.len <= kHostLocal.len && kHostSvdCheck.off + kHostSvdCheck.len <= kHostLocal.len);

// ---- device area (stream-ordered: a region is reused behind the kernels that read it) -----------------------
constexpr Region kDevResult{0, 8, "reduce_to_host: the reduced scalar"};
constexpr Region kDevIdentityDev{256, 8, "max_abs_dev_identity"};
constexpr Region kDevOrthEmax{320, 64, "orthogonalize: the 8 partial maxima of its first-order pass"};
constexpr Region kDevAmax{384, 8, "range_exponent: max |A|"};
constexpr Region kDevRangeAmax{392, 8, "range_controlled: max |A|"};
constexpr Region kDevPartials{512, 24576, "reduce_to_device: 3 x 1024 partial sums"};
constexpr Region kDevRangeProbe{32768, 7680, "probe_core_ranges: one norm per core (<= 960)"};
constexpr Region kDevCgState{40960, 64, "als_local_cg: rr, rr_prev, pq, ||b||^2, threshold; done, skip, status, iterations"};
constexpr Region kDevEigState{41024, 64, "als_local_eig: theta, theta_next, rr, ||M x0||^2, threshold; done, skip, status, iterations"};
constexpr Region kDevCgPartials{45056, 16384, "als_local_cg: 2 x 1024 partial sums (p.q / b.b and r.r)"};
constexpr Region kDevMap[] = {kDevResult,    kDevIdentityDev, kDevOrthEmax, kDevAmax,      kDevRangeAmax,
                              kDevPartials, kDevRangeProbe,  kDevCgState,  kDevEigState,   kDevCgPartials};
static_assert(disjoint_within(kDevMap, 0, kBytes), "device scratch regions overlap or leave the allocation");

template <class T>
T* at(void* base, const Region& r, size_t count) {
    XRS_REQUIRE(count * sizeof(T) <= r.len, std::string("scratch region too small -- ") + r.owner);
    return reinterpret_cast<T*>(static_cast<char*>(base) + r.off);
}
// the region as an array of T, of which `count` elements are about to be used
template <class T>
T* host(xrs_handle_t h, const Region& r, size_t count = 1) { return at<T>(h->host_scratch, r, count); }
template <class T>
T* dev(xrs_handle_t h, const Region& r, size_t count = 1) { return at<T>(h->dev_scratch, r, count); }

}  // namespace scratch
}  // namespace xrs
