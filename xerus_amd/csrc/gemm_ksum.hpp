// Host side of the summed GEMM xrs_gemm_ksum (gemm_ksum.hip): the argument checks and the slicing arithmetic, as
// plain C++ without any device dependency, so that a stand-alone host program can run them (tools/ksum_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/xerus_amd.h"

namespace xrs {

constexpr size_t kKsumTable = 32;          // segments per launch (the by-value table)
constexpr size_t kKsumChunk = 16;          // K-step: the concatenated K is measured in chunks of 16 per segment
constexpr size_t kKsumTargetGroups = 512;  // two workgroups per CU of a 256-CU device
constexpr size_t kKsumMinChunks = 4;       // a slice contracts at least 64 k (where there are that many)
constexpr size_t kKsumMaxSlices = 64;      // bounds the slab scratch at 64 M N doubles per launch

struct KsumLaunch {
    size_t first, count;       // segments [first, first + count) of the call
    size_t chunks;             // their 16-wide chunks
    size_t chunks_per_slice;   // per workgroup row of the grid
    size_t slices;             // grid.y
    size_t slab0;              // first slab this launch writes
};

struct KsumPlan {
    size_t tile = 64, tiles_m = 0, tiles_n = 0;
    size_t slabs = 0;                    // over all launches; 1: the one launch writes C itself, 0: C = 0
    std::vector<KsumLaunch> launches;   // launches whose segments are all empty are left out
};

// A function of the shape arguments only: the same call is cut the same way on every run.
inline KsumPlan ksum_plan(size_t M, size_t N, size_t count, const size_t* K) {
    KsumPlan p;
    // 64 x 64 tiles only where their grid alone fills a 256-CU device. Below that the 32 x 32 grid has four times
    // the workgroups and needs fewer slices or none (measured at 2720 x 136, DESIGN §3.12: 15.1 against 20.0 us at two
    // terms of K = 128, 21.3 against 23.5 at three, 49.2 against 46.0 at eight)
    const size_t big = ((M + 63) / 64) * ((N + 63) / 64);
    p.tile = (M <= 32 || N <= 32 || big < 256) ? 32 : 64;
    p.tiles_m = (M + p.tile - 1) / p.tile;
    p.tiles_n = (N + p.tile - 1) / p.tile;
    const size_t tiles = p.tiles_m * p.tiles_n;
    for (size_t j0 = 0; j0 < count; j0 += kKsumTable) {
        KsumLaunch l{};
        l.first = j0;
        l.count = std::min<size_t>(kKsumTable, count - j0);
        for (size_t s = 0; s < l.count; ++s) l.chunks += (K[j0 + s] + kKsumChunk - 1) / kKsumChunk;
        if (l.chunks == 0) continue;
        size_t slices = std::max<size_t>(1, kKsumTargetGroups / tiles);
        slices = std::min({slices, (l.chunks + kKsumMinChunks - 1) / kKsumMinChunks, kKsumMaxSlices});
        l.chunks_per_slice = (l.chunks + slices - 1) / slices;
        l.slices = (l.chunks + l.chunks_per_slice - 1) / l.chunks_per_slice;
        l.slab0 = p.slabs;
        p.slabs += l.slices;
        p.launches.push_back(l);
    }
    return p;
}

inline bool ksum_overlaps(const double* a, size_t na, const double* b, size_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 8 * nb && b0 < a0 + 8 * na;
}

// null when the arguments are legal, else what is wrong with them. No pointer is dereferenced but the tables.
inline const char* ksum_check(const double* C, size_t M, size_t N, size_t count, const double* const* A, const size_t* lda,
                              const size_t* K, const double* const* B, const size_t* ldb) {
    if (!(C && A && lda && K && B && ldb)) return "null argument";
    if (count < 1) return "count must be at least 1";
    if (count >= (size_t(1) << 31)) return "too many segments";
    if (M == 0 || N == 0) return "M and N must be positive";
    if (M >= (size_t(1) << 30) || N >= (size_t(1) << 30) || M > (size_t(1) << 40) / N) return "result too large";
    size_t chunks = 0;
    for (size_t j = 0; j < count; ++j) {
        if (K[j] == 0) continue;   // contributes nothing; its pointers are not looked at
        if (!(A[j] && B[j])) return "null operand of a segment with K > 0";
        if (K[j] >= (size_t(1) << 31)) return "segment K too large";
        if (lda[j] < K[j] || ldb[j] < N) return "leading dimension smaller than the row length";
        if (lda[j] >= (size_t(1) << 40) || ldb[j] >= (size_t(1) << 40)) return "leading dimension too large";
        const size_t na = (M - 1) * lda[j] + K[j], nb = (K[j] - 1) * ldb[j] + N;
        if (ksum_overlaps(C, M * N, A[j], na) || ksum_overlaps(C, M * N, B[j], nb)) return "C must not alias an operand";
        chunks += (K[j] + kKsumChunk - 1) / kKsumChunk;
        if (chunks >= (size_t(1) << 31)) return "concatenated K too large";
    }
    return nullptr;
}

// C = alpha sum_j A_j B_j, enqueued only (gemm_ksum.hip); the arguments are checked (xrs::Error, XRS_EINVAL)
void gemm_ksum(xrs_handle_t h, double* C, size_t M, size_t N, double alpha, size_t count, const double* const* A,
               const size_t* lda, const size_t* K, const double* const* B, const size_t* ldb);

}  // namespace xrs
