// Stand-alone host check of xrs_gemm_ksum's argument checking and slicing arithmetic (xerus_amd/csrc/gemm_ksum.hpp),
// meant to be built with the host sanitizers; it needs no GPU and no HIP:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ixerus_amd/csrc \
//         tools/ksum_host_check.cpp -o tools/bin/ksum_host_check && tools/bin/ksum_host_check
//
// It walks shapes from 1 x 1 to the envelope's ends and segment counts around the table size, and checks of every plan
// that the slices of a launch cover its chunks exactly once, that slabs are numbered consecutively over the launches,
// that empty launches are left out, and that every illegal argument set is named. Operand pointers are made up from a
// host array and never dereferenced by the code under test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_ksum.hpp"

using namespace xrs;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static void check_plan(size_t M, size_t N, const std::vector<size_t>& K) {
    const KsumPlan p = ksum_plan(M, N, K.size(), K.data());
    EXPECT(p.tile == 32 || p.tile == 64);
    EXPECT(p.tiles_m * p.tile >= M && (p.tiles_m - 1) * p.tile < M);
    EXPECT(p.tiles_n * p.tile >= N && (p.tiles_n - 1) * p.tile < N);
    size_t slabs = 0, seen_chunks = 0, all_chunks = 0;
    for (size_t k : K) all_chunks += (k + kKsumChunk - 1) / kKsumChunk;
    for (const KsumLaunch& l : p.launches) {
        EXPECT(l.first % kKsumTable == 0 && l.count >= 1 && l.count <= kKsumTable && l.first + l.count <= K.size());
        size_t chunks = 0;
        for (size_t s = 0; s < l.count; ++s) chunks += (K[l.first + s] + kKsumChunk - 1) / kKsumChunk;
        EXPECT(chunks == l.chunks && chunks > 0);
        EXPECT(l.slices >= 1 && l.slices <= kKsumMaxSlices);
        EXPECT(l.chunks_per_slice * l.slices >= l.chunks);              // every chunk belongs to a slice
        EXPECT(l.chunks_per_slice * (l.slices - 1) < l.chunks);         // and no slice is empty
        EXPECT(l.slab0 == slabs);
        slabs += l.slices;
        seen_chunks += chunks;
    }
    EXPECT(slabs == p.slabs);
    EXPECT(seen_chunks == all_chunks);
    const KsumPlan again = ksum_plan(M, N, K.size(), K.data());         // a function of the shapes only
    EXPECT(again.slabs == p.slabs && again.launches.size() == p.launches.size() && again.tile == p.tile);
}

int main() {
    // ---- plans
    const size_t shapes[][2] = {{1, 1}, {16, 16}, {37, 19}, {65, 130}, {2720, 136}, {2880, 144}, {1, 100000}, {100000, 1}, {4096, 4096}};
    const size_t kset[] = {0, 1, 3, 4, 15, 16, 17, 130, 512, 100000};
    for (const auto& sh : shapes)
        for (size_t count : {size_t(1), size_t(2), size_t(5), size_t(31), size_t(32), size_t(33), size_t(64), size_t(65), size_t(200)})
            for (size_t shift = 0; shift < 10; ++shift) {
                std::vector<size_t> K(count);
                for (size_t j = 0; j < count; ++j) K[j] = kset[(j * 7 + shift) % 10];
                check_plan(sh[0], sh[1], K);
                std::vector<size_t> zeros(count, 0);
                const KsumPlan p = ksum_plan(sh[0], sh[1], count, zeros.data());
                EXPECT(p.slabs == 0 && p.launches.empty());
            }
    {   // the test suite's sliced case: one tile, 8 x 512 -> 256 chunks in 64 slices of 4
        std::vector<size_t> K(8, 512);
        const KsumPlan p = ksum_plan(16, 16, 8, K.data());
        EXPECT(p.tile == 32 && p.launches.size() == 1 && p.launches[0].slices == 64 && p.launches[0].chunks_per_slice == 4);
    }

    // ---- argument checks (pointers are only compared)
    std::vector<double> arena(1 << 16);
    double* base = arena.data();
    const size_t M = 16, N = 16;
    double* C = base;
    const double* A[3] = {base + 1000, base + 2000, base + 3000};
    const double* B[3] = {base + 4000, base + 5000, base + 6000};
    size_t lda[3] = {16, 20, 16}, ldb[3] = {16, 16, 24}, K[3] = {16, 17, 0};
    EXPECT(ksum_check(C, M, N, 3, A, lda, K, B, ldb) == nullptr);   // ragged, padded rows, an empty segment
    {
        const double* An[3] = {A[0], A[1], nullptr};
        const double* Bn[3] = {B[0], B[1], nullptr};
        EXPECT(ksum_check(C, M, N, 3, An, lda, K, Bn, ldb) == nullptr);   // null at K = 0
        An[0] = nullptr;
        EXPECT(ksum_check(C, M, N, 3, An, lda, K, Bn, ldb) != nullptr);   // null at K > 0
    }
    EXPECT(ksum_check(nullptr, M, N, 3, A, lda, K, B, ldb) != nullptr);
    EXPECT(ksum_check(C, M, N, 0, A, lda, K, B, ldb) != nullptr);
    EXPECT(ksum_check(C, 0, N, 3, A, lda, K, B, ldb) != nullptr);
    EXPECT(ksum_check(C, M, size_t(1) << 31, 3, A, lda, K, B, ldb) != nullptr);
    EXPECT(ksum_check(C, size_t(1) << 29, size_t(1) << 29, 3, A, lda, K, B, ldb) != nullptr);
    {
        size_t bad[3] = {8, 17, 16};
        EXPECT(ksum_check(C, M, N, 3, A, bad, K, B, ldb) != nullptr);     // lda < K
        EXPECT(ksum_check(C, M, N, 3, A, lda, K, B, bad) != nullptr);     // ldb < N
        size_t huge[3] = {size_t(1) << 31, 17, 0};
        EXPECT(ksum_check(C, M, N, 3, A, lda, huge, B, ldb) != nullptr);  // K too large (and above lda)
    }
    {   // aliasing: C overlapping the first or the last element of an operand
        const double* Aa[3] = {C + M * N - 1, A[1], A[2]};
        EXPECT(ksum_check(C, M, N, 3, Aa, lda, K, B, ldb) != nullptr);
        const double* Ab[3] = {C + M * N, A[1], A[2]};
        EXPECT(ksum_check(C, M, N, 3, Ab, lda, K, B, ldb) == nullptr);
        const double* Bb[3] = {B[0], C + 30000 - ((K[1] - 1) * ldb[1] + N), B[2]};   // ends where C begins
        EXPECT(ksum_check(C + 30000, M, N, 3, A, lda, K, Bb, ldb) == nullptr);
        const double* Bc[3] = {B[0], C + 30000 - ((K[1] - 1) * ldb[1] + N) + 1, B[2]};
        EXPECT(ksum_check(C + 30000, M, N, 3, A, lda, K, Bc, ldb) != nullptr);
        EXPECT(ksum_check(C, M, N, 1, &A[0], lda, K, reinterpret_cast<const double* const*>(&C), ldb) != nullptr);
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ksum_host_check: ok");
    return 0;
}
