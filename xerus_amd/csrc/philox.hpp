// The counter-based Gaussian matrix G(seed, stream) of the randomized sketches: an infinite
// matrix whose entry (i, c) depends on (seed, stream, i, c) only, so every kernel -- the fused sketch, the
// materialising one, whatever tiling either uses -- sees the same bits.
//
//   words    W(i, q) = Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
//            SC'11) with key = (seed low 32, seed high 32) and counter = (q low 32, q high 32, i, stream),
//            q = c / 4; rows and streams are below 2^32.
//   normals  Box-Muller in fp32, widened to fp64: with u1 = (w0 + 1) 2^-32 in (0, 1], u2 = w1 2^-32,
//            G(i, 4q) = sqrt(-2 ln u1) cos 2 pi u2, G(i, 4q + 1) = the same with sin; (w2, w3) give
//            G(i, 4q + 2), G(i, 4q + 3) likewise. |G| <= sqrt(64 ln 2) = 6.66.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace xrs {
namespace philox {

struct Words {
    uint32_t w[4];
};

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;   // round multipliers
constexpr uint32_t kKey0 = 0x9E3779B9u, kKey1 = 0xBB67AE85u;   // key increments (golden ratio, sqrt 3 - 1)

__host__ __device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                        uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = uint64_t(kMul0) * c0, p1 = uint64_t(kMul1) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c1 = uint32_t(p1);
        c3 = uint32_t(p0);
        c0 = n0;
        c2 = n2;
        k0 += kKey0;
        k1 += kKey1;
    }
    return Words{{c0, c1, c2, c3}};
}

// W(i, q)
__host__ __device__ __forceinline__ Words words(uint64_t seed, uint32_t stream, uint32_t i, uint64_t q) {
    return philox4x32_10(uint32_t(q), uint32_t(q >> 32), i, stream, uint32_t(seed), uint32_t(seed >> 32));
}

#ifdef __HIPCC__
// one Box-Muller pair on the fp32 transcendental units: v_log_f32 (log2), v_sqrt_f32, v_sin_f32 / v_cos_f32
// (argument in revolutions, so u2 goes in as it is)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, double& c, double& s) {
    const float u1 = (float(wa) + 1.0f) * 0x1p-32f;   // (0, 1]: the sum rounds, it never wraps
    const float u2 = float(wb) * 0x1p-32f;            // [0, 1]
    const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));   // -2 ln 2 log2 u1
    c = double(r * __builtin_amdgcn_cosf(u2));
    s = double(r * __builtin_amdgcn_sinf(u2));
}

// THE definition of G: g[j] = G(i, 4 q + j), j = 0..3. Every kernel that needs G calls this function.
__device__ __forceinline__ void gauss4(uint64_t seed, uint32_t stream, uint32_t i, uint64_t q, double (&g)[4]) {
    const Words x = words(seed, stream, i, q);
    box_muller(x.w[0], x.w[1], g[0], g[1]);
    box_muller(x.w[2], x.w[3], g[2], g[3]);
}
#endif

}  // namespace philox
}  // namespace xrs
