// Device helpers shared by the iterations on the local operator (als_local.hip: CG, als_eig.hip: LOBPCG): the
// launch shape of their vector kernels (CB, CMAXB, blocks_for) and the sum of the block partials in one fixed order
// (sum_partials), which makes every block hold the same scalar without a grid barrier or a floating-point atomic.
// The sum over a block itself is reduce_dev.hpp's block_sum_all, wave partials added sequentially from 0.0.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "reduce_dev.hpp"

namespace xrs {
namespace als_local {

constexpr int CB = 256;       // threads per block
constexpr int CMAXB = 1024;   // max blocks (= partial sums per reduction)

// the block's sum, in every thread
__device__ __forceinline__ double block_sum_all(double v) {
    __shared__ double part[CB / 64];
    const double s = xrs::block_sum_all<Order::from_zero, CB / 64>(v, part);
    __syncthreads();
    return s;
}

// the sum of nb block partials, in every thread of every block in the same order
__device__ __forceinline__ double sum_partials(const double* __restrict__ partial, int nb) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += CB) acc += partial[i];
    return block_sum_all(acc);
}

inline int blocks_for(size_t n) { return int(std::max<size_t>(1, std::min<size_t>(CMAXB, (n + size_t(CB) * 4 - 1) / (size_t(CB) * 4)))); }

}  // namespace als_local
}  // namespace xrs
