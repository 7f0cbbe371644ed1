// Cross-lane and workgroup reductions of the kernels, one name per variant. The order in which partial results
// are combined is part of a kernel's contract (several results are bit-reproducible between builds), and so is
// the NaN rule of a maximum: two variants that look alike are different functions here. A new kernel picks one;
// it does not write the loop again. Device-only, internal linkage: each kernel file gets its own copy.
//   wave level       wave_reduce(v, op) and its front ends (64 lanes, xor butterfly, offsets 32 .. 1: every lane
//                    ends with the result); wave_arg_best (value + index, the lower index wins ties)
//   workgroup level  wave_partials (lane 0 of each wave writes red[wave], __syncthreads), then a named order
//                    over the partials: sum_pairwise4, sum_from_zero<NW>, sum_chain4 (sums), max_nan_from_first<NW>;
//                    block_sum_all / block_sum_t0<order, NW> are wave_sum + wave_partials + that order.
//                    None of them ends with a barrier: a caller that writes `red` again places its own.
//                    A kernel whose barrier is not a plain __syncthreads (a fence, an LDS-only barrier, work
//                    between the write and the barrier) uses the wave level and keeps its barrier and combine.
//   block_sum_tree   the LDS tree over all NT threads: another summation order than the shuffle form
//   block_trace      the per-wave partials of trace(A), for the trace-times-shift prologues
//   dpp, gsum<G>     sums over groups of 8 / 16 / 32 / 64 lanes without the LDS crossbar
//   fp64_max_as_float, wave_max_atomic   the max slots of the fp32 products
#pragma once
#include <hip/hip_runtime.h>

namespace xrs {

namespace {

// ---------------------------------------------------------------------------------------------- wave level
// v = op(v, the value of lane l ^ o) for o = 32, 16, .. 1
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
    return wave_reduce(v, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ int wave_sum(int v) {
    return wave_reduce(v, [](int a, int b) { return a + b; });
}
// fmax / fmin: a NaN operand is dropped
__device__ __forceinline__ double wave_fmax(double v) {
    return wave_reduce(v, [](double a, double b) { return fmax(a, b); });
}
__device__ __forceinline__ double wave_fmin(double v) {
    return wave_reduce(v, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ float wave_fmaxf(float v) {
    return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); });
}
// the other lane's value only where it compares greater / less: a NaN in another lane is skipped, an own NaN stays
__device__ __forceinline__ double wave_max_gt(double v) {
    return wave_reduce(v, [](double a, double b) { return b > a ? b : a; });
}
__device__ __forceinline__ double wave_min_lt(double v) {
    return wave_reduce(v, [](double a, double b) { return b < a ? b : a; });
}
// NaN-propagating max: a NaN in any lane is the result
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double wave_max_nan(double v) {
    return wave_reduce(v, [](double a, double b) { return max_nan(a, b); });
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
    return wave_reduce(v, [](unsigned a, unsigned b) { return max(a, b); });
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
    return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return b > a ? b : a; });
}

// The best value of the wave and its index, in every lane: another lane's pair replaces the own one where
// better(its value, own value), or where the values are equal and its index is lower.
template <class I, class Better>
__device__ __forceinline__ void wave_arg_best(double& v, I& idx, Better better) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const I oi = __shfl_xor(idx, o, 64);
        if (better(ov, v) || (ov == v && oi < idx)) {
            v = ov;
            idx = oi;
        }
    }
}

// ----------------------------------------------------------------------------------------- workgroup level
// lane 0 of every wave writes its value to red[wave]; barrier
template <class T>
__device__ __forceinline__ void wave_partials(T v, T* red) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
}

// The orders over the wave partials. They differ in rounding, and from_zero turns a sum of -0.0 partials into +0.0.
enum class Order {
    pairwise4,   // (r0 + r1) + (r2 + r3)
    from_zero,   // ((0.0 + r0) + r1) + .. over NW partials
    chain4,      // ((r0 + r1) + r2) + r3
};
__device__ __forceinline__ double sum_pairwise4(const double* red) { return (red[0] + red[1]) + (red[2] + red[3]); }
__device__ __forceinline__ double sum_chain4(const double* red) { return red[0] + red[1] + red[2] + red[3]; }
template <int NW>
__device__ __forceinline__ double sum_from_zero(const double* red) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) s += red[i];
    return s;
}
template <Order O, int NW>
__device__ __forceinline__ double combine_sum(const double* red) {
    static_assert(O == Order::from_zero || NW == 4, "the fixed orders are over four waves");
    if constexpr (O == Order::pairwise4) return sum_pairwise4(red);
    else if constexpr (O == Order::chain4) return sum_chain4(red);
    else return sum_from_zero<NW>(red);
}
// NaN-propagating max of NW partials, starting from the first
template <int NW>
__device__ __forceinline__ double max_nan_from_first(const double* red) {
    double m = red[0];
    for (int i = 1; i < NW; ++i) m = max_nan(m, red[i]);
    return m;
}

// The sum over a workgroup of NW waves (red: NW doubles of LDS), the wave partials combined in order O.
// _all: in every thread. _t0: in thread 0, the other threads return 0.0 and do not read red.
template <Order O, int NW = 4>
__device__ __forceinline__ double block_sum_all(double v, double* red) {
    wave_partials(wave_sum(v), red);
    return combine_sum<O, NW>(red);
}
template <Order O, int NW = 4>
__device__ __forceinline__ double block_sum_t0(double v, double* red) {
    wave_partials(wave_sum(v), red);
    double s = 0.0;
    if (threadIdx.x == 0) s = combine_sum<O, NW>(red);
    return s;
}
// NaN-propagating max over a workgroup of NW waves, valid in thread 0 (the other threads return their wave's)
template <int NW = 4>
__device__ __forceinline__ double block_max_nan_t0(double v, double* red) {
    v = wave_max_nan(v);
    wave_partials(v, red);
    if (threadIdx.x == 0) v = max_nan_from_first<NW>(red);
    return v;
}

// Fixed-order sum over the NT threads of a workgroup by an LDS tree (every thread returns the total): thread t
// adds the value of thread t + o for o = NT / 2 .. 1. Not the order of the shuffle forms above.
template <int NT>
__device__ double block_sum_tree(double v) {
    __shared__ double red[NT];
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (int(threadIdx.x) < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double t = red[0];
    __syncthreads();
    return t;
}

// Wave partials of trace(A) (A: n x n, row-major) of a workgroup of NT threads into red[0 .. NT / 64); barrier.
// The caller combines them in its own order (sum_pairwise4 / sum_from_zero / sum_chain4).
template <int NT, class N>
__device__ __forceinline__ void block_trace(const double* A, N n, double* red) {
    double tr = 0.0;
    for (N i = threadIdx.x; i < n; i += NT) tr += A[size_t(i) * n + i];
    wave_partials(wave_sum(tr), red);
}

// ------------------------------------------------------------------------------------------- DPP group sums
// Cross-lane sums without the LDS crossbar (a __shfl_xor of a double is two ds_bpermute round trips, the
// bulk of a column step when chained): DPP row rotations within 16 lanes, v_permlane16_swap across the
// two rows of a 32-lane half, v_permlane32_swap across the halves.
// DPP move of a double (two 32-bit moves); CTRL is a DPP16 control word whose every lane has a valid
// source (row rotations / mirrors / quad permutations), so no "old" value is needed (mov_dpp: no
// zero-initialised destination, which update_dpp(0, ...) costs two extra moves per double)
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// v + (the value of lane l ^ 16): the two results of v_permlane16_swap(v, v) are {own, partner} on every lane
// (odd rows get the even rows in the first, even rows the odd rows in the second), so their sum is the pair
// sum without the per-lane select -- one dependent operation less per level, bit-identical (a + b = b + a)
__device__ __forceinline__ double addx16(double v) {
    const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}
__device__ __forceinline__ double addx32(double v) {   // v + (the value of lane l ^ 32), v_permlane32_swap
    const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
    return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
}

// Sum over a group of G (8, 16, 32 or 64) consecutive lanes. Every lane of the group ends with the same bits:
// each step adds two values that are equal up to the order of operands of commutative adds.
//   G >= 16: row_ror 8, 4, 2, 1 (rotations of an increasingly periodic sequence), then addx16, addx32
//   G = 8:   row_half_mirror (i <-> 7-i), quad_perm [2,3,0,1] (i <-> i^2), quad_perm [1,0,3,2] (i <-> i^1)
template <int G>
__device__ __forceinline__ double gsum(double v) {
    if constexpr (G == 16 || G == 32 || G == 64) {
        v += dpp<0x128>(v);
        v += dpp<0x124>(v);
        v += dpp<0x122>(v);
        v += dpp<0x121>(v);
        if constexpr (G >= 32) v = addx16(v);
        if constexpr (G == 64) v = addx32(v);
    } else {
        static_assert(G == 8, "groups of 8, 16, 32 or 64 lanes");
        v += dpp<0x141>(v);
        v += dpp<0x4E>(v);
        v += dpp<0xB1>(v);
    }
    return v;
}

// ------------------------------------------------------------------------- max slots of the fp32 products
// an fp64 max|.| as a float for the max slots: above FLT_MAX -> inf, a nonzero max below the fp32 range -> the
// smallest denormal (so that the check sees it as out of range, not as a zero core)
__device__ __forceinline__ float fp64_max_as_float(double m) {
    const float f = float(m);
    return (m > 0.0 && f == 0.0f) ? __uint_as_float(1u) : f;
}
// the wave's max of m >= 0 into the word w (the bit patterns of non-negative floats order like the values)
__device__ __forceinline__ void wave_max_atomic(unsigned* w, float m) {
    m = wave_fmaxf(m);
    if ((threadIdx.x & 63) == 0) atomicMax(w, __float_as_uint(m));
}

}  // namespace

}  // namespace xrs
