// block_scan.h -- the integer block primitives behind every count / scan / write-at-offset-plus-rank stage of libdtk
// (anchors.hip, track_mfma.hip, of_prep.hip, flow_traj.hip, jpeg.hip).  Device code only.
//
// One contract for all of them:
//   * every thread of the block calls, and the block is the compile-time WAVES * 64 threads;
//   * a primitive may be called repeatedly and inside loops.  The primitives own their LDS: one array of WAVES values per value
//     type, shared by EVERY call site of a kernel, whichever primitive it is.  So each call opens with a barrier -- the array may
//     still be read from the previous call -- and has a second one between its write and its reads;
//   * integer types only (int and unsigned long long are in use).  The float reductions of the library pin their summation
//     order to the bit and stay where they are.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// inclusive scan over the wave's 64 lanes
template <class T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x % WAVE;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const T y = __shfl_up(v, o, WAVE);
        if (lane >= o) v += y;
    }
    return v;
}

// The step all block primitives share.  `wave_value` is what the wave contributes, read from its LAST lane; returns the sum over
// the waves below this one, total = the sum over all waves, in every thread.
template <int WAVES, class T>
__device__ __forceinline__ T block_wave_offset(T wave_value, T& total) {
    __shared__ T ws[WAVES];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == WAVE - 1) ws[wave] = wave_value;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T s = ws[w];
        base += w < wave ? s : (T)0;
        total += s;
    }
    return base;
}

// exclusive scan of one value per thread, in thread order; total = the block's sum, in every thread
template <int WAVES, class T>
__device__ __forceinline__ T block_scan_excl(T v, T& total) {
    const T incl = wave_scan_incl(v);
    return block_wave_offset<WAVES>(incl, total) + incl - v;
}

// the block's sum of one int per thread; every thread holds it
template <int WAVES>
__device__ __forceinline__ int block_sum_i(int v) {
    int total;
    block_wave_offset<WAVES>(wave_sum_i(v), total);
    return total;
}

// the number of set flags in the block; every thread holds it
template <int WAVES>
__device__ __forceinline__ int block_count(bool v) {
    int total;
    block_wave_offset<WAVES>((int)__popcll(__ballot(v)), total);
    return total;
}

// the number of set flags in the threads below this one: the rank of a set flag among the block's, in thread order
template <int WAVES>
__device__ __forceinline__ int block_rank(bool v) {
    const unsigned long long m = __ballot(v);
    int total;
    return block_wave_offset<WAVES>((int)__popcll(m), total) + (int)__popcll(m & ((1ull << (threadIdx.x % WAVE)) - 1ull));
}

// One block per segment: block b turns the counts c[b * n .. b * n + n) into their exclusive offsets in place and writes their sum
// to total[b].  (Internal linkage: every translation unit that launches it has its own.)
template <int WAVES>
static __global__ __launch_bounds__(WAVES * WAVE) void block_offsets_kernel(int32_t* __restrict__ c, int n,
                                                                            int32_t* __restrict__ total) {
    c += (size_t)blockIdx.x * n;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += WAVES * WAVE) {
        const int i = i0 + threadIdx.x;
        int sum;
        const int excl = block_scan_excl<WAVES>(i < n ? c[i] : 0, sum);
        if (i < n) c[i] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}
#endif
