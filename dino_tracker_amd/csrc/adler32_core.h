// adler32_core.h -- the block-sum form of the Adler-32 (RFC 1950 section 9), shared by the decoder (inflate.hip: adler32_kernel
// COMPARES it with a stream's trailer) and the encoder (deflate.hip: adler32_store_kernel WRITES it there).  Device code only.
#pragma once
#include "common.h"

#ifdef __HIPCC__
constexpr int ATHREADS = 256, AGROUP = 16;
constexpr unsigned ADLER_MOD = 65521u;

// The Adler-32 of d[0 .. N): s1 = 1 + sum d[i], s2 = N + sum (N - i) d[i], both mod 65521.  Every thread of the ATHREADS-wide block
// calls; THREAD 0 holds the result.
// A tile of 16 x 256 bytes: thread t reads the bytes tile + 256 j + t, whose weights are N - tile - t - 256 j, so its share is
// w * sum d[j] - 256 sum j d[j] with w = (N - tile - t) mod 65521
__device__ __forceinline__ unsigned adler32_block(const uint8_t* __restrict__ d, long long N) {
    __shared__ unsigned long long part[3][ATHREADS / WAVE];
    const int tid = threadIdx.x;
    unsigned long long s1 = 0, a = 0, b = 0;
    for (long long tile = 0; tile < N; tile += (long long)ATHREADS * AGROUP) {
        unsigned sum = 0, wsum = 0;
#pragma unroll
        for (int j = 0; j < AGROUP; ++j) {
            const long long i = tile + (long long)j * ATHREADS + tid;
            const unsigned v = i < N ? d[i] : 0u;
            sum += v;
            wsum += (unsigned)j * v;
        }
        s1 += sum;
        a = (a + (unsigned long long)((N - tile - tid) % ADLER_MOD + ADLER_MOD) % ADLER_MOD * sum) % ADLER_MOD;
        b += (unsigned long long)ATHREADS * wsum;
    }
    unsigned long long v[3] = {s1 % ADLER_MOD, a, b % ADLER_MOD};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int r = wave_sum_i((int)v[k]);   // 64 values below 65521
        if ((tid & (WAVE - 1)) == 0) part[k][tid / WAVE] = (unsigned long long)r;
    }
    __syncthreads();
    unsigned value = 0;
    if (tid == 0) {
        unsigned long long t[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k)
            for (int w = 0; w < ATHREADS / WAVE; ++w) t[k] += part[k][w];
        const unsigned c1 = (unsigned)((1 + t[0]) % ADLER_MOD);
        const unsigned c2 = (unsigned)(((unsigned long long)(N % ADLER_MOD) + t[1] + ADLER_MOD - t[2] % ADLER_MOD) % ADLER_MOD);
        value = (c2 << 16) | c1;
    }
    return value;
}
#endif
