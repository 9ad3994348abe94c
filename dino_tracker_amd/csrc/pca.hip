// pca.hip -- the PCA foreground masks of preprocessing/create_fg_mask.py on the device:
//
//   dtk_pca_moments : mean[C] and the centred Gram  cov = sum_n (x^_n - mu)(x^_n - mu)^T  of a token-major volume [N][C]
//                     (x^ = F.normalize(x) when `normalize`), two passes: row norms + mean, then the Gram on the matrix cores.
//   dtk_pca_project : colors[N][q] = x^_n . V[j] (rows NOT centred, as the reference projects them) + min / max per component.
//   dtk_fg_mask     : (c - min) / (max - min) < thr on one component -> token mask [T][h][w] and its nearest upsampling
//                     [T][H][W] (destination row y reads source row floor(y h / H)), 0 / 255.
//
// The Gram.  The contraction index is the TOKEN, so for v_mfma_f32_32x32x16_f16 both operands are column reads of one
// token-major tile: lane (r = l & 31, hf = l >> 5) needs X[16 s + 8 hf + j][32 cb + r], j < 8, for A (cb = a channel block of
// the output's rows) and for B (of its columns).  One LDS image per stage serves both through ds_read_b64_tr_b16: a 16-lane
// group reads 4 token rows x 16 channels and receives them channel-on-lane; two reads make a fragment.  Any k order is right
// as long as A and B use the same one, and they do: both come from tr_frag().  The instruction needs EXEC all ones, so the
// token tail is padded with rows that are exactly zero in both planes (pad, don't mask) and the only branch around the reads is
// wave-uniform.
//   image: [32 tokens][256 channels] fp16, hi and lo planes, rows of 512 + 64 bytes -- the pad moves the 4 rows of one read 16
//          banks apart, so a 32-lane half (4 rows x 64 bytes) covers the 64 banks once.  Columns 0..127 hold the panel of the
//          output block's rows, 128..255 that of its columns; a diagonal block stages one panel and reads it twice.
//   values: v = x * rnorm[n] - mu[c] (one fma), hi = fp16(v), lo = fp16(v - hi); three products lo.hi + hi.lo + hi.hi in fp32.
//          With `normalize` the values are scaled by 2^8 before the split (|v| <= 2, so nothing overflows, and lo stays a normal
//          fp16 down to |v| = 2^-11 instead of 2^-3); the reduction multiplies by 2^-16.  Both are exact.
//   work:  workgroup = (128 x 128 output block on or above the diagonal) x (chunk of tokens), 4 waves of 64 x 64; in a diagonal
//          block the wave below the diagonal computes nothing.  Register staging (the fp32 source rules LDS-DMA out), two LDS
//          buffers, one barrier per stage.  Every workgroup writes its partial block with vector stores; pca_reduce_kernel sums
//          the chunks in index order (in double) and writes element (i, j), i <= j, to both cov[i][j] and cov[j][i] -- no
//          floating-point atomics, so two calls are bit-identical and cov is exactly symmetric.
#include <math.h>
#include <algorithm>
#include "common.h"

namespace {

typedef _Float16 half_t;
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4 lds_s4;

constexpr int PCA_THREADS = 256;
constexpr int PCA_KT = 32;                         // tokens per stage
constexpr int PCA_BLK = 128;                       // channels per panel = side of a workgroup's output block
constexpr int PCA_ROWB = 2 * PCA_BLK * 2 + 64;     // bytes per token row of the image (two panels + the bank pad)
constexpr int PCA_PLANE = PCA_KT * PCA_ROWB;
constexpr int PCA_BUF = 2 * PCA_PLANE;             // hi + lo
constexpr int PCA_LDS = 2 * PCA_BUF;               // two stages
constexpr int PCA_MAX_GROUPS = 2048;               // workgroups of the row passes (partials per column)
constexpr int PCA_MAX_CHUNKS = 4096;
constexpr int PCA_Q = 8;

template <int C>
struct RowMap {   // a wave holds one row: lane l owns columns VEC * l + 64 * VEC * k + e
    static constexpr int VEC = C == 384 ? 2 : 4;
    static constexpr int K = C / (64 * VEC);
    static constexpr int PER = K * VEC;
};

template <int C>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int lane, float (&v)[RowMap<C>::PER]) {
    typedef RowMap<C> M;
#pragma unroll
    for (int k = 0; k < M::K; ++k) {
        const float* p = row + M::VEC * lane + 64 * M::VEC * k;
        if constexpr (M::VEC == 4) {
            const float4 t = *reinterpret_cast<const float4*>(p);
            v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
        } else {
            const float2 t = *reinterpret_cast<const float2*>(p);
            v[2 * k] = t.x, v[2 * k + 1] = t.y;
        }
    }
}

template <int C>
__device__ __forceinline__ float row_scale(const float (&v)[RowMap<C>::PER], int normalize) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < RowMap<C>::PER; ++i) ss = fmaf(v[i], v[i], ss);
    ss = wave_sum(ss);
    return normalize ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : 1.f;   // F.normalize: x / max(||x||, eps)
}

// ---- pass 1: rnorm[n] = 1 / max(||x_n||, 1e-12) (1 when !normalize), psum[group][c] = sum of x^ over the group's rows --------
template <int C>
__global__ __launch_bounds__(PCA_THREADS) void pca_rowstats_kernel(const float* __restrict__ x, long long N, int normalize,
                                                                   long long rows_per_group, float* __restrict__ rnorm,
                                                                   float* __restrict__ psum) {
    typedef RowMap<C> M;
    __shared__ float red[PCA_THREADS / WAVE][C];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const long long r0 = (long long)blockIdx.x * rows_per_group;
    const long long r1 = r0 + rows_per_group < N ? r0 + rows_per_group : N;
    float acc[M::PER];
#pragma unroll
    for (int i = 0; i < M::PER; ++i) acc[i] = 0.f;
    for (long long n = r0 + w; n < r1; n += PCA_THREADS / WAVE) {   // wave-uniform
        float v[M::PER];
        load_row<C>(x + (size_t)n * C, lane, v);
        const float inv = row_scale<C>(v, normalize);
        if (lane == 0) rnorm[n] = inv;
#pragma unroll
        for (int i = 0; i < M::PER; ++i) acc[i] += v[i] * inv;
    }
#pragma unroll
    for (int k = 0; k < M::K; ++k)
#pragma unroll
        for (int e = 0; e < M::VEC; ++e) red[w][M::VEC * lane + 64 * M::VEC * k + e] = acc[M::VEC * k + e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += PCA_THREADS)
        psum[(size_t)blockIdx.x * C + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// mean[c] = (sum over the groups, in a fixed order, of psum[g][c]) / N: 32 columns per block, the groups dealt to 32 slices
constexpr int PCA_MEAN_COLS = 32, PCA_MEAN_SLICES = 32;
__global__ __launch_bounds__(PCA_MEAN_COLS * PCA_MEAN_SLICES) void pca_mean_kernel(const float* __restrict__ psum, int groups, int C,
                                                                                   long long N, float* __restrict__ mean) {
    __shared__ double part[PCA_MEAN_SLICES][PCA_MEAN_COLS];
    const int col = threadIdx.x % PCA_MEAN_COLS, slice = threadIdx.x / PCA_MEAN_COLS;
    const int c = blockIdx.x * PCA_MEAN_COLS + col;   // C is a multiple of 32
    double s = 0.0;
    for (int g = slice; g < groups; g += PCA_MEAN_SLICES) s += (double)psum[(size_t)g * C + c];
    part[slice][col] = s;
    __syncthreads();
    if (slice == 0) {
        double t = 0.0;
        for (int k = 0; k < PCA_MEAN_SLICES; ++k) t += part[k][col];
        mean[c] = (float)(t / (double)N);
    }
}

// ---- pass 2: the centred Gram ------------------------------------------------------------------------------------------------
// fragment of the 32x32x16 operand for channels col .. col + 31 (image columns) and the 16 tokens of k-step ks, from the plane
// at `plane`: `lane_off` is the lane's part of the address -- token row 8 hf + q of the step, columns 16 (group & 1) + 4 p
__device__ __forceinline__ h8 tr_frag(const char* plane, int ks, int col, int lane_off) {
    const char* p = plane + (16 * ks) * PCA_ROWB + col * 2 + lane_off;
    const h4 a = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(p)));
    const h4 b = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(p + 4 * PCA_ROWB)));
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

struct Stage {
    float4 v[8];
    float s[8];
};

__global__ __launch_bounds__(PCA_THREADS, 2) void pca_gram_kernel(const float* __restrict__ x, long long N, int C,
                                                                  long long chunk_rows, const float* __restrict__ rnorm,
                                                                  const float* __restrict__ mean, float scale,
                                                                  float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // grid (block pairs, chunks): the workgroups of one chunk are dispatched together and walk the same tokens
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    // block pair (bi <= bj) of this workgroup
    const int nb = C / PCA_BLK;
    int bi = 0, rest = blockIdx.x;
    while (rest >= nb - bi) {
        rest -= nb - bi;
        ++bi;
    }
    const int bj = bi + rest;
    const bool diag = bi == bj;
    const long long r0 = (long long)blockIdx.y * chunk_rows;
    const long long r1 = r0 + chunk_rows < N ? r0 + chunk_rows : N;
    const int stages = (int)((r1 - r0 + PCA_KT - 1) / PCA_KT);

    // staging: a thread owns 4 channels of one panel and every (256 >> sh)-th token row of the stage
    const int sh = diag ? 5 : 6;
    const int col4 = tid & ((1 << sh) - 1), row0 = tid >> sh, rows_per_it = PCA_THREADS >> sh, nit = PCA_KT / rows_per_it;
    const int gcol = col4 < 32 ? bi * PCA_BLK + 4 * col4 : bj * PCA_BLK + 4 * (col4 - 32);
    float4 mu = *reinterpret_cast<const float4*>(mean + gcol);
    mu.x *= scale, mu.y *= scale, mu.z *= scale, mu.w *= scale;

    // The loads of a stage are unconditional and nothing in fetch() reads their results: a row past the chunk loads the chunk's
    // last row instead and is zeroed in stash().  (A load inside `if (n < r1)` followed by arithmetic on its result made the
    // compiler wait for every earlier load of the stage inside each branch: eight round trips per stage instead of one.)
    auto fetch = [&](int t, Stage& st) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            if (it < nit) {
                const long long n = r0 + (long long)t * PCA_KT + it * rows_per_it + row0;
                const long long nc = n < r1 ? n : r1 - 1;
                st.v[it] = *reinterpret_cast<const float4*>(x + (size_t)nc * C + gcol);
                st.s[it] = rnorm[nc];
            }
        }
    };
    auto stash = [&](int t, const Stage& st, char* buf) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            if (it < nit) {
                const bool ok = r0 + (long long)t * PCA_KT + it * rows_per_it + row0 < r1;
                const float sc = st.s[it] * scale;
                float e[4] = {fmaf(st.v[it].x, sc, -mu.x), fmaf(st.v[it].y, sc, -mu.y), fmaf(st.v[it].z, sc, -mu.z),
                              fmaf(st.v[it].w, sc, -mu.w)};
                h4 hi, lo;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float v = ok ? e[c] : 0.f;   // rows past the chunk: exactly zero in both planes
                    hi[c] = (half_t)v;
                    lo[c] = (half_t)(v - (float)hi[c]);
                }
                char* p = buf + (it * rows_per_it + row0) * PCA_ROWB + col4 * 8;
                *reinterpret_cast<h4*>(p) = hi;
                *reinterpret_cast<h4*>(p + PCA_PLANE) = lo;
            }
        }
    };

    const int wi = w >> 1, wj = w & 1;
    const bool active = !(diag && wi > wj);             // wave-uniform
    const int acol = 64 * wi, bcol = (diag ? 0 : PCA_BLK) + 64 * wj;
    const int lane_off = (8 * (lane >> 5) + ((lane & 15) >> 2)) * PCA_ROWB + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
    f16v acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    Stage st;
    fetch(0, st);
    stash(0, st, smem);
    __syncthreads();
    for (int t = 0; t < stages; ++t) {
        const char* cur = smem + (t & 1) * PCA_BUF;
        const bool more = t + 1 < stages;
        if (more) fetch(t + 1, st);
        if (active) {
#pragma unroll
            for (int ks = 0; ks < PCA_KT / 16; ++ks) {
                h8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    ah[m] = tr_frag(cur, ks, acol + 32 * m, lane_off);
                    al[m] = tr_frag(cur + PCA_PLANE, ks, acol + 32 * m, lane_off);
                    bh[m] = tr_frag(cur, ks, bcol + 32 * m, lane_off);
                    bl[m] = tr_frag(cur + PCA_PLANE, ks, bcol + 32 * m, lane_off);
                }
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[m], bh[n], acc[m][n], 0, 0, 0);
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bl[n], acc[m][n], 0, 0, 0);
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[m], bh[n], acc[m][n], 0, 0, 0);
                    }
            }
        }
        if (more) stash(t + 1, st, smem + ((t + 1) & 1) * PCA_BUF);
        __syncthreads();
    }
    if (!active) return;
    // C/D map of the 32x32 tile: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    float* out = partial + (size_t)blockIdx.y * C * C;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int i0 = bi * PCA_BLK + 64 * wi + 32 * m, j0 = bj * PCA_BLK + 64 * wj + 32 * n;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                out[(size_t)(i0 + row) * C + j0 + (lane & 31)] = acc[m][n][r];
            }
        }
}

// cov[i][j] = cov[j][i] = unscale * sum over the chunks, in chunk order, of partial[k][i][j]  (i <= j: every such element lies
// in a 64 x 64 tile that pca_gram_kernel computed)
__global__ __launch_bounds__(PCA_THREADS) void pca_reduce_kernel(const float* __restrict__ partial, int chunks, int C,
                                                                 float unscale, float* __restrict__ cov) {
    const int idx = blockIdx.x * PCA_THREADS + threadIdx.x;
    const int i = idx / C, j = idx - i * C;
    if (i >= C || i > j) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += (double)partial[(size_t)k * C * C + idx];
    const float v = (float)s * unscale;
    cov[(size_t)i * C + j] = v;
    cov[(size_t)j * C + i] = v;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(PCA_THREADS) void pca_project_kernel(const float* __restrict__ x, long long N, int normalize,
                                                                  long long rows_per_group, const float* __restrict__ V, int q,
                                                                  float* __restrict__ colors, float* __restrict__ pmm) {
    typedef RowMap<C> M;
    __shared__ float Vs[PCA_Q * C];
    __shared__ float smm[PCA_THREADS / WAVE][2 * PCA_Q];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    for (int i = threadIdx.x; i < q * C; i += PCA_THREADS) Vs[i] = V[i];
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * rows_per_group;
    const long long r1 = r0 + rows_per_group < N ? r0 + rows_per_group : N;
    float mn[PCA_Q], mx[PCA_Q];
#pragma unroll
    for (int j = 0; j < PCA_Q; ++j) mn[j] = INFINITY, mx[j] = -INFINITY;
    for (long long n = r0 + w; n < r1; n += PCA_THREADS / WAVE) {   // wave-uniform
        float v[M::PER];
        load_row<C>(x + (size_t)n * C, lane, v);
        const float inv = row_scale<C>(v, normalize);
#pragma unroll
        for (int i = 0; i < M::PER; ++i) v[i] *= inv;
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < PCA_Q; ++j) {
            if (j < q) {
                float d = 0.f;
#pragma unroll
                for (int k = 0; k < M::K; ++k)
#pragma unroll
                    for (int e = 0; e < M::VEC; ++e)
                        d = fmaf(v[M::VEC * k + e], Vs[j * C + M::VEC * lane + 64 * M::VEC * k + e], d);
                d = wave_sum(d);
                mn[j] = fminf(mn[j], d);
                mx[j] = fmaxf(mx[j], d);
                mine = lane == j ? d : mine;
            }
        }
        if (lane < q) colors[(size_t)n * q + lane] = mine;
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < PCA_Q; ++j) smm[w][j] = mn[j], smm[w][PCA_Q + j] = mx[j];
    }
    __syncthreads();
    if (threadIdx.x < 2 * PCA_Q) {
        const int o = threadIdx.x;
        float r = smm[0][o];
        for (int k = 1; k < PCA_THREADS / WAVE; ++k) r = o < PCA_Q ? fminf(r, smm[k][o]) : fmaxf(r, smm[k][o]);
        pmm[(size_t)blockIdx.x * 2 * PCA_Q + o] = r;
    }
}

// one wave per output: minmax[j] = min, minmax[8 + j] = max over the groups
__global__ __launch_bounds__(WAVE) void pca_minmax_kernel(const float* __restrict__ pmm, int groups, float* __restrict__ minmax) {
    const int o = blockIdx.x;
    const float sign = o < PCA_Q ? -1.f : 1.f;
    float r = -INFINITY;
    for (int g = threadIdx.x; g < groups; g += WAVE) r = fmaxf(r, sign * pmm[(size_t)g * 2 * PCA_Q + o]);
    r = wave_max(r);
    if (threadIdx.x == 0) minmax[o] = sign * r;
}

// ---- masks --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PCA_THREADS) void fg_token_mask_kernel(const float* __restrict__ colors, int q, int comp,
                                                                    const float* __restrict__ minmax, float thr, int flip,
                                                                    long long n_tokens, uint8_t* __restrict__ tok) {
    const long long n = (long long)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (n >= n_tokens) return;
    const float mn = minmax[comp], mx = minmax[PCA_Q + comp];
    float t = (colors[(size_t)n * q + comp] - mn) / (mx - mn);   // max == min: 0 / 0 = NaN compares false, as in the reference
    if (flip) t = 1.f - t;
    tok[n] = t < thr ? 255 : 0;
}

// F.interpolate(mode="nearest"): destination (y, x) reads source (floor(y h / H), floor(x w / W))
__global__ __launch_bounds__(PCA_THREADS) void fg_upsample_kernel(const uint8_t* __restrict__ tok, int h, int w, int H, int W,
                                                                  uint8_t* __restrict__ mask) {
    const int xx = blockIdx.x * PCA_THREADS + threadIdx.x, y = blockIdx.y, t = blockIdx.z;
    if (xx >= W) return;
    const int sy = (int)(((long long)y * h) / H), sx = (int)(((long long)xx * w) / W);
    mask[((size_t)t * H + y) * W + xx] = tok[((size_t)t * h + sy) * w + sx];
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool pca_width_ok(int C) { return C == 384 || C == 768 || C == 1024; }

int row_groups(long long N) { return (int)std::min<long long>(PCA_MAX_GROUPS, (N + 3) / 4); }

// tokens per chunk (a multiple of the stage) for a request; 0 = enough chunks for ~4 workgroups per CU, at least 512 rows each
long long gram_chunk_rows(long long N, int C, long long request) {
    long long rows = request;
    if (rows <= 0) {
        const int nb = C / PCA_BLK;
        const long long want = std::max(1, 1024 / (nb * (nb + 1) / 2));
        rows = std::max<long long>((N + want - 1) / want, 512);
    }
    return (rows + PCA_KT - 1) / PCA_KT * PCA_KT;
}

struct MomentsLayout {
    long long chunk_rows;
    int chunks, groups;
    size_t rnorm, psum, partial, bytes;
};

MomentsLayout moments_layout(long long N, int C, long long request) {
    MomentsLayout L;
    L.chunk_rows = gram_chunk_rows(N, C, request);
    const long long chunks = (N + L.chunk_rows - 1) / L.chunk_rows;
    L.chunks = (int)std::min<long long>(chunks, PCA_MAX_CHUNKS + 1);
    L.groups = row_groups(N);
    L.rnorm = 0;
    L.psum = L.rnorm + align256((size_t)N * sizeof(float));
    L.partial = L.psum + align256((size_t)L.groups * C * sizeof(float));
    L.bytes = L.partial + align256((size_t)L.chunks * C * C * sizeof(float));
    return L;
}

template <int C>
int moments_rows(const float* x, long long N, int normalize, const MomentsLayout& L, float* rnorm, float* psum, hipStream_t st) {
    const long long per = (N + L.groups - 1) / L.groups;
    DTK_LAUNCH("pca_rowstats", pca_rowstats_kernel<C>, dim3(L.groups), dim3(PCA_THREADS), 0, st, x, N, normalize, per, rnorm, psum);
    return 0;
}

template <int C>
int project_rows(const float* x, long long N, int normalize, int groups, const float* V, int q, float* colors, float* pmm,
                 hipStream_t st) {
    const long long per = (N + groups - 1) / groups;
    DTK_LAUNCH("pca_project", pca_project_kernel<C>, dim3(groups), dim3(PCA_THREADS), 0, st, x, N, normalize, per, V, q, colors,
               pmm);
    return 0;
}

}  // namespace

extern "C" size_t dtk_pca_moments_workspace_bytes(int64_t N, int32_t C, int64_t chunk_rows) {
    if (N <= 0 || !pca_width_ok(C) || chunk_rows < 0) return 0;
    return moments_layout(N, C, chunk_rows).bytes;
}

extern "C" int dtk_pca_moments(const float* x, int64_t N, int32_t C, int32_t normalize, int64_t chunk_rows, float* mean,
                               float* cov, void* workspace, size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(pca_width_ok(C), "pca_moments: C must be 384, 768 or 1024, got %d", C);
    DTK_REQUIRE(N > 0 && chunk_rows >= 0, "pca_moments: bad sizes N=%lld chunk_rows=%lld", (long long)N, (long long)chunk_rows);
    DTK_REQUIRE(x && mean && cov && workspace, "pca_moments: null pointer");
    const MomentsLayout L = moments_layout(N, C, chunk_rows);
    DTK_REQUIRE(L.chunks <= PCA_MAX_CHUNKS, "pca_moments: chunk_rows=%lld makes more than %d chunks of N=%lld", (long long)chunk_rows,
                PCA_MAX_CHUNKS, (long long)N);
    if (workspace_bytes < L.bytes) {
        dtk_set_error("pca_moments: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
        return DTK_E_WORKSPACE;
    }
    hipStream_t st = dtk_stream(stream);
    char* ws = static_cast<char*>(workspace);
    float* rnorm = reinterpret_cast<float*>(ws + L.rnorm);
    float* psum = reinterpret_cast<float*>(ws + L.psum);
    float* partial = reinterpret_cast<float*>(ws + L.partial);
    const int rc = C == 384 ? moments_rows<384>(x, N, normalize, L, rnorm, psum, st)
                 : C == 768 ? moments_rows<768>(x, N, normalize, L, rnorm, psum, st)
                            : moments_rows<1024>(x, N, normalize, L, rnorm, psum, st);
    if (rc) return rc;
    DTK_LAUNCH("pca_mean", pca_mean_kernel, dim3(C / PCA_MEAN_COLS), dim3(PCA_MEAN_COLS * PCA_MEAN_SLICES), 0, st, psum, L.groups,
               C, (long long)N, mean);
    DTK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pca_gram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                PCA_LDS));
    const int nb = C / PCA_BLK;
    const float scale = normalize ? 256.f : 1.f;
    DTK_LAUNCH("pca_gram", pca_gram_kernel, dim3(nb * (nb + 1) / 2, L.chunks), dim3(PCA_THREADS), PCA_LDS, st, x, (long long)N,
               C, L.chunk_rows, rnorm, mean, scale, partial);
    DTK_LAUNCH("pca_reduce", pca_reduce_kernel, dim3(dtk_cdiv((long long)C * C, PCA_THREADS)), dim3(PCA_THREADS), 0, st, partial,
               L.chunks, C, 1.f / (scale * scale), cov);
    return 0;
}

extern "C" size_t dtk_pca_project_workspace_bytes(int64_t N) {
    if (N <= 0) return 0;
    return align256((size_t)row_groups(N) * 2 * PCA_Q * sizeof(float));
}

extern "C" int dtk_pca_project(const float* x, int64_t N, int32_t C, int32_t normalize, const float* V, int32_t q, float* colors,
                               float* minmax, void* workspace, size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(pca_width_ok(C), "pca_project: C must be 384, 768 or 1024, got %d", C);
    DTK_REQUIRE(q >= 1 && q <= PCA_Q, "pca_project: q must be 1 .. %d, got %d", PCA_Q, q);
    DTK_REQUIRE(N > 0, "pca_project: bad size N=%lld", (long long)N);
    DTK_REQUIRE(x && V && colors && minmax && workspace, "pca_project: null pointer");
    const size_t need = dtk_pca_project_workspace_bytes(N);
    if (workspace_bytes < need) {
        dtk_set_error("pca_project: workspace %zu < %zu bytes", workspace_bytes, need);
        return DTK_E_WORKSPACE;
    }
    hipStream_t st = dtk_stream(stream);
    float* pmm = static_cast<float*>(workspace);
    const int groups = row_groups(N);
    const int rc = C == 384 ? project_rows<384>(x, N, normalize, groups, V, q, colors, pmm, st)
                 : C == 768 ? project_rows<768>(x, N, normalize, groups, V, q, colors, pmm, st)
                            : project_rows<1024>(x, N, normalize, groups, V, q, colors, pmm, st);
    if (rc) return rc;
    DTK_LAUNCH("pca_minmax", pca_minmax_kernel, dim3(2 * PCA_Q), dim3(WAVE), 0, st, pmm, groups, minmax);
    return 0;
}

extern "C" int dtk_fg_mask(const float* colors, int32_t q, int32_t comp, const float* minmax, float thr, int32_t flip, int32_t T,
                           int32_t h, int32_t w, int32_t H, int32_t W, uint8_t* mask, uint8_t* token_mask, void* stream) {
    DTK_REQUIRE(q >= 1 && q <= PCA_Q && comp >= 0 && comp < q, "fg_mask: q must be 1 .. %d and comp below it, got q=%d comp=%d",
                PCA_Q, q, comp);
    DTK_REQUIRE(T > 0 && h > 0 && w > 0 && H > 0 && W > 0 && T <= 65535 && H <= 65535, "fg_mask: bad sizes T=%d grid %dx%d image %dx%d",
                T, h, w, H, W);
    DTK_REQUIRE(colors && minmax && mask && token_mask, "fg_mask: null pointer");
    hipStream_t st = dtk_stream(stream);
    const long long n_tokens = (long long)T * h * w;
    DTK_LAUNCH("fg_token_mask", fg_token_mask_kernel, dim3(dtk_cdiv(n_tokens, PCA_THREADS)), dim3(PCA_THREADS), 0, st, colors, q,
               comp, minmax, thr, flip, n_tokens, token_mask);
    DTK_LAUNCH("fg_upsample", fg_upsample_kernel, dim3(dtk_cdiv(W, PCA_THREADS), H, T), dim3(PCA_THREADS), 0, st, token_mask, h, w,
               H, W, mask);
    return 0;
}
