// of_prep.hip -- optical-flow trajectory preprocessing on the device (SURVEY 8f N1 inputs):
//
//   dtk_traj_start_fg   : preprocessing/split_trajectories_to_fg_bg.py:61-67 -- first tracked frame of every trajectory, its
//                         point rounded half-to-even, the foreground mask read there.
//   dtk_nearest_traj    : preprocessing_dino_bb/of_filter_dino_best_buddies.py:9-29 + :50-54 -- for every frame t and every
//                         token-grid point g the trajectory n nearest to it at t, argmin over (d^2, n): first index on ties,
//                         NaN = +inf, 0 when frame t has no tracked point.
//   dtk_of_filter_keep  : of_filter_dino_best_buddies.py:83-94 -- the keep flag of every best buddy of every frame pair.
//
// Trajectories are [N][T][2] fp32 (x, y), NaN where a point is not tracked (a point is untracked if either coordinate is NaN,
// `isnan().any(dim=-1)`).  The nearest search compacts the tracked points of every frame first (order-preserving, so a lane
// scanning candidates in list order sees increasing n and a strict `<` keeps the first minimum), then brute-forces
// (grid point x candidate) pairs with packed fp32 and merges the candidate splits with a 64-bit atomicMin on the key
// (bits(d^2) << 32 | n): d^2 >= 0, so its IEEE bits order like the value and the key orders like (d^2, n).
#include <math.h>
#include <algorithm>
#include "block_scan.h"

namespace {

constexpr int OF_BLOCK = 256;          // rows per block of the compaction passes; threads of every kernel here
constexpr int NN_PTS = 4;              // grid points per lane of the nearest search
constexpr int NN_TILE = 1024;          // candidates per LDS tile
constexpr unsigned long long NN_EMPTY = ~0ull;

typedef float f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool tracked(float x, float y) { return !(isnan(x) || isnan(y)); }

// ---- fg / bg split ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OF_BLOCK) void traj_start_fg_kernel(const float* __restrict__ traj, int N, int T,
                                                                 const uint8_t* __restrict__ masks, int Tm, int H, int W,
                                                                 uint8_t* __restrict__ fg, int32_t* __restrict__ err) {
    const long long n = (long long)blockIdx.x * OF_BLOCK + threadIdx.x;
    if (n >= N) return;
    const f2* row = reinterpret_cast<const f2*>(traj) + (size_t)n * T;
    int s = 0;
    f2 p = {NAN, NAN};
    for (; s < T; ++s) {
        p = row[s];
        if (tracked(p.x, p.y)) break;
    }
    // torch.round == rint (half to even); .int() of an integral float
    const float rx = rintf(p.x), ry = rintf(p.y);
    const bool ok = s < T && s < Tm && rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H;
    uint8_t v = 0;
    if (ok) v = masks[((size_t)s * H + (int)ry) * W + (int)rx] > 0 ? 1 : 0;
    else atomicAdd(err, 1);
    fg[n] = v;
}

// ---- nearest trajectory: order-preserving compaction of every frame's tracked points -------------------------------------
// count[t * nblk + b] = tracked points of frame t among the rows of block b
__global__ __launch_bounds__(OF_BLOCK) void nn_count_kernel(const float* __restrict__ traj, int N, int T, int nblk,
                                                            int32_t* __restrict__ count) {
    const int b = blockIdx.x, t = blockIdx.y;
    const long long n = (long long)b * OF_BLOCK + threadIdx.x;
    bool v = false;
    if (n < N) {
        const f2 p = reinterpret_cast<const f2*>(traj)[(size_t)n * T + t];
        v = tracked(p.x, p.y);
    }
    const int c = block_count<OF_BLOCK / WAVE>(v);
    if (threadIdx.x == 0) count[(size_t)t * nblk + b] = c;
}

// frame t's tracked points in row order: pts[t * N + k] = (x, y), ids[t * N + k] = n
__global__ __launch_bounds__(OF_BLOCK) void nn_compact_kernel(const float* __restrict__ traj, int N, int T, int nblk,
                                                              const int32_t* __restrict__ offs, f2* __restrict__ pts,
                                                              int32_t* __restrict__ ids) {
    const int b = blockIdx.x, t = blockIdx.y;
    const long long n = (long long)b * OF_BLOCK + threadIdx.x;
    f2 p = {NAN, NAN};
    if (n < N) p = reinterpret_cast<const f2*>(traj)[(size_t)n * T + t];
    const bool v = tracked(p.x, p.y);
    const int rank = block_rank<OF_BLOCK / WAVE>(v);
    if (v) {
        const size_t at = (size_t)t * N + offs[(size_t)t * nblk + b] + rank;
        pts[at] = p;
        ids[at] = (int32_t)n;
    }
}

__global__ __launch_bounds__(OF_BLOCK) void nn_init_kernel(unsigned long long* __restrict__ key, size_t n) {
    for (size_t i = (size_t)blockIdx.x * OF_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * OF_BLOCK) key[i] = NN_EMPTY;
}

// grid (gblk, T, ksplit): block (gb, t, k) owns grid points gb * 1024 + threadIdx.x + 256 j (j < 4) of frame t and scans
// the candidate tiles k, k + ksplit, ... of the frame in order.
__global__ __launch_bounds__(OF_BLOCK) void nn_search_kernel(const f2* __restrict__ pts, const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ total, int N, int gh, int gw,
                                                             float origin, float stride, unsigned long long* __restrict__ key) {
    __shared__ f2 s_pt[NN_TILE];
    __shared__ int32_t s_id[NN_TILE];
    const int t = blockIdx.y, k = blockIdx.z, ksplit = gridDim.z;
    const int G = gh * gw;
    const int cnt = total[t];
    const int ntiles = (cnt + NN_TILE - 1) / NN_TILE;
    if (k >= ntiles) return;
    const f2* fp = pts + (size_t)t * N;
    const int32_t* fi = ids + (size_t)t * N;

    // points j and j + 1 share one packed register pair
    f2 gx[NN_PTS / 2], gy[NN_PTS / 2];
    float best[NN_PTS];
    int bn[NN_PTS];
#pragma unroll
    for (int j = 0; j < NN_PTS; ++j) {
        const int g = blockIdx.x * (OF_BLOCK * NN_PTS) + threadIdx.x + j * OF_BLOCK;
        const int gc = g < G ? g : G - 1;
        gx[j / 2][j % 2] = origin + stride * (float)(gc % gw);
        gy[j / 2][j % 2] = origin + stride * (float)(gc / gw);
        best[j] = INFINITY;
        bn[j] = -1;
    }
    for (int tile = k; tile < ntiles; tile += ksplit) {
        const int c0 = tile * NN_TILE;
        const int nc = min(NN_TILE, cnt - c0);
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += OF_BLOCK) {
            s_pt[i] = fp[c0 + i];
            s_id[i] = fi[c0 + i];
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < nc; ++i) {
            const f2 c = s_pt[i];
            const int id = s_id[i];
            const f2 cx = {c.x, c.x}, cy = {c.y, c.y};
#pragma unroll
            for (int h = 0; h < NN_PTS / 2; ++h) {
                const f2 dx = cx - gx[h], dy = cy - gy[h];
                const f2 d2 = dx * dx + dy * dy;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int j = 2 * h + e;
                    const bool lt = d2[e] < best[j];   // candidates arrive in increasing n: strict < keeps the first minimum
                    best[j] = lt ? d2[e] : best[j];
                    bn[j] = lt ? id : bn[j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NN_PTS; ++j) {
        const int g = blockIdx.x * (OF_BLOCK * NN_PTS) + threadIdx.x + j * OF_BLOCK;
        if (g < G && bn[j] >= 0) {
            const unsigned long long kv = ((unsigned long long)__float_as_uint(best[j]) << 32) | (unsigned)bn[j];
            atomicMin(key + (size_t)t * G + g, kv);
        }
    }
}

__global__ __launch_bounds__(OF_BLOCK) void nn_finish_kernel(const unsigned long long* __restrict__ key, size_t n,
                                                             int32_t* __restrict__ idx) {
    const size_t i = (size_t)blockIdx.x * OF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long kv = key[i];
    idx[i] = kv == NN_EMPTY ? 0 : (int32_t)(unsigned)(kv & 0xffffffffull);   // all-inf argmin = 0
}

// ---- optical-flow filter ------------------------------------------------------------------------------------------------------
// torch's floor_divide of floats (c10 div_floor_floating): Python semantics, not floor(a / b)
__device__ __forceinline__ float div_floor(float a, float b) {
    const float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.f && (b < 0.f) != (mod < 0.f)) div -= 1.f;
    if (div == 0.f) return copysignf(0.f, a / b);
    float fl = floorf(div);
    if (div - fl > 0.5f) fl += 1.f;
    return fl;
}

__device__ __forceinline__ bool cell_of(const float* xy, float origin, float stride, int gh, int gw, int* cell) {
    const float cx = div_floor(xy[0] - origin, stride), cy = div_floor(xy[1] - origin, stride);
    if (!(cx >= 0.f && cx < (float)gw && cy >= 0.f && cy < (float)gh)) return false;
    *cell = (int)cy * gw + (int)cx;
    return true;
}

__device__ __forceinline__ bool lost(const float* traj, int T, int n, int t) {
    const f2 p = reinterpret_cast<const f2*>(traj)[(size_t)n * T + t];
    return !tracked(p.x, p.y);
}

// one block per frame pair p = (s, t), entries pair_off[p] .. pair_off[p + 1]
__global__ __launch_bounds__(OF_BLOCK) void of_filter_kernel(const float* __restrict__ traj, int N, int T,
                                                             const int32_t* __restrict__ idx, int gh, int gw, float origin,
                                                             float stride, const float* __restrict__ src,
                                                             const float* __restrict__ tgt, const int32_t* __restrict__ pair_off,
                                                             const int32_t* __restrict__ pair_st, uint8_t* __restrict__ keep,
                                                             int32_t* __restrict__ err) {
    const int p = blockIdx.x;
    const int s = pair_st[2 * p], t = pair_st[2 * p + 1];
    const int e0 = pair_off[p], e1 = pair_off[p + 1];
    const int G = gh * gw;
    const bool frames_ok = s >= 0 && s < T && t >= 0 && t < T;
    int bad = 0;
    for (int e = e0 + threadIdx.x; e < e1; e += OF_BLOCK) {
        int cs, ct;
        uint8_t v = 0;
        if (frames_ok && cell_of(src + 2 * (size_t)e, origin, stride, gh, gw, &cs) &&
            cell_of(tgt + 2 * (size_t)e, origin, stride, gh, gw, &ct)) {
            const int ns = idx[(size_t)s * G + cs], nt = idx[(size_t)t * G + ct];
            // the reference keeps a buddy when BOTH trajectories are lost at the other frame (of_filter_dino_best_buddies.py:93)
            if (ns >= 0 && ns < N && nt >= 0 && nt < N) v = (lost(traj, T, ns, t) && lost(traj, T, nt, s)) ? 1 : 0;
            else ++bad;
        } else {
            ++bad;
        }
        keep[e] = v;
    }
    if (bad) atomicAdd(err, bad);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct NnLayout {
    size_t pts, ids, count, total, key, bytes;
};

NnLayout nn_layout(int N, int T, int G) {
    const int nblk = dtk_cdiv(N, OF_BLOCK);
    NnLayout L;
    L.pts = 0;
    L.ids = L.pts + align256((size_t)N * T * sizeof(f2));
    L.count = L.ids + align256((size_t)N * T * sizeof(int32_t));
    L.total = L.count + align256((size_t)nblk * T * sizeof(int32_t));
    L.key = L.total + align256((size_t)T * sizeof(int32_t));
    L.bytes = L.key + align256((size_t)T * G * sizeof(unsigned long long));
    return L;
}

}  // namespace

extern "C" int dtk_traj_start_fg(const float* traj, int N, int T, const uint8_t* masks, int Tm, int H, int W, uint8_t* fg,
                                 int32_t* err, void* stream) {
    DTK_REQUIRE(N >= 0 && T > 0 && Tm > 0 && H > 0 && W > 0, "traj_start_fg: bad sizes N=%d T=%d masks %dx%dx%d", N, T, Tm, H, W);
    DTK_REQUIRE(traj && masks && fg && err, "traj_start_fg: null pointer");
    hipStream_t st = dtk_stream(stream);
    DTK_HIP(dtk_zero_async(err, sizeof(int32_t), st));
    if (N == 0) return 0;
    DTK_LAUNCH("traj_start_fg", traj_start_fg_kernel, dim3(dtk_cdiv(N, OF_BLOCK)), dim3(OF_BLOCK), 0, st, traj, N, T, masks, Tm,
               H, W, fg, err);
    return 0;
}

extern "C" size_t dtk_nearest_traj_workspace_bytes(int N, int T, int gh, int gw) {
    if (N < 0 || T <= 0 || gh <= 0 || gw <= 0) return 0;
    return nn_layout(N, T, gh * gw).bytes;
}

extern "C" int dtk_nearest_traj(const float* traj, int N, int T, int gh, int gw, float origin, float stride, int32_t* idx,
                                void* workspace, size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(N >= 0 && T > 0 && gh > 0 && gw > 0 && stride > 0.f, "nearest_traj: bad sizes N=%d T=%d grid %dx%d", N, T, gh, gw);
    DTK_REQUIRE((long long)gh * gw < (1LL << 31) / NN_PTS, "nearest_traj: grid too large");
    DTK_REQUIRE(idx && (traj || N == 0), "nearest_traj: null pointer");
    const int G = gh * gw;
    const NnLayout L = nn_layout(N, T, G);
    if (workspace_bytes < L.bytes) {
        dtk_set_error("nearest_traj: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
        return DTK_E_WORKSPACE;
    }
    hipStream_t st = dtk_stream(stream);
    char* ws = static_cast<char*>(workspace);
    f2* pts = reinterpret_cast<f2*>(ws + L.pts);
    int32_t* ids = reinterpret_cast<int32_t*>(ws + L.ids);
    int32_t* count = reinterpret_cast<int32_t*>(ws + L.count);
    int32_t* total = reinterpret_cast<int32_t*>(ws + L.total);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(ws + L.key);
    const size_t TG = (size_t)T * G;
    const unsigned init_blocks = (unsigned)std::min<size_t>(8192, (TG + OF_BLOCK - 1) / OF_BLOCK);
    DTK_LAUNCH("nn_init", nn_init_kernel, dim3(init_blocks), dim3(OF_BLOCK), 0, st, key, TG);
    if (N > 0) {
        const int nblk = dtk_cdiv(N, OF_BLOCK);
        DTK_LAUNCH("nn_count", nn_count_kernel, dim3(nblk, T), dim3(OF_BLOCK), 0, st, traj, N, T, nblk, count);
        // one block per frame: count[t][*] -> exclusive offsets in place, total[t]
        DTK_LAUNCH("nn_scan", block_offsets_kernel<OF_BLOCK / WAVE>, dim3(T), dim3(OF_BLOCK), 0, st, count, nblk, total);
        DTK_LAUNCH("nn_compact", nn_compact_kernel, dim3(nblk, T), dim3(OF_BLOCK), 0, st, traj, N, T, nblk, count, pts, ids);
        // candidate splits: ~16 blocks per CU over (grid blocks x frames), never more than the tiles of a full frame
        const int gblk = dtk_cdiv(G, OF_BLOCK * NN_PTS);
        const int max_tiles = dtk_cdiv(N, NN_TILE);
        int ksplit = dtk_cdiv(4096, (long long)gblk * T);
        ksplit = std::max(1, std::min(ksplit, std::min(max_tiles, 65535)));
        DTK_LAUNCH("nn_search", nn_search_kernel, dim3(gblk, T, ksplit), dim3(OF_BLOCK), 0, st, pts, ids, total, N, gh, gw,
                   origin, stride, key);
    }
    DTK_LAUNCH("nn_finish", nn_finish_kernel, dim3((unsigned)((TG + OF_BLOCK - 1) / OF_BLOCK)), dim3(OF_BLOCK), 0, st, key, TG,
               idx);
    return 0;
}

extern "C" int dtk_of_filter_keep(const float* traj, int N, int T, const int32_t* idx, int gh, int gw, float origin,
                                  float stride, const float* src, const float* tgt, const int32_t* pair_off,
                                  const int32_t* pair_st, int P, uint8_t* keep, int32_t* err, void* stream) {
    DTK_REQUIRE(N > 0 && T > 0 && gh > 0 && gw > 0 && P >= 0 && stride > 0.f, "of_filter_keep: bad sizes N=%d T=%d P=%d", N, T, P);
    DTK_REQUIRE(traj && idx && err && (P == 0 || (pair_off && pair_st)), "of_filter_keep: null pointer");
    hipStream_t st = dtk_stream(stream);
    DTK_HIP(dtk_zero_async(err, sizeof(int32_t), st));
    if (P == 0) return 0;
    DTK_LAUNCH("of_filter", of_filter_kernel, dim3(P), dim3(OF_BLOCK), 0, st, traj, N, T, idx, gh, gw, origin, stride, src, tgt,
               pair_off, pair_st, keep, err);
    return 0;
}
