// flow_traj.hip -- long-range trajectories chained from consecutive-frame optical flow, on the device: the second half of
// preprocessing/extract_trajectories.py (everything after the RAFT network).
//
//   dtk_flow_pack        : [n][2][h][w] planar flow -> [n][h][w] (x, y) pairs, so that a bilinear corner is one 8-byte load.
//   dtk_flow_cycle_masks : get_flows_with_masks :75-93 -- consistent[i + 1] = cycle error of (bflow[i], fflow[i]) < threshold AND the
//                          pixel is the rounded forward-warp target of some pixel of frame i; consistent[0] = 0.
//   dtk_flow_traj_start  : save_trajectories :208-256 for one starting frame s -- the start mask (inconsistent, or no kept
//                          trajectory of an earlier start passes through), its ordered compaction, one thread per live pixel
//                          walking frames s .. T - 1 (optionally with the direct-flow filter :143-158, :251-255) into a frame-major
//                          slab, and the ordered offsets of the rows that reach min_trajectory_length.  Leaves the row count on the
//                          device.
//   dtk_flow_traj_emit   : :258-266 -- the kept rows as [n][T][2] with NaN outside the live run (slab -> rows through LDS, so that
//                          both sides are contiguous per wave), and every live point of a kept row marked in visited[T][h][w].
//
// The arithmetic is the specification (include/dtk.h): fp32, one IEEE operation per step in grid_sample's order, no contraction,
// correctly rounded division and square root -- the results are bit-identical to the same operations issued one ATen op at a time.
// The reference's per-component mask and its one_nan_least pass reduce to one flag per trajectory: the mask only ever shrinks, so
// a thread stops at its first dead step.
#include <math.h>
#include "block_scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int FT_BLOCK = 256;   // threads of every kernel here; pixels / live trajectories per block of the compaction passes
constexpr int FT_CHUNK = 16;    // frames per LDS tile of the emit pass
constexpr int FT_PITCH = FT_CHUNK + 1;

typedef float f2 __attribute__((ext_vector_type(2)));

// grid_sample(align_corners=True) written out: x -> normalised -> source index, as the reference's bilinear_sampler and ATen do
__device__ __forceinline__ float src_index(float x, float size_m1) {
    const float g = __fdiv_rn(2.f * x, size_m1) - 1.f;
    return __fdiv_rn(g + 1.f, 2.f) * size_m1;
}

// four corner terms in the order nw, ne, sw, se, summed from zero; a corner outside the image contributes zero
__device__ __forceinline__ f2 corners(const f2* __restrict__ img, int h, int w, float ix, float iy) {
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float x1 = x0 + 1.f, y1 = y0 + 1.f;
    const float wx0 = x1 - ix, wx1 = ix - x0, wy0 = y1 - iy, wy1 = iy - y0;
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const bool bx0 = x0 >= 0.f && x0 <= wm1, bx1 = x1 >= 0.f && x1 <= wm1;   // false for NaN / inf
    const bool by0 = y0 >= 0.f && y0 <= hm1, by1 = y1 >= 0.f && y1 <= hm1;
    f2 acc = {0.f, 0.f};
    if (bx0 && by0) acc += img[(size_t)(int)y0 * w + (int)x0] * (wx0 * wy0);
    if (bx1 && by0) acc += img[(size_t)(int)y0 * w + (int)x1] * (wx1 * wy0);
    if (bx0 && by1) acc += img[(size_t)(int)y1 * w + (int)x0] * (wx0 * wy1);
    if (bx1 && by1) acc += img[(size_t)(int)y1 * w + (int)x1] * (wx1 * wy1);
    return acc;
}

__device__ __forceinline__ f2 bilinear_zero(const f2* __restrict__ img, int h, int w, f2 p) {
    return corners(img, h, w, src_index(p.x, (float)(w - 1)), src_index(p.y, (float)(h - 1)));
}

// border padding (utils.bilinear_interpolate_video): the source index is clamped to the image before the floor
__device__ __forceinline__ f2 bilinear_border(const f2* __restrict__ img, int h, int w, f2 p) {
    const float wm1 = (float)(w - 1), hm1 = (float)(h - 1);
    const float ix = fminf(wm1, fmaxf(src_index(p.x, wm1), 0.f));
    const float iy = fminf(hm1, fmaxf(src_index(p.y, hm1), 0.f));
    return corners(img, h, w, ix, iy);
}

__device__ __forceinline__ float dist(f2 a, f2 b) {
    const float dx = a.x - b.x, dy = a.y - b.y;
    return __fsqrt_rn(dx * dx + dy * dy);
}

__device__ __forceinline__ bool inside(f2 p, int h, int w) {
    return p.x >= 0.f && p.x <= (float)(w - 1) && p.y >= 0.f && p.y <= (float)(h - 1);
}

// torch.round (half to even) of a point, then the bounds test on the integral floats; false for NaN
__device__ __forceinline__ bool rounded_cell(f2 p, int h, int w, size_t* cell) {
    const float rx = rintf(p.x), ry = rintf(p.y);
    if (!(rx >= 0.f && rx <= (float)(w - 1) && ry >= 0.f && ry <= (float)(h - 1))) return false;
    *cell = (size_t)(int)ry * w + (int)rx;
    return true;
}

// ---- repack ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FT_BLOCK) void flow_pack_kernel(const float* __restrict__ src, f2* __restrict__ dst, size_t frames,
                                                             size_t hw) {
    const size_t total = frames * hw;
    for (size_t i = (size_t)blockIdx.x * FT_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * FT_BLOCK) {
        const size_t n = i / hw, p = i - n * hw;
        const f2 v = {src[(2 * n) * hw + p], src[(2 * n + 1) * hw + p]};
        dst[i] = v;
    }
}

__global__ __launch_bounds__(FT_BLOCK) void fill_bytes_kernel(uint8_t* __restrict__ p, size_t n, uint8_t v) {
    for (size_t i = (size_t)blockIdx.x * FT_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * FT_BLOCK) p[i] = v;
}

// ---- consistency masks -------------------------------------------------------------------------------------------------------
// grid (pixel blocks, T - 1): frame i's pixels mark their rounded forward-warp target in out[i + 1] (every store writes 1)
__global__ __launch_bounds__(FT_BLOCK) void warp_hit_kernel(const f2* __restrict__ fpk, int h, int w, uint8_t* __restrict__ out) {
    const int hw = h * w, i = blockIdx.y;
    const int p = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (p >= hw) return;
    const f2 g = {(float)(p % w), (float)(p / w)};
    size_t cell;
    if (rounded_cell(g + fpk[(size_t)i * hw + p], h, w, &cell)) out[(size_t)(i + 1) * hw + cell] = 1;
}

// out[i + 1][p] &= cycle error < threshold
__global__ __launch_bounds__(FT_BLOCK) void cycle_mask_kernel(const f2* __restrict__ fpk, const f2* __restrict__ bpk, int h, int w,
                                                              float threshold, uint8_t* __restrict__ out) {
    const int hw = h * w, i = blockIdx.y;
    const int p = blockIdx.x * FT_BLOCK + threadIdx.x;
    if (p >= hw) return;
    const f2 g = {(float)(p % w), (float)(p / w)};
    const f2 c1 = g + bpk[(size_t)i * hw + p];
    const f2 c2 = c1 + bilinear_zero(fpk + (size_t)i * hw, h, w, c1);
    const size_t at = (size_t)(i + 1) * hw + p;
    out[at] = (out[at] != 0 && dist(g, c2) < threshold) ? 1 : 0;
}

// ---- ordered compaction (count, block_offsets_kernel, write at offset + rank: the primitives of block_scan.h) ------------------
__device__ __forceinline__ bool start_live(const uint8_t* consistent, const uint8_t* visited, int p, int hw) {
    return p < hw && (consistent[p] == 0 || visited[p] == 0);
}

__global__ __launch_bounds__(FT_BLOCK) void start_count_kernel(const uint8_t* __restrict__ consistent,
                                                               const uint8_t* __restrict__ visited, int hw,
                                                               int32_t* __restrict__ count) {
    const int c = block_count<FT_BLOCK / WAVE>(start_live(consistent, visited, blockIdx.x * FT_BLOCK + threadIdx.x, hw));
    if (threadIdx.x == 0) count[blockIdx.x] = c;
}

__global__ __launch_bounds__(FT_BLOCK) void start_compact_kernel(const uint8_t* __restrict__ consistent,
                                                                 const uint8_t* __restrict__ visited, int hw,
                                                                 const int32_t* __restrict__ offs, int32_t* __restrict__ pix) {
    const int p = blockIdx.x * FT_BLOCK + threadIdx.x;
    const bool v = start_live(consistent, visited, p, hw);
    const int r = block_rank<FT_BLOCK / WAVE>(v);
    if (v) pix[offs[blockIdx.x] + r] = p;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
// thread i < *n_live walks live pixel pix[i] from frame s: slab[f * hw + i] = its position at frame s + f for f < len[i] (the live
// run; nothing is written behind it), and the block's number of rows with len >= min_len goes to keep_count[blockIdx.x].
template <bool DIRECT>
__global__ __launch_bounds__(FT_BLOCK) void walk_kernel(const f2* __restrict__ fpk, const f2* __restrict__ bpk,
                                                        const f2* __restrict__ dfwd, const f2* __restrict__ dback, int T, int h,
                                                        int w, int s, float threshold, float direct_threshold, int min_len,
                                                        const int32_t* __restrict__ n_live, const int32_t* __restrict__ pix,
                                                        f2* __restrict__ slab, int32_t* __restrict__ len,
                                                        int32_t* __restrict__ keep_count) {
    const size_t hw = (size_t)h * w;
    const int i = blockIdx.x * FT_BLOCK + threadIdx.x;
    int L = 0;
    if (i < *n_live) {
        const int p = pix[i];
        const f2 start = {(float)(p % w), (float)(p / w)};
        f2 pos = start;
        slab[i] = pos;
        L = 1;
        for (int k = 0; k < T - 1 - s; ++k) {
            const f2* ff = fpk + (size_t)(s + k) * hw;
            const f2* bf = bpk + (size_t)(s + k) * hw;
            const f2 nxt = pos + bilinear_zero(ff, h, w, pos);
            const f2 back = nxt + bilinear_zero(bf, h, w, nxt);
            bool live = dist(pos, back) < threshold && inside(nxt, h, w);
            if (DIRECT) {
                const f2 d = start + dfwd[(size_t)k * hw + p];
                const f2 d2 = d + bilinear_border(dback + (size_t)k * hw, h, w, d);
                const float dmask = (dist(start, d2) < threshold && inside(d, h, w)) ? 1.f : 0.f;
                live = live && dist(nxt, d) * dmask < direct_threshold;
            }
            if (!live) break;
            pos = nxt;
            slab[(size_t)L * hw + i] = pos;
            ++L;
        }
        len[i] = L;
    }
    const int kept = block_count<FT_BLOCK / WAVE>(L >= min_len);
    if (threadIdx.x == 0) keep_count[blockIdx.x] = kept;
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
// block b owns live trajectories b * 256 .. + 255, one wave per 64 of them.  The kept ones are rows keep_off[b] + rank of the
// output.  Per chunk of 16 frames a wave reads slab[f][its 64 trajectories] (contiguous), parks the points in its LDS tile and
// writes them back as 16-frame pieces of rows (128 contiguous bytes per row, four rows per step).
__global__ __launch_bounds__(FT_BLOCK) void emit_kernel(const f2* __restrict__ slab, const int32_t* __restrict__ len,
                                                        const int32_t* __restrict__ n_live, const int32_t* __restrict__ keep_off,
                                                        int T, int h, int w, int s, int min_len, int n_rows, f2* __restrict__ rows,
                                                        uint8_t* __restrict__ visited) {
    __shared__ f2 tile[FT_BLOCK / WAVE][WAVE][FT_PITCH];
    const size_t hw = (size_t)h * w;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const int i = blockIdx.x * FT_BLOCK + threadIdx.x;
    const int L = i < *n_live ? len[i] : 0;
    const bool keep = L >= min_len;
    int row = keep_off[blockIdx.x] + block_rank<FT_BLOCK / WAVE>(keep);
    if (!keep || row >= n_rows) row = -1;
    const f2 nan2 = {NAN, NAN};
    for (int t0 = 0; t0 < T; t0 += FT_CHUNK) {
        __syncthreads();
        for (int j = 0; j < FT_CHUNK; ++j) {
            const int f = t0 + j - s;
            f2 v = nan2;
            if (row >= 0 && f >= 0 && f < L) {
                v = slab[(size_t)f * hw + i];
                size_t cell;
                if (rounded_cell(v, h, w, &cell)) visited[(size_t)(s + f) * hw + cell] = 1;
            }
            tile[wv][lane][j] = v;
        }
        __syncthreads();
        const int j = lane & (FT_CHUNK - 1), sub = lane / FT_CHUNK;
        for (int q = 0; q < WAVE; q += WAVE / FT_CHUNK) {
            const int l = q + sub;
            const int r = __shfl(row, l, WAVE);
            if (r >= 0 && t0 + j < T) rows[(size_t)r * T + t0 + j] = tile[wv][l][j];
        }
    }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct TrajLayout {
    size_t pix, len, live_off, keep_off, totals, slab, bytes;
};

TrajLayout traj_layout(int T, int h, int w) {
    const size_t hw = (size_t)h * w;
    const size_t nblk = (hw + FT_BLOCK - 1) / FT_BLOCK;
    TrajLayout L;
    L.pix = 0;
    L.len = L.pix + align256(hw * sizeof(int32_t));
    L.live_off = L.len + align256(hw * sizeof(int32_t));
    L.keep_off = L.live_off + align256(nblk * sizeof(int32_t));
    L.totals = L.keep_off + align256(nblk * sizeof(int32_t));
    L.slab = L.totals + 256;
    L.bytes = L.slab + align256((size_t)T * hw * sizeof(f2));
    return L;
}

bool sizes_ok(int T, int h, int w) { return T >= 2 && h >= 2 && w >= 2 && (long long)h * w < (1LL << 30); }

// blocks of a grid-stride pass over n elements: at most 4096 (1 M threads in flight keep every CU busy; the rest strides)
unsigned span_blocks(size_t n) {
    const size_t b = (n + FT_BLOCK - 1) / FT_BLOCK;
    return (unsigned)(b < 4096 ? (b ? b : 1) : 4096);
}

}  // namespace

extern "C" int dtk_flow_pack(const float* flow, float* packed, int32_t n, int32_t h, int32_t w, void* stream) {
    DTK_REQUIRE(n >= 0 && h > 0 && w > 0 && (long long)h * w < (1LL << 30), "flow_pack: bad sizes n=%d %dx%d", n, h, w);
    DTK_REQUIRE(n == 0 || (flow && packed), "flow_pack: null pointer");
    if (n == 0) return 0;
    const size_t hw = (size_t)h * w;
    DTK_LAUNCH("flow_pack", flow_pack_kernel, dim3(span_blocks((size_t)n * hw)), dim3(FT_BLOCK), 0, dtk_stream(stream), flow,
               reinterpret_cast<f2*>(packed), (size_t)n, hw);
    return 0;
}

extern "C" int dtk_flow_cycle_masks(const float* fpk, const float* bpk, int32_t T, int32_t h, int32_t w, float threshold,
                                    uint8_t* consistent, void* stream) {
    DTK_REQUIRE(sizes_ok(T, h, w), "flow_cycle_masks: bad sizes T=%d %dx%d (T >= 2, h, w >= 2)", T, h, w);
    DTK_REQUIRE(fpk && bpk && consistent, "flow_cycle_masks: null pointer");
    hipStream_t st = dtk_stream(stream);
    const size_t hw = (size_t)h * w;
    DTK_LAUNCH("flow_mask_clear", fill_bytes_kernel, dim3(span_blocks((size_t)T * hw)), dim3(FT_BLOCK), 0, st, consistent,
               (size_t)T * hw, (uint8_t)0);
    const dim3 grid(dtk_cdiv(hw, FT_BLOCK), T - 1);
    DTK_LAUNCH("flow_warp_hit", warp_hit_kernel, grid, dim3(FT_BLOCK), 0, st, reinterpret_cast<const f2*>(fpk), h, w, consistent);
    DTK_LAUNCH("flow_cycle_mask", cycle_mask_kernel, grid, dim3(FT_BLOCK), 0, st, reinterpret_cast<const f2*>(fpk),
               reinterpret_cast<const f2*>(bpk), h, w, threshold, consistent);
    return 0;
}

extern "C" size_t dtk_flow_traj_workspace_bytes(int32_t T, int32_t h, int32_t w) {
    if (!sizes_ok(T, h, w)) return 0;
    return traj_layout(T, h, w).bytes;
}

extern "C" int dtk_flow_traj_start(const float* fpk, const float* bpk, const uint8_t* consistent, const uint8_t* visited,
                                   int32_t T, int32_t h, int32_t w, int32_t s, float threshold, int32_t min_trajectory_length,
                                   const float* direct_fwd, const float* direct_back, int32_t use_direct, float direct_threshold,
                                   int32_t* n_rows, void* workspace, size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(sizes_ok(T, h, w), "flow_traj_start: bad sizes T=%d %dx%d (T >= 2, h, w >= 2)", T, h, w);
    DTK_REQUIRE(s >= 0 && s < T, "flow_traj_start: starting frame %d outside [0, %d)", s, T);
    DTK_REQUIRE(min_trajectory_length >= 1 && min_trajectory_length <= T, "flow_traj_start: min_trajectory_length %d outside [1, %d]",
                min_trajectory_length, T);
    DTK_REQUIRE(fpk && bpk && consistent && visited && n_rows && workspace, "flow_traj_start: null pointer");
    const bool steps = s < T - 1;
    DTK_REQUIRE(!use_direct || !steps || (direct_fwd && direct_back), "flow_traj_start: a direct-flow threshold without direct flows");
    DTK_REQUIRE(use_direct || (!direct_fwd && !direct_back), "flow_traj_start: direct flows without a direct-flow threshold");
    const TrajLayout L = traj_layout(T, h, w);
    if (workspace_bytes < L.bytes) {
        dtk_set_error("flow_traj_start: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
        return DTK_E_WORKSPACE;
    }
    hipStream_t st = dtk_stream(stream);
    char* ws = static_cast<char*>(workspace);
    int32_t* pix = reinterpret_cast<int32_t*>(ws + L.pix);
    int32_t* len = reinterpret_cast<int32_t*>(ws + L.len);
    int32_t* live_off = reinterpret_cast<int32_t*>(ws + L.live_off);
    int32_t* keep_off = reinterpret_cast<int32_t*>(ws + L.keep_off);
    int32_t* n_live = reinterpret_cast<int32_t*>(ws + L.totals);
    f2* slab = reinterpret_cast<f2*>(ws + L.slab);
    const int hw = h * w;
    const int nblk = dtk_cdiv(hw, FT_BLOCK);
    const uint8_t* cons_s = consistent + (size_t)s * hw;
    const uint8_t* vis_s = visited + (size_t)s * hw;
    DTK_LAUNCH("flow_start_count", start_count_kernel, dim3(nblk), dim3(FT_BLOCK), 0, st, cons_s, vis_s, hw, live_off);
    DTK_LAUNCH("flow_scan", block_offsets_kernel<FT_BLOCK / WAVE>, dim3(1), dim3(FT_BLOCK), 0, st, live_off, nblk, n_live);
    DTK_LAUNCH("flow_start_compact", start_compact_kernel, dim3(nblk), dim3(FT_BLOCK), 0, st, cons_s, vis_s, hw, live_off, pix);
    const f2* fp = reinterpret_cast<const f2*>(fpk);
    const f2* bp = reinterpret_cast<const f2*>(bpk);
    if (use_direct) {
        DTK_LAUNCH("flow_walk_direct", walk_kernel<true>, dim3(nblk), dim3(FT_BLOCK), 0, st, fp, bp,
                   reinterpret_cast<const f2*>(direct_fwd), reinterpret_cast<const f2*>(direct_back), T, h, w, s, threshold,
                   direct_threshold, min_trajectory_length, n_live, pix, slab, len, keep_off);
    } else {
        DTK_LAUNCH("flow_walk", walk_kernel<false>, dim3(nblk), dim3(FT_BLOCK), 0, st, fp, bp, (const f2*)nullptr,
                   (const f2*)nullptr, T, h, w, s, threshold, 0.f, min_trajectory_length, n_live, pix, slab, len, keep_off);
    }
    DTK_LAUNCH("flow_scan", block_offsets_kernel<FT_BLOCK / WAVE>, dim3(1), dim3(FT_BLOCK), 0, st, keep_off, nblk, n_rows);
    return 0;
}

extern "C" int dtk_flow_traj_emit(int32_t T, int32_t h, int32_t w, int32_t s, int32_t min_trajectory_length, int32_t n_rows,
                                  float* rows, uint8_t* visited, const void* workspace, size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(sizes_ok(T, h, w), "flow_traj_emit: bad sizes T=%d %dx%d (T >= 2, h, w >= 2)", T, h, w);
    DTK_REQUIRE(s >= 0 && s < T, "flow_traj_emit: starting frame %d outside [0, %d)", s, T);
    DTK_REQUIRE(min_trajectory_length >= 1 && min_trajectory_length <= T, "flow_traj_emit: min_trajectory_length %d outside [1, %d]",
                min_trajectory_length, T);
    DTK_REQUIRE(n_rows >= 0 && n_rows <= h * w, "flow_traj_emit: n_rows %d outside [0, %d]", n_rows, h * w);
    DTK_REQUIRE(visited && workspace && (rows || n_rows == 0), "flow_traj_emit: null pointer");
    const TrajLayout L = traj_layout(T, h, w);
    if (workspace_bytes < L.bytes) {
        dtk_set_error("flow_traj_emit: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
        return DTK_E_WORKSPACE;
    }
    if (n_rows == 0) return 0;
    const char* ws = static_cast<const char*>(workspace);
    DTK_LAUNCH("flow_emit", emit_kernel, dim3(dtk_cdiv((long long)h * w, FT_BLOCK)), dim3(FT_BLOCK), 0, dtk_stream(stream),
               reinterpret_cast<const f2*>(ws + L.slab), reinterpret_cast<const int32_t*>(ws + L.len),
               reinterpret_cast<const int32_t*>(ws + L.totals), reinterpret_cast<const int32_t*>(ws + L.keep_off), T, h, w, s,
               min_trajectory_length, n_rows, reinterpret_cast<f2*>(rows), visited);
    return 0;
}
