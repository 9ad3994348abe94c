// render.hip -- track videos on the device: the dotted tracks and the rainbow trails of visualization/viz_utils_tapir.py
// (plot_tracks_v2, plot_tracks_tails) as a tiled, ordered alpha-blending rasteriser.  The picture is defined in docs/RENDER.md;
// the stages, one export each (include/dtk.h):
//
//   dtk_render_prims       : one thread per (frame, j, n) writes the 48-byte record of one primitive, in draw order
//   dtk_render_pred_gt_prims : one thread per (frame, n) writes the two records of a prediction-against-ground-truth point
//                            (visualization/visualize_pred_vs_gt.py:13-38): displacement line + disc, cross, or line + ring
//   dtk_render_tile_counts : per record, the number of 16 x 16 tiles its grown bounding box meets
//   dtk_render_tile_keys   : per (tile, record) one 64-bit key  (frame, tile) << 32 | record index  at the record's offset in the
//                            exclusive prefix sum of the counts.  The caller sorts the keys; they are unique, so the sorted
//                            array is a function of the records alone, and ascending order inside a tile is draw order.
//   dtk_render_blend       : one workgroup of 256 threads per tile, one pixel per thread.  The tile's records are staged through
//                            LDS 256 at a time (12 KiB: three float4 per record, every lane of a wave reads the SAME address, so
//                            the reads are broadcasts without bank conflicts) and blended in order in registers.
//
// Nothing here uses an atomic: every output word has exactly one writer, so two calls give the same bits.
#include <math.h>
#include <algorithm>
#include "common.h"

namespace {

constexpr int RT = DTK_RENDER_TILE;
constexpr int RW = DTK_RENDER_RECORD_WORDS;
constexpr int RCHUNK = DTK_RENDER_CHUNK;
constexpr int RTHREADS = 256;
static_assert(RT * RT == RTHREADS && RCHUNK == RTHREADS && RW == 12, "one pixel and one staged record per thread");

// np.maximum(np.minimum(...)) semantics: a NaN stays a NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float clamp_np(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// the clamped track point (reference :719-720): [0, W] x [0, H]
__device__ __forceinline__ float2 track_point(const float* __restrict__ points, int n, int t, int T, float W, float H) {
    const float2 p = *reinterpret_cast<const float2*>(points + ((size_t)n * T + t) * 2);
    return make_float2(clamp_np(p.x, 0.f, W), clamp_np(p.y, 0.f, H));
}

// P(n, j) seen from frame i: maps[i][j] applied to the clamped point of frame j (reference :725-737)
__device__ __forceinline__ float2 mapped_point(const float* __restrict__ m, float2 p) {
    const float X = m[0] * p.x + m[1] * p.y + m[2];
    const float Y = m[3] * p.x + m[4] * p.y + m[5];
    const float w = m[6] * p.x + m[7] * p.y + m[8];
    const float sgn = w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f);   // np.sign: 0 at 0 (the division then gives inf / NaN, as there)
    const float den = fmaxf(1e-12f, fabsf(w)) * sgn;
    return make_float2(X / den, Y / den);
}

__device__ __forceinline__ void store_record(float* __restrict__ rec, int kind, float x0, float y0, float x1, float y1, float size,
                                             const float* __restrict__ col, float a, float inv_len2, int frame) {
    float4* q = reinterpret_cast<float4*>(rec);
    q[0] = make_float4(__int_as_float(kind), x0, y0, x1);
    q[1] = make_float4(y1, size, col[0], col[1]);
    q[2] = make_float4(col[2], a, inv_len2, __int_as_float(frame));
}

__global__ __launch_bounds__(RTHREADS) void render_prims_kernel(const float* __restrict__ points, const uint8_t* __restrict__ occ,
                                                                const float* __restrict__ maps, const float* __restrict__ colors,
                                                                int N, int T, int f0, int H, int W, int mode, int marker_kind,
                                                                float marker_size, float half_width, int trail_fade,
                                                                float* __restrict__ records) {
    const int fi = blockIdx.y, i = f0 + fi;
    const long long idx = (long long)blockIdx.x * RTHREADS + threadIdx.x;
    const long long in_frame = mode == DTK_RENDER_TAILS ? (long long)N * (i + 1) : N;
    if (idx >= in_frame) return;
    const int slot = (int)(idx / N), n = (int)(idx - (long long)slot * N);
    const long long base = mode == DTK_RENDER_TAILS
                               ? (long long)N * ((long long)i * (i + 1) / 2 - (long long)f0 * (f0 + 1) / 2)
                               : (long long)N * fi;
    float* rec = records + (size_t)(base + idx) * RW;
    const float* col = colors + (size_t)n * 3;
    const float Wf = (float)W, Hf = (float)H;
    if (slot == 0) {
        const float2 p = track_point(points, n, i, T, Wf, Hf);
        const float a = 1.f - (float)(occ[(size_t)n * T + i] != 0);
        store_record(rec, marker_kind, p.x, p.y, p.x, p.y, marker_size, col, a, 0.f, fi);
        return;
    }
    const int j = i - slot;   // 0 .. i - 1: the segment P(n, j) -> P(n, j + 1)
    float2 p0 = mapped_point(maps + ((size_t)i * T + j) * 9, track_point(points, n, j, T, Wf, Hf));
    float2 p1 = track_point(points, n, j + 1, T, Wf, Hf);
    if (j + 1 < i) p1 = mapped_point(maps + ((size_t)i * T + j + 1) * 9, p1);
    const bool oof = p0.x < 1.f || p0.y < 1.f || p1.x < 1.f || p1.y < 1.f || p0.x > Wf || p1.x > Wf || p0.y > Hf || p1.y > Hf;
    p0.x = clamp_np(p0.x, 1.f, Wf - 1.f), p0.y = clamp_np(p0.y, 1.f, Hf - 1.f);
    p1.x = clamp_np(p1.x, 1.f, Wf - 1.f), p1.y = clamp_np(p1.y, 1.f, Hf - 1.f);
    float a = (1.f - (float)(occ[(size_t)n * T + j] != 0)) * (1.f - (float)(occ[(size_t)n * T + j + 1] != 0)) * (oof ? 0.f : 1.f);
    if (trail_fade) a *= fmaxf(1.f - 0.9f * ((float)(i - j) / ((float)(i + 1) * 0.99f)), 0.1f);
    const float dx = p1.x - p0.x, dy = p1.y - p0.y, len2 = dx * dx + dy * dy;
    store_record(rec, DTK_RENDER_SEGMENT, p0.x, p0.y, p1.x, p1.y, half_width, col, a, len2 > 0.f ? 1.f / len2 : 0.f, fi);
}

// overlay_pred_gt_on_frame (visualize_pred_vs_gt.py:21-38) on integer points: exactly two records per (frame, point)
__global__ __launch_bounds__(RTHREADS) void render_pred_gt_prims_kernel(const int32_t* __restrict__ pred_xy,
                                                                        const int32_t* __restrict__ gt_xy,
                                                                        const uint8_t* __restrict__ pred_occ,
                                                                        const uint8_t* __restrict__ gt_occ,
                                                                        const float* __restrict__ colors, int N, int T, int f0,
                                                                        int thickness, int radius, int cross_size,
                                                                        float* __restrict__ records) {
    const int fi = blockIdx.y, i = f0 + fi;
    const int n = blockIdx.x * RTHREADS + threadIdx.x;
    if (n >= N) return;
    const size_t at = (size_t)n * T + i;
    float* rec = records + ((size_t)fi * N + n) * 2 * RW;
    const float* col = colors + (size_t)n * 3;
    const float red[3] = {1.f, 0.f, 0.f};
    const float px = (float)pred_xy[2 * at], py = (float)pred_xy[2 * at + 1];
    const float gx = (float)gt_xy[2 * at], gy = (float)gt_xy[2 * at + 1];
    const bool pocc = pred_occ[at] != 0, gocc = gt_occ[at] != 0;
    if (pocc && gocc) {   // drawn nowhere: two records with a = 0
        const float none[3] = {0.f, 0.f, 0.f};
        store_record(rec, DTK_RENDER_SEGMENT, 0.f, 0.f, 0.f, 0.f, 0.f, none, 0.f, 0.f, fi);
        store_record(rec + RW, DTK_RENDER_SEGMENT, 0.f, 0.f, 0.f, 0.f, 0.f, none, 0.f, 0.f, fi);
        return;
    }
    if (!pocc && gocc) {   // the cross: two diagonals of +- cross_size
        const float r = (float)cross_size, hw = (float)thickness * 0.5f;
        const float len2 = 8.f * r * r, inv = len2 > 0.f ? __fdiv_rn(1.f, len2) : 0.f;
        store_record(rec, DTK_RENDER_SEGMENT, px - r, py - r, px + r, py + r, hw, col, 1.f, inv, fi);
        store_record(rec + RW, DTK_RENDER_SEGMENT, px - r, py + r, px + r, py - r, hw, col, 1.f, inv, fi);
        return;
    }
    const float dx = gx - px, dy = gy - py, len2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));   // as numpy: no FMA
    const float hw = (float)(pocc ? thickness / 2 : thickness) * 0.5f;   // cv2 thickness // 2 where the prediction is occluded
    store_record(rec, DTK_RENDER_SEGMENT, px, py, gx, gy, hw, red, 1.f, len2 > 0.f ? __fdiv_rn(1.f, len2) : 0.f, fi);
    if (pocc) store_record(rec + RW, DTK_RENDER_RING, px, py, px, py, (float)radius, col, 1.f, 1.f, fi);   // word [10]: hw = 1
    else store_record(rec + RW, DTK_RENDER_DISC, px, py, px, py, (float)radius, col, 1.f, 0.f, fi);
}

struct TileBox {
    int tx0, tx1, ty0, ty1, frame;
    __device__ int count() const { return (tx1 - tx0 + 1) * (ty1 - ty0 + 1); }
};

// the tiles the record's bounding box meets; false = none (a <= 0, not finite, outside the frame, foreign frame index)
__device__ __forceinline__ bool tile_box(const float* __restrict__ rec, int F, int H, int W, TileBox& b) {
    const float4 q0 = *reinterpret_cast<const float4*>(rec);
    const float4 q1 = *reinterpret_cast<const float4*>(rec + 4);
    const float4 q2 = *reinterpret_cast<const float4*>(rec + 8);
    const int kind = __float_as_int(q0.x);
    const float x0 = q0.y, y0 = q0.z, x1 = q0.w, y1 = q1.x, size = q1.y, a = q2.y;
    b.frame = __float_as_int(q2.w);
    if (!(a > 0.f) || b.frame < 0 || b.frame >= F) return false;
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && isfinite(size))) return false;
    float grow = size + (kind == DTK_RENDER_DIAMOND ? 0.70711f : 0.5f);   // coverage is 0 beyond it (docs/RENDER.md)
    if (kind == DTK_RENDER_RING) {   // the stroke reaches r + hw; word [10] is its half width
        if (!isfinite(q2.z)) return false;
        grow += q2.z;
    }
    const float xmin = fminf(x0, x1) - grow, xmax = fmaxf(x0, x1) + grow;
    const float ymin = fminf(y0, y1) - grow, ymax = fmaxf(y0, y1) + grow;
    if (!(xmax >= 0.f && ymax >= 0.f && xmin <= (float)(W - 1) && ymin <= (float)(H - 1))) return false;
    const int cx0 = (int)floorf(fmaxf(xmin, 0.f)), cx1 = (int)ceilf(fminf(xmax, (float)(W - 1)));
    const int cy0 = (int)floorf(fmaxf(ymin, 0.f)), cy1 = (int)ceilf(fminf(ymax, (float)(H - 1)));
    b.tx0 = cx0 / RT, b.tx1 = cx1 / RT, b.ty0 = cy0 / RT, b.ty1 = cy1 / RT;
    return true;
}

__global__ __launch_bounds__(RTHREADS) void render_tile_counts_kernel(const float* __restrict__ records, long long P, int F, int H,
                                                                      int W, int32_t* __restrict__ counts) {
    const long long p = (long long)blockIdx.x * RTHREADS + threadIdx.x;
    if (p >= P) return;
    TileBox b;
    counts[p] = tile_box(records + (size_t)p * RW, F, H, W, b) ? b.count() : 0;
}

__global__ __launch_bounds__(RTHREADS) void render_tile_keys_kernel(const float* __restrict__ records,
                                                                    const int64_t* __restrict__ offsets, long long P, int F, int H,
                                                                    int W, int tiles_x, int tiles_y, long long K,
                                                                    int64_t* __restrict__ keys) {
    const long long p = (long long)blockIdx.x * RTHREADS + threadIdx.x;
    if (p >= P) return;
    TileBox b;
    if (!tile_box(records + (size_t)p * RW, F, H, W, b)) return;
    long long o = offsets[p];
    if (o < 0 || o + b.count() > K) return;   // offsets that are not the prefix sum of these records' counts: write nothing
    for (int ty = b.ty0; ty <= b.ty1; ++ty)
        for (int tx = b.tx0; tx <= b.tx1; ++tx)
            keys[o++] = ((int64_t)(((long long)b.frame * tiles_y + ty) * tiles_x + tx) << 32) | (int64_t)p;
}

__global__ __launch_bounds__(RTHREADS) void render_blend_kernel(const uint8_t* __restrict__ frames_in,
                                                                const float* __restrict__ records, long long P,
                                                                const int64_t* __restrict__ keys, long long K,
                                                                const int64_t* __restrict__ tile_start, int H, int W,
                                                                uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
    __shared__ float4 stage[RCHUNK * 3];
    const int tid = threadIdx.x;
    const long long tile = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    long long s = tile_start[tile], e = tile_start[tile + 1];
    s = s < 0 ? 0 : s;
    e = e > K ? K : e;
    const int px = blockIdx.x * RT + (tid & (RT - 1)), py = blockIdx.y * RT + tid / RT;
    const bool inside = px < W && py < H;   // ragged right / bottom tiles
    const size_t pix = (((size_t)blockIdx.z * H + py) * W + px) * 3;
    float cr = 0.f, cg = 0.f, cb = 0.f;
    if (inside) {
        cr = (float)frames_in[pix] / 255.f;
        cg = (float)frames_in[pix + 1] / 255.f;
        cb = (float)frames_in[pix + 2] / 255.f;
    }
    const float fx = (float)px, fy = (float)py;
    for (long long base = s; base < e; base += RCHUNK) {   // block-uniform
        const int n = (int)(e - base < RCHUNK ? e - base : RCHUNK);
        if (tid < n) {
            const long long p = (long long)(keys[base + tid] & 0xffffffffLL);
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0, q2 = q0;   // a = 0: draws nothing
            if (p < P) {
                const float4* r = reinterpret_cast<const float4*>(records + (size_t)p * RW);
                q0 = r[0], q1 = r[1], q2 = r[2];
            }
            stage[3 * tid] = q0, stage[3 * tid + 1] = q1, stage[3 * tid + 2] = q2;
        }
        __syncthreads();
        if (inside) {
            for (int k = 0; k < n; ++k) {
                const float4 q0 = stage[3 * k], q1 = stage[3 * k + 1], q2 = stage[3 * k + 2];
                const int kind = __float_as_int(q0.x);   // workgroup-uniform
                const float ax = fx - q0.y, ay = fy - q0.z;
                float cov;
                if (kind == DTK_RENDER_DIAMOND) {
                    cov = 0.5f + (q1.y - fabsf(ax) - fabsf(ay)) / 1.41421356237f;
                } else if (kind == DTK_RENDER_RING) {
                    cov = 0.5f + q2.z - fabsf(sqrtf(ax * ax + ay * ay) - q1.y);
                } else {   // a disc is a zero-length segment
                    const float dx = q0.w - q0.y, dy = q1.x - q0.z;
                    float t = (ax * dx + ay * dy) * q2.z;
                    t = fminf(fmaxf(t, 0.f), 1.f);
                    const float ex = ax - t * dx, ey = ay - t * dy;
                    cov = 0.5f + q1.y - sqrtf(ex * ex + ey * ey);
                }
                cov = fminf(fmaxf(cov, 0.f), 1.f);
                if (cov > 0.f) {
                    const float w = q2.y * cov, keep = 1.f - w;
                    cr = cr * keep + q1.z * w;
                    cg = cg * keep + q1.w * w;
                    cb = cb * keep + q2.x * w;
                }
            }
        }
        __syncthreads();
    }
    if (!inside) return;
    out_u8[pix] = (uint8_t)floorf(255.f * cr + 0.5f);
    out_u8[pix + 1] = (uint8_t)floorf(255.f * cg + 0.5f);
    out_u8[pix + 2] = (uint8_t)floorf(255.f * cb + 0.5f);
    if (out_f32) out_f32[pix] = cr, out_f32[pix + 1] = cg, out_f32[pix + 2] = cb;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool frame_ok(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0 || F > 65535 || H > 32768 || W > 32768) return false;
    const long long tiles = (long long)dtk_cdiv(W, RT) * dtk_cdiv(H, RT);
    return tiles <= 65535LL * 65535LL && tiles * F < (1LL << 31) && dtk_cdiv(H, RT) <= 65535;
}

}  // namespace

extern "C" int64_t dtk_render_prim_count(int32_t mode, int32_t N, int32_t f0, int32_t F) {
    if (N < 0 || f0 < 0 || F < 0 || (mode != DTK_RENDER_DOTTED && mode != DTK_RENDER_TAILS)) return -1;
    if (mode == DTK_RENDER_DOTTED) return (int64_t)N * F;
    const int64_t a = f0, b = (int64_t)f0 + F;
    return (int64_t)N * (b * (b + 1) / 2 - a * (a + 1) / 2);
}

extern "C" size_t dtk_render_group_bytes(int64_t prims, int64_t keys, int32_t F, int32_t H, int32_t W) {
    if (prims < 0 || keys < 0 || !frame_ok(F, H, W)) return 0;
    const size_t tiles = (size_t)F * dtk_cdiv(W, RT) * dtk_cdiv(H, RT);
    size_t b = align256((size_t)prims * RW * 4);           // records
    b += align256((size_t)prims * 4);                      // counts
    b += 2 * align256((size_t)prims * 8);                  // their inclusive and exclusive prefix sums (int64)
    b += 3 * align256((size_t)keys * 8);                   // keys, sorted keys, the sort's permutation
    b += align256((tiles + 1) * 8) * 2;                    // tile boundaries and tile starts
    b += 2 * align256((size_t)F * H * W * 3);              // frames in, frames out
    return b;
}

extern "C" int dtk_render_prims(const float* points, const uint8_t* occluded, const float* maps, const float* colors, int32_t N,
                                int32_t T, int32_t f0, int32_t F, int32_t H, int32_t W, int32_t mode, int32_t marker_kind,
                                float marker_size, float half_width, int32_t trail_fade, float* records, void* stream) {
    DTK_REQUIRE(mode == DTK_RENDER_DOTTED || mode == DTK_RENDER_TAILS, "render_prims: mode must be 0 (dotted) or 1 (tails), got %d", mode);
    DTK_REQUIRE(marker_kind == DTK_RENDER_DISC || marker_kind == DTK_RENDER_DIAMOND,
                "render_prims: marker_kind must be 1 (disc) or 2 (diamond), got %d", marker_kind);
    DTK_REQUIRE(N > 0 && T > 0 && f0 >= 0 && F > 0 && F <= 65535 && f0 + (long long)F <= T,
                "render_prims: bad sizes N=%d T=%d frames %d .. %d + %d", N, T, f0, f0, F);
    DTK_REQUIRE(frame_ok(F, H, W), "render_prims: bad frame size %d x %d (x %d frames)", W, H, F);
    DTK_REQUIRE(marker_size >= 0.f && half_width >= 0.f && isfinite(marker_size) && isfinite(half_width),
                "render_prims: marker_size and half_width must be finite and >= 0");
    DTK_REQUIRE(points && occluded && colors && records, "render_prims: null pointer");
    DTK_REQUIRE(mode == DTK_RENDER_DOTTED || maps, "render_prims: the trail mode needs the frame-to-frame maps");
    DTK_REQUIRE(dtk_render_prim_count(mode, N, f0, F) < (1LL << 31), "render_prims: more than 2^31 records in one frame group");
    const long long widest = mode == DTK_RENDER_TAILS ? (long long)N * (f0 + F) : N;
    DTK_LAUNCH("render_prims", render_prims_kernel, dim3(dtk_cdiv(widest, RTHREADS), F), dim3(RTHREADS), 0, dtk_stream(stream),
               points, occluded, maps, colors, N, T, f0, H, W, mode, marker_kind, marker_size, half_width, trail_fade, records);
    return 0;
}

extern "C" int dtk_render_tile_counts(const float* records, int64_t P, int32_t F, int32_t H, int32_t W, int32_t* counts,
                                      void* stream) {
    DTK_REQUIRE(P >= 0 && P < (1LL << 31), "render_tile_counts: record count %lld outside 0 .. 2^31 - 1", (long long)P);
    DTK_REQUIRE(frame_ok(F, H, W), "render_tile_counts: bad frame size %d x %d (x %d frames)", W, H, F);
    if (P == 0) return 0;
    DTK_REQUIRE(records && counts, "render_tile_counts: null pointer");
    DTK_LAUNCH("render_tile_counts", render_tile_counts_kernel, dim3(dtk_cdiv(P, RTHREADS)), dim3(RTHREADS), 0, dtk_stream(stream),
               records, (long long)P, F, H, W, counts);
    return 0;
}

extern "C" int dtk_render_tile_keys(const float* records, const int64_t* offsets, int64_t P, int32_t F, int32_t H, int32_t W,
                                    int64_t K, int64_t* keys, void* stream) {
    DTK_REQUIRE(P >= 0 && P < (1LL << 31) && K >= 0, "render_tile_keys: bad counts P=%lld K=%lld", (long long)P, (long long)K);
    DTK_REQUIRE(frame_ok(F, H, W), "render_tile_keys: bad frame size %d x %d (x %d frames)", W, H, F);
    if (P == 0 || K == 0) return 0;
    DTK_REQUIRE(records && offsets && keys, "render_tile_keys: null pointer");
    DTK_LAUNCH("render_tile_keys", render_tile_keys_kernel, dim3(dtk_cdiv(P, RTHREADS)), dim3(RTHREADS), 0, dtk_stream(stream),
               records, offsets, (long long)P, F, H, W, dtk_cdiv(W, RT), dtk_cdiv(H, RT), (long long)K, keys);
    return 0;
}

extern "C" int dtk_render_blend(const uint8_t* frames_in, const float* records, int64_t P, const int64_t* sorted_keys, int64_t K,
                                const int64_t* tile_start, int32_t F, int32_t H, int32_t W, uint8_t* out_u8, float* out_f32,
                                void* stream) {
    DTK_REQUIRE(P >= 0 && P < (1LL << 31) && K >= 0, "render_blend: bad counts P=%lld K=%lld", (long long)P, (long long)K);
    DTK_REQUIRE(frame_ok(F, H, W), "render_blend: bad frame size %d x %d (x %d frames)", W, H, F);
    DTK_REQUIRE(frames_in && tile_start && out_u8, "render_blend: null pointer");
    DTK_REQUIRE(K == 0 || (records && sorted_keys), "render_blend: K=%lld keys but no records / keys", (long long)K);
    DTK_LAUNCH("render_blend", render_blend_kernel, dim3(dtk_cdiv(W, RT), dtk_cdiv(H, RT), F), dim3(RTHREADS), 0,
               dtk_stream(stream), frames_in, records, (long long)P, sorted_keys, (long long)K, tile_start, H, W, out_u8, out_f32);
    return 0;
}

extern "C" int dtk_render_pred_gt_prims(const int32_t* pred_xy, const int32_t* gt_xy, const uint8_t* pred_occluded,
                                        const uint8_t* gt_occluded, const float* colors, int32_t N, int32_t T, int32_t f0,
                                        int32_t F, int32_t thickness, int32_t radius, int32_t cross_size, float* records,
                                        void* stream) {
    DTK_REQUIRE(N > 0 && T > 0 && f0 >= 0 && F > 0 && F <= 65535 && f0 + (long long)F <= T,
                "render_pred_gt_prims: bad sizes N=%d T=%d frames %d .. %d + %d", N, T, f0, f0, F);
    DTK_REQUIRE(thickness >= 1 && radius >= 0 && cross_size >= 0 && thickness <= 4096 && radius <= 4096 && cross_size <= 4096,
                "render_pred_gt_prims: thickness %d must be 1 .. 4096, radius %d and cross_size %d 0 .. 4096", thickness, radius,
                cross_size);
    DTK_REQUIRE(2LL * N * F < (1LL << 31), "render_pred_gt_prims: more than 2^31 records in one frame group");
    DTK_REQUIRE(pred_xy && gt_xy && pred_occluded && gt_occluded && colors && records, "render_pred_gt_prims: null pointer");
    DTK_LAUNCH("render_pred_gt_prims", render_pred_gt_prims_kernel, dim3(dtk_cdiv(N, RTHREADS), F), dim3(RTHREADS), 0,
               dtk_stream(stream), pred_xy, gt_xy, pred_occluded, gt_occluded, colors, N, T, f0, thickness, radius, cross_size,
               records);
    return 0;
}
