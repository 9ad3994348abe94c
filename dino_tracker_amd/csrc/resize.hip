// resize.hip -- video ingest: Pillow's 8-bit separable resampler (Image.resize on uint8 frames) on the device, bit for bit.
// The filter is the caller's: per axis an int32 [out][ksize] table of 22-bit fixed-point weights and an int32 [out][2] table of
// (first input index, count), built on the host exactly as Pillow builds them (dino_tracker_amd/video_io.py).  A pass is
//     acc = 2^21 + sum_j in[first + j] * k[j]   (int32; the products are exact 24-bit multiplies),   out = clamp(acc >> 22, 0, 255)
// horizontal first, vertical on the horizontal pass's uint8 result.  Two forms, one export (include/dtk.h, dtk_resize_u8):
//
//   resize_fused_kernel : one workgroup of 256 threads per TILE_H x TILE_W output tile.  A wave takes an input row the tile needs,
//                         runs the horizontal pass for the tile's columns (a lane per interleaved byte, so neighbouring lanes read
//                         neighbouring input bytes; the tile's weights and bounds are copied to LDS first where they fit, because
//                         their rows are ksize * 4 bytes apart per pixel) into LDS as uint8 -- or copies the bytes when W == w --
//                         then, after one barrier, a wave takes an output row and runs the vertical pass down LDS columns with
//                         wave-uniform weights, and stores the result in its final form (uint8 HWC, or fp32 CHW through the
//                         caller's 256-entry u8 -> float table).  Input bytes are read once, plus the rows two vertically
//                         adjacent tiles share.
//   resize_h_kernel / resize_v_kernel : the same two passes as two launches, one thread per output byte, with the intermediate
//                         [N][H][w][C] in the caller's workspace.  Taken when the rows of one tile do not fit in LDS (extreme vertical
//                         down-scaling of tall frames) or on request (DTK_RESIZE_FORCE_GENERAL).
//
// Rows are addressed by the byte: a pitch such as 53 * 3 = 159 is no multiple of 4, and nothing here assumes one.  Every table entry
// is clamped to the frame (and, in the fused form, to the tile's staged rows) before it becomes an address.
#include <algorithm>
#include "common.h"

namespace {

constexpr int TW = DTK_RESIZE_TILE_W, TH = DTK_RESIZE_TILE_H;
constexpr int RTHREADS = 256, RWAVES = RTHREADS / WAVE;
constexpr int LDS_MAX = 64 * 1024;
constexpr int MAX_FRAMES_PER_LAUNCH = 65535;   // gridDim.y

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> 22;   // arithmetic
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (first, count) of output index i, clamped so that first .. first + count - 1 lies in [lo, hi) and count <= ksize
__device__ __forceinline__ void bounds_of(const int32_t* __restrict__ b, int i, int ksize, int lo, int hi, int& first, int& count) {
    int f = b[2 * i], n = b[2 * i + 1];
    f = f < lo ? lo : (f > hi ? hi : f);
    n = n > ksize ? ksize : n;
    n = n > hi - f ? hi - f : n;
    first = f, count = n < 0 ? 0 : n;
}

// acc over `count` taps `stride` bytes apart
__device__ __forceinline__ int pass8(const uint8_t* __restrict__ p, int stride, const int32_t* __restrict__ k, int count) {
    int acc = 1 << 21;
    for (int j = 0; j < count; ++j) acc += __mul24((int)p[(size_t)j * stride], k[j]);
    return clip8(acc);
}

// bytes of the fused form's staged rows, rounded so that the int32 tables behind them are aligned
__host__ __device__ constexpr int staged_bytes(int rows, int C) { return (rows * TW * C + 15) & ~15; }

__device__ __forceinline__ void store_out(void* __restrict__ out, int form, const float* __restrict__ lut, size_t n, int y, int x, int c,
                                          int h, int w, int C, int v) {
    if (form == DTK_RESIZE_OUT_U8_HWC)
        reinterpret_cast<uint8_t*>(out)[((n * h + y) * w + x) * C + c] = (uint8_t)v;
    else
        reinterpret_cast<float*>(out)[((n * C + c) * h + y) * w + x] = lut[v];
}

template <int C>
__global__ __launch_bounds__(RTHREADS) void resize_fused_kernel(const uint8_t* __restrict__ in, int n0, int H, int W, int h, int w,
                                                                const int32_t* __restrict__ kx, const int32_t* __restrict__ bx,
                                                                int ksx, const int32_t* __restrict__ ky,
                                                                const int32_t* __restrict__ by, int ksy,
                                                                const float* __restrict__ lut, int form, int rows_cap, int tiles_x,
                                                                int kx_in_lds, void* __restrict__ out) {
    extern __shared__ __align__(16) uint8_t staged[];   // [rows_cap][E] uint8, then (kx_in_lds) the tile's weights and bounds
    constexpr int E = TW * C;
    int32_t* kw = reinterpret_cast<int32_t*>(staged + staged_bytes(rows_cap, C));   // [TW][ksx]
    int32_t* kb = kw + TW * ksx;                                                    // [TW][2], clamped
    const size_t n = (size_t)n0 + blockIdx.y;
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * TW, y0 = tile_y * TH, y1 = min(y0 + TH, h);
    const int tw = min(TW, w - x0), xe = tw * C;   // the tile's real columns, in pixels and in bytes
    int r0 = y0, r1 = y1;                          // input rows the tile needs: [r0, r1)
    if (ky) {
        int f, cnt;
        bounds_of(by, y0, ksy, 0, H, r0, cnt);
        bounds_of(by, y1 - 1, ksy, 0, H, f, cnt);
        r1 = min(f + cnt, r0 + rows_cap);
        r1 = max(r1, r0);
    }
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
    const uint8_t* src = in + n * H * W * C;
    if (kx_in_lds) {   // the tile's columns are consecutive rows of kx / bx: one coalesced copy
        for (int i = threadIdx.x; i < tw * ksx; i += RTHREADS) kw[i] = kx[(size_t)x0 * ksx + i];
        for (int i = threadIdx.x; i < tw; i += RTHREADS) bounds_of(bx, x0 + i, ksx, 0, W, kb[2 * i], kb[2 * i + 1]);
        __syncthreads();
    }
    for (int r = r0 + wave; r < r1; r += RWAVES) {
        const uint8_t* row = src + (size_t)r * W * C;
        uint8_t* dst = staged + (r - r0) * E;
        for (int e = lane; e < xe; e += WAVE) {
            int v;
            if (kx) {
                const int xl = e / C, c = e - xl * C, x = x0 + xl;
                if (kx_in_lds) {   // ksx is odd: the lanes' weight rows start in distinct banks
                    v = pass8(row + (size_t)kb[2 * xl] * C + c, C, kw + xl * ksx, kb[2 * xl + 1]);
                } else {
                    int f, cnt;
                    bounds_of(bx, x, ksx, 0, W, f, cnt);
                    v = pass8(row + (size_t)f * C + c, C, kx + (size_t)x * ksx, cnt);
                }
            } else {
                v = row[(size_t)x0 * C + e];
            }
            dst[e] = (uint8_t)v;
        }
    }
    __syncthreads();
    for (int y = y0 + wave; y < y1; y += RWAVES) {
        int f = y, cnt = 1;
        if (ky) bounds_of(by, y, ksy, r0, r1, f, cnt);
        const uint8_t* col = staged + (f - r0) * E;
        const int32_t* k = ky ? ky + (size_t)y * ksy : nullptr;
        for (int i = lane; i < xe; i += WAVE) {
            int xl, c;
            if (form == DTK_RESIZE_OUT_U8_HWC) {   // neighbouring lanes: neighbouring bytes of the interleaved row
                xl = i / C, c = i - xl * C;
            } else {                               // neighbouring lanes: neighbouring floats of one plane's row
                c = i / tw, xl = i - c * tw;
            }
            const int e = xl * C + c;
            const int v = ky ? pass8(col + e, E, k, cnt) : (int)col[e];
            store_out(out, form, lut, n, y, x0 + xl, c, h, w, C, v);
        }
    }
}

// general form, horizontal pass: one thread per byte of [rows][w][C]; rows = N * H.  `last` (H == h): the output in its final form.
template <int C>
__global__ __launch_bounds__(RTHREADS) void resize_h_kernel(const uint8_t* __restrict__ in, int H, int W, int w,
                                                            const int32_t* __restrict__ kx, const int32_t* __restrict__ bx, int ksx,
                                                            const float* __restrict__ lut, int form, int last, int blocks_per_row,
                                                            void* __restrict__ out) {
    const size_t r = blockIdx.x / blocks_per_row;
    const int e = (blockIdx.x - (unsigned)r * blocks_per_row) * RTHREADS + threadIdx.x;
    if (e >= w * C) return;
    const int x = e / C, c = e - x * C;
    int f, cnt;
    bounds_of(bx, x, ksx, 0, W, f, cnt);
    const int v = pass8(in + (r * W + f) * C + c, C, kx + (size_t)x * ksx, cnt);
    if (last) {
        const size_t n = r / H;
        store_out(out, form, lut, n, (int)(r - n * H), x, c, H, w, C, v);
    } else {
        reinterpret_cast<uint8_t*>(out)[r * w * C + e] = (uint8_t)v;
    }
}

// general form, vertical pass over src [N][H][w][C] (the intermediate, or the input when W == w); ky == null: H == h, a plain
// change of form.  One thread per output value; rows = N * h.
template <int C>
__global__ __launch_bounds__(RTHREADS) void resize_v_kernel(const uint8_t* __restrict__ src, int H, int h, int w,
                                                            const int32_t* __restrict__ ky, const int32_t* __restrict__ by, int ksy,
                                                            const float* __restrict__ lut, int form, int blocks_per_row,
                                                            void* __restrict__ out) {
    const size_t r = blockIdx.x / blocks_per_row;
    const int i = (blockIdx.x - (unsigned)r * blocks_per_row) * RTHREADS + threadIdx.x;
    if (i >= w * C) return;
    const size_t n = r / h;
    const int y = (int)(r - n * h);
    int x, c;
    if (form == DTK_RESIZE_OUT_U8_HWC) {
        x = i / C, c = i - x * C;
    } else {
        c = i / w, x = i - c * w;
    }
    const int E = w * C, e = x * C + c;
    int f = y, cnt = 1;
    if (ky) bounds_of(by, y, ksy, 0, H, f, cnt);
    const uint8_t* col = src + (n * H + f) * E + e;
    const int v = ky ? pass8(col, E, ky + (size_t)y * ksy, cnt) : (int)col[0];
    store_out(out, form, lut, n, y, x, c, h, w, C, v);
}

// rows of LDS one tile of the fused form needs at most (include/dtk.h)
long long fused_rows(int H, int h, int ksize_y) {
    if (H == h) return TH;
    return std::min<long long>(H, (long long)(TH - 1) * H / h + ksize_y + 1);
}

bool use_fused(int H, int C, int h, int ksize_y, int options) {
    return !(options & DTK_RESIZE_FORCE_GENERAL) && fused_rows(H, h, ksize_y) * TW * C <= LDS_MAX;
}

bool sizes_ok(int N, int H, int W, int C, int h, int w) {
    return N > 0 && H > 0 && W > 0 && h > 0 && w > 0 && (C == 1 || C == 3);
}

}  // namespace

extern "C" size_t dtk_resize_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, int32_t ksize_y,
                                             int32_t options) {
    if (!sizes_ok(N, H, W, C, h, w) || (H != h && ksize_y < 1) || (options & ~DTK_RESIZE_FORCE_GENERAL)) return 0;
    if (H == h || W == w || use_fused(H, C, h, ksize_y, options)) return 0;
    return (size_t)N * H * w * C;
}

extern "C" int dtk_resize_u8(const uint8_t* in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t h, int32_t w, const int32_t* kx,
                             const int32_t* bx, int32_t ksize_x, const int32_t* ky, const int32_t* by, int32_t ksize_y,
                             const float* u8_to_f32, int32_t out_form, int32_t options, void* out, void* workspace,
                             size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(C == 1 || C == 3, "resize_u8: C must be 1 or 3, got %d", C);
    DTK_REQUIRE(N > 0 && H > 0 && W > 0 && h > 0 && w > 0, "resize_u8: sizes must be positive, got N=%d %d x %d -> %d x %d", N, H, W, h, w);
    DTK_REQUIRE(out_form == DTK_RESIZE_OUT_U8_HWC || out_form == DTK_RESIZE_OUT_F32_CHW,
                "resize_u8: out_form must be 0 (uint8 HWC) or 1 (fp32 CHW), got %d", out_form);
    DTK_REQUIRE(!(options & ~DTK_RESIZE_FORCE_GENERAL), "resize_u8: unknown option bits 0x%x", options & ~DTK_RESIZE_FORCE_GENERAL);
    DTK_REQUIRE(in && out, "resize_u8: null pointer (in / out)");
    DTK_REQUIRE(out_form == DTK_RESIZE_OUT_U8_HWC || u8_to_f32, "resize_u8: null pointer (the fp32 form needs the u8 -> float table)");
    const bool hpass = W != w, vpass = H != h;
    DTK_REQUIRE(!hpass || (kx && bx), "resize_u8: null pointer (horizontal tables, W %d -> %d)", W, w);
    DTK_REQUIRE(!vpass || (ky && by), "resize_u8: null pointer (vertical tables, H %d -> %d)", H, h);
    DTK_REQUIRE((!hpass || ksize_x >= 1) && (!vpass || ksize_y >= 1), "resize_u8: ksize must be >= 1, got %d (x) %d (y)", ksize_x, ksize_y);
    if (!hpass) kx = bx = nullptr;
    if (!vpass) ky = by = nullptr;
    const long long in_row = (long long)W * C, out_row = (long long)w * C;
    DTK_REQUIRE(in_row < (1LL << 31) && out_row < (1LL << 31), "resize_u8: a row of %d or %d pixels is too long", W, w);
    hipStream_t st = dtk_stream(stream);
    if (use_fused(H, C, h, ksize_y, options)) {
        const int rows_cap = (int)fused_rows(H, h, ksize_y), tiles_x = dtk_cdiv(w, TW);
        const long long tiles = (long long)tiles_x * dtk_cdiv(h, TH);
        DTK_REQUIRE(tiles < (1LL << 31), "resize_u8: %lld tiles per frame", tiles);
        // the tile's horizontal weights and bounds go to LDS too where they fit beside the rows (not at 259 taps)
        const size_t kx_bytes = hpass ? (size_t)TW * (ksize_x + 2) * 4 : 0;
        const int kx_in_lds = hpass && staged_bytes(rows_cap, C) + kx_bytes <= (size_t)LDS_MAX;
        const size_t lds = staged_bytes(rows_cap, C) + (kx_in_lds ? kx_bytes : 0);
        for (int n0 = 0; n0 < N; n0 += MAX_FRAMES_PER_LAUNCH) {
            const dim3 grid((unsigned)tiles, (unsigned)std::min(N - n0, MAX_FRAMES_PER_LAUNCH));
            if (C == 3)
                DTK_LAUNCH("resize_fused", resize_fused_kernel<3>, grid, dim3(RTHREADS), lds, st, in, n0, H, W, h, w, kx, bx, ksize_x, ky,
                           by, ksize_y, u8_to_f32, out_form, rows_cap, tiles_x, kx_in_lds, out);
            else
                DTK_LAUNCH("resize_fused", resize_fused_kernel<1>, grid, dim3(RTHREADS), lds, st, in, n0, H, W, h, w, kx, bx, ksize_x, ky,
                           by, ksize_y, u8_to_f32, out_form, rows_cap, tiles_x, kx_in_lds, out);
        }
        return 0;
    }
    const int bpr = dtk_cdiv(out_row, RTHREADS);
    const long long hblocks = (long long)N * H * bpr, vblocks = (long long)N * h * bpr;
    DTK_REQUIRE(hblocks < (1LL << 31) && vblocks < (1LL << 31), "resize_u8: %lld rows are too many for one launch", (long long)N * std::max(H, h));
    const uint8_t* vsrc = in;
    if (hpass) {
        void* hdst = out;
        if (vpass) {
            const size_t need = (size_t)N * H * w * C;
            DTK_REQUIRE(workspace && workspace_bytes >= need, "resize_u8: the general form needs a workspace of %zu bytes, got %zu", need,
                        workspace_bytes);
            hdst = workspace;
            vsrc = reinterpret_cast<const uint8_t*>(workspace);
        }
        if (C == 3)
            DTK_LAUNCH("resize_h", resize_h_kernel<3>, dim3((unsigned)hblocks), dim3(RTHREADS), 0, st, in, H, W, w, kx, bx, ksize_x,
                       u8_to_f32, out_form, (int)!vpass, bpr, hdst);
        else
            DTK_LAUNCH("resize_h", resize_h_kernel<1>, dim3((unsigned)hblocks), dim3(RTHREADS), 0, st, in, H, W, w, kx, bx, ksize_x,
                       u8_to_f32, out_form, (int)!vpass, bpr, hdst);
        if (!vpass) return 0;
    }
    if (C == 3)
        DTK_LAUNCH("resize_v", resize_v_kernel<3>, dim3((unsigned)vblocks), dim3(RTHREADS), 0, st, vsrc, H, h, w, ky, by, ksize_y,
                   u8_to_f32, out_form, bpr, out);
    else
        DTK_LAUNCH("resize_v", resize_v_kernel<1>, dim3((unsigned)vblocks), dim3(RTHREADS), 0, st, vsrc, H, h, w, ky, by, ksize_y,
                   u8_to_f32, out_form, bpr, out);
    return 0;
}
