// jpeg_decode.hip -- video ingest: a baseline JPEG decoder (SOF0, 8 bit, 4:2:0 / 4:2:2 / 4:4:4 in one interleaved scan or one gray
// component, the file's own Huffman and quantisation tables, any restart interval) whose arithmetic is written down in docs/JPEG_DECODE.md and is integer throughout:
// what libjpeg-turbo's default path (slow-integer IDCT, "fancy" upsampling) computes, so the pixels equal Pillow's.  The header is
// parsed on the host (dino_tracker_amd/video_in.py); the device sees validated tables and a table of SEGMENTS -- the restart
// intervals of every frame, or a frame's whole scan.  Three kernels:
//
// The kernels are templates over the sampling S (jpeg_entropy.h: B blocks per MCU, the block -> component schedule, the MCU's size):
//
//   jpeg_entropy_kernel  : decoding is sequential inside a segment, so ONE WAVE per segment.  The lanes build the frame's Huffman
//                          look-ups (six, two for gray) in LDS (9-bit first level, maxcode / valoff beyond), and stage the segment's bytes into LDS in
//                          chunks, a byte per lane, dropping the 0x00 after every 0xFF (ballot + popcount gives each kept byte its
//                          place).  Lane 0 walks the bits with jpeg_entropy.h's block loop into a 64-coefficient LDS block, which the
//                          wave then writes as one contiguous 128-byte store and zeroes again.  Before every block at least
//                          MARGIN bytes are staged ahead of the reader (a block is at most 16 + 15 + 63 * 31 bits = 248 bytes)
//                          unless the segment's end is staged.
//   jpeg_idct_kernel     : eight lanes per block: lane j dequantises and runs the column pass of column j, the passes exchange through
//                          LDS, lane j runs the row pass of row j and stores its eight samples as one 8-byte write into the Y, Cb
//                          or Cr plane of the workspace (planes padded to whole MCUs, 64 B bytes per MCU).
//   jpeg_colour_kernel   : a lane per pair of pixels (2c, 2c + 1) of a row: the h2v2 or h2v1 "fancy" upsampling with its context
//                          clamped to the REAL chroma plane (plain replication when that plane is at most two samples wide, none
//                          for 4:4:4), the colour conversion, six bytes of interleaved RGB.
//   jpeg_gray_kernel     : the Y plane cut to H x W.
//
// Safety (docs/JPEG_DECODE.md section 5): the entropy kernel writes only the blocks of its segment's own MCU range, reads only its
// segment's bytes, and its loop count is bounded by the segment's MCU count; a segment entry that does not fit the stream or the
// frame is not decoded at all.
#include <algorithm>
#include "common.h"
#include "jpeg_entropy.h"

static_assert(JPG_S_CODE == DTK_JPEG_S_CODE && JPG_S_INDEX == DTK_JPEG_S_INDEX && JPG_S_OVERRUN == DTK_JPEG_S_OVERRUN &&
                  JPG_S_LEFTOVER == DTK_JPEG_S_LEFTOVER && JPG_S_RANGE == DTK_JPEG_S_RANGE && JPG_S_SEGMENT == DTK_JPEG_S_SEGMENT,
              "the status bits of jpeg_entropy.h are dtk.h's");
static_assert(JPG_TABLE_BYTES == DTK_JPEG_HUFF_BYTES, "raw Huffman table size");
static_assert(JPG_420 == DTK_JPEG_420 && JPG_422 == DTK_JPEG_422 && JPG_444 == DTK_JPEG_444 && JPG_GRAY == DTK_JPEG_GRAY,
              "the samplings of jpeg_entropy.h are dtk.h's");

namespace {

constexpr int EBUF = 4096;      // staged, unstuffed bytes of a segment
constexpr int MARGIN = 256;     // bytes ahead of the reader before a block starts; a block is at most 248
constexpr int ESLACK = 16;      // zero bytes kept behind the staged data: the reader's window looks one word ahead
constexpr int SEG_FIELDS = DTK_JPEG_SEGMENT_FIELDS;
constexpr long long SEG_MAX_BYTES = 1ll << 28;   // bit positions are 32-bit
constexpr int MAX_FRAMES_PER_LAUNCH = 65535;
static_assert(EBUF % 64 == 0 && MARGIN + 64 + 4 <= EBUF, "a refill always stages at least one row of 64 bytes");

__constant__ uint8_t ZZ_OF_NAT[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                      41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                      46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// grid (segments), one wave each.  segs int64 [nseg][5]: frame, byte offset, byte length, first MCU, MCU count.
// huff uint8 [F][components][2][272] (component, DC / AC).  coef int16 [F][mcus][B][64].
template <int S>
__global__ __launch_bounds__(WAVE) void jpeg_entropy_kernel(const uint8_t* __restrict__ stream, long long stream_bytes,
                                                            const long long* __restrict__ segs, const uint8_t* __restrict__ huff,
                                                            int F, int mcus, int16_t* __restrict__ coef, int* __restrict__ status) {
    constexpr int B = jpg_blocks_per_mcu(S), NT = 2 * jpg_components(S);
    __shared__ JpgHuff tab[NT];
    __shared__ uint32_t buf[(EBUF + ESLACK) / 4];
    __shared__ uint32_t blk[32];   // 64 int16
    __shared__ uint32_t ctl[2];    // the reader's bit position, dead
    const int lane = threadIdx.x;
    const long long* sg = segs + (size_t)blockIdx.x * SEG_FIELDS;
    const long long f = sg[0], off = sg[1], len = sg[2], m0 = sg[3], nm = sg[4];
    if (f < 0 || f >= F) return;
    if (off < 0 || len < 0 || len > SEG_MAX_BYTES || off > stream_bytes - len || m0 < 0 || nm < 1 || m0 > mcus - nm) {
        if (lane == 0) atomicOr(&status[f], JPG_S_SEGMENT);
        return;
    }
    for (int t = 0; t < NT; ++t) jpg_huff_clear(&tab[t], lane, WAVE);
    if (lane < 32) blk[lane] = 0u;
    if (lane < 2) ctl[lane] = 0u;
    __syncthreads();
    for (int t = 0; t < NT; ++t) jpg_huff_fill(huff + ((size_t)f * NT + t) * JPG_TABLE_BYTES, &tab[t], lane, WAVE);
    __syncthreads();

    const uint8_t* src = stream + off;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(buf);
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + ((size_t)f * mcus + m0) * B * 64);
    long long raw_pos = 0;   // the next raw byte to stage (wave-uniform)
    int fill = 0;            // unstuffed bytes in buf (wave-uniform)
    int pred[3] = {0, 0, 0}, st = 0;   // lane 0's
    uint32_t iters = 0;
    const int nb = (int)nm * B;
    int k = 0;               // the block's place in its MCU (wave-uniform)
    for (int b = 0; b < nb; ++b) {
        uint32_t pos = ctl[0];
        const bool dead = ctl[1] != 0u;
        if (!dead && raw_pos < len && (long long)fill * 8 - (long long)pos < MARGIN * 8) {
            // move what is unread to the front (whole words), then stage rows of 64 raw bytes while a row fits
            const int base = min((int)(pos >> 5), fill / 4), nw = (fill + 3) / 4 - base;   // nw <= MARGIN / 4 + 2
            uint32_t keep[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) keep[i] = lane + 64 * i < nw ? buf[base + lane + 64 * i] : 0u;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (lane + 64 * i < nw) buf[lane + 64 * i] = keep[i];
            __syncthreads();
            fill -= 4 * base;
            pos -= 32u * (uint32_t)base;
            while (raw_pos < len && fill + 64 <= EBUF) {
                const long long i = raw_pos + lane;
                const bool valid = i < len;
                const unsigned v = valid ? src[i] : 0u, prev = valid && i > 0 ? src[i - 1] : 0u;
                const bool kept = valid && !(v == 0u && prev == 0xffu);
                const unsigned long long mask = __ballot(kept);
                if (kept) bytes[fill + __popcll(mask & ((1ull << lane) - 1ull))] = (uint8_t)v;
                fill += __popcll(mask);
                raw_pos += 64;
            }
            if (lane < ESLACK) bytes[fill + lane] = 0;
            __syncthreads();
        }
        if (lane == 0) {
            if (!dead) {
                JpgBits bits;
                jpg_bits_start(bits, buf, (uint32_t)fill * 8u, pos);
                const int comp = jpg_block_component(B, k);
                const int s = jpg_decode_block(bits, tab[2 * comp], tab[2 * comp + 1], pred[comp], reinterpret_cast<int16_t*>(blk), iters);
                st |= s;
                pos = bits.pos;
                if (s) ctl[1] = 1u;
            }
            ctl[0] = pos;
        }
        if (++k == B) k = 0;
        __syncthreads();
        if (lane < 32) {
            dst[(size_t)b * 32 + lane] = blk[lane];
            blk[lane] = 0u;
        }
        __syncthreads();
    }
    if (lane == 0) {
        const uint32_t pos = ctl[0];
        if (!st) {
            if (pos > (uint32_t)fill * 8u) st |= JPG_S_OVERRUN;
            else if (raw_pos < len || (uint32_t)fill * 8u - pos > 7u) st |= JPG_S_LEFTOVER;
        }
        if (st) atomicOr(&status[f], st);
    }
}

// ---- inverse DCT: the 13-bit fixed-point pass of docs/JPEG_DECODE.md section 2, 32-bit wrap-around arithmetic (unsigned) -----------
template <int N>
__device__ __forceinline__ void idct_pass(const int (&in)[8], int (&o)[8]) {
    typedef unsigned U;
    const U i0 = (U)in[0], i1 = (U)in[1], i2 = (U)in[2], i3 = (U)in[3], i4 = (U)in[4], i5 = (U)in[5], i6 = (U)in[6], i7 = (U)in[7];
    U z1 = (i2 + i6) * 4433u;
    const U t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
    const U t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
    const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    U a0 = i7, a1 = i5, a2 = i3, a3 = i1;
    z1 = a0 + a3;
    U z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const U z5 = (z3 + z4) * 9633u;
    a0 *= 2446u, a1 *= 16819u, a2 *= 25172u, a3 *= 12299u;
    z1 = 0u - z1 * 7373u, z2 = 0u - z2 * 20995u, z3 = z5 - z3 * 16069u, z4 = z5 - z4 * 3196u;
    a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
    constexpr U HALF = 1u << (N - 1);
    o[0] = (int)(t10 + a3 + HALF) >> N, o[7] = (int)(t10 - a3 + HALF) >> N;
    o[1] = (int)(t11 + a2 + HALF) >> N, o[6] = (int)(t11 - a2 + HALF) >> N;
    o[2] = (int)(t12 + a1 + HALF) >> N, o[5] = (int)(t12 - a1 + HALF) >> N;
    o[3] = (int)(t13 + a0 + HALF) >> N, o[4] = (int)(t13 - a0 + HALF) >> N;
}

constexpr int ITHREADS = 256, IBLOCKS = ITHREADS / 8;

// grid (ceil(mcus * B / 32), frames of this launch).  planes: per frame Y [MH mh][MW mw] (the MCU's size in pixels), then for the
// colour samplings Cb, Cr [8 mh][8 mw]: 64 B bytes per MCU.
template <int S>
__global__ __launch_bounds__(ITHREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ qtables,
                                                             int f0, int mw, int mcus, uint8_t* __restrict__ planes,
                                                             int* __restrict__ status) {
    constexpr int B = jpg_blocks_per_mcu(S), NC = jpg_components(S), NY = B < 3 ? B : B - 2;   // blocks, components, luma blocks
    constexpr int MW = jpg_mcu_width(S), MH = jpg_mcu_height(S), HY = MW / 8;                  // HY luma blocks side by side
    __shared__ int work[IBLOCKS][8][9];
    const int tid = threadIdx.x, lb = tid / 8, j = tid % 8;
    const size_t f = (size_t)f0 + blockIdx.y;
    const int gb = blockIdx.x * IBLOCKS + lb;   // block of the frame
    const bool active = gb < mcus * B;
    const int m = gb / B, k = gb - m * B;
    if (active) {
        const int16_t* c = coef + (f * mcus * B + gb) * 64;
        const uint8_t* q = qtables + (f * NC + jpg_block_component(B, k)) * 64;
        int d[8], o[8];
        bool wide = false;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int z = ZZ_OF_NAT[v * 8 + j];
            d[v] = (int)c[z] * (int)q[z];
            wide |= d[v] > 2047 || d[v] < -2047;
        }
        if (wide && status) atomicOr(&status[f], JPG_S_RANGE);
        idct_pass<11>(d, o);
#pragma unroll
        for (int v = 0; v < 8; ++v) work[lb][v][j] = o[v];
    }
    __syncthreads();
    if (active) {
        int d[8], o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = work[lb][j][u];
        idct_pass<18>(d, o);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lo |= (unsigned)min(255, max(0, o[u] + 128)) << (8 * u);
            hi |= (unsigned)min(255, max(0, o[u + 4] + 128)) << (8 * u);
        }
        const int my = m / mw, mx = m - my * mw;
        uint8_t* frame = planes + f * (size_t)mcus * (64 * B);
        uint8_t* p;
        if (k < NY) p = frame + ((size_t)(my * MH + (k / HY) * 8 + j) * mw * MW + mx * MW + (k % HY) * 8);
        else p = frame + (size_t)mcus * (64 * k) + ((size_t)(my * 8 + j) * mw * 8 + mx * 8);
        *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
    }
}

__device__ __forceinline__ int clamp255(int v) { return min(255, max(0, v)); }

// grid (ceil(ceil(W / 2) / 256), H, frames of this launch): thread c of row y makes the pixels (y, 2c) and (y, 2c + 1).  S is one of
// the three colour samplings.  The chroma context is clamped to the REAL plane of ch x cw samples; a plane at most two samples wide is
// replicated, not filtered -- in both directions (docs/JPEG_DECODE.md section 3).
template <int S>
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, int f0, int H, int W, int mw, int mcus,
                                                          uint8_t* __restrict__ out) {
    constexpr int B = jpg_blocks_per_mcu(S), NY = B - 2, MW = jpg_mcu_width(S);
    const int c = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (c >= (W + 1) / 2) return;
    const size_t f = (size_t)f0 + blockIdx.z;
    const uint8_t* frame = planes + f * (size_t)mcus * (64 * B);
    const int pitch = mw * 8;
    int up[2][2];   // [component][pixel]
    if (S == JPG_444) {
        const int x1 = min(2 * c + 1, W - 1);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint8_t* a = frame + (size_t)mcus * (64 * (NY + k)) + (size_t)y * pitch;
            up[k][0] = a[2 * c] - 128, up[k][1] = a[x1] - 128;
        }
    } else {
        const int cw = (W + 1) / 2;
        const int cl = max(c - 1, 0), cr_ = min(c + 1, cw - 1);
        if (S == JPG_422) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint8_t* a = frame + (size_t)mcus * (64 * (NY + k)) + (size_t)y * pitch;
                const int s = a[c];
                up[k][0] = (cw > 2 ? (3 * s + a[cl] + 1) >> 2 : s) - 128;
                up[k][1] = (cw > 2 ? (3 * s + a[cr_] + 2) >> 2 : s) - 128;
            }
        } else {
            const int ch = (H + 1) / 2;
            const int r = y >> 1, rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint8_t* a = frame + (size_t)mcus * (64 * (NY + k)) + (size_t)r * pitch;
                const uint8_t* b = frame + (size_t)mcus * (64 * (NY + k)) + (size_t)rn * pitch;
                if (cw > 2) {
                    const int sl = 3 * a[cl] + b[cl], s = 3 * a[c] + b[c], sr = 3 * a[cr_] + b[cr_];
                    up[k][0] = ((3 * s + sl + 8) >> 4) - 128;
                    up[k][1] = ((3 * s + sr + 7) >> 4) - 128;
                } else {
                    up[k][0] = up[k][1] = a[c] - 128;
                }
            }
        }
    }
    const uint8_t* yrow = frame + (size_t)y * mw * MW;
    uint8_t* o = out + ((f * H + y) * (size_t)W + 2 * c) * 3;
#pragma unroll
    for (int px = 0; px < 2; ++px) {
        if (2 * c + px >= W) break;
        const int Y = yrow[2 * c + px], cb = up[0][px], cr = up[1][px];
        o[3 * px + 0] = (uint8_t)clamp255(Y + ((91881 * cr + 32768) >> 16));
        o[3 * px + 1] = (uint8_t)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        o[3 * px + 2] = (uint8_t)clamp255(Y + ((116130 * cb + 32768) >> 16));
    }
}

// grid (ceil(W / 256), H, frames of this launch): the gray sampling's only plane, cut to H x W
__global__ __launch_bounds__(256) void jpeg_gray_kernel(const uint8_t* __restrict__ planes, int f0, int H, int W, int mw, int mcus,
                                                        uint8_t* __restrict__ out) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t f = (size_t)f0 + blockIdx.z;
    out[(f * H + y) * (size_t)W + x] = planes[f * (size_t)mcus * 64 + (size_t)y * mw * 8 + x];
}

bool sizes_ok(int F, int H, int W) { return F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }
long long mcus_of(int S, int H, int W) {
    const int mh = jpg_mcu_height(S), mw = jpg_mcu_width(S);
    return (long long)((H + mh - 1) / mh) * ((W + mw - 1) / mw);
}

template <int S>
int entropy_launch(const uint8_t* stream, long long stream_bytes, const int64_t* segments, int n_segments, const uint8_t* huffman, int F,
                   int mcus, int16_t* coef_out, int32_t* status, hipStream_t st) {
    DTK_LAUNCH("jpeg_entropy", jpeg_entropy_kernel<S>, dim3((unsigned)n_segments), dim3(WAVE), 0, st, stream, stream_bytes,
               reinterpret_cast<const long long*>(segments), huffman, F, mcus, coef_out, status);
    return 0;
}

template <int S>
int pixels_launch(const int16_t* coef, const uint8_t* qtables, int F, int H, int W, uint8_t* out, int32_t* status, uint8_t* planes,
                  hipStream_t st) {
    constexpr int B = jpg_blocks_per_mcu(S);
    const int mw = (W + jpg_mcu_width(S) - 1) / jpg_mcu_width(S), mcus = (int)mcus_of(S, H, W);
    for (int f0 = 0; f0 < F; f0 += MAX_FRAMES_PER_LAUNCH) {
        const unsigned nf = (unsigned)std::min(F - f0, MAX_FRAMES_PER_LAUNCH);
        DTK_LAUNCH("jpeg_idct", jpeg_idct_kernel<S>, dim3((unsigned)dtk_cdiv((long long)mcus * B, IBLOCKS), nf), dim3(ITHREADS), 0, st,
                   coef, qtables, f0, mw, mcus, planes, status);
        if constexpr (S == JPG_GRAY) {
            DTK_LAUNCH("jpeg_gray", jpeg_gray_kernel, dim3((unsigned)dtk_cdiv(W, 256), (unsigned)H, nf), dim3(256), 0, st, planes, f0, H, W,
                       mw, mcus, out);
        } else {
            DTK_LAUNCH("jpeg_colour", jpeg_colour_kernel<S>, dim3((unsigned)dtk_cdiv((W + 1) / 2, 256), (unsigned)H, nf), dim3(256), 0, st,
                       planes, f0, H, W, mw, mcus, out);
        }
    }
    return 0;
}

}  // namespace

extern "C" size_t dtk_jpeg_decode_workspace_bytes_sampled(int32_t sampling, int32_t F, int32_t H, int32_t W) {
    if (!jpg_sampling_ok(sampling) || !sizes_ok(F, H, W)) return 0;
    return ((size_t)F * mcus_of(sampling, H, W) * 64 * jpg_blocks_per_mcu(sampling) + 255) & ~(size_t)255;
}

extern "C" int dtk_jpeg_decode_coefficients_sampled(int32_t sampling, const uint8_t* stream, int64_t stream_bytes,
                                                    const int64_t* segments, const int64_t* segments_host, int32_t n_segments,
                                                    const uint8_t* huffman, int32_t F, int32_t H, int32_t W, int16_t* coef_out,
                                                    int32_t* status, void* stream_) {
    DTK_REQUIRE(jpg_sampling_ok(sampling), "jpeg_decode_coefficients: sampling must be DTK_JPEG_420, _422, _444 or _GRAY (0 .. 3), got %d",
                sampling);
    DTK_REQUIRE(sizes_ok(F, H, W), "jpeg_decode_coefficients: F >= 1 and 1 <= H, W <= 65535 are required, got F=%d %d x %d", F, H, W);
    DTK_REQUIRE(stream && segments && segments_host && huffman && coef_out && status,
                "jpeg_decode_coefficients: null pointer (stream / segments / segments_host / huffman / coef_out / status)");
    DTK_REQUIRE(stream_bytes >= 1 && n_segments >= 1, "jpeg_decode_coefficients: stream_bytes and n_segments must be positive, got %lld, %d",
                (long long)stream_bytes, n_segments);
    const long long mcus = mcus_of(sampling, H, W);
    for (int s = 0; s < n_segments; ++s) {
        const int64_t* g = segments_host + (size_t)s * SEG_FIELDS;
        DTK_REQUIRE(g[0] >= 0 && g[0] < F && g[1] >= 0 && g[2] >= 0 && g[2] <= SEG_MAX_BYTES && g[1] <= stream_bytes - g[2] && g[3] >= 0 &&
                        g[4] >= 1 && g[3] <= mcus - g[4],
                    "jpeg_decode_coefficients: segment %d (frame %lld, bytes %lld + %lld, MCUs %lld + %lld) does not fit %d frames, "
                    "%lld bytes, %lld MCUs",
                    s, (long long)g[0], (long long)g[1], (long long)g[2], (long long)g[3], (long long)g[4], F, (long long)stream_bytes,
                    mcus);
    }
    hipStream_t st = dtk_stream(stream_);
    DTK_HIP(dtk_zero_async(status, (size_t)F * 4, st));
    switch (sampling) {
        case JPG_420: return entropy_launch<JPG_420>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, coef_out, status, st);
        case JPG_422: return entropy_launch<JPG_422>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, coef_out, status, st);
        case JPG_444: return entropy_launch<JPG_444>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, coef_out, status, st);
        default: return entropy_launch<JPG_GRAY>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, coef_out, status, st);
    }
}

extern "C" int dtk_jpeg_pixels_sampled(int32_t sampling, const int16_t* coef, const uint8_t* qtables, int32_t F, int32_t H, int32_t W,
                                       uint8_t* out, int32_t* status, void* workspace, void* stream) {
    DTK_REQUIRE(jpg_sampling_ok(sampling), "jpeg_pixels: sampling must be DTK_JPEG_420, _422, _444 or _GRAY (0 .. 3), got %d", sampling);
    DTK_REQUIRE(sizes_ok(F, H, W), "jpeg_pixels: F >= 1 and 1 <= H, W <= 65535 are required, got F=%d %d x %d", F, H, W);
    DTK_REQUIRE(coef && qtables && out && workspace, "jpeg_pixels: null pointer (coef / qtables / out / workspace)");
    uint8_t* planes = reinterpret_cast<uint8_t*>(workspace);
    hipStream_t st = dtk_stream(stream);
    switch (sampling) {
        case JPG_420: return pixels_launch<JPG_420>(coef, qtables, F, H, W, out, status, planes, st);
        case JPG_422: return pixels_launch<JPG_422>(coef, qtables, F, H, W, out, status, planes, st);
        case JPG_444: return pixels_launch<JPG_444>(coef, qtables, F, H, W, out, status, planes, st);
        default: return pixels_launch<JPG_GRAY>(coef, qtables, F, H, W, out, status, planes, st);
    }
}

// the entry points from before the other samplings: 4:2:0
extern "C" size_t dtk_jpeg_decode_workspace_bytes(int32_t F, int32_t H, int32_t W) {
    return dtk_jpeg_decode_workspace_bytes_sampled(JPG_420, F, H, W);
}

extern "C" int dtk_jpeg_decode_coefficients(const uint8_t* stream, int64_t stream_bytes, const int64_t* segments,
                                            const int64_t* segments_host, int32_t n_segments, const uint8_t* huffman, int32_t F,
                                            int32_t H, int32_t W, int16_t* coef_out, int32_t* status, void* stream_) {
    return dtk_jpeg_decode_coefficients_sampled(JPG_420, stream, stream_bytes, segments, segments_host, n_segments, huffman, F, H, W,
                                                coef_out, status, stream_);
}

extern "C" int dtk_jpeg_pixels(const int16_t* coef, const uint8_t* qtables, int32_t F, int32_t H, int32_t W, uint8_t* out,
                               int32_t* status, void* workspace, void* stream) {
    return dtk_jpeg_pixels_sampled(JPG_420, coef, qtables, F, H, W, out, status, workspace, stream);
}
