// jpeg_progressive.hip -- video ingest: the entropy stage of PROGRESSIVE JPEG files (SOF2, 8 bit, Huffman; docs/JPEG_DECODE.md,
// "Progressive files").  A progressive file codes its coefficients in several scans: each scan holds one band [Ss, Se] of the zigzag
// coefficients, of one component or (DC only) of all three interleaved, either for the first time down to bit Al or as a refinement
// that adds bit Al.  The output is the int16 [F][MCUs][B][64] layout of jpeg_decode.hip, so dtk_jpeg_pixels_sampled follows unchanged.
// The host (dino_tracker_amd/video_in.py) walks the markers and hands over a table of SEGMENTS -- the restart intervals of every scan
// of every frame, or whole scans -- each with its LEVEL: a scan that refines what an earlier one wrote has a higher level than it.
//
//   jpeg_progressive_kernel : launched ONCE PER LEVEL, in stream order, so a refinement sees what its predecessors wrote.  ONE WAVE per
//                             segment, as in jpeg_entropy_kernel: the lanes build the segment's look-ups in LDS (up to three DC tables
//                             or one AC table), stage and unstuff the bytes in chunks (ballot + popcount), lane 0 walks the bits with
//                             jpeg_entropy.h's per-block routines.  The coefficients move through LDS in GROUPS of GROUP blocks: before
//                             lane 0 needs them the lanes zero the group's bands (first scans) or load them from memory (refinement
//                             scans), afterwards they write them back.
//
// THE STORE RULE.  Scans of one level write different coefficients of the SAME block concurrently (the DC scan and four AC scans share
// level 0).  A wave therefore loads and stores only the int16s inside its own [Ss, Se] band of the blocks it covers, one 2-byte access
// each: no whole-block 128-byte store, no wider store that could overlap a neighbour band, and read-modify-write on its own int16s
// only.
//
// Safety (docs/JPEG_DECODE.md section 5): a row of the table that does not fit the stream, the frame count, the scan's unit count or
// the table count decodes nothing (jpg_prog_row_ok, checked on the host copy by the library and on the device copy here); the loop
// count is the segment's block count; the reader never leaves the staged bytes.
#include <algorithm>
#include "common.h"
#include "jpeg_entropy.h"

static_assert(JPG_PROG_FIELDS == DTK_JPEG_PROG_FIELDS, "the segment row of jpeg_entropy.h is dtk.h's");

namespace {

constexpr int EBUF = 4096;      // staged, unstuffed bytes of a segment
constexpr int MARGIN = 256;     // bytes ahead of the reader before a block starts; a block is at most 63 * 31 bits = 245 bytes
constexpr int ESLACK = 16;      // zero bytes kept behind the staged data: the reader's window looks one word ahead
constexpr int GROUP = 32;       // blocks whose bands are staged in LDS together
constexpr long long SEG_MAX_BYTES = 1ll << 28;   // bit positions are 32-bit
static_assert(EBUF % 64 == 0 && MARGIN + 64 + 4 <= EBUF, "a refill always stages at least one row of 64 bytes");

// grid (segments of this level), one wave each.  segs int64 [n][JPG_PROG_FIELDS] (dtk.h), tables uint8 [n_tables][272],
// coef int16 [F][mcus][B][64].
template <int S>
__global__ __launch_bounds__(WAVE) void jpeg_progressive_kernel(const uint8_t* __restrict__ stream, long long stream_bytes,
                                                                const long long* __restrict__ segs, int level,
                                                                const uint8_t* __restrict__ tables, int n_tables, int F, int H, int W,
                                                                int16_t* coef, int* __restrict__ status) {
    constexpr int B = jpg_blocks_per_mcu(S);
    __shared__ JpgHuff tab[3];
    __shared__ uint32_t buf[(EBUF + ESLACK) / 4];
    __shared__ int16_t band[GROUP * 64];
    __shared__ uint32_t ctl[2];    // the reader's bit position, dead
    const int lane = threadIdx.x;
    const long long* sg = segs + (size_t)blockIdx.x * JPG_PROG_FIELDS;
    const long long f = sg[0];
    if (f < 0 || f >= F) return;
    if (!jpg_prog_row_ok(sg, S, F, H, W, stream_bytes, n_tables, SEG_MAX_BYTES) || sg[3] != level) {
        if (lane == 0) atomicOr(&status[f], JPG_S_SEGMENT);
        return;
    }
    const long long off = sg[1], len = sg[2], u0 = sg[9], nu = sg[10];
    const JpgScan sc = {(int)sg[4], (int)sg[5], (int)sg[6], (int)sg[7], (int)sg[8]};
    const int ntab = sc.Ss == 0 ? (sc.Ah ? 0 : sc.comp < 0 ? 3 : 1) : 1;
    for (int t = 0; t < ntab; ++t) jpg_huff_clear(&tab[t], lane, WAVE);
    if (lane < 2) ctl[lane] = 0u;
    __syncthreads();
    for (int t = 0; t < ntab; ++t) jpg_huff_fill(tables + (size_t)sg[11 + t] * JPG_TABLE_BYTES, &tab[t], lane, WAVE);
    __syncthreads();

    const uint8_t* src = stream + off;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(buf);
    int16_t* frame = coef + (size_t)f * (size_t)jpg_mcus(S, H, W) * B * 64;
    const long long nb = sc.comp < 0 ? nu * B : nu;   // units <= 67 M MCUs x 6: fits
    const int width = sc.Se - sc.Ss + 1;
    long long raw_pos = 0;   // the next raw byte to stage (wave-uniform)
    int fill = 0;            // unstuffed bytes in buf (wave-uniform)
    int pred[3] = {0, 0, 0}, st = 0;   // lane 0's
    uint32_t run = 0, iters = 0;       // lane 0's
    int k = 0;               // the block's place in its MCU (wave-uniform; the interleaved scan)
    bool dead = false;
    for (long long g0 = 0; g0 < nb && !dead; g0 += GROUP) {
        const int gn = (int)min((long long)GROUP, nb - g0);
        // the group's bands: zero for a first scan, what the earlier levels wrote for a refinement -- this scan's int16s only
        for (int i = lane; i < gn * width; i += WAVE) {
            const int j = i / width, c = sc.Ss + (i - j * width);
            band[j * 64 + c] = sc.Ah ? frame[jpg_scan_block(S, sc.comp, u0, g0 + j, W) * 64 + c] : (int16_t)0;
        }
        __syncthreads();
        for (int j = 0; j < gn; ++j) {
            uint32_t pos = ctl[0];
            dead = ctl[1] != 0u;
            if (dead) break;
            if (raw_pos < len && (long long)fill * 8 - (long long)pos < MARGIN * 8) {
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
                JpgBits bits;
                jpg_bits_start(bits, buf, (uint32_t)fill * 8u, pos);
                int16_t* out = band + j * 64;
                const uint32_t left = (uint32_t)min(nb - g0 - j, 0x7fffffffll);
                int s;
                if (sc.Ss == 0) {
                    const int c = sc.comp < 0 ? jpg_block_component(B, k) : 0;
                    s = sc.Ah ? jpg_prog_dc_refine(bits, sc.Al, out, iters) : jpg_prog_dc_first(bits, tab[c], pred[c], sc.Al, out, iters);
                } else {
                    s = sc.Ah ? jpg_prog_ac_refine(bits, tab[0], sc.Ss, sc.Se, sc.Al, run, left, out, iters)
                              : jpg_prog_ac_first(bits, tab[0], sc.Ss, sc.Se, sc.Al, run, left, out, iters);
                }
                st |= s;
                if (s) ctl[1] = 1u;
                ctl[0] = bits.pos;
            }
            if (++k == B) k = 0;
            __syncthreads();
        }
        // the bands go back.  After a fault the blocks behind the faulty one still hold what was loaded (or zero, which is what a first
        // scan finds in memory): writing them changes nothing.
        for (int i = lane; i < gn * width; i += WAVE) {
            const int j = i / width, c = sc.Ss + (i - j * width);
            frame[jpg_scan_block(S, sc.comp, u0, g0 + j, W) * 64 + c] = band[j * 64 + c];
        }
        __syncthreads();
        dead = ctl[1] != 0u;
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

template <int S>
int level_launch(const uint8_t* stream, long long stream_bytes, const int64_t* segments, int n, int level, const uint8_t* tables,
                 int n_tables, int F, int H, int W, int16_t* coef, int32_t* status, hipStream_t st) {
    DTK_LAUNCH("jpeg_progressive", jpeg_progressive_kernel<S>, dim3((unsigned)n), dim3(WAVE), 0, st, stream, stream_bytes,
               reinterpret_cast<const long long*>(segments), level, tables, n_tables, F, H, W, coef, status);
    return 0;
}

}  // namespace

extern "C" int dtk_jpeg_decode_progressive(int32_t sampling, const uint8_t* stream, int64_t stream_bytes, const int64_t* segments,
                                           const int64_t* segments_host, int32_t n_segments, const uint8_t* tables, int32_t n_tables,
                                           int32_t F, int32_t H, int32_t W, int16_t* coef, int32_t* status, void* stream_) {
    DTK_REQUIRE(jpg_sampling_ok(sampling), "jpeg_decode_progressive: sampling must be DTK_JPEG_420, _422, _444 or _GRAY (0 .. 3), got %d",
                sampling);
    DTK_REQUIRE(F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535,
                "jpeg_decode_progressive: F >= 1 and 1 <= H, W <= 65535 are required, got F=%d %d x %d", F, H, W);
    DTK_REQUIRE(stream && segments && segments_host && tables && coef && status,
                "jpeg_decode_progressive: null pointer (stream / segments / segments_host / tables / coef / status)");
    DTK_REQUIRE(stream_bytes >= 1 && n_segments >= 1 && n_tables >= 1,
                "jpeg_decode_progressive: stream_bytes, n_segments and n_tables must be positive, got %lld, %d, %d", (long long)stream_bytes,
                n_segments, n_tables);
    long long level = 0;
    for (int s = 0; s < n_segments; ++s) {
        const long long* g = reinterpret_cast<const long long*>(segments_host) + (size_t)s * JPG_PROG_FIELDS;
        DTK_REQUIRE(jpg_prog_row_ok(g, sampling, F, H, W, stream_bytes, n_tables, SEG_MAX_BYTES) && g[3] >= level,
                    "jpeg_decode_progressive: segment %d (frame %lld, bytes %lld + %lld, level %lld, band %lld-%lld, Ah %lld, Al %lld, "
                    "component %lld, units %lld + %lld, tables %lld %lld %lld) does not fit %d frames, %lld bytes, %lld units, %d tables, "
                    "or its level is below the row before it",
                    s, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], F, (long long)stream_bytes,
                    g[8] >= -1 && g[8] < jpg_components(sampling) ? jpg_scan_units(sampling, (int)g[8], H, W) : -1ll, n_tables);
        level = g[3];
    }
    hipStream_t st = dtk_stream(stream_);
    DTK_HIP(dtk_zero_async(status, (size_t)F * 4, st));
    DTK_HIP(dtk_zero_async(coef, (size_t)F * (size_t)jpg_mcus(sampling, H, W) * jpg_blocks_per_mcu(sampling) * 128, st));
    for (int a = 0; a < n_segments;) {
        const long long lv = segments_host[(size_t)a * JPG_PROG_FIELDS + 3];
        int b = a;
        while (b < n_segments && segments_host[(size_t)b * JPG_PROG_FIELDS + 3] == lv) ++b;
        const int64_t* rows = segments + (size_t)a * JPG_PROG_FIELDS;
        int rc;
        switch (sampling) {
            case JPG_420: rc = level_launch<JPG_420>(stream, stream_bytes, rows, b - a, (int)lv, tables, n_tables, F, H, W, coef, status, st); break;
            case JPG_422: rc = level_launch<JPG_422>(stream, stream_bytes, rows, b - a, (int)lv, tables, n_tables, F, H, W, coef, status, st); break;
            case JPG_444: rc = level_launch<JPG_444>(stream, stream_bytes, rows, b - a, (int)lv, tables, n_tables, F, H, W, coef, status, st); break;
            default: rc = level_launch<JPG_GRAY>(stream, stream_bytes, rows, b - a, (int)lv, tables, n_tables, F, H, W, coef, status, st); break;
        }
        if (rc) return rc;
        a = b;
    }
    return 0;
}
