// jpeg.hip -- video output: a baseline JPEG encoder (SOF0, 8 bit, 4:2:0, interleaved scan, restart interval DTK_JPEG_RESTART MCUs)
// whose arithmetic is written down in docs/JPEG.md and is integer throughout, so the bytes do not depend on the device.  Three
// stages with their hand-offs in the caller's workspace (include/dtk.h, dtk_jpeg_encode):
//
//   jpeg_transform_kernel : one workgroup of 256 threads per strip of STRIP = 4 MCUs (64 x 16 pixels).  The strip's interleaved RGB
//                           rows are read once, a lane per byte, into LDS with the coordinates clamped to the frame (that IS the
//                           edge replication of Y, and of chroma to the right); Y and the 2 x 2 downsampled Cb / Cr are formed in
//                           LDS; then eight lanes own one 8 x 8 block: lane j runs the row pass of row j, the passes exchange through
//                           LDS, lane j runs the column pass of column j and quantises.  The strip's 24 blocks leave as one
//                           contiguous run of int16 [MCU][6][64] in zigzag order.
//   jpeg_code_kernel      : one workgroup per restart interval -- intervals are independent by construction (the DC predictors restart
//                           and the bit stream is byte-aligned at every RST marker).  A thread per block finds the block's bit
//                           count, the counts are scanned, the thread codes the block again into an LDS bit buffer at its offset
//                           (32 bits at a time with LDS atomic ORs: neighbouring blocks share a word), and the workgroup copies the
//                           bytes out with a 0x00 after every 0xFF, a byte per lane, into the interval's slot.
//   jpeg_frame_scan_kernel, jpeg_offsets_kernel, jpeg_copy_kernel : the interval lengths of a frame and the frame lengths of the
//                           call are scanned, and header, intervals with their RST markers and EOI are copied into one byte stream.
//                           Nothing is written to `out` unless the whole stream fits out_capacity.
//
// Sizes: a coded block is at most 20 + 63 * 26 = 1658 bits (docs/JPEG.md section 6; the coder clamps a coefficient to the range the
// Huffman tables can express, which the transform never leaves, so the bound holds whatever the coefficient buffer contains), an
// interval at most 16 * 6 * 1658 bits = 19 896 bytes before stuffing and twice that after it: DTK_JPEG_INTERVAL_BYTES.
#include <algorithm>
#include "block_scan.h"

namespace {

constexpr int R = DTK_JPEG_RESTART;
constexpr int STRIP = 4;                                   // MCUs per workgroup of the transform stage
constexpr int THREADS = 256, WAVES = THREADS / WAVE;
constexpr int BLOCK_BITS_MAX = 20 + 63 * 26;               // DC: 9-bit code + 11 bits; AC: 16-bit code + 10 bits
constexpr int INTERVAL_BITS_MAX = R * 6 * BLOCK_BITS_MAX;  // 159 168
constexpr int INTERVAL_WORDS = INTERVAL_BITS_MAX / 32 + 2;
constexpr int SLOT = DTK_JPEG_INTERVAL_BYTES;
constexpr int CZ_STRIDE = 66;                              // int16 per staged block: 33 words, so a lane per block meets no bank twice
constexpr int MAX_FRAMES_PER_LAUNCH = 65535;               // gridDim.y
static_assert(2 * (INTERVAL_BITS_MAX / 8) <= SLOT, "an interval's slot holds its worst case");
static_assert(SLOT % 64 == 0 && R * 6 <= THREADS, "slot alignment; a thread per block of an interval");

// zigzag index of the coefficient at natural (row-major) position v * 8 + u
__constant__ uint8_t ZZ_OF_NATURAL[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                          41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                          46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ---- Annex K.3: the four typical Huffman tables as (length << 16 | code) by symbol, built at compile time ---------------------------
struct HuffSpec {
    uint8_t bits[16];    // codes of length 1 .. 16
    uint8_t vals[162];   // symbols in code order
};
struct HuffCodes {
    uint32_t e[256];
};
constexpr HuffCodes make_codes(const HuffSpec& s) {
    HuffCodes t{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) t.e[s.vals[k++]] = ((unsigned)len << 16) | code++;
        code <<= 1;
    }
    return t;
}
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
     0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
     0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
     0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
     0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
     0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
     0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
     0xF9, 0xFA}};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
     0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
     0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
     0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
     0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
     0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
     0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
     0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
     0xF9, 0xFA}};
// [0]: luma, [1]: chroma; the 256 AC entries, then the 16 DC entries (categories 0 .. 11)
constexpr int HUFF_WORDS = 256 + 16;
struct HuffAll {
    uint32_t e[2][HUFF_WORDS];
};
constexpr HuffAll make_all() {
    HuffAll a{};
    const HuffCodes ac[2] = {make_codes(AC_LUMA), make_codes(AC_CHROMA)}, dc[2] = {make_codes(DC_LUMA), make_codes(DC_CHROMA)};
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < 256; ++i) a.e[c][i] = ac[c].e[i];
        for (int i = 0; i < 16; ++i) a.e[c][256 + i] = dc[c].e[i];
    }
    return a;
}
__constant__ HuffAll HUFF = make_all();

// ---- forward DCT: the 13-bit fixed-point Loeffler-Ligtenberg-Moschytz pass of docs/JPEG.md section 3 ----------------------------------
// FIRST: outputs 0 and 4 are shifted left by 2, the others descaled by 11; second pass: 0 and 4 descaled by 2, the others by 15.
template <bool FIRST>
__device__ __forceinline__ void dct_pass(const int (&d)[8], int (&o)[8]) {
    constexpr int N = FIRST ? 11 : 15, HALF = 1 << (N - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if constexpr (FIRST) {
        o[0] = (t10 + t11) * 4;
        o[4] = (t10 - t11) * 4;
    } else {
        o[0] = (t10 + t11 + 2) >> 2;
        o[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    o[2] = (z1 + t13 * 6270 + HALF) >> N;
    o[6] = (z1 - t12 * 15137 + HALF) >> N;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 = -z1 * 7373, z2 = -z2 * 20995, z3 = -z3 * 16069 + z5, z4 = -z4 * 3196 + z5;
    o[7] = (a4 + z1 + z3 + HALF) >> N;
    o[5] = (a5 + z2 + z4 + HALF) >> N;
    o[3] = (a6 + z2 + z3 + HALF) >> N;
    o[1] = (a7 + z1 + z4 + HALF) >> N;
}

__device__ __forceinline__ int quantise(int c, int q) {   // round half away from zero; the divisions truncate
    const unsigned q8 = 8u * (unsigned)q, a = (unsigned)(c < 0 ? -c : c);
    const int v = (int)((a + q8 / 2) / q8);
    return c < 0 ? -v : v;
}

// grid (strips * mh, frames of this launch).  coef: int16 [F][mh * mw][6][64], zigzag.
__global__ __launch_bounds__(THREADS) void jpeg_transform_kernel(const uint8_t* __restrict__ frames, int f0, int H, int W, int mw,
                                                                 int strips, const uint8_t* __restrict__ qtables,
                                                                 int16_t* __restrict__ coef) {
    constexpr int PW = STRIP * 16, ROW = PW * 3, NB = STRIP * 6;
    __shared__ uint8_t rgb[16][ROW];          // the strip's pixels, coordinates clamped to the frame
    __shared__ int16_t ys[16][PW];            // Y - 128
    __shared__ int16_t cs[2][8][PW / 2];      // Cb - 128, Cr - 128 after the downsample
    __shared__ int work[NB][8][9];            // between the passes: [block][row][u], rows padded to 9 words (no bank met twice)
    __shared__ __align__(4) int16_t outq[NB * 64];
    __shared__ uint8_t qt[128];
    const int tid = threadIdx.x;
    const size_t f = (size_t)f0 + blockIdx.y;
    const int my = blockIdx.x / strips, mx0 = (blockIdx.x - my * strips) * STRIP;
    const int y0 = my * 16, x0 = mx0 * 16;
    const uint8_t* src = frames + f * H * W * 3;
    if (tid < 128) qt[tid] = qtables[tid];
    for (int i = tid; i < 16 * ROW; i += THREADS) {
        const int ly = i / ROW, e = i - ly * ROW, px = e / 3, c = e - px * 3;
        const int sy = min(y0 + ly, H - 1), sx = min(x0 + px, W - 1);
        rgb[ly][e] = src[((size_t)sy * W + sx) * 3 + c];
    }
    __syncthreads();
    for (int i = tid; i < 16 * PW; i += THREADS) {
        const int ly = i / PW, lx = i - ly * PW;
        const int r = rgb[ly][3 * lx], g = rgb[ly][3 * lx + 1], b = rgb[ly][3 * lx + 2];
        ys[ly][lx] = (int16_t)(((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128);
    }
    // chroma row r of the frame averages the pixel rows 2 r', 2 r' + 1 with r' = min(r, He / 2 - 1), He = H rounded up to even: the
    // last DOWNSAMPLED row is what repeats down to the MCU boundary.  r' lies in this MCU row, and the staged rows are clamped to H - 1.
    const int last_crow = (H + (H & 1)) / 2 - 1;
    for (int i = tid; i < 2 * 8 * (PW / 2); i += THREADS) {
        const int comp = i / (8 * (PW / 2)), j = i - comp * 8 * (PW / 2), r = j / (PW / 2), c = j - r * (PW / 2);
        const int lr = 2 * min(my * 8 + r, last_crow) - y0;
        int sum = 1 + (c & 1);   // the bias 1, 2, 1, 2, ... along the row (a strip starts at an even chroma column)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* p = &rgb[lr + (k >> 1)][3 * (2 * c + (k & 1))];
            const int rr = p[0], g = p[1], b = p[2];
            sum += comp == 0 ? (-11059 * rr - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
                             : (32768 * rr - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
        }
        cs[comp][r][c] = (int16_t)((sum >> 2) - 128);
    }
    __syncthreads();
    // eight lanes per block: block = MCU jm of the strip, k = Y00 Y01 Y10 Y11 Cb Cr
    const int blk = tid / 8, j = tid % 8, jm = blk / 6, k = blk - jm * 6;
    const bool active = blk < NB;
    // a Y block beyond the last block column / row that holds a real pixel is not transformed
    const bool dummy = active && k < 4 && (2 * (mx0 + jm) + (k & 1) >= (W + 7) / 8 || 2 * my + (k >> 1) >= (H + 7) / 8);
    const int16_t* first = k < 4 ? &ys[(k >> 1) * 8][jm * 16 + (k & 1) * 8] : &cs[k - 4][0][jm * 8];
    const int pitch = k < 4 ? PW : PW / 2;
    if (active && !dummy) {
        int d[8], o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = first[j * pitch + u];
        dct_pass<true>(d, o);
#pragma unroll
        for (int u = 0; u < 8; ++u) work[blk][j][u] = o[u];
    }
    __syncthreads();
    if (active) {
        int d[8], o[8] = {};
        if (!dummy) {
#pragma unroll
            for (int y = 0; y < 8; ++y) d[y] = work[blk][y][j];
            dct_pass<false>(d, o);
        }
        const uint8_t* q = qt + (k < 4 ? 0 : 64);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int z = ZZ_OF_NATURAL[v * 8 + j];
            outq[blk * 64 + z] = dummy ? (int16_t)0 : (int16_t)quantise(o[v], q[z]);
        }
    }
    __syncthreads();
    // a dummy block's DC repeats the previous block's of its MCU (which may be dummy too; Y00 never is)
    if (tid < STRIP) {
        for (int kk = 1; kk < 4; ++kk)
            if (2 * (mx0 + tid) + (kk & 1) >= (W + 7) / 8 || 2 * my + (kk >> 1) >= (H + 7) / 8)
                outq[(tid * 6 + kk) * 64] = outq[(tid * 6 + kk - 1) * 64];
    }
    __syncthreads();
    const int nm = min(STRIP, mw - mx0);
    const size_t mcus = (size_t)mw * gridDim.x / strips;   // gridDim.x = strips * mh
    uint32_t* dst = reinterpret_cast<uint32_t*>(coef + ((f * mcus + (size_t)my * mw + mx0) * 6) * 64);
    const uint32_t* from = reinterpret_cast<const uint32_t*>(outq);
    for (int i = tid; i < nm * 6 * 32; i += THREADS) dst[i] = from[i];
}

// the bits of one block, most significant first, into `buf` from bit `pos` (EMIT), or only their count
template <bool EMIT>
struct BitSink {
    uint32_t* buf;
    unsigned long long acc = 0;
    int held, word, total = 0;
    __device__ BitSink(uint32_t* b, int pos) : buf(b), held(pos & 31), word(pos >> 5) {}
    __device__ __forceinline__ void put(unsigned v, int n) {   // n <= 27
        total += n;
        if (EMIT) {
            acc = (acc << n) | v;
            held += n;
            if (held >= 32) {
                held -= 32;
                atomicOr(&buf[word++], (uint32_t)(acc >> held));
            }
        }
    }
    __device__ __forceinline__ void put_code(uint32_t entry) { put(entry & 0xffffu, (int)(entry >> 16)); }
    __device__ __forceinline__ void flush() {
        if (EMIT && held > 0) atomicOr(&buf[word], (uint32_t)(acc << (32 - held)));
    }
};

// category (bit length of |v|) and the value bits of v: v itself, or the low bits of v - 1 when negative
__device__ __forceinline__ void categorise(int v, int& size, unsigned& bits) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    size = 32 - __clz((int)a);
    bits = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
}

// z: 64 coefficients in zigzag order (LDS); huff: the component's AC entries, then its DC entries.  Values are clamped to what the
// tables can express (|difference| <= 2047, |AC| <= 1023): the transform never leaves that range, and the clamp makes
// BLOCK_BITS_MAX hold for ANY coefficient buffer, so that no bit lands outside the buffer.
template <bool EMIT>
__device__ int code_block(const int16_t* z, int pred, const uint32_t* huff, uint32_t* buf, int pos) {
    BitSink<EMIT> sink(buf, pos);
    int size;
    unsigned bits;
    categorise(max(-2047, min(2047, (int)z[0] - pred)), size, bits);
    const uint32_t dc = huff[256 + size];
    sink.put(((dc & 0xffffu) << size) | bits, (int)(dc >> 16) + size);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = max(-1023, min(1023, (int)z[k]));
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) sink.put_code(huff[0xF0]);   // ZRL: sixteen zeros
        categorise(v, size, bits);
        const uint32_t ac = huff[(run << 4) | size];
        sink.put(((ac & 0xffffu) << size) | bits, (int)(ac >> 16) + size);
        run = 0;
    }
    if (run) sink.put_code(huff[0x00]);   // EOB, only when the block ends in zeros
    sink.flush();
    return sink.total;
}

// grid (intervals per frame, frames of this launch).  slots: [F][n_int][SLOT] bytes, ilen: uint32 [F][n_int].
__global__ __launch_bounds__(THREADS) void jpeg_code_kernel(const int16_t* __restrict__ coef, int f0, int mcus, int n_int,
                                                            uint8_t* __restrict__ slots, uint32_t* __restrict__ ilen) {
    __shared__ __align__(4) int16_t cz[R * 6][CZ_STRIDE];
    __shared__ uint32_t bitbuf[INTERVAL_WORDS];
    __shared__ uint32_t huff[2][HUFF_WORDS];
    const int tid = threadIdx.x;
    const size_t f = (size_t)f0 + blockIdx.y;
    const int it = blockIdx.x, m0 = it * R, nm = min(R, mcus - m0), nb = nm * 6;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(coef + ((f * mcus + m0) * 6) * 64);
    for (int i = tid; i < nb * 32; i += THREADS)
        *reinterpret_cast<uint32_t*>(&cz[i / 32][2 * (i % 32)]) = src[i];
    for (int i = tid; i < 2 * HUFF_WORDS; i += THREADS) huff[i / HUFF_WORDS][i % HUFF_WORDS] = HUFF.e[i / HUFF_WORDS][i % HUFF_WORDS];
    __syncthreads();
    // DC prediction: the previous block of the same component inside the interval, 0 at its start
    const int m = tid / 6, k = tid - m * 6, comp = k < 4 ? 0 : 1;
    int pred = 0;
    if (tid < nb) {
        if (k >= 1 && k <= 3) pred = cz[tid - 1][0];
        else if (m > 0) pred = cz[tid - (k == 0 ? 3 : 6)][0];
    }
    const int len = tid < nb ? code_block<false>(cz[tid], pred, huff[comp], nullptr, 0) : 0;
    int total_bits;
    const int pos = block_scan_excl<WAVES>(len, total_bits);
    for (int i = tid; i < total_bits / 32 + 1; i += THREADS) bitbuf[i] = 0u;
    __syncthreads();
    if (tid < nb) code_block<true>(cz[tid], pred, huff[comp], bitbuf, pos);
    __syncthreads();
    const int pad = -total_bits & 7;   // the partial byte is completed with 1-bits
    if (tid == 0 && pad) bitbuf[total_bits >> 5] |= ((1u << pad) - 1u) << (32 - (total_bits & 31) - pad);
    __syncthreads();
    // a byte per lane; a 0x00 follows every 0xFF.  An output position is the byte's index plus the 0xFF bytes before it.
    const int nbytes = (total_bits + 7) / 8;
    uint8_t* slot = slots + (f * n_int + it) * SLOT;
    int stuffed = 0;
    for (int i0 = 0; i0 < nbytes; i0 += THREADS) {
        const int i = i0 + tid;
        const unsigned byte = i < nbytes ? (bitbuf[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu : 0u;
        const int ff = byte == 0xffu;
        int chunk;
        const int o = i + stuffed + block_scan_excl<WAVES>(ff, chunk);
        if (i < nbytes && o + 1 < SLOT) {
            slot[o] = (uint8_t)byte;
            if (ff) slot[o + 1] = 0;
        }
        stuffed += chunk;
    }
    if (tid == 0) ilen[f * n_int + it] = (uint32_t)min(nbytes + stuffed, SLOT);
}

// one workgroup per frame: where each interval (with the RST marker in front of all but the first) starts in the frame's file,
// and the file's length: header, intervals, markers, EOI
__global__ __launch_bounds__(THREADS) void jpeg_frame_scan_kernel(const uint32_t* __restrict__ ilen, int n_int, int header_bytes,
                                                                  unsigned long long* __restrict__ ioff,
                                                                  unsigned long long* __restrict__ flen) {
    const size_t f = blockIdx.x;
    unsigned long long at = (unsigned long long)header_bytes;
    for (int i0 = 0; i0 < n_int; i0 += THREADS) {
        const int i = i0 + (int)threadIdx.x;
        const unsigned long long mine = i < n_int ? (unsigned long long)ilen[f * n_int + i] + (i > 0 ? 2u : 0u) : 0ull;
        unsigned long long chunk;
        const unsigned long long o = block_scan_excl<WAVES>(mine, chunk);
        if (i < n_int) ioff[f * n_int + i] = at + o;
        at += chunk;
    }
    if (threadIdx.x == 0) flen[f] = at + 2;
}

// one workgroup: offsets[f] = where frame f starts in the stream, offsets[F] = *needed = the stream's length
__global__ __launch_bounds__(THREADS) void jpeg_offsets_kernel(const unsigned long long* __restrict__ flen, int F,
                                                               long long* __restrict__ offsets, long long* __restrict__ needed) {
    unsigned long long at = 0;
    for (int f0 = 0; f0 < F; f0 += THREADS) {
        const int f = f0 + (int)threadIdx.x;
        unsigned long long chunk;
        const unsigned long long o = block_scan_excl<WAVES>(f < F ? flen[f] : 0ull, chunk);
        if (f < F) offsets[f] = (long long)(at + o);
        at += chunk;
    }
    if (threadIdx.x == 0) {
        offsets[F] = (long long)at;
        *needed = (long long)at;
    }
}

// grid (intervals per frame, frames of this launch).  Writes nothing unless the whole stream fits.
__global__ __launch_bounds__(THREADS) void jpeg_copy_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ ilen,
                                                            const unsigned long long* __restrict__ ioff,
                                                            const long long* __restrict__ offsets, int F, int f0, int n_int,
                                                            const uint8_t* __restrict__ header, int header_bytes,
                                                            uint8_t* __restrict__ out, unsigned long long capacity) {
    if ((unsigned long long)offsets[F] > capacity) return;
    const size_t f = (size_t)f0 + blockIdx.y;
    const int it = blockIdx.x, tid = threadIdx.x;
    uint8_t* file = out + offsets[f];
    if (it == 0)
        for (int i = tid; i < header_bytes; i += THREADS) file[i] = header[i];
    const uint32_t n = ilen[f * n_int + it];
    uint8_t* dst = file + ioff[f * n_int + it];
    if (it > 0) {
        if (tid == 0) dst[0] = 0xff, dst[1] = (uint8_t)(0xd0 + ((it - 1) & 7));
        dst += 2;
    }
    const uint8_t* from = slots + (f * n_int + it) * SLOT;
    for (uint32_t i = tid; i < n; i += THREADS) dst[i] = from[i];
    if (it == n_int - 1 && tid == 0) dst[n] = 0xff, dst[n + 1] = 0xd9;
}

struct Layout {
    long long mw, mh, mcus, n_int;
    size_t coef, slots, ioff, flen, ilen, total;   // byte offsets into the workspace
};

bool sizes_ok(int F, int H, int W) { return F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }

Layout layout_of(int F, int H, int W) {
    Layout l;
    l.mw = (W + 15) / 16, l.mh = (H + 15) / 16, l.mcus = l.mw * l.mh, l.n_int = (l.mcus + R - 1) / R;
    l.coef = 0;
    l.slots = l.coef + (size_t)F * l.mcus * 6 * 64 * sizeof(int16_t);
    l.ioff = l.slots + (size_t)F * l.n_int * SLOT;
    l.flen = l.ioff + (size_t)F * l.n_int * 8;
    l.ilen = l.flen + (size_t)F * 8;
    l.total = (l.ilen + (size_t)F * l.n_int * 4 + 255) & ~(size_t)255;
    return l;
}

int transform(const uint8_t* frames, int F, int H, int W, const uint8_t* qtables, int16_t* coef, hipStream_t st) {
    const Layout l = layout_of(F, H, W);
    const int strips = dtk_cdiv(l.mw, STRIP);
    for (int f0 = 0; f0 < F; f0 += MAX_FRAMES_PER_LAUNCH) {
        const dim3 grid((unsigned)(strips * l.mh), (unsigned)std::min(F - f0, MAX_FRAMES_PER_LAUNCH));
        DTK_LAUNCH("jpeg_transform", jpeg_transform_kernel, grid, dim3(THREADS), 0, st, frames, f0, H, W, (int)l.mw, strips, qtables,
                   coef);
    }
    return 0;
}

}  // namespace

extern "C" size_t dtk_jpeg_workspace_bytes(int32_t F, int32_t H, int32_t W) {
    return sizes_ok(F, H, W) ? layout_of(F, H, W).total : 0;
}

extern "C" int dtk_jpeg_coefficients(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const uint8_t* qtables, int16_t* coef_out,
                                     void* stream) {
    DTK_REQUIRE(sizes_ok(F, H, W), "jpeg_coefficients: F >= 1 and 1 <= H, W <= 65535 are required, got F=%d %d x %d", F, H, W);
    DTK_REQUIRE(frames && qtables && coef_out, "jpeg_coefficients: null pointer (frames / qtables / coef_out)");
    return transform(frames, F, H, W, qtables, coef_out, dtk_stream(stream));
}

extern "C" int dtk_jpeg_encode(const uint8_t* frames, int32_t F, int32_t H, int32_t W, const uint8_t* qtables, const uint8_t* header,
                               int32_t header_bytes, uint8_t* out, size_t out_capacity, int64_t* offsets, int64_t* needed,
                               void* workspace, void* stream) {
    DTK_REQUIRE(sizes_ok(F, H, W), "jpeg_encode: F >= 1 and 1 <= H, W <= 65535 are required, got F=%d %d x %d", F, H, W);
    DTK_REQUIRE(frames && qtables && header && out && offsets && needed && workspace,
                "jpeg_encode: null pointer (frames / qtables / header / out / offsets / needed / workspace)");
    DTK_REQUIRE(header_bytes >= 1, "jpeg_encode: header_bytes must be positive, got %d", header_bytes);
    const Layout l = layout_of(F, H, W);
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + l.coef);
    uint8_t* slots = ws + l.slots;
    unsigned long long* ioff = reinterpret_cast<unsigned long long*>(ws + l.ioff);
    unsigned long long* flen = reinterpret_cast<unsigned long long*>(ws + l.flen);
    uint32_t* ilen = reinterpret_cast<uint32_t*>(ws + l.ilen);
    hipStream_t st = dtk_stream(stream);
    const int rc = transform(frames, F, H, W, qtables, coef, st);
    if (rc) return rc;
    const int n_int = (int)l.n_int;
    for (int f0 = 0; f0 < F; f0 += MAX_FRAMES_PER_LAUNCH) {
        const dim3 grid((unsigned)n_int, (unsigned)std::min(F - f0, MAX_FRAMES_PER_LAUNCH));
        DTK_LAUNCH("jpeg_code", jpeg_code_kernel, grid, dim3(THREADS), 0, st, coef, f0, (int)l.mcus, n_int, slots, ilen);
    }
    DTK_LAUNCH("jpeg_assemble", jpeg_frame_scan_kernel, dim3((unsigned)F), dim3(THREADS), 0, st, ilen, n_int, header_bytes, ioff, flen);
    DTK_LAUNCH("jpeg_assemble", jpeg_offsets_kernel, dim3(1), dim3(THREADS), 0, st, flen, F, reinterpret_cast<long long*>(offsets),
               reinterpret_cast<long long*>(needed));
    for (int f0 = 0; f0 < F; f0 += MAX_FRAMES_PER_LAUNCH) {
        const dim3 grid((unsigned)n_int, (unsigned)std::min(F - f0, MAX_FRAMES_PER_LAUNCH));
        DTK_LAUNCH("jpeg_assemble", jpeg_copy_kernel, grid, dim3(THREADS), 0, st, slots, ilen, ioff,
                   reinterpret_cast<const long long*>(offsets), F, f0, n_int, header, header_bytes, out,
                   (unsigned long long)out_capacity);
    }
    return 0;
}
