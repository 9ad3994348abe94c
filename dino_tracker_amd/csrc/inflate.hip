// inflate.hip -- PNG ingest: zlib / DEFLATE decoding, the Adler-32 check and the PNG row filters (docs/PNG_DECODE.md).  The file is
// parsed on the host (dino_tracker_amd/png_in.py); the device sees one contiguous zlib stream per frame.  Three kernels:
//
//   inflate_kernel      : a stream has no synchronisation points, so ONE WAVE per stream.  The stream-level logic is
//                         inflate_core.h's.  The decode chain -- bits -> table entry -> token -- is wave-uniform: every lane holds
//                         the same reader state (scalar registers), the tables and the staged input are read from LDS at one address.
//                         Input is staged through LDS in chunks by all lanes; before every element at least MARGIN bytes lie ahead
//                         of the reader (a dynamic block's header is at most 562 bytes, a token 6) unless the stream's end is staged.
//                         The last 32 KiB of output live in an LDS ring: literals go there, a match is copied there by the lanes in
//                         parallel (a distance shorter than the length replicates its period), back-references never touch global
//                         memory.  The ring is written out in aligned pieces by all lanes; what lies behind `flushed` is final.
//                         Dynamic blocks: one lane reads the header and sorts the symbols, all lanes fill the look-ups.
//   adler32_kernel      : a block per stream: s1 = 1 + sum d[i], s2 = N + sum (N - i) d[i], both mod 65521, from per-thread sums
//                         over 16-byte groups (adler32_core.h, shared with the encoder); compared with the stream's last four bytes.
//   png_unfilter_kernel : a wave per frame walks blocks of 64 rows as a skewed wavefront: lane k owns row r0 + k and handles pixel x
//                         at step x + k; its up bytes are what lane k - 1 made one step earlier (one cross-lane move of the packed
//                         pixel), its up-left bytes are its own previous up bytes.  Lane 63 leaves its row in the carry row of the
//                         workspace, from which lane 0 of the next block reads.
//
// Safety (docs/PNG_DECODE.md section 4): inflate_kernel reads only its stream's bytes (every staged byte's index is compared with
// the stream's length), writes only [0, expected) of its output range (literal, match and stored copies are refused beyond it
// BEFORE they are made), and every iteration of its loop consumes at least one bit or produces at least one byte, or ends it.
#include <algorithm>
#include <vector>
#include "common.h"
#include "adler32_core.h"
#include "inflate_core.h"

static_assert(INF_S_HEADER == DTK_INFLATE_S_HEADER && INF_S_BTYPE == DTK_INFLATE_S_BTYPE && INF_S_STORED == DTK_INFLATE_S_STORED &&
                  INF_S_TABLE == DTK_INFLATE_S_TABLE && INF_S_CODE == DTK_INFLATE_S_CODE && INF_S_DISTANCE == DTK_INFLATE_S_DISTANCE &&
                  INF_S_OVERRUN == DTK_INFLATE_S_OVERRUN && INF_S_LENGTH == DTK_INFLATE_S_LENGTH && INF_S_ADLER == DTK_INFLATE_S_ADLER &&
                  INF_S_STREAM == DTK_INFLATE_S_STREAM,
              "the status bits of inflate_core.h are dtk.h's");

namespace {

constexpr int IBUF = 4096;          // staged bytes of a stream
constexpr int ISTEP = 256;          // bytes all lanes stage at once: a word per lane
constexpr int MARGIN = 1024;        // bytes ahead of the reader before an element starts
constexpr int ISLACK = 16;          // zero bytes kept behind the staged data
constexpr int RING = INF_WINDOW;    // bytes of output history
constexpr int FLUSH = 8192;         // unflushed bytes that trigger a flush
constexpr int STORED_STEP = 2048;   // bytes of a stored block copied per iteration
constexpr int FIELDS = DTK_INFLATE_STREAM_FIELDS;
constexpr long long MAX_IN = 1ll << 28;    // bit positions are 32-bit
constexpr long long MAX_OUT = 1ll << 30;   // output positions are 32-bit
static_assert(IBUF % ISTEP == 0 && MARGIN + ISTEP + 4 <= IBUF, "a refill always stages at least one step");
static_assert(FLUSH + STORED_STEP + 258 <= RING, "what is not flushed is never overwritten");
static_assert((RING & (RING - 1)) == 0, "ring positions are masked");

struct InfShared {
    InfLitCode lit;
    InfDistCode dist;
    InfClenCode clen;
    uint32_t ibuf[(IBUF + ISLACK) / 4];
    uint8_t lens[INF_MAX_LENS];
    uint32_t ctl[4];   // one lane's results for the wave: status, bit position, hlit, hdist
    uint8_t ring[RING];
};
static_assert(sizeof(InfShared) <= 48 * 1024, "several streams share a CU");

// ring [from, to) -> out, by all lanes; dwords where out is aligned
__device__ __forceinline__ void flush_ring(const uint8_t* ring, uint8_t* __restrict__ out, uint32_t from, uint32_t to, int lane) {
    const uint32_t head = min((uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(out + from) & 3u)) & 3u), to - from);
    if ((uint32_t)lane < head) out[from + lane] = ring[(from + lane) & (RING - 1)];
    const uint32_t body = from + head, words = (to - body) / 4;
    for (uint32_t w = lane; w < words; w += WAVE) {
        const uint32_t p = body + 4 * w;
        const uint32_t v = (uint32_t)ring[p & (RING - 1)] | ((uint32_t)ring[(p + 1) & (RING - 1)] << 8) |
                           ((uint32_t)ring[(p + 2) & (RING - 1)] << 16) | ((uint32_t)ring[(p + 3) & (RING - 1)] << 24);
        *reinterpret_cast<uint32_t*>(out + p) = v;
    }
    const uint32_t tail = body + 4 * words;
    if (tail + lane < to) out[tail + lane] = ring[(tail + lane) & (RING - 1)];
}

// grid (streams), one wave each.  streams int64 [n][4]: byte offset in `in`, byte length, byte offset in `out`, expected bytes.
__global__ __launch_bounds__(WAVE) void inflate_kernel(const uint8_t* __restrict__ in, long long in_bytes,
                                                       const long long* __restrict__ streams, int wrapper,
                                                       uint8_t* __restrict__ out_all, long long out_bytes, int* __restrict__ status) {
    __shared__ InfShared sh;
    const int lane = threadIdx.x;
    const long long* sg = streams + (size_t)blockIdx.x * FIELDS;
    const long long off = sg[0], len = sg[1], ooff = sg[2], olen_ = sg[3];
    if (off < 0 || len < 0 || len > MAX_IN || off > in_bytes - len || ooff < 0 || olen_ < 0 || olen_ > MAX_OUT || ooff > out_bytes - olen_) {
        if (lane == 0) atomicOr(&status[blockIdx.x], INF_S_STREAM);
        return;
    }
    const uint8_t* src = in + off;
    uint8_t* out = out_all + ooff;
    const uint32_t olen = (uint32_t)olen_;
    uint8_t* ibytes = reinterpret_cast<uint8_t*>(sh.ibuf);

    long long raw_pos = 0;     // the next byte of the stream to stage
    long long base = 0;        // the stream position of ibuf[0]
    int fill = 0;              // staged bytes
    uint32_t opos = 0, flushed = 0;
    int st = 0;
    InfBits bits;
    inf_bits_start(bits, sh.ibuf, 0u, 0u, 0u);

    enum { M_ZLIB, M_BLOCK, M_STORED, M_TOKENS, M_TRAILER, M_DONE };
    int mode = wrapper ? M_ZLIB : M_BLOCK;
    bool last = false;
    uint32_t stored_left = 0;

    while (mode != M_DONE) {
        // ---- housekeeping: input ahead of the reader, room in the ring ------------------------------------------------------
        if (raw_pos < len && (long long)fill * 8 - (long long)bits.pos < MARGIN * 8) {
            const int keep0 = min((int)(bits.pos >> 5), fill / 4), nw = (fill + 3) / 4 - keep0;   // whole words stay
            __syncthreads();
            for (int i = 0; i < nw; i += WAVE) {
                const uint32_t v = i + lane < nw ? sh.ibuf[keep0 + i + lane] : 0u;
                __syncthreads();
                if (i + lane < nw) sh.ibuf[i + lane] = v;
                __syncthreads();
            }
            fill -= 4 * keep0;
            base += 4 * keep0;
            const uint32_t pos = bits.pos - 32u * (uint32_t)keep0;
            while (raw_pos < len && fill + ISTEP <= IBUF) {   // fill is a multiple of 4 until the stream's end is staged
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long i = raw_pos + 4 * lane + k;
                    if (i < len) v |= (uint32_t)src[i] << (8 * k);
                }
                sh.ibuf[fill / 4 + lane] = v;
                const int got = (int)min((long long)ISTEP, len - raw_pos);
                fill += got;
                raw_pos += got;
            }
            if (lane < ISLACK / 4) sh.ibuf[(fill + 3) / 4 + lane] = 0u;
            __syncthreads();
            inf_bits_start(bits, sh.ibuf, (uint32_t)(fill + 3) / 4u + 1u, (uint32_t)fill * 8u, pos);
        }
        if (opos - flushed >= FLUSH) {
            // up to the last position at which `out` is dword-aligned: the next flush starts aligned
            const uint32_t to = opos - (uint32_t)(reinterpret_cast<uintptr_t>(out + opos) & 3u);
            __syncthreads();
            flush_ring(sh.ring, out, flushed, to, lane);
            flushed = to;
        }

        if (mode == M_ZLIB) {
            st = inf_zlib_header(bits);
            mode = st ? M_DONE : M_BLOCK;
        } else if (mode == M_BLOCK) {
            last = inf_take(bits, 1) != 0u;
            const uint32_t type = inf_take(bits, 2);
            if (inf_over(bits)) st = INF_S_OVERRUN;
            else if (type == 3u) st = INF_S_BTYPE;
            else if (type == 0u) {
                inf_consume(bits, (int)((8u - (bits.pos & 7u)) & 7u));
                const uint32_t n = inf_take(bits, 16), nn = inf_take(bits, 16);
                if (inf_over(bits)) st = INF_S_OVERRUN;
                else if ((n ^ nn) != 0xffffu) st = INF_S_STORED;
                else if (n > olen - opos) st = INF_S_LENGTH;
                stored_left = n;
                mode = M_STORED;
            } else {
                int hlit = 288, hdist = 32;
                __syncthreads();
                if (type == 1u) {
                    inf_fixed_lens(sh.lens, lane, WAVE);
                } else {
                    if (lane == 0) {
                        InfBits mine = bits;
                        int a = 0, b = 0;
                        sh.ctl[0] = (uint32_t)inf_read_dynamic(mine, &sh.clen, sh.lens, a, b);
                        sh.ctl[1] = mine.pos, sh.ctl[2] = (uint32_t)a, sh.ctl[3] = (uint32_t)b;
                    }
                    __syncthreads();
                    st = (int)INF_UNIFORM(sh.ctl[0]);
                    hlit = min((int)INF_UNIFORM(sh.ctl[2]), 288), hdist = min((int)INF_UNIFORM(sh.ctl[3]), 32);
                    inf_bits_start(bits, sh.ibuf, bits.limit, bits.avail_bits, INF_UNIFORM(sh.ctl[1]));
                }
                if (!st) {
                    inf_code_clear(&sh.lit, lane, WAVE);
                    inf_code_clear(&sh.dist, lane, WAVE);
                    __syncthreads();
                    if (lane == 0) {
                        inf_code_sort(sh.lens, hlit, INF_KIND_LITLEN, &sh.lit);
                        inf_code_sort(sh.lens + hlit, hdist, INF_KIND_DIST, &sh.dist);
                    }
                    __syncthreads();
                    st = (int)(INF_UNIFORM(sh.lit.status) | INF_UNIFORM(sh.dist.status));
                    inf_code_fill(sh.lens, &sh.lit, lane, WAVE);
                    inf_code_fill(sh.lens + hlit, &sh.dist, lane, WAVE);
                    __syncthreads();
                }
                mode = M_TOKENS;
            }
            if (st) mode = M_DONE;
        } else if (mode == M_STORED) {
            if (stored_left == 0u) {
                mode = last ? M_TRAILER : M_BLOCK;
            } else {
                // the reader is byte-aligned here; what is staged beyond it is copied, at most STORED_STEP bytes at a time
                const uint32_t at = bits.pos >> 3, have = (uint32_t)fill > at ? (uint32_t)fill - at : 0u;
                const uint32_t n = min(min(stored_left, have), (uint32_t)STORED_STEP);   // <= olen - opos: checked at the header
                if (n == 0u) {
                    st = INF_S_OVERRUN;   // nothing staged beyond the reader means the stream's end is staged (MARGIN)
                    mode = M_DONE;
                } else {
                    for (uint32_t i = lane; i < n; i += WAVE) sh.ring[(opos + i) & (RING - 1)] = ibytes[at + i];
                    __syncthreads();
                    opos += n;
                    stored_left -= n;
                    inf_bits_start(bits, sh.ibuf, bits.limit, bits.avail_bits, bits.pos + 8u * n);
                }
            }
        } else if (mode == M_TOKENS) {
            // tokens until the block ends, a fault, or housekeeping is due
            while (true) {
                int mlen = 0, mdist = 0;
                const int t = inf_token(bits, sh.lit, sh.dist, mlen, mdist, st);
                if (t >= 0) {
                    if (opos >= olen) {
                        st = INF_S_LENGTH;
                        mode = M_DONE;
                        break;
                    }
                    sh.ring[opos & (RING - 1)] = (uint8_t)t;   // every lane stores it: each lane later reads what it wrote itself
                    ++opos;
                } else if (t == INF_TOKEN_MATCH) {
                    if ((uint32_t)mdist > opos) st = INF_S_DISTANCE;
                    else if ((uint32_t)mlen > olen - opos) st = INF_S_LENGTH;
                    if (st) {
                        mode = M_DONE;
                        break;
                    }
                    const uint32_t from = opos - (uint32_t)mdist;
                    if (mdist == 1) {
                        const uint8_t v = sh.ring[from & (RING - 1)];
                        for (int i = lane; i < mlen; i += WAVE) sh.ring[(opos + i) & (RING - 1)] = v;
                    } else if (mdist >= mlen) {
                        for (int i = lane; i < mlen; i += WAVE) sh.ring[(opos + i) & (RING - 1)] = sh.ring[(from + i) & (RING - 1)];
                    } else {
                        for (int i = lane; i < mlen; i += WAVE)
                            sh.ring[(opos + i) & (RING - 1)] = sh.ring[(from + (uint32_t)(i % mdist)) & (RING - 1)];
                    }
                    __syncthreads();   // later tokens read these bytes from other lanes' stores
                    opos += (uint32_t)mlen;
                } else if (t == INF_TOKEN_EOB) {
                    mode = last ? M_TRAILER : M_BLOCK;
                    break;
                } else {
                    mode = M_DONE;
                    break;
                }
                if ((raw_pos < len && (long long)fill * 8 - (long long)bits.pos < MARGIN * 8) || opos - flushed >= FLUSH) break;
            }
        } else {   // M_TRAILER: the final block has ended
            if (opos != olen) st = INF_S_LENGTH;
            else if (wrapper && len - (base + (long long)((bits.pos + 7u) >> 3)) < 4) st = INF_S_OVERRUN;
            mode = M_DONE;
        }
    }
    // what was decoded, then zeros up to the expected size
    __syncthreads();
    flush_ring(sh.ring, out, flushed, opos, lane);
    for (uint32_t i = opos + lane; i < olen; i += WAVE) out[i] = 0;
    if (lane == 0 && st) atomicOr(&status[blockIdx.x], st);
}

// ---- Adler-32 ------------------------------------------------------------------------------------------------------------------
// grid (streams).  A stream whose status is already set is left alone: its output is not what the trailer describes.
__global__ __launch_bounds__(ATHREADS) void adler32_kernel(const uint8_t* __restrict__ in, long long in_bytes,
                                                           const long long* __restrict__ streams, const uint8_t* __restrict__ out_all,
                                                           long long out_bytes, int* __restrict__ status) {
    const int tid = threadIdx.x;
    const long long* sg = streams + (size_t)blockIdx.x * FIELDS;
    const long long off = sg[0], len = sg[1], ooff = sg[2], N = sg[3];
    if (off < 0 || len < 0 || len > MAX_IN || off > in_bytes - len || ooff < 0 || N < 0 || N > MAX_OUT || ooff > out_bytes - N) {
        if (tid == 0) atomicOr(&status[blockIdx.x], INF_S_STREAM);
        return;
    }
    if (status[blockIdx.x] != 0) return;
    if (len < 4) {
        if (tid == 0) atomicOr(&status[blockIdx.x], INF_S_OVERRUN);
        return;
    }
    const unsigned value = adler32_block(out_all + ooff, N);   // adler32_core.h: thread 0 holds it
    if (tid == 0) {
        const uint8_t* tr = in + off + len - 4;
        const unsigned want = ((unsigned)tr[0] << 24) | ((unsigned)tr[1] << 16) | ((unsigned)tr[2] << 8) | tr[3];
        if (value != want) atomicOr(&status[blockIdx.x], INF_S_ADLER);
    }
}

// ---- PNG row filters -----------------------------------------------------------------------------------------------------------
// grid (frames), one wave each.  raw [F][H][1 + W bpp], out [F][H][W][bpp], carry [F][W] packed pixels (workspace).
template <int BPP>
__global__ __launch_bounds__(WAVE) void png_unfilter_kernel(const uint8_t* __restrict__ raw_all, int H, int W,
                                                            const uint8_t* __restrict__ lut_all, uint8_t* __restrict__ out_all,
                                                            uint32_t* __restrict__ carry_all, int* __restrict__ status) {
    const int lane = threadIdx.x;
    const size_t f = blockIdx.x, pitch = 1 + (size_t)W * BPP;
    const uint8_t* raw_f = raw_all + f * (size_t)H * pitch;
    uint8_t* out_f = out_all + f * (size_t)H * W * BPP;
    uint32_t* carry = carry_all + f * (size_t)W;
    const uint8_t* lut = lut_all ? lut_all + f * 256 : nullptr;
    bool bad = false;
    for (int r0 = 0; r0 < H; r0 += WAVE) {
        const int row = r0 + lane;
        const bool mine = row < H;
        const uint8_t* rr = raw_f + (size_t)(mine ? row : 0) * pitch;
        uint8_t* orow = out_f + (size_t)(mine ? row : 0) * W * BPP;
        int filter = mine ? rr[0] : 0;
        if (filter > 4) bad = true, filter = 0;
        uint32_t cur = 0, up = 0, left = 0;   // packed pixels: this lane's last result, the row above at x - 1, this row at x - 1
        uint32_t next_raw = 0;
        if (mine) {
#pragma unroll
            for (int c = 0; c < BPP; ++c) next_raw |= (uint32_t)rr[1 + c] << (8 * c);
        }
        for (int s = 0; s < W + WAVE - 1; ++s) {
            const int x = s - lane;
            const bool act = mine && x >= 0 && x < W;
            // the row above at x: lane k - 1's result of the step before; lane 0 reads the carry row (zeros above the image)
            uint32_t above = (uint32_t)__shfl_up((int)cur, 1);
            if (lane == 0) above = (r0 > 0 && act) ? carry[x] : 0u;
            const uint32_t upleft = x > 0 ? up : 0u, a = x > 0 ? left : 0u;
            const uint32_t rawpx = next_raw;
            if (mine && x + 1 >= 0 && x + 1 < W) {   // the next step's bytes, requested before this step's arithmetic
                next_raw = 0;
#pragma unroll
                for (int c = 0; c < BPP; ++c) next_raw |= (uint32_t)rr[1 + (size_t)(x + 1) * BPP + c] << (8 * c);
            }
            if (act) {
                uint32_t px = 0;
#pragma unroll
                for (int c = 0; c < BPP; ++c) {
                    const int v = inf_unfilter_byte(filter, (rawpx >> (8 * c)) & 255, (a >> (8 * c)) & 255, (above >> (8 * c)) & 255,
                                                    (upleft >> (8 * c)) & 255);
                    px |= (uint32_t)v << (8 * c);
                    orow[(size_t)x * BPP + c] = (BPP == 1 && lut) ? lut[v] : (uint8_t)v;
                }
                cur = px;
                left = px;
                up = above;
                if (lane == WAVE - 1) carry[x] = px;
            }
        }
        // lane 63's carry row is read by lane 0 of the next block
        __threadfence();
        __syncthreads();
    }
    if (__any(bad) && lane == 0) atomicOr(&status[f], DTK_PNG_S_FILTER);
}

bool png_sizes_ok(int F, int H, int W, int bpp) { return F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (bpp == 1 || bpp == 3); }

// the host copy of a stream table: every entry inside the buffers, output ranges disjoint
int check_streams(const char* who, const int64_t* t, int n, int64_t in_bytes, int64_t out_bytes) {
    std::vector<std::pair<int64_t, int64_t>> ranges;
    for (int s = 0; s < n; ++s) {
        const int64_t* g = t + (size_t)s * FIELDS;
        DTK_REQUIRE(g[0] >= 0 && g[1] >= 0 && g[1] <= MAX_IN && g[0] <= in_bytes - g[1] && g[2] >= 0 && g[3] >= 0 && g[3] <= MAX_OUT &&
                        g[2] <= out_bytes - g[3],
                    "%s: stream %d (input %lld + %lld, output %lld + %lld) does not fit %lld input and %lld output bytes", who, s,
                    (long long)g[0], (long long)g[1], (long long)g[2], (long long)g[3], (long long)in_bytes, (long long)out_bytes);
        if (g[3] > 0) ranges.emplace_back(g[2], g[2] + g[3]);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i)
        DTK_REQUIRE(ranges[i].first >= ranges[i - 1].second, "%s: output ranges overlap at byte %lld", who, (long long)ranges[i].first);
    return 0;
}

}  // namespace

extern "C" int dtk_inflate(const uint8_t* in, int64_t in_bytes, const int64_t* streams, const int64_t* streams_host, int32_t n_streams,
                           int32_t wrapper, uint8_t* out, int64_t out_bytes, int32_t* status, void* stream) {
    DTK_REQUIRE(in && streams && streams_host && out && status, "inflate: null pointer (in / streams / streams_host / out / status)");
    DTK_REQUIRE(in_bytes >= 1 && out_bytes >= 1 && n_streams >= 1, "inflate: in_bytes, out_bytes and n_streams must be positive, got %lld, %lld, %d",
                (long long)in_bytes, (long long)out_bytes, n_streams);
    DTK_REQUIRE(wrapper == 0 || wrapper == 1, "inflate: wrapper must be 0 (raw) or 1 (zlib), got %d", wrapper);
    if (int rc = check_streams("inflate", streams_host, n_streams, in_bytes, out_bytes)) return rc;
    hipStream_t st = dtk_stream(stream);
    DTK_HIP(dtk_zero_async(status, (size_t)n_streams * 4, st));
    DTK_LAUNCH("inflate", inflate_kernel, dim3((unsigned)n_streams), dim3(WAVE), 0, st, in, (long long)in_bytes,
               reinterpret_cast<const long long*>(streams), (int)wrapper, out, (long long)out_bytes, status);
    return 0;
}

extern "C" int dtk_adler32(const uint8_t* in, int64_t in_bytes, const int64_t* streams, const int64_t* streams_host, int32_t n_streams,
                           const uint8_t* out, int64_t out_bytes, int32_t* status, void* stream) {
    DTK_REQUIRE(in && streams && streams_host && out && status, "adler32: null pointer (in / streams / streams_host / out / status)");
    DTK_REQUIRE(in_bytes >= 1 && out_bytes >= 1 && n_streams >= 1, "adler32: in_bytes, out_bytes and n_streams must be positive, got %lld, %lld, %d",
                (long long)in_bytes, (long long)out_bytes, n_streams);
    if (int rc = check_streams("adler32", streams_host, n_streams, in_bytes, out_bytes)) return rc;
    hipStream_t st = dtk_stream(stream);
    DTK_LAUNCH("adler32", adler32_kernel, dim3((unsigned)n_streams), dim3(ATHREADS), 0, st, in, (long long)in_bytes,
               reinterpret_cast<const long long*>(streams), out, (long long)out_bytes, status);
    return 0;
}

extern "C" size_t dtk_png_unfilter_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t bpp) {
    return png_sizes_ok(F, H, W, bpp) ? (((size_t)F * W * 4 + 255) & ~(size_t)255) : 0;
}

extern "C" int dtk_png_unfilter(const uint8_t* raw, int32_t F, int32_t H, int32_t W, int32_t bpp, const uint8_t* lut, uint8_t* out,
                                int32_t* status, void* workspace, void* stream) {
    DTK_REQUIRE(png_sizes_ok(F, H, W, bpp), "png_unfilter: F >= 1, 1 <= H, W <= 65535 and bpp 1 or 3 are required, got F=%d %d x %d bpp=%d",
                F, H, W, bpp);
    DTK_REQUIRE(raw && out && status && workspace, "png_unfilter: null pointer (raw / out / status / workspace)");
    DTK_REQUIRE(!lut || bpp == 1, "png_unfilter: a palette table applies to bpp = 1 only");
    hipStream_t st = dtk_stream(stream);
    uint32_t* carry = reinterpret_cast<uint32_t*>(workspace);
    if (bpp == 1)
        DTK_LAUNCH("png_unfilter", png_unfilter_kernel<1>, dim3((unsigned)F), dim3(WAVE), 0, st, raw, (int)H, (int)W, lut, out, carry, status);
    else
        DTK_LAUNCH("png_unfilter", png_unfilter_kernel<3>, dim3((unsigned)F), dim3(WAVE), 0, st, raw, (int)H, (int)W, lut, out, carry, status);
    return 0;
}
