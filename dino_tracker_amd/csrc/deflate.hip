// deflate.hip -- PNG output: the PNG row filters, DEFLATE / zlib compression, the CRC-32 and the assembly of whole files
// (docs/PNG_ENCODE.md).  The mirror of inflate.hip.  Kernels:
//
//   png_filter_kernel      : a block per row.  Encoding filters read ORIGINAL pixels, so every byte is independent; the adaptive rule
//                            sums |filtered byte as int8| for the five filters over the row (block sums) and takes the smallest.
//   deflate_segment_kernel : ONE WAVE per segment of DTK_DEFLATE_SEGMENT bytes, which it holds in LDS.  No reference crosses a
//                            segment, so the segments of all streams compress in parallel.  The wave walks the segment in TILES of 64
//                            positions: every lane looks for a match at its own position (distance 1, a near and a far distance the
//                            caller names -- a pixel and a row of a PNG --, and the newest earlier position with the same 3-byte hash),
//                            then the wave resolves the greedy parse of the tile from the lanes' results, then the tile's positions enter
//                            the hash table by atomicMax.  A position only ever sees positions of EARLIER tiles in the table and the
//                            table's state after a tile does not depend on the order of the lanes' updates, so the bytes are a pure
//                            function of the input.  Tokens go to the workspace, their histograms to LDS.  Then the block type is
//                            chosen from exact costs (stored / fixed / dynamic; the dynamic code is built in LDS, lengths limited to
//                            15 and 7), and the tokens are coded 64 at a time through a small LDS bit buffer into the segment's slot.
//   block_offsets_kernel   : block_scan.h's: where each segment starts in its stream.
//   stream_offsets_kernel  : the int64 scan over the streams: offsets and *needed.
//   deflate_copy_kernel    : slots -> out, with the zlib header; nothing unless the whole output fits.
//   adler32_store_kernel   : adler32_core.h's block sums over the stream's INPUT, written where adler32_kernel compares it.
//   crc32_kernel           : table-driven CRC-32 over pieces of 64 bytes, a block per 16 KiB; the pieces are combined by
//                            multiplication with x^(8 len) mod P and XORed into the range's word (order-independent).
//   png_frame_kernel / png_crc_store_kernel : signature + IHDR, the IDAT framing, IEND.
//
// Safety: every kernel re-checks its table entry against the buffer sizes; a segment's coded form is only chosen when its exact size
// is below the stored form's, which is what a slot holds, and every slot write is clamped to the slot besides.
#include <algorithm>
#include "common.h"
#include "block_scan.h"
#include "adler32_core.h"

namespace {

constexpr int SEG = DTK_DEFLATE_SEGMENT;
constexpr int SLOT = SEG + 64;               // bytes of a segment's slot: the stored form is 5 + SEG
constexpr int HASH_BITS = 12;
constexpr int CAP = 32;                      // bytes a lane compares per candidate; the wave extends the chosen match to 258
constexpr int MAXLEN = 258, MINLEN = 3;
constexpr int TOO_FAR = 4096;                // a match of three bytes further back costs more than its literals
constexpr int NLIT = 286, NDIST = 30, NCLEN = 19, NSYM = NLIT + NDIST;
constexpr int EOB = 256;
constexpr int STAGE_WORDS = 104;             // 7 pending bits + 64 tokens of at most 48 bits, and two words of spill
constexpr int HDR_ITEMS = 4 + NCLEN + NSYM + 1;
constexpr long long MAX_STREAM = 1ll << 30;  // bytes of one stream: segment counts and per-stream sums stay 32-bit
constexpr int MAX_PER_LAUNCH = 65535;        // grid.y
constexpr int FIELDS = DTK_DEFLATE_RANGE_FIELDS;
constexpr int CT = 256;                      // threads of the copy / filter / CRC kernels
constexpr int CW = CT / WAVE;
static_assert(SEG % WAVE == 0 && SEG <= 32768, "distances are at most 32768 and tiles are whole");

__constant__ uint8_t CLEN_ORDER[NCLEN] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- 1. the row filters ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth_predictor(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filter_byte(int t, int x, int a, int b, int c) {
    const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? ((a + b) >> 1) : paeth_predictor(a, b, c);
    return (x - pred) & 255;
}

// grid (rows, frames of this launch).  frames [F][H][W][BPP] -> raw [F][H][1 + W BPP].
template <int BPP>
__global__ __launch_bounds__(CT) void png_filter_kernel(const uint8_t* __restrict__ frames, int f0, int H, int W, int filter,
                                                        uint8_t* __restrict__ raw) {
    const int tid = threadIdx.x, row = blockIdx.x, nb = W * BPP;
    const size_t r = ((size_t)f0 + blockIdx.y) * H + row;
    const uint8_t* cur = frames + r * nb;
    const uint8_t* up = cur - nb;
    const bool has_up = row > 0;
    uint8_t* dst = raw + r * ((size_t)nb + 1);
    int chosen = filter;
    if (filter == 5) {
        int s[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < nb; i += CT) {
            const int x = cur[i], a = i >= BPP ? cur[i - BPP] : 0, b = has_up ? up[i] : 0, c = (has_up && i >= BPP) ? up[i - BPP] : 0;
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                const int v = filter_byte(t, x, a, b, c);
                s[t] += v < 128 ? v : 256 - v;
            }
        }
        int best = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const int total = block_sum_i<CW>(s[t]);
            if (total < best) best = total, chosen = t;   // ties: the lowest filter number
        }
    }
    if (tid == 0) dst[0] = (uint8_t)chosen;
    for (int i = tid; i < nb; i += CT) {
        const int x = cur[i], a = i >= BPP ? cur[i - BPP] : 0, b = has_up ? up[i] : 0, c = (has_up && i >= BPP) ? up[i - BPP] : 0;
        dst[1 + i] = (uint8_t)filter_byte(chosen, x, a, b, c);
    }
}

// ---- 2. DEFLATE ------------------------------------------------------------------------------------------------------------------
// scratch of the code construction; it shares its LDS with the hash table, which is dead by then
struct Builder {
    uint32_t weight[2 * NLIT];
    uint16_t parent[2 * NLIT];
    uint16_t depth[2 * NLIT];
    uint16_t sorted[NLIT];
    uint16_t items[NSYM];        // the run-length coded code lengths: symbol | extra << 8
    uint32_t hdr[HDR_ITEMS];     // a dynamic block's header as (bits | count << 24)
    int n_items, n_hdr, ok;
};

struct DefShared {
    uint32_t in[(SEG + 16) / 4];
    union {
        int hash[1 << HASH_BITS];
        Builder b;
    } u;
    uint32_t freq[NSYM];         // literal/length symbols, then distance symbols
    uint32_t cfreq[NCLEN];
    uint16_t code[NSYM];         // bit-reversed: the stream takes Huffman codes from their most significant bit
    uint8_t len[NSYM];
    uint16_t ccode[NCLEN];
    uint8_t clen[NCLEN];
    uint32_t stage[STAGE_WORDS];
};
static_assert(sizeof(DefShared) <= 53 * 1024, "three segments share a CU's 160 KiB");

__device__ __forceinline__ int lit_extra(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }
__device__ __forceinline__ int dist_extra(int s) { return s < 4 ? 0 : (s >> 1) - 1; }
// length 3 .. 258 -> symbol, extra bit count and value
__device__ __forceinline__ void length_symbol(int length, int& sym, int& eb, int& ev) {
    const int l = length - 3;
    if (length == 258) sym = 285, eb = 0, ev = 0;
    else if (l < 8) sym = 257 + l, eb = 0, ev = 0;
    else {
        eb = (31 - __clz(l)) - 2;
        sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3);
        ev = l & ((1 << eb) - 1);
    }
}
// distance 1 .. 32768 -> symbol, extra bit count and value
__device__ __forceinline__ void distance_symbol(int dist, int& sym, int& eb, int& ev) {
    const int d = dist - 1;
    if (d < 4) sym = d, eb = 0, ev = 0;
    else {
        eb = (31 - __clz(d)) - 1;
        sym = 2 * (eb + 1) + ((d >> eb) & 1);
        ev = d & ((1 << eb) - 1);
    }
}
__device__ __forceinline__ int fixed_lit_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// Code lengths of at most L bits for freq[0 .. n) into lens[0 .. n); every lane calls.  A Huffman tree over the used symbols (sorted
// by rank, merged by the two-queue method), depths clamped to L, then the Kraft sum is brought back to exactly 1: while it is
// above, the deepest symbol below L (the rarest of them) grows by a bit; while it is below, the deepest symbol whose step still fits
// (the most frequent of them) shrinks by one.  `single`: a code of one symbol (or none: then symbol 0) is that symbol at length 1 -- the
// distance code; otherwise symbols 0 and 1 are counted once where fewer than two are used, so that the code is complete.
// Returns false when the sum could not be restored (the caller then does without a dynamic block).
__device__ bool build_lengths(const uint32_t* freq, int n, int L, uint8_t* lens, bool single, Builder& b) {
    const int lane = threadIdx.x;
    __syncthreads();
    int used = 0;
    for (int i = lane; i < n; i += WAVE) {
        used += freq[i] != 0u;
        lens[i] = 0;
    }
    used = wave_sum_i(used);
    __syncthreads();
    if (single && used <= 1) {
        for (int i = lane; i < n; i += WAVE)
            if (freq[i] != 0u || (used == 0 && i == 0)) lens[i] = 1;
        __syncthreads();
        return true;
    }
    const bool force = used < 2;
    auto eff = [&](int i) -> uint32_t { return freq[i] ? freq[i] : ((force && i < 2) ? 1u : 0u); };
    int m = 0;
    for (int i = lane; i < n; i += WAVE) m += eff(i) != 0u;
    m = wave_sum_i(m);
    for (int i = lane; i < n; i += WAVE) {
        const uint32_t fi = eff(i);
        if (!fi) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint32_t fj = eff(j);
            rank += fj != 0u && (fj < fi || (fj == fi && j < i));
        }
        b.sorted[rank] = (uint16_t)i;
        b.weight[rank] = fi;
    }
    __syncthreads();
    if (lane == 0) {
        int leaf = 0, node = m;
        for (int next = m; next < 2 * m - 1; ++next) {
            uint32_t w = 0;
            for (int t = 0; t < 2; ++t) {
                const int x = (leaf < m && (node >= next || b.weight[leaf] <= b.weight[node])) ? leaf++ : node++;
                b.parent[x] = (uint16_t)next;
                w += b.weight[x];
            }
            b.weight[next] = w;
        }
        b.depth[2 * m - 2] = 0;
        for (int k = 2 * m - 3; k >= m; --k) b.depth[k] = b.depth[b.parent[k]] + 1;
    }
    __syncthreads();
    for (int k = lane; k < m; k += WAVE) lens[b.sorted[k]] = (uint8_t)min((int)b.depth[b.parent[k]] + 1, L);
    __syncthreads();
    if (lane == 0) {
        const long long T = 1ll << L;
        long long K = 0;
        for (int k = 0; k < m; ++k) K += 1ll << (L - lens[b.sorted[k]]);
        bool ok = true;
        while (K > T && ok) {
            int best = -1, blen = 0;
            for (int k = 0; k < m; ++k) {
                const int l = lens[b.sorted[k]];
                if (l < L && l > blen) blen = l, best = b.sorted[k];
            }
            if (best < 0) ok = false;
            else K -= 1ll << (L - ++lens[best]);
        }
        while (K < T && ok) {
            int best = -1, blen = 0;
            for (int k = m - 1; k >= 0; --k) {
                const int l = lens[b.sorted[k]];
                if (l > 1 && l > blen && (1ll << (L - l)) <= T - K) blen = l, best = b.sorted[k];
            }
            if (best < 0) ok = false;
            else K += 1ll << (L - lens[best]--);
        }
        b.ok = ok && K == T;
    }
    __syncthreads();
    return b.ok != 0;
}

// canonical codes of lens[0 .. n), bit-reversed; lane 0 works, every lane calls
__device__ void assign_codes(const uint8_t* lens, int n, uint16_t* code) {
    __syncthreads();
    if (threadIdx.x == 0) {
        int count[16], next[16];
        for (int l = 0; l < 16; ++l) count[l] = 0;
        for (int i = 0; i < n; ++i) ++count[lens[i]];
        count[0] = 0;
        int c = 0;
        for (int l = 1; l < 16; ++l) {
            c = (c + count[l - 1]) << 1;
            next[l] = c;
        }
        for (int i = 0; i < n; ++i) {
            const int l = lens[i];
            code[i] = l ? (uint16_t)(__brev((unsigned)next[l]++) >> (32 - l)) : 0;
        }
    }
    __syncthreads();
}

// 64 (bits, count) pairs, lane order, into the slot: the LDS stage collects them behind the pending bits, whole bytes leave
struct Emitter {
    uint8_t* out;
    int pos, pend;
};
__device__ void emit_round(DefShared& sh, Emitter& e, unsigned long long bits, int n) {
    const int lane = threadIdx.x;
    const int incl = wave_scan_incl(n);
    const int total = e.pend + __shfl(incl, WAVE - 1);
    if (n) {
        const int off = e.pend + incl - n, w = off >> 5, s = off & 31;
        atomicOr(&sh.stage[w], (uint32_t)(bits << s));
        const unsigned long long rest = s ? bits >> (32 - s) : bits >> 32;
        if ((uint32_t)rest) atomicOr(&sh.stage[w + 1], (uint32_t)rest);
        if (rest >> 32) atomicOr(&sh.stage[w + 2], (uint32_t)(rest >> 32));
    }
    __syncthreads();
    const int nbytes = total >> 3;
    for (int i = lane; i < nbytes; i += WAVE)
        if (e.pos + i < SLOT) e.out[e.pos + i] = (uint8_t)(sh.stage[i >> 2] >> (8 * (i & 3)));
    const uint32_t carry = (total & 7) ? (sh.stage[nbytes >> 2] >> (8 * (nbytes & 3))) & 255u : 0u;
    __syncthreads();
    for (int i = lane; i <= (total >> 5) + 2 && i < STAGE_WORDS; i += WAVE) sh.stage[i] = i == 0 ? carry : 0u;
    __syncthreads();
    e.pos += nbytes;
    e.pend = total & 7;
}

// grid (segments per stream, streams of this launch), one wave each.  ranges int64 [n][2]: byte offset in `in`, byte length.
// slots [n][max_segs][SLOT], tokens uint32 [n][max_segs][SEG], seg_len / seg_off int32 [n][max_segs] (both receive the length).
__global__ __launch_bounds__(WAVE) void deflate_segment_kernel(const uint8_t* __restrict__ in, long long in_bytes,
                                                               const long long* __restrict__ ranges, int s0, int max_segs, int near_d,
                                                               int far_d, uint8_t* __restrict__ slots, uint32_t* __restrict__ tokens,
                                                               int32_t* __restrict__ seg_len, int32_t* __restrict__ seg_off) {
    __shared__ DefShared sh;
    const int lane = threadIdx.x;
    const size_t s = (size_t)s0 + blockIdx.y;
    const int seg = blockIdx.x;
    const size_t g = s * max_segs + seg;
    long long off = ranges[s * FIELDS], len = ranges[s * FIELDS + 1];
    if (off < 0 || len < 0 || len > MAX_STREAM || off > in_bytes - len) off = 0, len = 0;   // refused on the host; an empty stream here
    const int nseg = len ? (int)((len + SEG - 1) / SEG) : 1;
    if (seg >= nseg) {
        if (lane == 0) seg_len[g] = 0, seg_off[g] = 0;
        return;
    }
    const int n = (int)min((long long)SEG, len - (long long)seg * SEG);
    const bool last = seg == nseg - 1;
    const uint8_t* src = in + off + (long long)seg * SEG;
    uint8_t* slot = slots + g * SLOT;
    uint32_t* tok = tokens + g * SEG;
    const uint8_t* ib = reinterpret_cast<const uint8_t*>(sh.in);

    for (int w = lane; w < (n + 16) / 4 + 1 && w < (SEG + 16) / 4; w += WAVE) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * w + k < n) v |= (uint32_t)src[4 * w + k] << (8 * k);
        sh.in[w] = v;
    }
    for (int i = lane; i < (1 << HASH_BITS); i += WAVE) sh.u.hash[i] = -1;
    for (int i = lane; i < NSYM; i += WAVE) sh.freq[i] = i == EOB ? 1u : 0u;
    for (int i = lane; i < NCLEN; i += WAVE) sh.cfreq[i] = 0u;
    for (int i = lane; i < STAGE_WORDS; i += WAVE) sh.stage[i] = 0u;
    __syncthreads();

    // ---- the parse: tiles of 64 positions ------------------------------------------------------------------------------------------
    int cover = 0, ntok = 0;   // the first position no token covers yet; tokens so far
    for (int t0 = 0; t0 < n; t0 += WAVE) {
        const int p = t0 + lane, tl = min(WAVE, n - t0);
        const bool hashed = p + MINLEN <= n;
        uint32_t h = 0;
        if (hashed) h = (((uint32_t)ib[p] | ((uint32_t)ib[p + 1] << 8) | ((uint32_t)ib[p + 2] << 16)) * 0x9E3779B1u) >> (32 - HASH_BITS);
        if (cover < t0 + tl) {
            int mlen = 0, mdist = 0;
            if (hashed && p >= cover) {
                const int maxl = min(MAXLEN, n - p), lim = min(CAP, maxl);
                const int cand[4] = {1, near_d, far_d, sh.u.hash[h] >= 0 ? p - sh.u.hash[h] : 0};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int d = cand[c];
                    if (d < 1 || d > p || mlen >= lim) continue;
                    int k = 0;
                    while (k < lim && ib[p + k] == ib[p + k - d]) ++k;
                    if (k > mlen) mlen = k, mdist = d;
                }
                if (mlen < MINLEN || (mlen == MINLEN && mdist > TOO_FAR)) mlen = 0;
            }
            // the greedy walk over the tile: literals up to the next lane that holds a match, then that match
            const unsigned long long has = __ballot(mlen > 0);
            unsigned long long starts = 0, matches = 0;
            int c = max(cover - t0, 0);
            while (c < tl) {
                const unsigned long long rest = has & ~((1ull << c) - 1ull);
                const int nm = rest ? min((int)__ffsll((long long)rest) - 1, tl) : tl;
                if (nm > c) starts |= ((nm < 64 ? (1ull << nm) : 0ull) - 1ull) & ~((1ull << c) - 1ull);
                if (nm >= tl) {
                    c = tl;
                    break;
                }
                int length = __shfl(mlen, nm);
                const int dist = __shfl(mdist, nm), at = t0 + nm, maxl = min(MAXLEN, n - at);
                if (length >= CAP && length < maxl) {   // all lanes extend it, 64 bytes a step
                    while (length < maxl) {
                        const int k = length + lane;
                        const bool differs = k >= maxl || ib[at + k] != ib[at + k - dist];
                        const unsigned long long bad = __ballot(differs);
                        if (bad) {
                            length += (int)__ffsll((long long)bad) - 1;
                            break;
                        }
                        length += WAVE;
                    }
                    length = min(length, maxl);
                    if (lane == nm) mlen = length;
                }
                starts |= 1ull << nm;
                matches |= 1ull << nm;
                c = nm + length;
            }
            cover = t0 + c;
            const bool mine = (starts >> lane) & 1ull, is_match = (matches >> lane) & 1ull;
            if (mine) {
                const int rank = ntok + (int)__popcll(starts & ((1ull << lane) - 1ull));
                if (is_match) {
                    int sym, eb, ev;
                    length_symbol(mlen, sym, eb, ev);
                    atomicAdd(&sh.freq[sym], 1u);
                    distance_symbol(mdist, sym, eb, ev);
                    atomicAdd(&sh.freq[NLIT + sym], 1u);
                    tok[rank] = 0x80000000u | ((uint32_t)(mlen - MINLEN) << 15) | (uint32_t)(mdist - 1);
                } else {
                    atomicAdd(&sh.freq[ib[p]], 1u);
                    tok[rank] = ib[p];
                }
            }
            ntok += (int)__popcll(starts);
        }
        __syncthreads();   // every look-up of the tile is done
        if (hashed) atomicMax(&sh.u.hash[h], p);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();       // the tokens are read back by other lanes; the hash table is dead

    // ---- the block type ------------------------------------------------------------------------------------------------------------
    // bits of the token stream under the fixed code, EOB included
    int fixed_bits = 0;
    for (int i = lane; i < NSYM; i += WAVE)
        fixed_bits += (int)sh.freq[i] * (i < NLIT ? fixed_lit_len(i) + lit_extra(i) : 5 + dist_extra(i - NLIT));
    fixed_bits = 3 + wave_sum_i(fixed_bits);

    Builder& b = sh.u.b;
    bool dyn_ok = build_lengths(sh.freq, NLIT, 15, sh.len, false, b);
    dyn_ok = build_lengths(sh.freq + NLIT, NDIST, 15, sh.len + NLIT, true, b) && dyn_ok;
    int hlit = 0, hdist = 0;
    for (int i = lane; i < NSYM; i += WAVE) {
        if (!sh.len[i]) continue;
        if (i < NLIT) hlit = max(hlit, i + 1);
        else hdist = max(hdist, i - NLIT + 1);
    }
    hlit = max(257, wave_allreduce_bits(hlit, [](int x, int y) { return max(x, y); }));
    hdist = max(1, wave_allreduce_bits(hdist, [](int x, int y) { return max(x, y); }));
    if (lane == 0) {   // the code lengths hlit + hdist in one sequence, run-length coded with 16 / 17 / 18
        int ni = 0, i = 0;
        const int total = hlit + hdist;
        auto at = [&](int k) { return (int)(k < hlit ? sh.len[k] : sh.len[NLIT + k - hlit]); };
        auto put = [&](int sym, int extra) {
            b.items[ni++] = (uint16_t)(sym | (extra << 8));
            ++sh.cfreq[sym];
        };
        while (i < total) {
            const int v = at(i);
            int run = 1;
            while (i + run < total && at(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) {
                    const int r = min(run, 138);
                    put(18, r - 11);
                    run -= r;
                }
                if (run >= 3) put(17, run - 3), run = 0;
                while (run-- > 0) put(0, 0);
            } else {
                put(v, 0);
                --run;
                while (run >= 3) {
                    const int r = min(run, 6);
                    put(16, r - 3);
                    run -= r;
                }
                while (run-- > 0) put(v, 0);
            }
        }
        b.n_items = ni;
    }
    __syncthreads();
    const int n_items = b.n_items;
    dyn_ok = build_lengths(sh.cfreq, NCLEN, 7, sh.clen, false, b) && dyn_ok;
    int hclen = 4;
    for (int k = 4; k < NCLEN; ++k)
        if (sh.clen[CLEN_ORDER[k]]) hclen = k + 1;
    int dyn_bits = 0;
    for (int i = lane; i < NSYM; i += WAVE)
        dyn_bits += (int)sh.freq[i] * (sh.len[i] + (i < NLIT ? lit_extra(i) : dist_extra(i - NLIT)));
    for (int i = lane; i < NCLEN; i += WAVE) dyn_bits += (int)sh.cfreq[i] * (sh.clen[i] + (i == 16 ? 2 : i == 17 ? 3 : i == 18 ? 7 : 0));
    dyn_bits = 3 + 14 + 3 * hclen + wave_sum_i(dyn_bits);

    // a coded block of a segment that is not the stream's last is followed by an empty stored block, which ends on a byte boundary
    auto coded_bytes = [&](int bits) { return last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; };
    const int stored_bytes = n + 5;
    int type = 0, best = stored_bytes;
    if (coded_bytes(fixed_bits) < best) type = 1, best = coded_bytes(fixed_bits);
    if (dyn_ok && coded_bytes(dyn_bits) < best) type = 2, best = coded_bytes(dyn_bits);

    if (type == 0) {
        if (lane == 0) {
            slot[0] = last ? 1 : 0;
            slot[1] = (uint8_t)n, slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)~n, slot[4] = (uint8_t)(~n >> 8);
        }
        for (int i = lane; i < n; i += WAVE) slot[5 + i] = ib[i];
        if (lane == 0) seg_len[g] = stored_bytes, seg_off[g] = stored_bytes;
        return;
    }

    // ---- the codes, the header, the tokens ---------------------------------------------------------------------------------------------
    if (type == 1) {
        __syncthreads();
        for (int i = lane; i < NSYM; i += WAVE) sh.len[i] = i < NLIT ? (uint8_t)fixed_lit_len(i) : 5;
    }
    assign_codes(sh.len, NLIT, sh.code);
    assign_codes(sh.len + NLIT, NDIST, sh.code + NLIT);
    if (type == 1) {   // the fixed literal/length code has 288 symbols: 286 and 287 take the last two 8-bit codes, so ours end two short
        __syncthreads();
        for (int i = lane; i < NLIT; i += WAVE) {
            const int c = i < 144 ? 0x30 + i : i < 256 ? 0x190 + i - 144 : i < 280 ? i - 256 : 0xC0 + i - 280;
            sh.code[i] = (uint16_t)(__brev((unsigned)c) >> (32 - sh.len[i]));
        }
        for (int i = lane; i < NDIST; i += WAVE) sh.code[NLIT + i] = (uint16_t)(__brev((unsigned)i) >> 27);
        __syncthreads();
    }
    if (type == 2) {
        assign_codes(sh.clen, NCLEN, sh.ccode);
        if (lane == 0) {
            int nh = 0;
            b.hdr[nh++] = (uint32_t)((last ? 1 : 0) | (2 << 1)) | (3u << 24);
            b.hdr[nh++] = (uint32_t)(hlit - 257) | (5u << 24);
            b.hdr[nh++] = (uint32_t)(hdist - 1) | (5u << 24);
            b.hdr[nh++] = (uint32_t)(hclen - 4) | (4u << 24);
            for (int k = 0; k < hclen; ++k) b.hdr[nh++] = (uint32_t)sh.clen[CLEN_ORDER[k]] | (3u << 24);
            for (int k = 0; k < n_items; ++k) {
                const int sym = b.items[k] & 255, extra = b.items[k] >> 8, l = sh.clen[sym];
                const int eb = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                b.hdr[nh++] = ((uint32_t)sh.ccode[sym] | ((uint32_t)extra << l)) | ((uint32_t)(l + eb) << 24);
            }
            b.n_hdr = nh;
        }
    } else if (lane == 0) {
        b.hdr[0] = (uint32_t)((last ? 1 : 0) | (1 << 1)) | (3u << 24);
        b.n_hdr = 1;
    }
    __syncthreads();
    Emitter e{slot, 0, 0};
    const int n_hdr = b.n_hdr;
    for (int k0 = 0; k0 < n_hdr; k0 += WAVE) {
        const uint32_t item = k0 + lane < n_hdr ? b.hdr[k0 + lane] : 0u;
        emit_round(sh, e, item & 0xffffffu, (int)(item >> 24));
    }
    for (int k0 = 0; k0 < ntok; k0 += WAVE) {
        unsigned long long bits = 0;
        int count = 0;
        if (k0 + lane < ntok) {
            const uint32_t t = tok[k0 + lane];
            if (t & 0x80000000u) {
                int sym, eb, ev;
                length_symbol((int)((t >> 15) & 255u) + MINLEN, sym, eb, ev);
                bits = sh.code[sym], count = sh.len[sym];
                bits |= (unsigned long long)ev << count, count += eb;
                distance_symbol((int)(t & 32767u) + 1, sym, eb, ev);
                bits |= (unsigned long long)sh.code[NLIT + sym] << count, count += sh.len[NLIT + sym];
                bits |= (unsigned long long)ev << count, count += eb;
            } else {
                bits = sh.code[t & 255u], count = sh.len[t & 255u];
            }
        }
        emit_round(sh, e, bits, count);
    }
    {   // the end of the block; then the byte boundary: zero bits after the stream's last block, an empty stored block elsewhere
        const int eob_len = sh.len[EOB], after = e.pend + eob_len + (last ? 0 : 3);
        unsigned long long bits = 0;
        int count = 0;
        if (lane == 0) bits = sh.code[EOB], count = eob_len;
        else if (lane == 1) count = (last ? 0 : 3) + ((8 - (after & 7)) & 7);
        else if (lane == 2 && !last) bits = 0xffff0000ull, count = 32;
        emit_round(sh, e, bits, count);
    }
    if (lane == 0) seg_len[g] = e.pos, seg_off[g] = e.pos;
}

// one workgroup: where each stream starts in `out`, and the total.  A stream is `fixed` bytes of framing and its segments.
__global__ __launch_bounds__(CT) void stream_offsets_kernel(const int32_t* __restrict__ totals, int n, long long fixed,
                                                            long long* __restrict__ offsets, long long* __restrict__ needed) {
    unsigned long long at = 0;
    for (int s0 = 0; s0 < n; s0 += CT) {
        const int s = s0 + (int)threadIdx.x;
        unsigned long long chunk;
        const unsigned long long o = block_scan_excl<CW>(s < n ? (unsigned long long)(totals[s] + fixed) : 0ull, chunk);
        if (s < n) offsets[s] = (long long)(at + o);
        at += chunk;
    }
    if (threadIdx.x == 0) {
        offsets[n] = (long long)at;
        *needed = (long long)at;
    }
}

// grid (segments per stream, streams of this launch).  Stream s's DEFLATE data starts `lead` bytes into its range of `out`.
__global__ __launch_bounds__(CT) void deflate_copy_kernel(const uint8_t* __restrict__ slots, const int32_t* __restrict__ seg_len,
                                                          const int32_t* __restrict__ seg_off, const long long* __restrict__ offsets,
                                                          int n, int s0, int max_segs, int lead, int wrapper, uint8_t* __restrict__ out,
                                                          unsigned long long capacity) {
    if ((unsigned long long)offsets[n] > capacity) return;
    const size_t s = (size_t)s0 + blockIdx.y, g = s * max_segs + blockIdx.x;
    const int tid = threadIdx.x, len = min(max(seg_len[g], 0), SLOT);
    uint8_t* dst = out + offsets[s] + lead;
    if (wrapper) {
        if (blockIdx.x == 0 && tid == 0) dst[0] = 0x78, dst[1] = 0x01;   // a 32 KiB window, no dictionary, level "fastest"
        dst += 2;
    }
    dst += seg_off[g];
    if (dst + len > out + offsets[s + 1]) return;   // cannot happen: the offsets are sums of these lengths
    const uint8_t* from = slots + g * SLOT;
    for (int i = tid; i < len; i += CT) dst[i] = from[i];
}

// grid (streams of this launch): the Adler-32 of the stream's input, big-endian behind its DEFLATE data
__global__ __launch_bounds__(ATHREADS) void adler32_store_kernel(const uint8_t* __restrict__ in, long long in_bytes,
                                                                 const long long* __restrict__ ranges, const int32_t* __restrict__ totals,
                                                                 const long long* __restrict__ offsets, int n, int s0, int lead,
                                                                 uint8_t* __restrict__ out, unsigned long long capacity) {
    if ((unsigned long long)offsets[n] > capacity) return;
    const size_t s = (size_t)s0 + blockIdx.x;
    long long off = ranges[s * FIELDS], len = ranges[s * FIELDS + 1];
    if (off < 0 || len < 0 || len > MAX_STREAM || off > in_bytes - len) off = 0, len = 0;
    const unsigned value = adler32_block(in + off, len);
    if (threadIdx.x == 0) {
        uint8_t* tr = out + offsets[s] + lead + 2 + totals[s];
        if (tr + 4 <= out + offsets[s + 1]) tr[0] = (uint8_t)(value >> 24), tr[1] = (uint8_t)(value >> 16), tr[2] = (uint8_t)(value >> 8), tr[3] = (uint8_t)value;
    }
}

// ---- 3. CRC-32 -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t CRC_POLY = 0xEDB88320u;   // the reflected polynomial: bit 31 is x^0
constexpr int CRC_PIECE = 64, CRC_CHUNK = CT * CRC_PIECE;

// a * b mod P, both reflected
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}
// x^(8 bytes) mod P by squaring
__device__ __forceinline__ uint32_t crc_xpow8(unsigned long long bytes) {
    uint32_t r = 0x80000000u, sq = 0x40000000u;   // 1 and x
    for (unsigned long long e = bytes * 8ull; e; e >>= 1) {
        if (e & 1ull) r = crc_mul(r, sq);
        sq = crc_mul(sq, sq);
    }
    return r;
}

// grid (16 KiB chunks of the longest range, ranges of this launch).  ranges int64 [n][2].  crc[r] starts at 0; a range with a negative
// length is skipped.  reg(A B) = reg(A) x^(8 |B|) + reg(B) for the register started at 0; the start value 0xFFFFFFFF adds
// 0xFFFFFFFF x^(8 len), the final inversion 0xFFFFFFFF.
__global__ __launch_bounds__(CT) void crc32_kernel(const uint8_t* __restrict__ data, long long data_bytes,
                                                   const long long* __restrict__ ranges, int r0, uint32_t* __restrict__ crc) {
    __shared__ uint32_t table[256];
    __shared__ uint32_t part[CW];
    const int tid = threadIdx.x;
    const size_t r = (size_t)r0 + blockIdx.y;
    const long long off = ranges[r * FIELDS], len = ranges[r * FIELDS + 1];
    if (off < 0 || len < 0 || off > data_bytes - len) return;
    const long long c0 = (long long)blockIdx.x * CRC_CHUNK;
    if (c0 >= len && blockIdx.x != 0) return;
    {
        uint32_t c = (uint32_t)tid;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
        table[tid] = c;
    }
    __syncthreads();
    const long long c1 = min(len, c0 + CRC_CHUNK);
    const long long ps = min(c1, c0 + (long long)tid * CRC_PIECE), pe = min(c1, ps + CRC_PIECE);
    uint32_t reg = 0;
    const uint8_t* d = data + off;
    for (long long i = ps; i < pe; ++i) reg = table[(reg ^ d[i]) & 255u] ^ (reg >> 8);
    uint32_t v = pe > ps ? crc_mul(reg, crc_xpow8((unsigned long long)(c1 - pe))) : 0u;
    v = (uint32_t)wave_allreduce_bits((int)v, [](int x, int y) { return x ^ y; });
    if ((tid & (WAVE - 1)) == 0) part[tid / WAVE] = v;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (int w = 0; w < CW; ++w) total ^= part[w];
        total = crc_mul(total, crc_xpow8((unsigned long long)(len - c1)));
        if (blockIdx.x == 0) total ^= crc_mul(0xFFFFFFFFu, crc_xpow8((unsigned long long)len)) ^ 0xFFFFFFFFu;
        atomicXor(&crc[r], total);
    }
}

// ---- 4. whole PNG files ----------------------------------------------------------------------------------------------------------
constexpr int PNG_HEADER = 33, PNG_LEAD = PNG_HEADER + 8, PNG_TAIL = 4 + 12;   // signature + IHDR; + length + "IDAT"; CRC + IEND

// one thread per frame: the table of the frames' raw scanlines
__global__ void png_raw_ranges_kernel(long long* __restrict__ ranges, int F, long long raw_bytes) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F) ranges[(size_t)f * FIELDS] = (long long)f * raw_bytes, ranges[(size_t)f * FIELDS + 1] = raw_bytes;
}

// grid (frames): everything of the file except the IDAT chunk's CRC, and the range that CRC covers (type + data)
__global__ __launch_bounds__(WAVE) void png_frame_kernel(const uint8_t* __restrict__ header, const long long* __restrict__ offsets, int F,
                                                         uint8_t* __restrict__ out, unsigned long long capacity,
                                                         long long* __restrict__ crc_ranges, uint32_t* __restrict__ crc) {
    const int f = blockIdx.x, lane = threadIdx.x;
    const bool fits = (unsigned long long)offsets[F] <= capacity;
    const long long z = offsets[f + 1] - offsets[f] - PNG_LEAD - PNG_TAIL;   // bytes of the zlib stream
    if (lane == 0) {
        crc_ranges[(size_t)f * FIELDS] = offsets[f] + PNG_HEADER + 4;
        crc_ranges[(size_t)f * FIELDS + 1] = (fits && z >= 0) ? z + 4 : -1;
        crc[f] = 0u;
    }
    if (!fits || z < 0) return;
    uint8_t* file = out + offsets[f];
    if (lane < PNG_HEADER) file[lane] = header[lane];
    if (lane < 4) file[PNG_HEADER + lane] = (uint8_t)((unsigned long long)z >> (24 - 8 * lane));
    if (lane < 4) file[PNG_HEADER + 4 + lane] = "IDAT"[lane];
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    if (lane < 12) file[PNG_LEAD + z + 4 + lane] = iend[lane];
}

__global__ void png_crc_store_kernel(const uint32_t* __restrict__ crc, const long long* __restrict__ offsets, int F,
                                     uint8_t* __restrict__ out, unsigned long long capacity) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F || (unsigned long long)offsets[F] > capacity) return;
    uint8_t* at = out + offsets[f + 1] - PNG_TAIL;
    const uint32_t v = crc[f];
    at[0] = (uint8_t)(v >> 24), at[1] = (uint8_t)(v >> 16), at[2] = (uint8_t)(v >> 8), at[3] = (uint8_t)v;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool png_sizes_ok(int F, int H, int W, int bpp) {
    return F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535 && (bpp == 1 || bpp == 3) &&
           (long long)H * (1 + (long long)W * bpp) <= MAX_STREAM;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct DefLayout {
    long long max_segs;
    size_t slots, tokens, seg_len, seg_off, totals, total;   // byte offsets into the workspace
};
DefLayout deflate_layout(long long n, long long longest) {
    DefLayout l;
    l.max_segs = std::max(1ll, (longest + SEG - 1) / SEG);
    const size_t segs = (size_t)n * l.max_segs;
    l.slots = 0;
    l.tokens = align256(l.slots + segs * SLOT);
    l.seg_len = align256(l.tokens + segs * SEG * 4);
    l.seg_off = align256(l.seg_len + segs * 4);
    l.totals = align256(l.seg_off + segs * 4);
    l.total = align256(l.totals + (size_t)n * 4);
    return l;
}

// the host copy of a range table: every entry inside the buffer; returns the longest range through `longest`
int check_ranges(const char* who, const int64_t* t, int n, int64_t bytes, int64_t limit, long long* longest) {
    *longest = 0;
    for (int s = 0; s < n; ++s) {
        const int64_t off = t[(size_t)s * FIELDS], len = t[(size_t)s * FIELDS + 1];
        DTK_REQUIRE(off >= 0 && len >= 0 && len <= limit && off <= bytes - len, "%s: range %d (%lld + %lld) does not fit %lld bytes (a range holds at most %lld)",
                    who, s, (long long)off, (long long)len, (long long)bytes, (long long)limit);
        *longest = std::max(*longest, (long long)len);
    }
    return 0;
}

// everything of dtk_deflate behind the checks.  Stream s occupies `lead` bytes, its (wrapped) DEFLATE data and `tail` bytes.
int deflate_run(const uint8_t* in, int64_t in_bytes, const int64_t* ranges, int n, long long longest, int wrapper, int near_d, int far_d,
                int lead, int tail, uint8_t* out, size_t capacity, int64_t* offsets, int64_t* needed, void* workspace, hipStream_t st) {
    const DefLayout l = deflate_layout(n, longest);
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* slots = ws + l.slots;
    uint32_t* tokens = reinterpret_cast<uint32_t*>(ws + l.tokens);
    int32_t* seg_len = reinterpret_cast<int32_t*>(ws + l.seg_len);
    int32_t* seg_off = reinterpret_cast<int32_t*>(ws + l.seg_off);
    int32_t* totals = reinterpret_cast<int32_t*>(ws + l.totals);
    const long long* rg = reinterpret_cast<const long long*>(ranges);
    long long* offs = reinterpret_cast<long long*>(offsets);
    const int ms = (int)l.max_segs;
    for (int s0 = 0; s0 < n; s0 += MAX_PER_LAUNCH) {
        const dim3 grid((unsigned)ms, (unsigned)std::min(n - s0, MAX_PER_LAUNCH));
        DTK_LAUNCH("deflate_segment", deflate_segment_kernel, grid, dim3(WAVE), 0, st, in, (long long)in_bytes, rg, s0, ms, near_d, far_d,
                   slots, tokens, seg_len, seg_off);
    }
    DTK_LAUNCH("deflate_assemble", block_offsets_kernel<CW>, dim3((unsigned)n), dim3(CT), 0, st, seg_off, ms, totals);
    DTK_LAUNCH("deflate_assemble", stream_offsets_kernel, dim3(1), dim3(CT), 0, st, totals, n, (long long)(lead + tail + (wrapper ? 6 : 0)),
               offs, reinterpret_cast<long long*>(needed));
    for (int s0 = 0; s0 < n; s0 += MAX_PER_LAUNCH) {
        const int count = std::min(n - s0, MAX_PER_LAUNCH);
        DTK_LAUNCH("deflate_assemble", deflate_copy_kernel, dim3((unsigned)ms, (unsigned)count), dim3(CT), 0, st, slots, seg_len, seg_off,
                   offs, n, s0, ms, lead, wrapper, out, (unsigned long long)capacity);
        if (wrapper)
            DTK_LAUNCH("deflate_adler32", adler32_store_kernel, dim3((unsigned)count), dim3(ATHREADS), 0, st, in, (long long)in_bytes, rg,
                       totals, offs, n, s0, lead, out, (unsigned long long)capacity);
    }
    return 0;
}

// crc[r] must be 0 before this
int crc_run(const uint8_t* data, int64_t data_bytes, const long long* ranges, int n, long long longest, uint32_t* crc, hipStream_t st) {
    const unsigned chunks = (unsigned)std::max(1ll, (longest + CRC_CHUNK - 1) / CRC_CHUNK);
    for (int r0 = 0; r0 < n; r0 += MAX_PER_LAUNCH)
        DTK_LAUNCH("crc32", crc32_kernel, dim3(chunks, (unsigned)std::min(n - r0, MAX_PER_LAUNCH)), dim3(CT), 0, st, data,
                   (long long)data_bytes, ranges, r0, crc);
    return 0;
}

long long bound_of(long long n) { return n + 5 * std::max(1ll, (n + SEG - 1) / SEG) + 6; }

struct PngLayout {
    long long raw_bytes;
    size_t raw, ranges, crc_ranges, crc, deflate, total;
};
PngLayout png_layout(int F, int H, int W, int bpp) {
    PngLayout l;
    l.raw_bytes = (long long)H * (1 + (long long)W * bpp);
    l.raw = 0;
    l.ranges = align256((size_t)F * l.raw_bytes);
    l.crc_ranges = align256(l.ranges + (size_t)F * FIELDS * 8);
    l.crc = align256(l.crc_ranges + (size_t)F * FIELDS * 8);
    l.deflate = align256(l.crc + (size_t)F * 4);
    l.total = l.deflate + deflate_layout(F, l.raw_bytes).total;
    return l;
}

int filter_run(const uint8_t* frames, int F, int H, int W, int bpp, int filter, uint8_t* raw, hipStream_t st) {
    for (int f0 = 0; f0 < F; f0 += MAX_PER_LAUNCH) {
        const dim3 grid((unsigned)H, (unsigned)std::min(F - f0, MAX_PER_LAUNCH));
        if (bpp == 1) DTK_LAUNCH("png_filter", png_filter_kernel<1>, grid, dim3(CT), 0, st, frames, f0, H, W, filter, raw);
        else DTK_LAUNCH("png_filter", png_filter_kernel<3>, grid, dim3(CT), 0, st, frames, f0, H, W, filter, raw);
    }
    return 0;
}

}  // namespace

extern "C" int dtk_png_filter(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t bpp, int32_t filter, uint8_t* raw,
                              void* stream) {
    DTK_REQUIRE(png_sizes_ok(F, H, W, bpp),
                "png_filter: F >= 1, 1 <= H, W <= 65535, bpp 1 or 3 and at most 2^30 raw bytes per frame are required, got F=%d %d x %d bpp=%d",
                F, H, W, bpp);
    DTK_REQUIRE(filter >= 0 && filter <= 5, "png_filter: filter must be 0 .. 4 or 5 (adaptive), got %d", filter);
    DTK_REQUIRE(frames && raw, "png_filter: null pointer (frames / raw)");
    return filter_run(frames, F, H, W, bpp, filter, raw, dtk_stream(stream));
}

extern "C" int64_t dtk_deflate_bound(int64_t n) { return n < 0 ? 0 : bound_of(n); }

extern "C" size_t dtk_deflate_workspace_bytes(const int64_t* ranges_host, int32_t n_streams) {
    if (!ranges_host || n_streams < 1) return 0;
    long long longest = 0;
    for (int s = 0; s < n_streams; ++s) {
        const int64_t len = ranges_host[(size_t)s * FIELDS + 1];
        if (len < 0 || len > MAX_STREAM) return 0;
        longest = std::max(longest, (long long)len);
    }
    return deflate_layout(n_streams, longest).total;
}

extern "C" int dtk_deflate(const uint8_t* in, int64_t in_bytes, const int64_t* ranges, const int64_t* ranges_host, int32_t n_streams,
                           int32_t wrapper, uint8_t* out, size_t out_capacity, int64_t* offsets, int64_t* needed, void* workspace,
                           void* stream) {
    DTK_REQUIRE(in && ranges && ranges_host && out && offsets && needed && workspace,
                "deflate: null pointer (in / ranges / ranges_host / out / offsets / needed / workspace)");
    DTK_REQUIRE(in_bytes >= 1 && n_streams >= 1, "deflate: in_bytes and n_streams must be positive, got %lld, %d", (long long)in_bytes, n_streams);
    DTK_REQUIRE(wrapper == 0 || wrapper == 1, "deflate: wrapper must be 0 (raw) or 1 (zlib), got %d", wrapper);
    long long longest;
    if (int rc = check_ranges("deflate", ranges_host, n_streams, in_bytes, MAX_STREAM, &longest)) return rc;
    return deflate_run(in, in_bytes, ranges, n_streams, longest, wrapper, 3, 0, 0, 0, out, out_capacity, offsets, needed, workspace,
                       dtk_stream(stream));
}

extern "C" int dtk_crc32(const uint8_t* data, int64_t data_bytes, const int64_t* ranges, const int64_t* ranges_host, int32_t n_ranges,
                         uint32_t* crc, void* stream) {
    DTK_REQUIRE(data && ranges && ranges_host && crc, "crc32: null pointer (data / ranges / ranges_host / crc)");
    DTK_REQUIRE(data_bytes >= 1 && n_ranges >= 1, "crc32: data_bytes and n_ranges must be positive, got %lld, %d", (long long)data_bytes, n_ranges);
    long long longest;
    if (int rc = check_ranges("crc32", ranges_host, n_ranges, data_bytes, (int64_t)1 << 40, &longest)) return rc;
    hipStream_t st = dtk_stream(stream);
    DTK_HIP(dtk_zero_async(crc, (size_t)n_ranges * 4, st));
    return crc_run(data, data_bytes, reinterpret_cast<const long long*>(ranges), n_ranges, longest, crc, st);
}

extern "C" size_t dtk_png_encode_workspace_bytes(int32_t F, int32_t H, int32_t W, int32_t bpp) {
    return png_sizes_ok(F, H, W, bpp) ? png_layout(F, H, W, bpp).total : 0;
}

extern "C" int dtk_png_encode(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t bpp, int32_t filter, const uint8_t* header,
                              uint8_t* out, size_t out_capacity, int64_t* offsets, int64_t* needed, void* workspace, void* stream) {
    DTK_REQUIRE(png_sizes_ok(F, H, W, bpp),
                "png_encode: F >= 1, 1 <= H, W <= 65535, bpp 1 or 3 and at most 2^30 raw bytes per frame are required, got F=%d %d x %d bpp=%d",
                F, H, W, bpp);
    DTK_REQUIRE(filter >= 0 && filter <= 5, "png_encode: filter must be 0 .. 4 or 5 (adaptive), got %d", filter);
    DTK_REQUIRE(frames && header && out && offsets && needed && workspace,
                "png_encode: null pointer (frames / header / out / offsets / needed / workspace)");
    const PngLayout l = png_layout(F, H, W, bpp);
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* raw = ws + l.raw;
    long long* ranges = reinterpret_cast<long long*>(ws + l.ranges);
    long long* crc_ranges = reinterpret_cast<long long*>(ws + l.crc_ranges);
    uint32_t* crc = reinterpret_cast<uint32_t*>(ws + l.crc);
    hipStream_t st = dtk_stream(stream);
    if (int rc = filter_run(frames, F, H, W, bpp, filter, raw, st)) return rc;
    DTK_LAUNCH("png_assemble", png_raw_ranges_kernel, dim3((unsigned)dtk_cdiv(F, CT)), dim3(CT), 0, st, ranges, F, l.raw_bytes);
    const int pitch = 1 + W * bpp;
    if (int rc = deflate_run(raw, (int64_t)F * l.raw_bytes, reinterpret_cast<const int64_t*>(ranges), F, l.raw_bytes, 1, bpp == 3 ? 3 : 2,
                             pitch <= SEG ? pitch : 0, PNG_LEAD, PNG_TAIL, out, out_capacity, offsets, needed, ws + l.deflate, st))
        return rc;
    const long long* offs = reinterpret_cast<const long long*>(offsets);
    DTK_LAUNCH("png_assemble", png_frame_kernel, dim3((unsigned)F), dim3(WAVE), 0, st, header, offs, F, out, (unsigned long long)out_capacity,
               crc_ranges, crc);
    if (int rc = crc_run(out, (int64_t)std::min<unsigned long long>(out_capacity, 1ull << 62), crc_ranges, F, bound_of(l.raw_bytes) + 4, crc, st))
        return rc;
    DTK_LAUNCH("png_assemble", png_crc_store_kernel, dim3((unsigned)dtk_cdiv(F, CT)), dim3(CT), 0, st, crc, offs, F, out,
               (unsigned long long)out_capacity);
    return 0;
}
