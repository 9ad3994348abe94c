// inflate_core.h -- the stream-level logic of DEFLATE (RFC 1951) and its zlib wrapper (RFC 1950), docs/PNG_DECODE.md section 2: an
// LSB-first bit reader over 32-bit words, the zlib header check, the code-length alphabet, canonical-code tables with the over- and
// under-subscription tests, symbol decoding, and the length / distance base and extra-bit tables.  Plain C++ that compiles for the
// host and for the device: the kernel in inflate.hip and the stand-alone host program tests/host/inflate_host.cpp (built with the
// sanitisers) run the same lines.  What differs between the two is only how bytes reach the reader and where output goes.
//
// What holds whatever the bytes contain:
//   * the reader never touches a word at or beyond `limit` (inf_word checks the index); past the end the bits are zero, and the
//     callers compare `pos` with `avail_bits` after every element they consume: INF_S_OVERRUN ends the stream there;
//   * every element consumes at least one bit, so a loop over elements ends after at most avail_bits + 1 of them;
//   * a table is only filled after its code lengths passed inf_code_sort, so no look-up entry of an over-subscribed code exists;
//     every table index is masked or range-checked on use.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD inline
#endif
// a value every lane of the wave holds alike (the decode chain is wave-uniform): on the device it moves to a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define INF_UNIFORM(x) ((uint32_t)(x))
#endif

// status bits (DTK_INFLATE_S_* in dtk.h)
#define INF_S_HEADER 1      // zlib header: CM != 8, window > 32 K, FCHECK fails, or FDICT set
#define INF_S_BTYPE 2       // block type 3
#define INF_S_STORED 4      // LEN != ~NLEN
#define INF_S_TABLE 8       // a code-length set that describes no usable code (see inf_code_sort, inf_read_dynamic)
#define INF_S_CODE 16       // litlen symbol 286 / 287, distance symbol 30 / 31, or no code matches
#define INF_S_DISTANCE 32   // a back-reference before the stream's first output byte
#define INF_S_OVERRUN 64    // input exhausted
#define INF_S_LENGTH 128    // output would exceed the expected size, or the final block ends short of it
#define INF_S_ADLER 256     // trailer mismatch (set by dtk_adler32)
#define INF_S_STREAM 512    // a stream-table entry outside the buffers: nothing decoded

constexpr int INF_LIT_LOOK = 10, INF_DIST_LOOK = 8, INF_CLEN_LOOK = 7;
constexpr int INF_MAX_LENS = 288 + 32;   // HLIT + HDIST code lengths of a dynamic block, or the fixed code's
constexpr int INF_WINDOW = 32768;

// ---- bits, LSB first ---------------------------------------------------------------------------------------------------------
// `words` are the stream's bytes as little-endian 32-bit words, `limit` of them readable (bytes beyond the data are zero).  The
// reader keeps the next bits in a 64-bit register, at least 32 of them valid at any time.
struct InfBits {
    const uint32_t* words;
    uint32_t limit;
    uint32_t avail_bits;
    uint32_t pos;    // bits consumed
    uint32_t next;   // index of the word after those in `acc`
    uint64_t acc;    // the bits from `pos` on, right-aligned
    int cnt;         // how many of them are valid: 33 .. 64
};

INF_HD uint32_t inf_word(const InfBits& b, uint32_t i) { return i < b.limit ? INF_UNIFORM(b.words[i]) : 0u; }

INF_HD void inf_bits_start(InfBits& b, const uint32_t* words, uint32_t limit, uint32_t avail_bits, uint32_t pos) {
    b.words = words, b.limit = limit, b.avail_bits = avail_bits, b.pos = pos;
    const uint32_t w = pos >> 5, s = pos & 31u;
    b.acc = (((uint64_t)inf_word(b, w + 1) << 32) | inf_word(b, w)) >> s;
    b.cnt = 64 - (int)s;
    b.next = w + 2;
}
INF_HD uint32_t inf_peek(const InfBits& b) { return (uint32_t)b.acc; }
INF_HD void inf_consume(InfBits& b, int n) {   // 0 <= n <= 32
    b.acc = n >= 32 ? b.acc >> 32 : b.acc >> n;
    b.cnt -= n;
    b.pos += (uint32_t)n;
    if (b.cnt <= 32) {
        b.acc |= (uint64_t)inf_word(b, b.next++) << b.cnt;
        b.cnt += 32;
    }
}
INF_HD uint32_t inf_take(InfBits& b, int n) {   // 0 <= n <= 16
    const uint32_t v = inf_peek(b) & ((1u << n) - 1u);
    inf_consume(b, n);
    return v;
}
INF_HD bool inf_over(const InfBits& b) { return b.pos > b.avail_bits; }

INF_HD uint32_t inf_rev32(uint32_t v) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return (v >> 16) | (v << 16);
}

// ---- zlib header (RFC 1950) ------------------------------------------------------------------------------------------------------
INF_HD int inf_zlib_header(InfBits& b) {
    const uint32_t cmf = inf_take(b, 8), flg = inf_take(b, 8);
    if (inf_over(b)) return INF_S_OVERRUN;
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return INF_S_HEADER;
    return 0;
}

// ---- canonical codes -------------------------------------------------------------------------------------------------------------
// A first level by the next LOOK bits -- (length << 9) | symbol for a code of at most LOOK bits, 0 where none starts -- and, for
// longer codes, the canonical second level: the symbols in code order with the largest code and the symbol offset of every length.
enum { INF_KIND_CLEN = 0, INF_KIND_LITLEN = 1, INF_KIND_DIST = 2 };

template <int LOOK, int MAXSYMS>
struct InfCode {
    uint16_t look[1 << LOOK];
    uint16_t syms[MAXSYMS];
    int32_t maxcode[16];   // [l], l = 1 .. 15: the largest code of length l, -1 where there is none
    int32_t valoff[16];    // [l]: index in syms of the first symbol of length l minus its code
    uint16_t next[16];     // scratch of the sort
    int32_t total;         // coded symbols
    int32_t status;        // what inf_code_sort found (the device reads it after a barrier)
    int32_t maxlen;        // the longest code (reported by the tests' host program)
};

// Build in three steps with a barrier between them on the device: inf_code_clear and inf_code_fill by lanes `lane`, `lane + n`, ...
// of n; inf_code_sort by ONE thread.  A single host thread calls all three, the shared ones with (0, 1).
template <int LOOK, int MAXSYMS>
INF_HD void inf_code_clear(InfCode<LOOK, MAXSYMS>* t, int lane, int n) {
    for (int i = lane; i < (1 << LOOK); i += n) t->look[i] = 0;
}

// Counts, the subscription tests and the symbols in code order, from lens[0 .. n).  Returns (and stores) 0 or INF_S_TABLE:
//   over-subscribed: always refused;
//   incomplete: refused for the code-length and the literal/length alphabet; a distance alphabet may be EMPTY (a block of literals
//     only) or hold ONE code of length 1 -- the incomplete code zlib accepts;
//   a literal/length alphabet without a code for 256 (end of block) is refused.
template <int LOOK, int MAXSYMS>
INF_HD int inf_code_sort(const uint8_t* lens, int n, int kind, InfCode<LOOK, MAXSYMS>* t) {
    if (n > MAXSYMS) n = MAXSYMS;
    int count[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) ++count[lens[i] & 15];
    int left = 1, code = 0, k = 0, status = 0, maxlen = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) {
            status = INF_S_TABLE;
            break;
        }
        t->maxcode[l] = count[l] ? code + count[l] - 1 : -1;
        t->valoff[l] = k - code;
        t->next[l] = (uint16_t)k;
        if (count[l]) maxlen = l;
        k += count[l];
        code = (code + count[l]) << 1;
    }
    t->maxcode[0] = -1, t->valoff[0] = 0, t->next[0] = 0;
    if (!status && left > 0) {
        const bool accepted = kind == INF_KIND_DIST && (k == 0 || (k == 1 && count[1] == 1));
        if (!accepted) status = INF_S_TABLE;
    }
    if (!status && kind == INF_KIND_LITLEN && (n <= 256 || lens[256] == 0)) status = INF_S_TABLE;
    if (!status)
        for (int i = 0; i < n; ++i) {
            const int l = lens[i] & 15;
            if (l) t->syms[t->next[l]++] = (uint16_t)i;
        }
    t->total = status ? 0 : k;
    t->status = status;
    t->maxlen = maxlen;
    return status;
}

template <int LOOK, int MAXSYMS>
INF_HD void inf_code_fill(const uint8_t* lens, InfCode<LOOK, MAXSYMS>* t, int lane, int n) {
    const int total = t->total;
    for (int k = lane; k < total && k < MAXSYMS; k += n) {
        const int sym = t->syms[k] % MAXSYMS, l = lens[sym] & 15;
        const int code = k - t->valoff[l];
        if (l < 1 || l > LOOK || code < 0 || (code >> l) != 0) continue;
        const uint32_t rev = inf_rev32((uint32_t)code) >> (32 - l);
        for (uint32_t e = rev; e < (1u << LOOK); e += 1u << l) t->look[e] = (uint16_t)((l << 9) | sym);
    }
}

// one symbol from the next bits (`window`, LSB first): its length (0: no code matches) and value
template <int LOOK, int MAXSYMS>
INF_HD int inf_symbol(const InfCode<LOOK, MAXSYMS>& t, uint32_t window, int& sym) {
    const uint32_t e = INF_UNIFORM(t.look[window & ((1u << LOOK) - 1u)]);
    if (e) {
        sym = (int)(e & 511u);
        return (int)(e >> 9);
    }
    const uint32_t rev = inf_rev32(window);   // the first bit of the stream on top: codes are packed MSB first
    for (int l = LOOK + 1; l <= 15; ++l) {
        const int code = (int)(rev >> (32 - l));
        if (code <= (int)INF_UNIFORM(t.maxcode[l])) {
            const int at = code + (int)INF_UNIFORM(t.valoff[l]);
            if (at < 0 || at >= MAXSYMS) return 0;
            sym = (int)INF_UNIFORM(t.syms[at]);
            return l;
        }
    }
    return 0;
}

typedef InfCode<INF_LIT_LOOK, 288> InfLitCode;
typedef InfCode<INF_DIST_LOOK, 32> InfDistCode;
typedef InfCode<INF_CLEN_LOOK, 19> InfClenCode;

// no code matches: the bits ran out (the window is padded with zeros) or the stream is damaged
INF_HD int inf_no_code(const InfBits& b, int longest) { return b.pos + (uint32_t)longest > b.avail_bits ? INF_S_OVERRUN : INF_S_CODE; }

// ---- block headers ---------------------------------------------------------------------------------------------------------------
// the fixed code of RFC 1951 3.2.6: 288 literal/length lengths, then 32 distance lengths
INF_HD void inf_fixed_lens(uint8_t* lens, int lane, int n) {
    for (int i = lane; i < INF_MAX_LENS; i += n) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
}

// The header of a dynamic block, by ONE thread: HLIT, HDIST, HCLEN, the code-length code and the hlit + hdist lengths it encodes
// into lens[0 .. hlit + hdist).  INF_S_TABLE: HLIT > 286 or HDIST > 30, a code-length code that is not complete, a repeat with no
// previous length or beyond the count.
INF_HD int inf_read_dynamic(InfBits& b, InfClenCode* cl, uint8_t* lens, int& hlit, int& hdist) {
    static constexpr uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    hlit = 257 + (int)inf_take(b, 5);
    hdist = 1 + (int)inf_take(b, 5);
    const int hclen = 4 + (int)inf_take(b, 4);
    if (inf_over(b)) return INF_S_OVERRUN;
    if (hlit > 286 || hdist > 30) return INF_S_TABLE;
    uint8_t cl_lens[19];
    for (int i = 0; i < 19; ++i) cl_lens[i] = 0;
    for (int i = 0; i < hclen; ++i) cl_lens[ORDER[i]] = (uint8_t)inf_take(b, 3);
    if (inf_over(b)) return INF_S_OVERRUN;
    inf_code_clear(cl, 0, 1);
    if (inf_code_sort(cl_lens, 19, INF_KIND_CLEN, cl)) return INF_S_TABLE;
    inf_code_fill(cl_lens, cl, 0, 1);
    const int total = hlit + hdist;
    int i = 0;
    while (i < total) {
        int sym = 0;
        const int n = inf_symbol(*cl, inf_peek(b), sym);
        if (n == 0) return inf_no_code(b, 7);
        inf_consume(b, n);
        if (inf_over(b)) return INF_S_OVERRUN;
        if (sym < 16) {
            lens[i++] = (uint8_t)sym;
            continue;
        }
        int rep, val = 0;
        if (sym == 16) {
            rep = 3 + (int)inf_take(b, 2);
            if (inf_over(b)) return INF_S_OVERRUN;
            if (i == 0) return INF_S_TABLE;
            val = lens[i - 1];
        } else if (sym == 17) {
            rep = 3 + (int)inf_take(b, 3);
        } else {
            rep = 11 + (int)inf_take(b, 7);
        }
        if (inf_over(b)) return INF_S_OVERRUN;
        if (i + rep > total) return INF_S_TABLE;
        for (int r = 0; r < rep; ++r) lens[i++] = (uint8_t)val;
    }
    return 0;
}

// ---- tokens ----------------------------------------------------------------------------------------------------------------------
enum { INF_TOKEN_EOB = -1, INF_TOKEN_MATCH = -2, INF_TOKEN_FAULT = -3 };

INF_HD int inf_length_base(int i) {   // i = symbol - 257, 0 .. 28
    static constexpr uint16_t BASE[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                          31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    return BASE[i];
}
INF_HD int inf_length_extra(int i) { return i < 8 || i == 28 ? 0 : (i - 4) >> 2; }
INF_HD int inf_dist_base(int i) {   // i = distance symbol, 0 .. 29
    static constexpr uint16_t BASE[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                          193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    return BASE[i];
}
INF_HD int inf_dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }

// One token: a literal (0 .. 255), INF_TOKEN_EOB, INF_TOKEN_MATCH with `mlen` (3 .. 258) and `mdist` (1 .. 32768), or
// INF_TOKEN_FAULT with `status`.  A token takes at most 15 + 5 + 15 + 13 = 48 bits.
INF_HD int inf_token(InfBits& b, const InfLitCode& lit, const InfDistCode& dist, int& mlen, int& mdist, int& status) {
    int sym = 0;
    int n = inf_symbol(lit, inf_peek(b), sym);
    if (n == 0) {
        status = inf_no_code(b, 15);
        return INF_TOKEN_FAULT;
    }
    inf_consume(b, n);
    if (inf_over(b)) {
        status = INF_S_OVERRUN;
        return INF_TOKEN_FAULT;
    }
    if (sym < 256) return sym;
    if (sym == 256) return INF_TOKEN_EOB;
    if (sym > 285) {
        status = INF_S_CODE;
        return INF_TOKEN_FAULT;
    }
    mlen = inf_length_base(sym - 257) + (int)inf_take(b, inf_length_extra(sym - 257));
    n = inf_symbol(dist, inf_peek(b), sym);
    if (n == 0) {
        status = inf_no_code(b, 15);
        return INF_TOKEN_FAULT;
    }
    inf_consume(b, n);
    if (inf_over(b)) {
        status = INF_S_OVERRUN;
        return INF_TOKEN_FAULT;
    }
    if (sym > 29) {
        status = INF_S_CODE;
        return INF_TOKEN_FAULT;
    }
    mdist = inf_dist_base(sym) + (int)inf_take(b, inf_dist_extra(sym));
    if (inf_over(b)) {
        status = INF_S_OVERRUN;
        return INF_TOKEN_FAULT;
    }
    return INF_TOKEN_MATCH;
}

// ---- PNG row filters (PNG specification section 9): one byte, from the reconstructed left, up and up-left bytes --------------------
INF_HD int inf_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;   // ties in the order a, b, c
}
INF_HD int inf_unfilter_byte(int filter, int raw, int a, int b, int c) {
    const int pred = filter == 1 ? a : filter == 2 ? b : filter == 3 ? (a + b) >> 1 : filter == 4 ? inf_paeth(a, b, c) : 0;
    return (raw + pred) & 255;
}
