// jpeg_entropy.h -- the sequential part of baseline-JPEG decoding (docs/JPEG_DECODE.md section 1): Huffman look-ups built from a DHT's
// raw counts and symbols, an MSB-first bit reader over UNSTUFFED bytes, and the decode loop of one 8 x 8 block.  Plain C++ that
// compiles for the host and for the device: the kernel in jpeg_decode.hip and the stand-alone host program tests/host/
// jpeg_entropy_host.cpp (built with the sanitisers) run the same lines.  At the end of the file: the same decoding cut into
// sub-streams that many lanes work on side by side (section 1b; csrc/jpeg_parallel.hip, tests/host/jpeg_parallel_host.cpp).
//
// What holds whatever the bytes and the tables contain (the tables the library is handed are validated by the caller, but nothing
// below relies on it):
//   * every iteration of the block loop advances the coefficient index by at least one or ends the block: at most 64 iterations per
//     block, so a segment of M MCUs of B blocks takes at most 64 * B * M -- inside the documented bound 8 * bytes + 64 * B * M;
//   * the reader never touches a word beyond the one that holds the last valid bit plus one (jpg_word checks the index): past
//     the end the window is zero and JPG_S_OVERRUN is set;
//   * a coefficient index beyond 63 ends the block with JPG_S_INDEX, a window no code matches ends it with JPG_S_CODE;
//   * every table index is masked or range-checked.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPG_HD __host__ __device__ __forceinline__
#else
#define JPG_HD inline
#endif

// status bits (DTK_JPEG_S_* in dtk.h)
#define JPG_S_CODE 1      // no code matches the next bits (or a DC category above 11)
#define JPG_S_INDEX 2     // a run carried the coefficient index beyond 63
#define JPG_S_OVERRUN 4   // bits were read past the segment's end
#define JPG_S_LEFTOVER 8  // more than 7 unread bits at the segment's end
#define JPG_S_RANGE 16    // |coefficient * Q| > 2047 (set by the pixel stage)
#define JPG_S_SEGMENT 32  // a segment-table entry outside the stream or the frame's MCUs: nothing decoded

// samplings (DTK_JPEG_* in dtk.h) and the MCU schedule that follows from them (docs/JPEG_DECODE.md section 0): the blocks of an MCU
// in scan order are the luma blocks, row by row, then Cb, then Cr; a single-component scan is not interleaved: one block.
#define JPG_420 0    // 2x2 1x1 1x1: Y00 Y01 Y10 Y11 Cb Cr, 16 x 16 pixels
#define JPG_422 1    // 2x1 1x1 1x1: Y0 Y1 Cb Cr, 16 wide x 8 high
#define JPG_444 2    // 1x1 1x1 1x1: Y Cb Cr, 8 x 8
#define JPG_GRAY 3   // one component: Y, 8 x 8

JPG_HD constexpr bool jpg_sampling_ok(int s) { return s >= JPG_420 && s <= JPG_GRAY; }
JPG_HD constexpr int jpg_blocks_per_mcu(int s) { return s == JPG_420 ? 6 : s == JPG_422 ? 4 : s == JPG_444 ? 3 : 1; }
JPG_HD constexpr int jpg_components(int s) { return s == JPG_GRAY ? 1 : 3; }
JPG_HD constexpr int jpg_mcu_width(int s) { return s == JPG_420 || s == JPG_422 ? 16 : 8; }
JPG_HD constexpr int jpg_mcu_height(int s) { return s == JPG_420 ? 16 : 8; }
// the component of block k (0 <= k < B) of an MCU of B blocks: all but the last two are luma
JPG_HD constexpr int jpg_block_component(int B, int k) { return B < 3 || k < B - 2 ? 0 : k - (B - 3); }

constexpr int JPG_LOOK_BITS = 9;
constexpr int JPG_TABLE_BYTES = 272;   // a raw table: 16 counts, then up to 256 symbols in code order

struct JpgHuff {
    uint16_t look[1 << JPG_LOOK_BITS];   // by the next 9 bits: (length << 8) | symbol of a code of at most 9 bits, else 0
    int32_t maxcode[17];                 // [l], l = 1 .. 16: the largest code of length l, -1 where there is none
    int32_t valoff[17];                  // [l]: index of the first symbol of length l minus its code
    uint8_t vals[256];
};

// Build in two steps with a barrier between them on the device: lanes `lane`, `lane + n`, ... of n.  A single host thread calls
// both with (0, 1).
JPG_HD void jpg_huff_clear(JpgHuff* t, int lane, int n) {
    for (int i = lane; i < (1 << JPG_LOOK_BITS); i += n) t->look[i] = 0;
}
JPG_HD void jpg_huff_fill(const uint8_t* raw, JpgHuff* t, int lane, int n) {
    // every lane walks the 16 counts (cheap); the symbols are shared out
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int cnt = raw[len - 1];
        if (lane == 0) {
            t->maxcode[len] = cnt ? code + cnt - 1 : -1;
            t->valoff[len] = k - code;
        }
        for (int i = lane; i < cnt; i += n) {
            const int sym_at = k + i, c = code + i;
            if (sym_at > 255) break;
            const uint8_t sym = raw[16 + sym_at];
            t->vals[sym_at] = sym;
            if (len <= JPG_LOOK_BITS && (c >> len) == 0) {   // an over-subscribed length writes nothing
                const int first = c << (JPG_LOOK_BITS - len), count = 1 << (JPG_LOOK_BITS - len);
                for (int e = 0; e < count; ++e) t->look[first + e] = (uint16_t)((len << 8) | sym);
            }
        }
        k += cnt;
        code = (code + cnt) << 1;
    }
    if (lane == 0) t->maxcode[0] = -1, t->valoff[0] = 0;
}

// the unstuffed bytes of a segment (or of the part of it that is staged) as big-endian-read 32-bit words.  `words` holds at least
// (avail_bits + 31) / 32 + 1 readable words, zero beyond the data.  The reader keeps the next bits in a 64-bit register, at least
// 32 of them at any time, and fetches the word after those ONE STEP EARLY (`ahead`): the memory read a symbol needs was issued while
// the symbol before it was decoded, so the only dependent read per symbol is the table look-up.
struct JpgBits {
    const uint32_t* words;
    uint32_t avail_bits;
    uint32_t pos;     // bits consumed
    uint32_t limit;   // readable words
    uint32_t next;    // index of the word after `ahead`
    uint32_t ahead;   // the word that follows the bits in `acc`
    uint64_t acc;     // the bits from `pos` on, left-aligned
    int cnt;          // how many of them are valid: 33 .. 64
};

JPG_HD uint32_t jpg_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
JPG_HD uint32_t jpg_word(const JpgBits& b, uint32_t i) { return i < b.limit ? jpg_bswap(b.words[i]) : 0u; }

JPG_HD void jpg_bits_start(JpgBits& b, const uint32_t* words, uint32_t avail_bits, uint32_t pos) {
    b.words = words, b.avail_bits = avail_bits, b.pos = pos, b.limit = (avail_bits + 31u) / 32u + 1u;
    const uint32_t w = pos >> 5, s = pos & 31u;
    b.acc = (((uint64_t)jpg_word(b, w) << 32) | jpg_word(b, w + 1)) << s;
    b.cnt = 64 - (int)s;
    b.ahead = jpg_word(b, w + 2);
    b.next = w + 3;
}

// the next 32 bits, MSB first; zero (and JPG_S_OVERRUN) when the position is at or beyond the end.  Bits of the window that lie
// beyond the end are whatever follows the data in `words` -- the callers keep zeros there.
JPG_HD uint32_t jpg_window(const JpgBits& b, int& status) {
    if (b.pos >= b.avail_bits) {
        status |= JPG_S_OVERRUN;
        return 0u;
    }
    return (uint32_t)(b.acc >> 32);
}

JPG_HD void jpg_consume(JpgBits& b, int n) {   // 0 <= n <= 31
    b.acc <<= n;
    b.cnt -= n;
    b.pos += (uint32_t)n;
    if (b.cnt <= 32) {
        b.acc |= (uint64_t)b.ahead << (32 - b.cnt);
        b.cnt += 32;
        b.ahead = jpg_word(b, b.next++);
    }
}

// one symbol: its length (0: none matches) and value
JPG_HD int jpg_symbol(const JpgHuff& t, uint32_t window, int& sym) {
    const unsigned e = t.look[window >> (32 - JPG_LOOK_BITS)];
    if (e) {
        sym = (int)(e & 0xffu);
        return (int)(e >> 8);
    }
    for (int len = JPG_LOOK_BITS + 1; len <= 16; ++len) {
        const int code = (int)(window >> (32 - len));
        if (code <= t.maxcode[len]) {
            sym = t.vals[(code + t.valoff[len]) & 255];
            return len;
        }
    }
    return 0;
}

// s bits after the `len`-bit code at the top of the window, sign-extended as T.81 F.2.2.1 (s <= 15)
JPG_HD int jpg_extend(uint32_t window, int len, int s) {
    if (s == 0) return 0;
    const int v = (int)((window << len) >> (32 - s));
    return (v >> (s - 1)) ? v : v - (1 << s) + 1;
}

// Decode one block into out[64] (zigzag order, ZEROED by the caller).  `pred` is the component's DC predictor.  Returns the status
// bits it met; JPG_S_CODE, JPG_S_INDEX and JPG_S_OVERRUN end the block where they happen.  `iters` counts loop iterations.
JPG_HD int jpg_decode_block(JpgBits& b, const JpgHuff& dc, const JpgHuff& ac, int& pred, int16_t* out, uint32_t& iters) {
    int status = 0, sym = 0;
    ++iters;
    uint32_t w = jpg_window(b, status);
    int len = jpg_symbol(dc, w, sym);
    if (status) return status;
    if (len == 0 || sym > 11) return JPG_S_CODE;
    pred = (int16_t)(pred + jpg_extend(w, len, sym));   // wraps to 16 bits: defined for any stream
    jpg_consume(b, len + sym);
    out[0] = (int16_t)pred;
    int k = 1;
    while (k < 64) {
        ++iters;
        w = jpg_window(b, status);
        if (status) return status;
        len = jpg_symbol(ac, w, sym);
        if (len == 0) return JPG_S_CODE;
        const int r = sym >> 4, s = sym & 15;
        jpg_consume(b, len + s);
        if (s == 0) {
            if (r != 15) break;   // EOB
            k += 16;              // ZRL
            continue;
        }
        k += r;
        if (k > 63) return JPG_S_INDEX;
        out[k++] = (int16_t)jpg_extend(w, len, s);
    }
    return 0;
}

// The blocks of nm whole MCUs of B blocks each, in scan order, from a reader that holds ALL of the segment's bits: block b goes to
// coef[b * 64 .. b * 64 + 63] (ZEROED by the caller).  tab[2 c], tab[2 c + 1]: component c's DC and AC look-ups; the predictors start
// at 0.  Stops at the first block that reports a status and returns it.  (The kernel runs the same schedule -- jpg_block_component
// with a wrapping counter -- around its staging of the bytes.)
JPG_HD int jpg_decode_mcus(JpgBits& b, const JpgHuff* tab, int B, int nm, int16_t* coef, uint32_t& iters) {
    int pred[3] = {0, 0, 0}, k = 0;
    for (long long blk = 0, n = (long long)nm * B; blk < n; ++blk) {
        const int comp = jpg_block_component(B, k);
        const int st = jpg_decode_block(b, tab[2 * comp], tab[2 * comp + 1], pred[comp], coef + blk * 64, iters);
        if (st) return st;
        if (++k == B) k = 0;
    }
    return 0;
}

// ---- progressive files (SOF2; docs/JPEG_DECODE.md, "Progressive files"; T.81 Annex G) -----------------------------------------------
// A scan codes the band [Ss, Se] of the zigzag coefficients of its blocks at bit position Al: DC bands (Ss = Se = 0) of one component
// or of all three interleaved, AC bands (Ss >= 1) of one component.  Ah = 0: the band's first scan; Ah > 0: a refinement that adds
// bit Al.  The four per-block routines below take the block's 64 coefficients `out` and touch out[Ss .. Se] only.  What holds
// whatever the bytes and the tables contain:
//   * every loop iteration consumes at least one bit, advances the coefficient index or ends the block; `iters` counts one per
//     block, one per symbol and one per coefficient position visited: at most JPG_PROG_ITERS_PER_BLOCK per block, so a segment of
//     n blocks takes at most 8 * bytes + JPG_PROG_ITERS_PER_BLOCK * n;
//   * an index beyond Se, or an end-of-band run longer than the `left` blocks of the segment, ends the block with JPG_S_INDEX;
//   * a refinement symbol whose size is neither 0 nor 1 ends it with JPG_S_CODE.
constexpr int JPG_PROG_ITERS_PER_BLOCK = 130;
constexpr int JPG_PROG_FIELDS = 14;   // a row of the segment table (DTK_JPEG_PROG_FIELDS in dtk.h)
constexpr int JPG_PROG_MAX_AL = 13;
constexpr int JPG_PROG_MAX_LEVEL = 255;

struct JpgScan {
    int Ss, Se, Ah, Al;
    int comp;   // the scan's component, -1: the interleaved DC scan of all three
};

// one bit; JPG_S_OVERRUN past the end
JPG_HD int jpg_bit(JpgBits& b, int& status) {
    const uint32_t w = jpg_window(b, status);
    if (status) return 0;
    jpg_consume(b, 1);
    return (int)(w >> 31);
}

JPG_HD int jpg_prog_dc_first(JpgBits& b, const JpgHuff& dc, int& pred, int Al, int16_t* out, uint32_t& iters) {
    int status = 0, sym = 0;
    ++iters;
    const uint32_t w = jpg_window(b, status);
    const int len = jpg_symbol(dc, w, sym);
    if (status) return status;
    if (len == 0 || sym > 11) return JPG_S_CODE;
    pred = (int16_t)(pred + jpg_extend(w, len, sym));   // wraps to 16 bits, as in jpg_decode_block
    jpg_consume(b, len + sym);
    out[0] = (int16_t)((uint32_t)pred << Al);
    return 0;
}

JPG_HD int jpg_prog_dc_refine(JpgBits& b, int Al, int16_t* out, uint32_t& iters) {
    int status = 0;
    ++iters;
    if (jpg_bit(b, status)) out[0] = (int16_t)(out[0] | (1 << Al));
    return status;
}

// an end-of-band symbol of category r behind the `len`-bit code at the top of w: the run's length, this block included
JPG_HD uint32_t jpg_prog_run(JpgBits& b, uint32_t w, int len, int r) {
    const uint32_t run = (1u << r) + (r ? (w << len) >> (32 - r) : 0u);
    jpg_consume(b, len + r);   // at most 16 + 14
    return run;
}

// `run`: the blocks of a pending end-of-band run, this one included (0: none); `left`: the blocks left in the segment, this one
// included
JPG_HD int jpg_prog_ac_first(JpgBits& b, const JpgHuff& ac, int Ss, int Se, int Al, uint32_t& run, uint32_t left, int16_t* out,
                             uint32_t& iters) {
    int status = 0, sym = 0;
    ++iters;
    if (run) {
        --run;   // the block consumes no bits
        return 0;
    }
    int k = Ss;
    while (k <= Se) {
        ++iters;
        const uint32_t w = jpg_window(b, status);
        if (status) return status;
        const int len = jpg_symbol(ac, w, sym);
        if (len == 0) return JPG_S_CODE;
        const int r = sym >> 4, s = sym & 15;
        if (s) {
            k += r;
            if (k > Se) return JPG_S_INDEX;
            jpg_consume(b, len + s);   // at most 16 + 15
            out[k++] = (int16_t)((uint32_t)jpg_extend(w, len, s) << Al);
        } else if (r == 15) {
            jpg_consume(b, len);
            k += 16;
            if (k > Se) return JPG_S_INDEX;
        } else {
            run = jpg_prog_run(b, w, len, r);
            if (run > left) {
                run = 0;
                return JPG_S_INDEX;
            }
            --run;
            break;
        }
    }
    return 0;
}

// a correction bit for the already non-zero out[k]
JPG_HD void jpg_prog_correct(JpgBits& b, int Al, int16_t* out, int k, int& status) {
    if (jpg_bit(b, status) && !(out[k] & (1 << Al))) out[k] = (int16_t)(out[k] + (out[k] > 0 ? (1 << Al) : -(1 << Al)));
}

JPG_HD int jpg_prog_ac_refine(JpgBits& b, const JpgHuff& ac, int Ss, int Se, int Al, uint32_t& run, uint32_t left, int16_t* out,
                              uint32_t& iters) {
    int status = 0, sym = 0;
    ++iters;
    int k = Ss;
    if (run == 0) {
        while (k <= Se) {
            ++iters;
            const uint32_t w = jpg_window(b, status);
            if (status) return status;
            const int len = jpg_symbol(ac, w, sym);
            if (len == 0) return JPG_S_CODE;
            int r = sym >> 4;
            const int s = sym & 15;
            int value = 0;
            if (s) {
                if (s != 1) return JPG_S_CODE;
                jpg_consume(b, len);
                value = jpg_bit(b, status) ? (1 << Al) : -(1 << Al);
                if (status) return status;
            } else if (r == 15) {
                jpg_consume(b, len);
            } else {
                run = jpg_prog_run(b, w, len, r);
                if (run > left) {
                    run = 0;
                    return JPG_S_INDEX;
                }
                break;
            }
            // pass r still-zero positions, correcting what is non-zero on the way; stop AT the next still-zero one
            for (; k <= Se; ++k) {
                ++iters;
                if (out[k]) {
                    jpg_prog_correct(b, Al, out, k, status);
                    if (status) return status;
                } else if (--r < 0) {
                    break;
                }
            }
            if (k > Se) return JPG_S_INDEX;
            if (value) out[k] = (int16_t)value;
            ++k;
        }
    }
    if (run) {
        for (; k <= Se; ++k) {
            ++iters;
            if (out[k]) {
                jpg_prog_correct(b, Al, out, k, status);
                if (status) return status;
            }
        }
        --run;
    }
    return 0;
}

// the real block grid of component c (0: luma) of an H x W picture: what a one-component scan walks
JPG_HD constexpr int jpg_comp_block_cols(int S, int c, int W) {
    return c == 0 || S == JPG_444 ? (W + 7) / 8 : ((W + 1) / 2 + 7) / 8;
}
JPG_HD constexpr int jpg_comp_block_rows(int S, int c, int H) { return c == 0 || S != JPG_420 ? (H + 7) / 8 : ((H + 1) / 2 + 7) / 8; }
JPG_HD constexpr long long jpg_mcus(int S, int H, int W) {
    return (long long)((H + jpg_mcu_height(S) - 1) / jpg_mcu_height(S)) * ((W + jpg_mcu_width(S) - 1) / jpg_mcu_width(S));
}
// the units a scan's restart segments count: MCUs for the interleaved scan, the component's real blocks otherwise
JPG_HD constexpr long long jpg_scan_units(int S, int comp, int H, int W) {
    return comp < 0 ? jpg_mcus(S, H, W) : (long long)jpg_comp_block_rows(S, comp, H) * jpg_comp_block_cols(S, comp, W);
}

// where block i of a segment that starts at unit u0 lies in the frame's MCU-major layout [MCUs][B][64]: its block index.  The
// interleaved scan's blocks follow the layout; block u of a one-component scan is (u / cols, u % cols) of the component's grid.
JPG_HD long long jpg_scan_block(int S, int comp, long long u0, long long i, int W) {
    const int B = jpg_blocks_per_mcu(S);
    if (comp < 0) return u0 * B + i;
    const long long u = u0 + i;
    const int cols = jpg_comp_block_cols(S, comp, W), mw = (W + jpg_mcu_width(S) - 1) / jpg_mcu_width(S);
    const long long by = u / cols;
    const int bx = (int)(u - by * cols);
    if (comp > 0) return (by * mw + bx) * B + (B - 3 + comp);
    const int h = jpg_mcu_width(S) / 8, v = jpg_mcu_height(S) / 8;
    return ((by / v) * mw + bx / h) * B + (by % v) * h + bx % h;
}

// A row of the segment table (dtk.h: frame, byte offset, byte length, level, Ss, Se, Ah, Al, component, first unit, units, three
// table indices) against the stream, the frame count, the sampling's unit counts and the table count.  The library checks the host
// copy before it launches anything, the kernel its device copy.
JPG_HD bool jpg_prog_row_ok(const long long* g, int S, int F, int H, int W, long long stream_bytes, int n_tables, long long max_bytes) {
    if (g[0] < 0 || g[0] >= F || g[1] < 0 || g[2] < 0 || g[2] > max_bytes || g[1] > stream_bytes - g[2]) return false;
    if (g[3] < 0 || g[3] > JPG_PROG_MAX_LEVEL) return false;
    const long long Ss = g[4], Se = g[5], Ah = g[6], Al = g[7], comp = g[8];
    if (Ss < 0 || Se < Ss || Se > 63 || (Ss == 0 && Se != 0) || Al < 0 || Al > JPG_PROG_MAX_AL || (Ah != 0 && Ah != Al + 1)) return false;
    if (comp < -1 || comp >= jpg_components(S) || (comp < 0 && (Ss != 0 || S == JPG_GRAY))) return false;
    const long long units = jpg_scan_units(S, (int)comp, H, W);
    if (g[9] < 0 || g[10] < 1 || g[9] > units - g[10]) return false;
    const int used = Ss == 0 ? (Ah ? 0 : comp < 0 ? 3 : 1) : 1;
    for (int t = 0; t < used; ++t)
        if (g[11 + t] < 0 || g[11 + t] >= n_tables) return false;
    return true;
}

// The blocks of one restart segment of a scan from a reader that holds ALL of its bits, into the frame's coefficients `coef`
// ([MCUs][B][64]; zero before the frame's first scan).  tab: the DC look-up per component of a DC first scan (tab[0] alone when the
// scan has one component), the AC look-up of an AC scan, unused by a DC refinement.  Predictors and the pending run start at zero.
// Stops at the first block that reports a status and returns it.  (The kernel runs the same routines around its staging of the bytes
// and of the coefficients.)
JPG_HD int jpg_decode_scan_segment(JpgBits& b, const JpgHuff* tab, int S, const JpgScan& sc, long long u0, long long nu, int W,
                                   int16_t* coef, uint32_t& iters) {
    const int B = jpg_blocks_per_mcu(S);
    const long long n = sc.comp < 0 ? nu * B : nu;
    int pred[3] = {0, 0, 0}, k = 0;
    uint32_t run = 0;
    for (long long i = 0; i < n; ++i) {
        int16_t* out = coef + jpg_scan_block(S, sc.comp, u0, i, W) * 64;
        const uint32_t left = (uint32_t)(n - i < 0x7fffffffll ? n - i : 0x7fffffffll);
        int st;
        if (sc.Ss == 0) {
            const int c = sc.comp < 0 ? jpg_block_component(B, k) : 0;
            st = sc.Ah ? jpg_prog_dc_refine(b, sc.Al, out, iters) : jpg_prog_dc_first(b, tab[c], pred[c], sc.Al, out, iters);
            if (++k == B) k = 0;
        } else {
            st = sc.Ah ? jpg_prog_ac_refine(b, tab[0], sc.Ss, sc.Se, sc.Al, run, left, out, iters)
                       : jpg_prog_ac_first(b, tab[0], sc.Ss, sc.Se, sc.Al, run, left, out, iters);
        }
        if (st) return st;
    }
    return 0;
}

// ---- decoding inside a segment in parallel (docs/JPEG_DECODE.md section 1b) ----------------------------------------------------------
// The unstuffed bytes of a baseline segment are cut into SUB-STREAMS of L bytes.  A decoder STATE is (p, c, k): the bit position, the
// block's place in its MCU, the zigzag index (0: a DC symbol is next).  jpg_step decodes ONE symbol exactly as jpg_decode_block does;
// a SPECULATIVE step that meets an invalid code, a DC category above 11, an index beyond 63 or the segment's end RECOVERS -- it skips
// one bit and ends the block -- so the map from a state to the next is total and the chain of entry states from (0, 0, 0) is well
// defined for any bytes.  What holds whatever the bytes and the tables contain:
//   * every step, valid or recovering, consumes at least one bit: jpg_advance takes at most `bound - p` steps;
//   * jpg_write_substream stores only to blocks [0, nb) of the `coef` it is handed and stops at the first status;
//   * the reader is JpgBits: no word beyond the one after the last valid bit is touched.
struct JpgState {
    uint32_t p;   // bit position in the unstuffed segment
    uint16_t c;   // the block's place in its MCU, 0 .. B - 1
    uint16_t k;   // zigzag index of the next coefficient; 0: the next symbol is a DC symbol
};
JPG_HD unsigned long long jpg_state_pack(const JpgState& s) {
    return ((unsigned long long)s.p << 32) | ((unsigned long long)s.c << 16) | (unsigned long long)s.k;
}
JPG_HD JpgState jpg_state_unpack(unsigned long long v) {
    JpgState s;
    s.p = (uint32_t)(v >> 32), s.c = (uint16_t)((v >> 16) & 0xffffu), s.k = (uint16_t)(v & 0xffffu);
    return s;
}
constexpr int JPG_SUBSEQ_DEFAULT = 128, JPG_SUBSEQ_MIN = 16, JPG_SUBSEQ_MAX = 1024;
JPG_HD constexpr bool jpg_subseq_ok(int L) { return L >= JPG_SUBSEQ_MIN && L <= JPG_SUBSEQ_MAX && L % 4 == 0; }

// One symbol from the reader `b`, which stands at s.p.  idx >= 0: coefficient `idx` of the current block takes `value` (for idx == 0
// the DC DIFFERENCE).  A strict step returns the status jpg_decode_block would (the state is then meaningless); a speculative step
// always returns 0.
JPG_HD int jpg_step(JpgBits& b, const JpgHuff* tab, int B, JpgState& s, bool speculative, int& idx, int& value) {
    int status = 0, sym = 0, next = 64, fault = 0;
    idx = -1, value = 0;
    const bool dc = s.k == 0;
    const int place = s.c < B ? s.c : 0;
    const JpgHuff& t = tab[2 * jpg_block_component(B, place) + (dc ? 0 : 1)];
    const uint32_t w = jpg_window(b, status);
    const int len = status ? 0 : jpg_symbol(t, w, sym);
    if (status) {
        fault = status;
    } else if (len == 0 || (dc && sym > 11)) {
        fault = JPG_S_CODE;
    } else if (dc) {
        idx = 0, value = jpg_extend(w, len, sym), next = 1;
        jpg_consume(b, len + sym);
    } else {
        const int r = sym >> 4, size = sym & 15;
        if (size == 0) {
            next = r != 15 ? 64 : (int)s.k + 16;   // EOB; ZRL (beyond 63 the block ends, as `while (k < 64)` does)
            jpg_consume(b, len);
        } else if ((int)s.k + r > 63) {
            fault = JPG_S_INDEX;
        } else {
            idx = (int)s.k + r, value = jpg_extend(w, len, size), next = idx + 1;
            jpg_consume(b, len + size);
        }
    }
    if (fault) {
        if (!speculative) return fault;
        jpg_consume(b, 1);   // the recovery rule: skip one bit (nothing was consumed yet), end the block
        next = 64;
    }
    if (next >= 64) {
        s.k = 0;
        s.c = (uint16_t)(place + 1 == B ? 0 : place + 1);
    } else {
        s.k = (uint16_t)next;
    }
    s.p = b.pos;
    return 0;
}

// f: speculative steps from s while s.p < bound.  Returns the number of blocks that START on the way (steps taken at k == 0).
JPG_HD uint32_t jpg_advance(JpgBits& b, const JpgHuff* tab, int B, JpgState& s, uint32_t bound, uint32_t& iters) {
    uint32_t starts = 0;
    int idx, value;
    while (s.p < bound) {
        ++iters;
        starts += s.k == 0 ? 1u : 0u;
        jpg_step(b, tab, B, s, true, idx, value);
    }
    return starts;
}

// The strict pass of one sub-stream: from its entry state s (the reader stands there) while s.p < bound, with `first` the number of
// blocks that start before the sub-stream.  Non-zero values go to coef[block * 64 + idx] of the segment's nb blocks (ZEROED by the
// caller), DC differences to index 0.  The chain stops at the segment's block count: the step that completes block nb - 1 sets
// `ended` and leaves the bit position behind it in end_pos.  Returns the first status it meets.
JPG_HD int jpg_write_substream(JpgBits& b, const JpgHuff* tab, int B, JpgState s, uint32_t bound, long long first, long long nb,
                               int16_t* coef, bool& ended, uint32_t& end_pos, uint32_t& iters) {
    if (first < 0) first = 0;
    if (first > nb + 1) first = nb + 1;
    long long next = first, cur = first - 1;
    if (s.k != 0 && (cur < 0 || cur >= nb)) return 0;   // inside a block outside the segment: behind its end, or behind an error
    int idx, value;
    while (s.p < bound) {
        if (s.k == 0) {
            if (next >= nb) return 0;
            cur = next++;
        }
        ++iters;
        const int st = jpg_step(b, tab, B, s, false, idx, value);
        if (st) return st;
        if (idx >= 0 && value != 0 && cur >= 0 && cur < nb) coef[cur * 64 + idx] = (int16_t)value;
        if (s.k == 0 && next == nb) {
            ended = true, end_pos = s.p;
            return 0;
        }
    }
    return 0;
}

// DC differences -> predictors: per component the running sum over the segment's blocks, wrapping to int16 as jpg_decode_block does
JPG_HD void jpg_dc_sums(int16_t* coef, long long first, long long count, int B, int (&pred)[3]) {
    int k = (int)(first % B);
    for (long long blk = first; blk < first + count; ++blk) {
        const int comp = jpg_block_component(B, k);
        pred[comp] = (int16_t)(pred[comp] + coef[blk * 64]);
        coef[blk * 64] = (int16_t)pred[comp];
        if (++k == B) k = 0;
    }
}

// the end check of the sequential kernel
JPG_HD int jpg_end_status(uint32_t pos, uint32_t avail_bits) {
    return pos > avail_bits ? JPG_S_OVERRUN : avail_bits - pos > 7u ? JPG_S_LEFTOVER : 0;
}

// The redo rule: a segment whose strict pass reported anything is zeroed and decoded by the sequential loop.
JPG_HD int jpg_decode_segment_sequential(const uint32_t* words, uint32_t avail_bits, const JpgHuff* tab, int B, int nm, int16_t* coef,
                                         uint32_t& iters) {
    JpgBits b;
    jpg_bits_start(b, words, avail_bits, 0u);
    int st = jpg_decode_mcus(b, tab, B, nm, coef, iters);
    if (!st) st = jpg_end_status(b.pos, avail_bits);
    return st;
}

JPG_HD uint32_t jpg_substreams(uint32_t unstuffed_bytes, int L) { return unstuffed_bytes ? (unstuffed_bytes + (uint32_t)L - 1u) / (uint32_t)L : 1u; }

// The whole of section 1b over one segment, one sub-stream after the other: what the kernel's lanes do side by side.  words: the
// unstuffed bytes as JpgBits takes them; states, counts: n = jpg_substreams(bytes, L) entries each; coef: nm * B * 64 values, ZEROED.
// rounds: how often the states were swept (at most n + 1).  Returns the status.
JPG_HD int jpg_decode_segment_substreams(const uint32_t* words, uint32_t unstuffed_bytes, const JpgHuff* tab, int B, int nm, int L,
                                         unsigned long long* states, int32_t* counts, int16_t* coef, uint32_t& rounds, uint32_t& iters) {
    const uint32_t avail = unstuffed_bytes * 8u, n = jpg_substreams(unstuffed_bytes, L);
    const long long nb = (long long)nm * B;
    JpgBits b;
    for (uint32_t i = 0; i < n; ++i) states[i] = (unsigned long long)(8u * (uint32_t)L * i) << 32;   // the guesses; e_0 is known
    rounds = 0;
    for (uint32_t round = 0; round <= n; ++round) {   // bounded by the number of sub-streams
        bool changed = false;
        ++rounds;
        for (uint32_t i = 0; i + 1 < n; ++i) {
            JpgState s = jpg_state_unpack(states[i]);
            jpg_bits_start(b, words, avail, s.p);
            for (uint32_t j = i + 1; j < n; ++j) {   // carry the state on until it meets an equal stored one
                jpg_advance(b, tab, B, s, 8u * (uint32_t)L * j, iters);
                if (states[j] == jpg_state_pack(s)) break;
                states[j] = jpg_state_pack(s), changed = true;
            }
        }
        if (!changed) break;
    }
    long long total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        JpgState s = jpg_state_unpack(states[i]);
        jpg_bits_start(b, words, avail, s.p);
        const long long c = jpg_advance(b, tab, B, s, i + 1 < n ? 8u * (uint32_t)L * (i + 1u) : avail, iters);
        counts[i] = (int32_t)(total < nb + 1 ? total : nb + 1);   // the exclusive scan, clamped: beyond nb nothing is decoded
        total += c;
    }
    int st = 0;
    bool ended = false;
    uint32_t end_pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const JpgState s = jpg_state_unpack(states[i]);
        jpg_bits_start(b, words, avail, s.p);
        st |= jpg_write_substream(b, tab, B, s, i + 1 < n ? 8u * (uint32_t)L * (i + 1u) : 0xffffffffu, counts[i], nb, coef, ended, end_pos,
                                  iters);
    }
    if (!st) {
        int pred[3] = {0, 0, 0};
        jpg_dc_sums(coef, 0, nb, B, pred);
        st = ended ? jpg_end_status(end_pos, avail) : JPG_S_OVERRUN;
    }
    if (st) {
        for (long long i = 0; i < nb * 64; ++i) coef[i] = 0;
        st = jpg_decode_segment_sequential(words, avail, tab, B, nm, coef, iters);
    }
    return st;
}
