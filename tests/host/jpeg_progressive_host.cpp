// A stand-alone HOST program around the progressive routines of dino_tracker_amd/csrc/jpeg_entropy.h: built by
// tests/test_jpeg_progressive_reference.py with -fsanitize=address,undefined and run directly (never loaded into Python).
//
//   jpeg_progressive_host CASE...     every CASE is a file written by tests/jpeg_prog_cases.case_file: a whole progressive JPEG file,
//                                     the segment rows and raw tables video_in.plan_jpeg_progressive made of it, and the coefficients
//                                     the restatement (tests/jpeg_prog_ref.py) expects.
//
// Per case: every row passes jpg_prog_row_ok; the rows are decoded in table order (they are ordered by level) with
// jpg_decode_scan_segment -- the per-block routines the kernel runs -- and the coefficients must equal the expected ones.  Then, for
// the first segment of each of the four scan kinds (DC first, DC refinement, AC first, AC refinement) that has at least two bytes,
// damaged copies are decoded into a copy of the coefficients as they stood before that segment: truncated at each of the first 64
// byte positions and one byte before the end, 48 single-bit flips, all-FF tails.  Without arguments only the built-in streams run: an
// end-of-band run longer than the blocks left (first and refinement scans), a refinement size other than 0 / 1, nonsense tables over
// random bytes, rows jpg_prog_row_ok must refuse, the block order of one-component scans.  Every buffer has exactly the size the
// decoder is entitled to -- the unstuffed bytes as (bits + 31) / 32 + 1 words, one frame of coefficients, the tables a scan uses --
// and the iteration bound of docs/JPEG_DECODE.md section 5, 8 * bytes + JPG_PROG_ITERS_PER_BLOCK * blocks, is asserted per stream.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../dino_tracker_amd/csrc/jpeg_entropy.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static uint32_t rng_state = 2026u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static const long long MAX_BYTES = 1ll << 28;
static int cases = 0, counts[64] = {0};

// one segment: unstuff into an exact-size word buffer, decode into `coef` (one frame), classify the end
static int decode_segment(const uint8_t* raw, size_t len, int S, const JpgScan& sc, long long u0, long long nu, int W,
                          const JpgHuff* tab, int16_t* coef, uint32_t* end_pos = nullptr, uint32_t* avail_bits = nullptr) {
    std::vector<uint8_t> un;
    for (size_t i = 0; i < len; ++i)
        if (!(raw[i] == 0 && i > 0 && raw[i - 1] == 0xff)) un.push_back(raw[i]);
    const uint32_t avail = (uint32_t)un.size() * 8u;
    const size_t nwords = (avail + 31) / 32 + 1;   // what jpg_window may touch
    uint32_t* words = (uint32_t*)calloc(nwords, 4);
    CHECK(words);
    if (!un.empty()) memcpy(words, un.data(), un.size());
    JpgBits bits;
    jpg_bits_start(bits, words, avail, 0u);
    uint32_t iters = 0;
    int st = jpg_decode_scan_segment(bits, tab, S, sc, u0, nu, W, coef, iters);
    if (!st) {
        if (bits.pos > avail) st |= JPG_S_OVERRUN;
        else if (avail - bits.pos > 7u) st |= JPG_S_LEFTOVER;
    }
    free(words);
    const uint64_t blocks = (uint64_t)(sc.comp < 0 ? nu * jpg_blocks_per_mcu(S) : nu);
    CHECK((uint64_t)iters <= 8ull * len + (uint64_t)JPG_PROG_ITERS_PER_BLOCK * blocks);   // the documented bound
    CHECK((uint64_t)iters <= (uint64_t)JPG_PROG_ITERS_PER_BLOCK * blocks);                // and what the loops' shape gives
    CHECK((st & ~(JPG_S_CODE | JPG_S_INDEX | JPG_S_OVERRUN | JPG_S_LEFTOVER)) == 0);
    if (end_pos) *end_pos = bits.pos;
    if (avail_bits) *avail_bits = avail;
    ++counts[st & 63], ++cases;
    return st;
}

// the tables a scan uses, in a buffer of exactly that many
static JpgHuff* build_tables(const long long* row, const uint8_t* raws, int& ntab) {
    ntab = row[4] == 0 ? (row[6] ? 0 : row[8] < 0 ? 3 : 1) : 1;
    JpgHuff* tab = (JpgHuff*)malloc((size_t)(ntab ? ntab : 1) * sizeof(JpgHuff));
    CHECK(tab);
    for (int t = 0; t < ntab; ++t) {
        jpg_huff_clear(&tab[t], 0, 1);
        jpg_huff_fill(raws + (size_t)row[11 + t] * JPG_TABLE_BYTES, &tab[t], 0, 1);
    }
    return tab;
}

static int run_row(const long long* row, const uint8_t* stream, const uint8_t* raws, int S, int W, int16_t* coef,
                   const std::vector<uint8_t>* bytes = nullptr, uint32_t* end_pos = nullptr, uint32_t* avail = nullptr) {
    int ntab;
    JpgHuff* tab = build_tables(row, raws, ntab);
    const JpgScan sc = {(int)row[4], (int)row[5], (int)row[6], (int)row[7], (int)row[8]};
    const size_t len = bytes ? bytes->size() : (size_t)row[2];
    uint8_t* seg = (uint8_t*)malloc(len ? len : 1);   // an exact-size copy: a read beyond is seen
    CHECK(seg);
    if (len) memcpy(seg, bytes ? bytes->data() : stream + row[1], len);
    const int st = decode_segment(seg, len, S, sc, row[9], row[10], W, tab, coef, end_pos, avail);
    free(seg), free(tab);
    return st;
}

static std::vector<uint8_t> read_file(const char* path) {
    FILE* fh = fopen(path, "rb");
    CHECK(fh);
    std::vector<uint8_t> v;
    uint8_t chunk[4096];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, fh)) > 0) v.insert(v.end(), chunk, chunk + n);
    fclose(fh);
    return v;
}

// a case file: int64 magic, S, H, W, rows, tables, stream bytes; the rows; the tables; the stream; the expected coefficients
static void run_case(const char* path) {
    const std::vector<uint8_t> file = read_file(path);
    CHECK(file.size() >= 56);
    long long head[7];
    memcpy(head, file.data(), sizeof head);
    CHECK(head[0] == 0x50524f47);
    const int S = (int)head[1], H = (int)head[2], W = (int)head[3], nrows = (int)head[4], ntables = (int)head[5];
    const long long nbytes = head[6];
    CHECK(jpg_sampling_ok(S) && nrows >= 1 && ntables >= 1 && nbytes >= 1);
    const size_t ncoef = (size_t)jpg_mcus(S, H, W) * jpg_blocks_per_mcu(S) * 64;
    CHECK(file.size() == 56 + (size_t)nrows * JPG_PROG_FIELDS * 8 + (size_t)ntables * JPG_TABLE_BYTES + (size_t)nbytes + ncoef * 2);
    std::vector<long long> rows((size_t)nrows * JPG_PROG_FIELDS);
    const uint8_t* at = file.data() + 56;
    memcpy(rows.data(), at, rows.size() * 8), at += rows.size() * 8;
    const std::vector<uint8_t> raws(at, at + (size_t)ntables * JPG_TABLE_BYTES);
    at += raws.size();
    const std::vector<uint8_t> stream(at, at + nbytes);
    at += nbytes;
    std::vector<int16_t> want(ncoef);
    memcpy(want.data(), at, ncoef * 2);

    int16_t* coef = (int16_t*)calloc(ncoef, 2);   // exactly one frame
    CHECK(coef);
    bool damaged[4] = {false, false, false, false};
    int kinds = 0;
    long long level = 0;
    for (int r = 0; r < nrows; ++r) {
        const long long* row = &rows[(size_t)r * JPG_PROG_FIELDS];
        CHECK(jpg_prog_row_ok(row, S, 1, H, W, nbytes, ntables, MAX_BYTES) && row[3] >= level);
        level = row[3];
        const int kind = (row[4] ? 2 : 0) + (row[6] ? 1 : 0);
        if (!damaged[kind] && row[2] >= 2) {
            damaged[kind] = true, ++kinds;
            const std::vector<uint8_t> good(stream.begin() + row[1], stream.begin() + row[1] + row[2]);
            int16_t* scratch = (int16_t*)malloc(ncoef * 2);
            CHECK(scratch);
            auto damage = [&](const std::vector<uint8_t>& v, uint32_t* pos, uint32_t* avail) {
                memcpy(scratch, coef, ncoef * 2);
                return run_row(row, stream.data(), raws.data(), S, W, scratch, &v, pos, avail);
            };
            for (size_t cut = 0; cut < 64 && cut < good.size(); ++cut) {   // truncations: never clean unless every bit was used
                if (cut + 1 == good.size() && cut > 0 && good[cut] == 0 && good[cut - 1] == 0xff) continue;   // only the stuffing
                uint32_t pos, avail;
                const int st = damage(std::vector<uint8_t>(good.begin(), good.begin() + cut), &pos, &avail);
                CHECK(st != 0 || pos == avail);
            }
            {
                const size_t cut = good.back() == 0 && good[good.size() - 2] == 0xff ? 2 : 1;
                uint32_t pos, avail;
                const int st = damage(std::vector<uint8_t>(good.begin(), good.end() - cut), &pos, &avail);
                CHECK(st != 0 || pos == avail);
            }
            for (int f = 0; f < 48; ++f) {   // single-bit flips: any outcome, within bounds
                std::vector<uint8_t> v = good;
                const size_t bit = rnd() % (v.size() * 8);
                v[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
                damage(v, nullptr, nullptr);
            }
            for (size_t tail : {size_t(1), size_t(2), size_t(17), good.size()}) {   // an all-FF tail
                std::vector<uint8_t> v = good;
                for (size_t k = v.size() - (tail < v.size() ? tail : v.size()); k < v.size(); ++k) v[k] = 0xff;
                damage(v, nullptr, nullptr);
            }
            free(scratch);
        }
        CHECK(run_row(row, stream.data(), raws.data(), S, W, coef) == 0);
    }
    CHECK(memcmp(coef, want.data(), ncoef * 2) == 0);
    free(coef);
    printf("%s: %d rows, %d scan kinds damaged\n", path, nrows, kinds);
}

static void raw_single(uint8_t* raw, uint8_t symbol) {   // one code, "0", for `symbol`
    memset(raw, 0, JPG_TABLE_BYTES);
    raw[0] = 1, raw[16] = symbol;
}

static void built_in() {
    // the block order of a one-component scan: 33 x 15 at 4:2:0 is 3 x 2 MCUs; luma walks 5 rows of 2 blocks (not 6), chroma 3 x 1
    CHECK(jpg_scan_units(JPG_420, -1, 33, 15) == 3 && jpg_scan_units(JPG_420, 0, 33, 15) == 10 && jpg_scan_units(JPG_420, 1, 33, 15) == 3);
    CHECK(jpg_scan_units(JPG_420, 0, 17, 33) == 15 && jpg_scan_units(JPG_420, 2, 17, 33) == 6 && jpg_scan_units(JPG_420, -1, 17, 33) == 6);
    CHECK(jpg_scan_units(JPG_422, 0, 17, 33) == 15 && jpg_scan_units(JPG_422, 1, 17, 33) == 9 && jpg_scan_units(JPG_422, -1, 17, 33) == 9);
    CHECK(jpg_scan_units(JPG_444, 2, 17, 33) == 15 && jpg_scan_units(JPG_GRAY, 0, 17, 33) == 15);
    {
        const long long luma[10] = {0, 1, 2, 3, 6, 7, 8, 9, 12, 13};   // MCU-major [3][6]: Y00 Y01 Y10 Y11 of each MCU row
        for (int u = 0; u < 10; ++u) CHECK(jpg_scan_block(JPG_420, 0, 0, u, 15) == luma[u]);
        for (int u = 0; u < 3; ++u) CHECK(jpg_scan_block(JPG_420, 1, 0, u, 15) == 6 * u + 4 && jpg_scan_block(JPG_420, 2, u, 0, 15) == 6 * u + 5);
        for (int i = 0; i < 18; ++i) CHECK(jpg_scan_block(JPG_420, -1, 1, i, 15) == 6 + i);
        // 17 x 33 at 4:2:2: 3 x 3 MCUs of 4 blocks, luma 3 rows of 5 blocks
        CHECK(jpg_scan_block(JPG_422, 0, 0, 4, 33) == 8 && jpg_scan_block(JPG_422, 0, 0, 5, 33) == 12 && jpg_scan_block(JPG_422, 2, 0, 8, 33) == 35);
        CHECK(jpg_scan_block(JPG_GRAY, 0, 3, 4, 33) == 7 && jpg_scan_block(JPG_444, 1, 0, 7, 33) == 22);
    }
    // rows jpg_prog_row_ok refuses: 16 x 16 at 4:2:0 is one MCU, four luma blocks; 64 stream bytes, one frame, two tables
    {
        const long long good[JPG_PROG_FIELDS] = {0, 0, 64, 0, 1, 5, 0, 2, 0, 0, 4, 1, 0, 0};
        CHECK(jpg_prog_row_ok(good, JPG_420, 1, 16, 16, 64, 2, MAX_BYTES));
        const struct { int field; long long value; } bad[] = {
            {0, 1}, {0, -1}, {1, 1}, {1, -1}, {2, 65}, {2, -1}, {3, -1}, {3, 256}, {4, 0}, {4, 6}, {4, -1}, {5, 64}, {6, 1}, {6, 2},
            {7, 14}, {7, -1}, {8, 3}, {8, -2}, {8, -1}, {9, 1}, {9, -1}, {10, 5}, {10, 0}, {11, 2}, {11, -1}};
        for (const auto& b : bad) {
            long long row[JPG_PROG_FIELDS];
            memcpy(row, good, sizeof row);
            row[b.field] = b.value;
            CHECK(!jpg_prog_row_ok(row, JPG_420, 1, 16, 16, 64, 2, MAX_BYTES));
        }
        const long long dc[JPG_PROG_FIELDS] = {0, 0, 64, 0, 0, 0, 0, 1, -1, 0, 1, 0, 1, 1};
        CHECK(jpg_prog_row_ok(dc, JPG_420, 1, 16, 16, 64, 2, MAX_BYTES) && !jpg_prog_row_ok(dc, JPG_GRAY, 1, 16, 16, 64, 2, MAX_BYTES));
        long long row[JPG_PROG_FIELDS];
        memcpy(row, dc, sizeof row), row[13] = 2;
        CHECK(!jpg_prog_row_ok(row, JPG_420, 1, 16, 16, 64, 2, MAX_BYTES));
        memcpy(row, dc, sizeof row), row[6] = 2, row[13] = 99;   // a DC refinement uses no table
        CHECK(jpg_prog_row_ok(row, JPG_420, 1, 16, 16, 64, 2, MAX_BYTES));
    }
    uint8_t raws[2 * JPG_TABLE_BYTES];
    int16_t* coef = (int16_t*)calloc(4 * 64, 2);   // gray 16 x 16: four blocks
    CHECK(coef);
    // an end-of-band run of category 14 (code "0", then fourteen 1-bits: 32 767 blocks) in a segment of four blocks
    raw_single(raws, 0xE0);
    {
        const std::vector<uint8_t> v = {0x7f, 0xfe};
        for (int ah = 0; ah < 2; ++ah) {
            const long long row[JPG_PROG_FIELDS] = {0, 0, 2, 0, 1, 63, ah ? 1 : 0, 0, 0, 0, 4, 0, 0, 0};
            CHECK(jpg_prog_row_ok(row, JPG_GRAY, 1, 16, 16, 2, 1, MAX_BYTES));
            CHECK(run_row(row, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_INDEX);
        }
        // category 2 with extra bits 00: a run of exactly four blocks fits
        raw_single(raws, 0x20);
        const std::vector<uint8_t> fits = {0x1f};
        const long long row[JPG_PROG_FIELDS] = {0, 0, 1, 0, 1, 63, 0, 0, 0, 0, 4, 0, 0, 0};
        CHECK(run_row(row, fits.data(), raws, JPG_GRAY, 16, coef) == 0);
        const std::vector<uint8_t> five = {0x3f};   // extra bits 01: five blocks
        CHECK(run_row(row, five.data(), raws, JPG_GRAY, 16, coef) == JPG_S_INDEX);
    }
    // a refinement symbol of size 2; a zero run that leaves the band in a first scan; a skip of 16 in a band of five
    {
        const std::vector<uint8_t> v = {0x00, 0x00};
        raw_single(raws, 0x02);
        const long long refine[JPG_PROG_FIELDS] = {0, 0, 2, 0, 1, 63, 1, 0, 0, 0, 4, 0, 0, 0};
        CHECK(run_row(refine, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_CODE);
        raw_single(raws, 0x71);
        const long long first[JPG_PROG_FIELDS] = {0, 0, 2, 0, 1, 5, 0, 0, 0, 0, 4, 0, 0, 0};
        CHECK(run_row(first, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_INDEX);
        const long long late[JPG_PROG_FIELDS] = {0, 0, 2, 0, 1, 5, 1, 0, 0, 0, 4, 0, 0, 0};
        CHECK(run_row(late, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_INDEX);
        raw_single(raws, 0xF0);
        CHECK(run_row(first, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_INDEX);
        CHECK(run_row(late, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_INDEX);
        raw_single(raws, 0x0C);   // a DC category above 11
        const long long dc[JPG_PROG_FIELDS] = {0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0};
        CHECK(run_row(dc, v.data(), raws, JPG_GRAY, 16, coef) == JPG_S_CODE);
    }
    // nonsense tables over random bytes, every scan kind, non-zero coefficients to correct: any outcome, within bounds
    for (int n = 0; n < 96; ++n) {
        for (int i = 0; i < 2 * JPG_TABLE_BYTES; ++i) raws[i] = (uint8_t)(n % 3 == 0 ? rnd() : rnd() % (i % JPG_TABLE_BYTES < 16 ? 4 : 256));
        for (int i = 0; i < 4 * 64; ++i) coef[i] = (int16_t)(rnd() % 3 == 0 ? (int)(rnd() % 65536) - 32768 : 0);
        std::vector<uint8_t> v(1 + rnd() % 200);
        for (auto& b : v) b = (uint8_t)rnd();
        const int kind = n % 4, al = (int)(rnd() % 14);
        const int ss = kind < 2 ? 0 : 1 + (int)(rnd() % 63), se = kind < 2 ? 0 : ss + (int)(rnd() % (64 - ss));
        const long long row[JPG_PROG_FIELDS] = {0, 0, (long long)v.size(), 0, ss, se, kind & 1 ? al + 1 : 0, al, 0, 0, 4, 1, 0, 0};
        CHECK(jpg_prog_row_ok(row, JPG_GRAY, 1, 16, 16, (long long)v.size(), 2, MAX_BYTES));
        run_row(row, v.data(), raws, JPG_GRAY, 16, coef);
    }
    free(coef);
}

int main(int argc, char** argv) {
    built_in();
    for (int i = 1; i < argc; ++i) run_case(argv[i]);
    printf("%d streams:", cases);
    for (int s = 0; s < 64; ++s)
        if (counts[s]) printf(" status %d x %d", s, counts[s]);
    printf("\nok\n");
    return 0;
}
