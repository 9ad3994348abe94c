// A stand-alone HOST program around dino_tracker_amd/csrc/jpeg_entropy.h, the decode loop the device kernel runs: built by
// tests/test_jpeg_decode_reference.py with -fsanitize=address,undefined and run directly (never loaded into Python).
//
//   jpeg_entropy_host                 a fixed, seeded list of streams: a valid one (decoded coefficients must equal what was coded),
//                                     then damaged ones -- truncated at each of the first 64 byte positions and one byte before the
//                                     end, 256 single-bit flips, an all-FF tail, random bytes -- with Annex K's DC table and an AC
//                                     table whose longest codes have 16 bits.
//   jpeg_entropy_host FILE...         case files written by the tests: 6 raw tables of 272 bytes (component x DC / AC), int32 MCU
//                                     count (little endian), the segment's raw bytes.  Prints "status iterations fnv1a(coefficients)".
//
// Every buffer is allocated at exactly the size the decoder is entitled to, so the sanitiser sees any access beyond it, and the
// iteration bound of docs/JPEG_DECODE.md section 5 is asserted for every stream.
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

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

struct Raw {
    uint8_t b[JPG_TABLE_BYTES];
};
static Raw raw_table(const int* counts, const std::vector<uint8_t>& vals) {
    Raw r;
    memset(r.b, 0, sizeof r.b);
    for (int i = 0; i < 16; ++i) r.b[i] = (uint8_t)counts[i];
    memcpy(r.b + 16, vals.data(), vals.size());
    return r;
}

// the whole segment: unstuff, decode nm MCUs, classify the end.  coef: exactly nm * 6 * 64 values.
static int decode_segment(const uint8_t* raw, size_t len, int nm, const JpgHuff* tab, int16_t* coef, uint32_t* iters_out) {
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
    int pred[3] = {0, 0, 0}, st = 0;
    uint32_t iters = 0;
    memset(coef, 0, (size_t)nm * 6 * 64 * sizeof(int16_t));
    for (int b = 0; b < nm * 6 && !st; ++b) {
        const int comp = b % 6 < 4 ? 0 : b % 6 - 3;
        st |= jpg_decode_block(bits, tab[2 * comp], tab[2 * comp + 1], pred[comp], coef + (size_t)b * 64, iters);
    }
    if (!st) {
        if (bits.pos > avail) st |= JPG_S_OVERRUN;
        else if (avail - bits.pos > 7u) st |= JPG_S_LEFTOVER;
    }
    free(words);
    CHECK((uint64_t)iters <= 8ull * len + 64ull * 6 * (uint64_t)nm);   // the documented bound
    CHECK((uint64_t)iters <= 64ull * 6 * (uint64_t)nm);                // and the tighter one the loop's shape gives
    *iters_out = iters;
    return st;
}

static void build(const Raw* raws, JpgHuff* tab) {
    for (int t = 0; t < 6; ++t) {
        jpg_huff_clear(&tab[t], 0, 1);
        jpg_huff_fill(raws[t].b, &tab[t], 0, 1);
    }
}

// ---- a small encoder for the fixed list -------------------------------------------------------------------------------------------
struct Codes {
    uint32_t code[256];
    int len[256];
};
static Codes codes_of(const Raw& r) {
    Codes c;
    memset(&c, 0, sizeof c);
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < r.b[len - 1]; ++i, ++k) c.code[r.b[16 + k]] = code++, c.len[r.b[16 + k]] = len;
        code <<= 1;
    }
    return c;
}
struct Sink {
    std::vector<uint8_t> out;
    uint64_t acc = 0;
    int held = 0;
    void put(uint32_t v, int n) {
        for (int i = n - 1; i >= 0; --i) {
            acc = (acc << 1) | ((v >> i) & 1u);
            if (++held == 8) {
                out.push_back((uint8_t)acc);
                if ((uint8_t)acc == 0xff) out.push_back(0);
                acc = 0, held = 0;
            }
        }
    }
    void finish() {
        while (held) put(1, 1);
    }
};
static int size_of(int v) {
    int a = v < 0 ? -v : v, s = 0;
    while (a) ++s, a >>= 1;
    return s;
}
static void put_value(Sink& s, const Codes& c, int sym, int v, int size) {
    CHECK(c.len[sym] > 0);
    s.put(c.code[sym], c.len[sym]);
    if (size) s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u), size);
}

static uint32_t fnv(const int16_t* p, size_t n) {
    uint32_t h = 2166136261u;
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < 2 * n; ++i) h = (h ^ b[i]) * 16777619u;
    return h;
}

static int run_file(const char* path) {
    FILE* fh = fopen(path, "rb");
    CHECK(fh);
    std::vector<uint8_t> data;
    uint8_t chunk[4096];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, fh)) > 0) data.insert(data.end(), chunk, chunk + n);
    fclose(fh);
    CHECK(data.size() >= 6 * JPG_TABLE_BYTES + 4);
    Raw raws[6];
    for (int t = 0; t < 6; ++t) memcpy(raws[t].b, data.data() + t * JPG_TABLE_BYTES, JPG_TABLE_BYTES);
    int32_t nm;
    memcpy(&nm, data.data() + 6 * JPG_TABLE_BYTES, 4);
    CHECK(nm >= 1 && nm <= (1 << 20));
    JpgHuff* tab = (JpgHuff*)malloc(6 * sizeof(JpgHuff));
    build(raws, tab);
    const size_t head = 6 * JPG_TABLE_BYTES + 4, len = data.size() - head;
    uint8_t* seg = (uint8_t*)malloc(len ? len : 1);   // an exact-size copy: reads beyond the segment are seen
    if (len) memcpy(seg, data.data() + head, len);
    int16_t* coef = (int16_t*)malloc((size_t)nm * 6 * 64 * sizeof(int16_t));
    uint32_t iters;
    const int st = decode_segment(seg, len, nm, tab, coef, &iters);
    printf("%d %u %08x\n", st, iters, fnv(coef, (size_t)nm * 6 * 64));
    free(coef), free(seg), free(tab);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i < argc; ++i) run_file(argv[i]);
        return 0;
    }
    // Annex K's luma DC table; an AC table with Annex K's luma counts (the longest 125 codes have 16 bits) over all 162 symbols
    const int dc_counts[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    const int ac_counts[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
    std::vector<uint8_t> dcv, acv;
    for (int i = 0; i < 12; ++i) dcv.push_back((uint8_t)i);
    acv.push_back(0x00), acv.push_back(0xF0);
    for (int s = 1; s <= 10; ++s)
        for (int r = 0; r < 16; ++r) acv.push_back((uint8_t)((r << 4) | s));
    CHECK(acv.size() == 162);
    Raw raws[6];
    for (int c = 0; c < 3; ++c) raws[2 * c] = raw_table(dc_counts, dcv), raws[2 * c + 1] = raw_table(ac_counts, acv);
    JpgHuff* tab = (JpgHuff*)malloc(6 * sizeof(JpgHuff));
    build(raws, tab);
    const Codes dcc = codes_of(raws[0]), acc = codes_of(raws[1]);

    const int nm = 5;
    std::vector<int16_t> want((size_t)nm * 6 * 64, 0);
    Sink sink;
    int pred[3] = {0, 0, 0};
    for (int b = 0; b < nm * 6; ++b) {
        int16_t* z = &want[(size_t)b * 64];
        const int comp = b % 6 < 4 ? 0 : b % 6 - 3;
        z[0] = (int16_t)((int)(rnd() % 2049) - 1024);
        const int density = b % 5;   // 0: DC only ... 4: dense, with long runs (ZRL) in between
        for (int k = 1; k < 64; ++k)
            if (density && rnd() % (density == 1 ? 40 : 6 - density) == 0) {
                const int size = 1 + (int)(rnd() % 10);
                z[k] = (int16_t)((int)(rnd() % (2u << size)) - (1 << size));
                if (z[k] > 1023) z[k] = 1023;
                if (z[k] < -1023) z[k] = -1023;
            }
        if (b == 7) memset(z + 1, 0, 63 * 2), z[63] = -1023;   // three ZRLs, then a run of 14 to the last coefficient: no EOB
        const int diff = z[0] - pred[comp];
        pred[comp] = z[0];
        put_value(sink, dcc, size_of(diff), diff, size_of(diff));
        int run = 0;
        for (int k = 1; k < 64; ++k) {
            if (!z[k]) {
                ++run;
                continue;
            }
            for (; run > 15; run -= 16) put_value(sink, acc, 0xF0, 0, 0);
            put_value(sink, acc, (run << 4) | size_of(z[k]), z[k], size_of(z[k]));
            run = 0;
        }
        if (run) put_value(sink, acc, 0x00, 0, 0);
    }
    sink.finish();
    const std::vector<uint8_t> good = sink.out;
    std::vector<int16_t> got((size_t)nm * 6 * 64);
    uint32_t iters;
    int counts[64] = {0}, cases = 0;

    auto run = [&](const std::vector<uint8_t>& bytes) {
        uint8_t* seg = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
        if (!bytes.empty()) memcpy(seg, bytes.data(), bytes.size());
        int16_t* coef = (int16_t*)malloc(got.size() * sizeof(int16_t));
        const int st = decode_segment(seg, bytes.size(), nm, tab, coef, &iters);
        memcpy(got.data(), coef, got.size() * sizeof(int16_t));
        free(coef), free(seg);
        ++counts[st & 63], ++cases;
        return st;
    };
    CHECK(run(good) == 0);
    CHECK(memcmp(got.data(), want.data(), want.size() * sizeof(int16_t)) == 0);
    for (size_t cut = 0; cut < 64 && cut < good.size(); ++cut)   // truncations: never clean
        CHECK(run(std::vector<uint8_t>(good.begin(), good.begin() + cut)) != 0);
    CHECK(run(std::vector<uint8_t>(good.begin(), good.end() - 1)) != 0);
    for (int i = 0; i < 256; ++i) {   // single-bit flips: any outcome, within bounds
        std::vector<uint8_t> v = good;
        const size_t bit = rnd() % (v.size() * 8);
        v[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
        run(v);
    }
    for (size_t tail : {size_t(1), size_t(2), size_t(17), good.size()}) {   // an all-FF tail
        std::vector<uint8_t> v = good;
        for (size_t i = v.size() - tail; i < v.size(); ++i) v[i] = 0xff;
        run(v);
    }
    {   // the tail as a marker would leave it: data, then FF bytes appended
        std::vector<uint8_t> v = good;
        v.insert(v.end(), 9, 0xff);
        CHECK(run(v) == JPG_S_LEFTOVER);
    }
    for (int i = 0; i < 64; ++i) {   // random bytes of random lengths
        std::vector<uint8_t> v(rnd() % 700);
        for (auto& x : v) x = (uint8_t)rnd();
        run(v);
    }
    {   // tables the caller should never pass: over-subscribed counts, all-zero counts -- memory-safe all the same
        Raw bad[6];
        memset(bad, 0xff, sizeof bad);
        JpgHuff* t2 = (JpgHuff*)malloc(6 * sizeof(JpgHuff));
        build(bad, t2);
        JpgHuff* keep = tab;
        tab = t2;
        run(good);
        memset(bad, 0, sizeof bad);
        build(bad, t2);
        CHECK(run(good) == JPG_S_CODE);
        tab = keep;
        free(t2);
    }
    free(tab);
    printf("%d streams:", cases);
    for (int s = 0; s < 64; ++s)
        if (counts[s]) printf(" status %d x %d", s, counts[s]);
    printf("\nok\n");
    return 0;
}
