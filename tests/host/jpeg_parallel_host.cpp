// A stand-alone HOST program around the sub-stream functions of dino_tracker_amd/csrc/jpeg_entropy.h (docs/JPEG_DECODE.md section
// 1b): built by tests/test_jpeg_parallel_reference.py with -fsanitize=address,undefined and run directly (never loaded into Python).
// It runs the functions the kernel in csrc/jpeg_parallel.hip runs -- the jpg_step chain to its fixpoint, the counts and their scan,
// the strict pass, the DC sums, the redo rule -- one sub-stream after the other (jpg_decode_segment_substreams), and requires the
// coefficients AND the status of jpg_decode_mcus with the sequential end check, for sub-streams of 16, 32 and 128 bytes.  For
// B = 1, 3, 4, 6 blocks per MCU: a seeded valid segment of 5 MCUs with a different pair of tables per component; truncations at each
// of the first 64 byte positions and before the last byte; 128 single-bit flips; all-FF tails; the valid bytes under nonsense tables;
// a segment whose DC predictor wraps around int16.  Every buffer has exactly the size the decoder is entitled to; the loop bounds --
// at most (sub-streams + 1) sweeps, every walk at most 8 x bytes steps -- are asserted for every stream.
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

static uint32_t rng_state = 2025u;
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

static long long max_rounds = 0, redone = 0;

// Both decoders over one segment, from buffers of exactly the entitled size; returns the status both gave.
static int decode_both(const uint8_t* raw, size_t len, int B, int nm, const JpgHuff* tab, int L, std::vector<int16_t>& got) {
    std::vector<uint8_t> un;
    for (size_t i = 0; i < len; ++i)
        if (!(raw[i] == 0 && i > 0 && raw[i - 1] == 0xff)) un.push_back(raw[i]);
    const uint32_t avail = (uint32_t)un.size() * 8u;
    const size_t nwords = (avail + 31) / 32 + 1;   // what the reader may touch
    uint32_t* words = (uint32_t*)calloc(nwords, 4);
    CHECK(words);
    if (!un.empty()) memcpy(words, un.data(), un.size());
    const size_t ncoef = (size_t)nm * B * 64;

    int16_t* want = (int16_t*)calloc(ncoef, sizeof(int16_t));
    uint32_t iters = 0;
    const int st_want = jpg_decode_segment_sequential(words, avail, tab, B, nm, want, iters);

    const uint32_t n = jpg_substreams((uint32_t)un.size(), L);
    unsigned long long* states = (unsigned long long*)malloc(n * sizeof(unsigned long long));
    int32_t* counts = (int32_t*)malloc(n * sizeof(int32_t));
    int16_t* coef = (int16_t*)calloc(ncoef, sizeof(int16_t));
    CHECK(states && counts && coef && want);
    uint32_t rounds = 0;
    iters = 0;
    const int st = jpg_decode_segment_substreams(words, (uint32_t)un.size(), tab, B, nm, L, states, counts, coef, rounds, iters);
    CHECK(st == st_want);
    CHECK(memcmp(coef, want, ncoef * sizeof(int16_t)) == 0);
    // the loop bounds: sweeps by the number of sub-streams; a walk, a count or a strict pass over the segment takes a step per bit
    // at most, and the redo the sequential bound
    CHECK(rounds >= 1 && rounds <= n + 1);
    CHECK((uint64_t)iters <= ((uint64_t)rounds * n + 2u) * (8ull * un.size() + 8u) + 64ull * B * (uint64_t)nm);
    if (rounds > max_rounds) max_rounds = rounds;
    redone += st != 0;
    got.assign(coef, coef + ncoef);
    free(coef), free(counts), free(states), free(want), free(words);
    return st;
}

int main() {
    const int samplings[4] = {JPG_GRAY, JPG_444, JPG_422, JPG_420}, blocks[4] = {1, 3, 4, 6};
    const int want_comp[4][6] = {{0}, {0, 1, 2}, {0, 0, 1, 2}, {0, 0, 0, 0, 1, 2}};
    const int subseq[3] = {16, 32, 128};
    CHECK(jpg_subseq_ok(16) && jpg_subseq_ok(1024) && jpg_subseq_ok(JPG_SUBSEQ_DEFAULT) && !jpg_subseq_ok(0) && !jpg_subseq_ok(12) &&
          !jpg_subseq_ok(18) && !jpg_subseq_ok(1028) && !jpg_subseq_ok(-16));
    {   // a state survives packing
        JpgState s;
        s.p = 0x89abcdefu, s.c = 5, s.k = 63;
        const JpgState t = jpg_state_unpack(jpg_state_pack(s));
        CHECK(t.p == s.p && t.c == s.c && t.k == s.k);
    }

    // per component its own tables: Annex K's luma DC counts over rotated symbol lists, and AC tables with Annex K's luma counts over
    // rotated lists of all 162 symbols
    const int dc_counts[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    const int ac_counts[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
    std::vector<uint8_t> acv;
    acv.push_back(0x00), acv.push_back(0xF0);
    for (int s = 1; s <= 10; ++s)
        for (int r = 0; r < 16; ++r) acv.push_back((uint8_t)((r << 4) | s));
    CHECK(acv.size() == 162);
    Raw raws[6];
    for (int c = 0; c < 3; ++c) {
        std::vector<uint8_t> d, a;
        for (int i = 0; i < 12; ++i) d.push_back((uint8_t)((i + 5 * c) % 12));
        for (size_t i = 0; i < acv.size(); ++i) a.push_back(acv[(i + 37 * c) % acv.size()]);
        raws[2 * c] = raw_table(dc_counts, d), raws[2 * c + 1] = raw_table(ac_counts, a);
    }
    Codes codes[6];
    for (int t = 0; t < 6; ++t) codes[t] = codes_of(raws[t]);

    int cases = 0, counts[64] = {0};
    const int nm = 5;
    for (int i = 0; i < 4; ++i) {
        const int B = blocks[i], NT = 2 * jpg_components(samplings[i]);
        JpgHuff* tab = (JpgHuff*)malloc((size_t)NT * sizeof(JpgHuff));   // gray: exactly two
        CHECK(tab);
        for (int t = 0; t < NT; ++t) {
            jpg_huff_clear(&tab[t], 0, 1);
            jpg_huff_fill(raws[t].b, &tab[t], 0, 1);
        }
        std::vector<int16_t> want((size_t)nm * B * 64, 0);
        Sink sink;
        int pred[3] = {0, 0, 0};
        for (int b = 0; b < nm * B; ++b) {
            int16_t* z = &want[(size_t)b * 64];
            const int comp = want_comp[i][b % B];
            z[0] = (int16_t)((int)(rnd() % 2049) - 1024);
            const int density = b % 5;   // 0: DC only ... 4: dense, with long runs (ZRL) in between
            for (int k = 1; k < 64; ++k)
                if (density && rnd() % (density == 1 ? 40 : 6 - density) == 0) {
                    const int size = 1 + (int)(rnd() % 10);
                    z[k] = (int16_t)((int)(rnd() % (2u << size)) - (1 << size));
                    if (z[k] > 1023) z[k] = 1023;
                    if (z[k] < -1023) z[k] = -1023;
                }
            if (b == 2) memset(z + 1, 0, 63 * 2), z[63] = -1023;   // three ZRLs, then a run of 14 to the last coefficient: no EOB
            const int diff = z[0] - pred[comp];
            pred[comp] = z[0];
            const Codes &dcc = codes[2 * comp], &acc = codes[2 * comp + 1];
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
        std::vector<int16_t> got;
        auto run = [&](const std::vector<uint8_t>& bytes, const JpgHuff* tables) {
            int st = 0;
            for (int L : subseq) {
                uint8_t* seg = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);   // exact-size copies: a read beyond is seen
                if (!bytes.empty()) memcpy(seg, bytes.data(), bytes.size());
                st = decode_both(seg, bytes.size(), B, nm, tables, L, got);
                free(seg);
                ++counts[st & 63], ++cases;
            }
            return st;
        };
        CHECK(good.size() > 64);
        CHECK(run(good, tab) == 0);
        CHECK(memcmp(got.data(), want.data(), want.size() * sizeof(int16_t)) == 0);
        for (size_t cut = 0; cut < 64; ++cut)   // truncations: never clean
            CHECK(run(std::vector<uint8_t>(good.begin(), good.begin() + cut), tab) != 0);
        {   // without its last data byte (a stuffed 00 behind an FF is none: cut both)
            const size_t cut = good.size() >= 2 && good.back() == 0 && good[good.size() - 2] == 0xff ? 2 : 1;
            CHECK(run(std::vector<uint8_t>(good.begin(), good.end() - cut), tab) != 0);
        }
        for (int f = 0; f < 128; ++f) {   // single-bit flips: any outcome, the same from both decoders
            std::vector<uint8_t> v = good;
            const size_t bit = rnd() % (v.size() * 8);
            v[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
            run(v, tab);
        }
        for (size_t tail : {size_t(1), size_t(2), size_t(17), good.size()}) {   // an all-FF tail
            std::vector<uint8_t> v = good;
            for (size_t k = v.size() - tail; k < v.size(); ++k) v[k] = 0xff;
            run(v, tab);
        }
        {   // the tail as a marker would leave it: data, then FF bytes appended
            std::vector<uint8_t> v = good;
            v.insert(v.end(), 9, 0xff);
            CHECK(run(v, tab) == JPG_S_LEFTOVER);
        }
        for (int t = 0; t < 16; ++t) {   // nonsense tables: random counts (over-subscribed lengths among them) and symbols
            JpgHuff* bad = (JpgHuff*)malloc((size_t)NT * sizeof(JpgHuff));
            CHECK(bad);
            for (int u = 0; u < NT; ++u) {
                Raw r;
                for (int k = 0; k < JPG_TABLE_BYTES; ++k) r.b[k] = (uint8_t)rnd();
                if (t & 1)
                    for (int k = 0; k < 16; ++k) r.b[k] = (uint8_t)(r.b[k] & 7);
                jpg_huff_clear(&bad[u], 0, 1);
                jpg_huff_fill(r.b, &bad[u], 0, 1);
            }
            run(good, bad);
            free(bad);
        }
        {   // twenty blocks per component of DC difference +2047: the predictors wrap around int16, in both decoders alike
            Sink s2;
            const int n2 = 20;
            for (int b = 0; b < n2 * B; ++b) {
                const int comp = want_comp[i][b % B];
                put_value(s2, codes[2 * comp], 11, 2047, 11);
                put_value(s2, codes[2 * comp + 1], 0x00, 0, 0);
            }
            s2.finish();
            for (int L : subseq) {
                CHECK(decode_both(s2.out.data(), s2.out.size(), B, n2, tab, L, got) == 0);
                CHECK(got[(size_t)(n2 * B - 1) * 64] == (int16_t)(2047 * n2));
                CHECK(2047 * n2 > 32767);
                ++counts[0], ++cases;
            }
        }
        free(tab);
    }
    printf("%d streams (%lld redone sequentially, at most %lld sweeps):", cases, redone, max_rounds);
    for (int s = 0; s < 64; ++s)
        if (counts[s]) printf(" status %d x %d", s, counts[s]);
    printf("\nok\n");
    return 0;
}
