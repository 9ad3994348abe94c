// inflate_host.cpp -- dino_tracker_amd/csrc/inflate_core.h on the CPU, for the sanitisers (tests/test_png_reference.py builds it with
// -fsanitize=address,undefined).  The stream-level logic -- bit reader, zlib header, code lengths, tables, tokens -- is the header's,
// the same lines the kernel runs; what is written here is the part that differs on the device: one thread, the whole stream
// readable at once, output into a plain buffer of exactly the expected size.
//
// usage: inflate_host CASE...   a case file is "INFC", int32 wrapper, int64 expected bytes (little-endian), then the stream.
// One line per case: status, CRC-32 of the output (expected bytes: what was decoded, then zeros), the longest code seen.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../dino_tracker_amd/csrc/inflate_core.h"

static uint32_t crc32_of(const std::vector<uint8_t>& d) {
    uint32_t c = 0xffffffffu;
    for (uint8_t v : d) {
        c ^= v;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

struct Tables {
    InfLitCode lit;
    InfDistCode dist;
    InfClenCode clen;
    uint8_t lens[INF_MAX_LENS];
};

static int inflate_stream(const std::vector<uint8_t>& in, int wrapper, std::vector<uint8_t>& out, int& longest) {
    // exactly the words that hold the bytes, the last one zero-filled: the sanitiser sees any read beyond them
    std::vector<uint32_t> words((in.size() + 3) / 4, 0u);
    if (!in.empty()) memcpy(words.data(), in.data(), in.size());
    std::vector<Tables> tables(1);
    Tables& t = tables[0];
    InfBits b;
    inf_bits_start(b, words.data(), (uint32_t)words.size(), (uint32_t)in.size() * 8u, 0u);
    size_t opos = 0;
    if (wrapper)
        if (int st = inf_zlib_header(b)) return st;
    for (bool last = false; !last;) {
        last = inf_take(b, 1) != 0u;
        const uint32_t type = inf_take(b, 2);
        if (inf_over(b)) return INF_S_OVERRUN;
        if (type == 3u) return INF_S_BTYPE;
        if (type == 0u) {
            inf_consume(b, (int)((8u - (b.pos & 7u)) & 7u));
            const uint32_t n = inf_take(b, 16), nn = inf_take(b, 16);
            if (inf_over(b)) return INF_S_OVERRUN;
            if ((n ^ nn) != 0xffffu) return INF_S_STORED;
            if (n > out.size() - opos) return INF_S_LENGTH;
            const size_t at = b.pos >> 3, have = in.size() > at ? in.size() - at : 0, m = n < have ? n : have;
            for (size_t i = 0; i < m; ++i) out[opos + i] = in[at + i];
            opos += m;
            if (m < n) return INF_S_OVERRUN;
            inf_bits_start(b, words.data(), (uint32_t)words.size(), (uint32_t)in.size() * 8u, b.pos + 8u * (uint32_t)m);
            continue;
        }
        int hlit = 288, hdist = 32;
        if (type == 1u) inf_fixed_lens(t.lens, 0, 1);
        else if (int st = inf_read_dynamic(b, &t.clen, t.lens, hlit, hdist)) return st;
        inf_code_clear(&t.lit, 0, 1);
        inf_code_clear(&t.dist, 0, 1);
        const int st_lit = inf_code_sort(t.lens, hlit, INF_KIND_LITLEN, &t.lit), st_dist = inf_code_sort(t.lens + hlit, hdist, INF_KIND_DIST, &t.dist);
        if (st_lit | st_dist) return st_lit | st_dist;
        inf_code_fill(t.lens, &t.lit, 0, 1);
        inf_code_fill(t.lens + hlit, &t.dist, 0, 1);
        if (t.lit.maxlen > longest) longest = t.lit.maxlen;
        while (true) {
            int mlen = 0, mdist = 0, st = 0;
            const int tok = inf_token(b, t.lit, t.dist, mlen, mdist, st);
            if (tok >= 0) {
                if (opos >= out.size()) return INF_S_LENGTH;
                out[opos++] = (uint8_t)tok;
            } else if (tok == INF_TOKEN_MATCH) {
                if ((size_t)mdist > opos) return INF_S_DISTANCE;
                if ((size_t)mlen > out.size() - opos) return INF_S_LENGTH;
                for (int i = 0; i < mlen; ++i, ++opos) out[opos] = out[opos - (size_t)mdist];
            } else if (tok == INF_TOKEN_EOB) {
                break;
            } else {
                return st;
            }
        }
    }
    if (opos != out.size()) return INF_S_LENGTH;
    if (wrapper && (long long)in.size() - (long long)((b.pos + 7u) >> 3) < 4) return INF_S_OVERRUN;
    return 0;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* fh = fopen(argv[a], "rb");
        if (!fh) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t chunk[4096];
        for (size_t n; (n = fread(chunk, 1, sizeof chunk, fh)) > 0;) file.insert(file.end(), chunk, chunk + n);
        fclose(fh);
        if (file.size() < 16 || memcmp(file.data(), "INFC", 4) != 0) {
            fprintf(stderr, "%s is not a case file\n", argv[a]);
            return 2;
        }
        int32_t wrapper;
        int64_t expected;
        memcpy(&wrapper, file.data() + 4, 4);
        memcpy(&expected, file.data() + 8, 8);
        if (expected < 0 || expected > (1ll << 30)) return 2;
        const std::vector<uint8_t> in(file.begin() + 16, file.end());
        std::vector<uint8_t> out((size_t)expected, 0);
        int longest = 0;
        const int status = inflate_stream(in, wrapper, out, longest);
        printf("%d %08x %d\n", status, crc32_of(out), longest);
    }
    return 0;
}
