// jpeg_parallel.hip -- video ingest: the entropy stage of a baseline JPEG segment decoded by MANY lanes (docs/JPEG_DECODE.md section
// 1b; Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018).  jpeg_decode.hip's entropy kernel walks a
// segment with one lane, which is all a file without restart markers offers it: one lane per frame.  Here the unstuffed bytes of a
// segment are cut into sub-streams of L bytes, every sub-stream starts decoding from a guess, and the entry states are iterated to
// their fixpoint -- the sequential decoder's own states, whether or not a guess ever synchronises.  Output: the coefficients and the
// status of dtk_jpeg_decode_coefficients_sampled for any bytes; a segment whose strict pass reports anything is decoded again by the
// sequential loop, so the equality on damaged streams holds by construction.
//
// ONE WORKGROUP PER SEGMENT, no protocol between workgroups, no host synchronisation.  1 024 lanes: the work is a chain of dependent
// table look-ups per lane (LDS latency, no arithmetic to speak of), so what helps is lanes in flight -- 16 waves are the most a CU
// holds for one workgroup, four per SIMD, which caps a lane at 128 VGPRs (the decode step needs far fewer), and the 8.5 KiB of
// look-ups are built once for all of them.  A frame folder gives tens of segments to 256 CUs: one workgroup per CU, so occupancy per CU
// is this workgroup's own.  Lane t owns sub-streams t, t + 1024, ...
//
// Phases (a barrier between each): zero the segment's coefficients and build the look-ups; unstuff the bytes into the workspace;
// speculate and iterate the states; count the blocks that start in each sub-stream and scan; the strict write pass; the DC sums;
// the end check; the sequential redo when the status is not zero.
//
// Safety (docs/JPEG_DECODE.md section 5): the segment-table checks are jpeg_entropy_kernel's; the segment's places in the workspace
// are checked against the workspace's size; every store of the write pass goes through jpg_write_substream's block-range check
// against the segment's own MCU range; the reader checks every word index against the unstuffed length; the scan's block indices are
// clamped.  Loop bounds: the sweep over the states runs at most (sub-streams + 1) times, a lane's walk in one sweep covers at most 32 sub-streams and
// so takes at most 8 x 32 x L steps (every step consumes a bit), every other loop is counted by bytes, sub-streams or blocks.
#include "block_scan.h"
#include "common.h"
#include "jpeg_entropy.h"

namespace {

constexpr int PT = 1024, PWAVES = PT / WAVE;   // lanes, waves of a workgroup
constexpr int UCH = 8;                         // raw bytes a lane unstuffs per round
// How far a lane carries a state on in one sweep.  Guesses that merge do so within a few sub-streams (p99 4.8, longest 8.6 on a real
// frame at 128 bytes), so the cap does not bind there; on a stream whose guesses never merge it keeps a sweep's work at WALK_MAX
// sub-streams per owned one instead of the rest of the segment, for n / WALK_MAX sweeps instead of a few.
constexpr uint32_t WALK_MAX = 32;
constexpr int SEG_FIELDS = DTK_JPEG_SEGMENT_FIELDS;
constexpr long long SEG_MAX_BYTES = 1ll << 28;   // bit positions are 32-bit
constexpr int SEG_PAD = 16;                      // workspace bytes per segment beyond its length: alignment to a word and the reader's zeros

// Where segment s (byte range [off, off + len) of the stream) lives in the workspace.  For segments whose byte ranges do not overlap
// and rise with s -- what the library requires of the host table -- the places are disjoint.
__host__ __device__ inline long long ws_byte_at(long long off, long long s) { return (off + SEG_PAD * s + 3) & ~3ll; }
__host__ __device__ inline long long ws_slot_at(long long off, long long s, int L) { return off / L + 2 * s; }
__host__ __device__ inline long long ws_bytes_cap(long long stream_bytes, long long nseg) { return (stream_bytes + SEG_PAD * (nseg + 1) + 255) & ~255ll; }
__host__ __device__ inline long long ws_slots_cap(long long stream_bytes, long long nseg, int L) { return (stream_bytes / L + 2 * nseg + 2 + 31) & ~31ll; }

__device__ __forceinline__ unsigned long long state_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void state_store(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// grid (segments), PT lanes each.  segs, huff, coef, status as jpeg_entropy_kernel's.  ws_bytes [bytes_cap]: unstuffed bytes;
// ws_states, ws_counts [slots_cap]: a state and a count per sub-stream.
template <int S>
__global__ __launch_bounds__(PT) void jpeg_parallel_kernel(const uint8_t* __restrict__ stream, long long stream_bytes,
                                                           const long long* __restrict__ segs, int nseg,
                                                           const uint8_t* __restrict__ huff, int F, int mcus, int L,
                                                           int16_t* __restrict__ coef, int* __restrict__ status, uint8_t* ws_bytes,
                                                           unsigned long long* ws_states, int* ws_counts) {
    constexpr int B = jpg_blocks_per_mcu(S), NT = 2 * jpg_components(S);
    __shared__ JpgHuff tab[NT];
    __shared__ int flag;             // a sweep changed a state
    __shared__ int seg_status;       // the strict pass's status bits
    __shared__ uint32_t seg_end[2];  // ended, the bit position behind the last block
    const int tid = threadIdx.x;
    const long long sidx = blockIdx.x;
    const long long* sg = segs + (size_t)sidx * SEG_FIELDS;
    const long long f = sg[0], off = sg[1], len = sg[2], m0 = sg[3], nm = sg[4];
    if (f < 0 || f >= F) return;
    const long long at = ws_byte_at(off, sidx), slot = ws_slot_at(off < 0 ? 0 : off, sidx, L);
    if (off < 0 || len < 0 || len > SEG_MAX_BYTES || off > stream_bytes - len || m0 < 0 || nm < 1 || m0 > mcus - nm ||
        at + len + SEG_PAD - 4 > ws_bytes_cap(stream_bytes, nseg) || slot + len / L + 2 > ws_slots_cap(stream_bytes, nseg, L)) {
        if (tid == 0) atomicOr(&status[f], JPG_S_SEGMENT);
        return;
    }
    const int nb = (int)nm * B;
    int16_t* out = coef + ((size_t)f * mcus + m0) * B * 64;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    const size_t nwords_out = (size_t)nb * 32;

    // ---- 0 / 1: the segment's coefficients are zero; the frame's look-ups stand in LDS
    for (size_t i = tid; i < nwords_out; i += PT) out32[i] = 0u;
    for (int t = 0; t < NT; ++t) jpg_huff_clear(&tab[t], tid, PT);
    if (tid == 0) flag = 0, seg_status = 0, seg_end[0] = 0u, seg_end[1] = 0u;
    __syncthreads();
    for (int t = 0; t < NT; ++t) jpg_huff_fill(huff + ((size_t)f * NT + t) * JPG_TABLE_BYTES, &tab[t], tid, PT);

    // ---- 2: unstuff.  A byte is dropped when it is 00 behind FF; the scan of the lanes' kept counts plus the running offset places
    // the rest.  len / (PT * UCH) + 1 rounds.
    const uint8_t* src = stream + off;
    uint8_t* bytes = ws_bytes + at;
    long long fill = 0;
    for (long long base = 0; base < len; base += (long long)PT * UCH) {
        const long long i0 = base + (long long)tid * UCH;
        unsigned v[UCH], keep = 0u;
        unsigned prev = i0 > 0 && i0 - 1 < len ? src[i0 - 1] : 0u;
#pragma unroll
        for (int j = 0; j < UCH; ++j) {
            v[j] = i0 + j < len ? src[i0 + j] : 0u;
            if (i0 + j < len && !(v[j] == 0u && prev == 0xffu)) keep |= 1u << j;
            prev = v[j];
        }
        int total;
        long long to = fill + block_scan_excl<PWAVES>((int)__popc(keep), total);
#pragma unroll
        for (int j = 0; j < UCH; ++j)
            if (keep >> j & 1u) bytes[to++] = (uint8_t)v[j];
        fill += total;
    }
    // the zeros JpgBits expects: up to the word after the one that holds the last bit
    if (tid < SEG_PAD - 4 && fill + tid < ((fill + 3) & ~3ll) + 4) bytes[fill + tid] = 0;
    const uint32_t unstuffed = (uint32_t)fill, avail = unstuffed * 8u, n = jpg_substreams(unstuffed, L);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(bytes);
    unsigned long long* states = ws_states + slot;
    int* counts = ws_counts + slot;

    // ---- 3: the guesses, then sweeps until nothing changes: at most n + 1 of them
    for (uint32_t i = tid; i < n; i += PT) state_store(&states[i], (unsigned long long)(8u * (uint32_t)L * i) << 32);
    __syncthreads();
    uint32_t iters = 0;
    JpgBits b;
    for (uint32_t sweep = 0; sweep <= n; ++sweep) {
        bool changed = false;
        for (uint32_t i = tid; i + 1 < n; i += PT) {
            JpgState s = jpg_state_unpack(state_load(&states[i]));
            jpg_bits_start(b, words, avail, s.p);
            const uint32_t stop = n - i - 1u < WALK_MAX ? n : i + 1u + WALK_MAX;
            for (uint32_t j = i + 1; j < stop; ++j) {   // carry the state on until it meets an equal stored one
                jpg_advance(b, tab, B, s, 8u * (uint32_t)L * j, iters);
                const unsigned long long mine = jpg_state_pack(s);
                if (state_load(&states[j]) == mine) break;
                state_store(&states[j], mine);
                changed = true;
            }
        }
        if (changed) flag = 1;
        __syncthreads();
        const int any = flag;
        __syncthreads();
        if (!any) break;
        if (tid == 0) flag = 0;
        __syncthreads();
    }

    // ---- 4: the blocks that start in each sub-stream, then their exclusive scan (clamped to the segment's block count + 1)
    for (uint32_t i = tid; i < n; i += PT) {
        JpgState s = jpg_state_unpack(state_load(&states[i]));
        jpg_bits_start(b, words, avail, s.p);
        const uint32_t c = jpg_advance(b, tab, B, s, i + 1 < n ? 8u * (uint32_t)L * (i + 1u) : avail, iters);
        counts[i] = (int)(c < (uint32_t)nb + 1u ? c : (uint32_t)nb + 1u);
    }
    __syncthreads();
    long long carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += PT) {
        const uint32_t i = i0 + tid;
        long long sum;
        const long long excl = block_scan_excl<PWAVES>(i < n ? (long long)counts[i] : 0ll, sum);
        if (i < n) counts[i] = (int)min(carry + excl, (long long)nb + 1);   // beyond nb nothing is decoded
        carry = min(carry + sum, (long long)nb + 1);
    }
    __syncthreads();

    // ---- 5: the strict write pass
    {
        int st = 0;
        bool ended = false;
        uint32_t end_pos = 0;
        for (uint32_t i = tid; i < n; i += PT) {
            const JpgState s = jpg_state_unpack(state_load(&states[i]));
            jpg_bits_start(b, words, avail, s.p);
            st |= jpg_write_substream(b, tab, B, s, i + 1 < n ? 8u * (uint32_t)L * (i + 1u) : 0xffffffffu, counts[i], nb, out, ended,
                                      end_pos, iters);
        }
        if (st) atomicOr(&seg_status, st);
        if (ended) seg_end[0] = 1u, seg_end[1] = end_pos;
    }
    __syncthreads();

    // ---- 6 / 7: DC differences -> predictors (lane t owns a run of consecutive blocks), and the end check
    int st = seg_status;
    if (!st) st = seg_end[0] ? jpg_end_status(seg_end[1], avail) : JPG_S_OVERRUN;
    if (!st) {
        const int run = (nb + PT - 1) / PT, first = min(tid * run, nb), count = min(run, nb - first);
        int sums[3] = {0, 0, 0}, k = first % B;
        for (int blk = first; blk < first + count; ++blk) {
            sums[jpg_block_component(B, k)] += out[(size_t)blk * 64];
            if (++k == B) k = 0;
        }
        int pred[3], total;
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[c] = (int16_t)block_scan_excl<PWAVES>(sums[c], total);
        jpg_dc_sums(out, first, count, B, pred);
    } else {
        // ---- 8: the sequential redo -- such a frame goes to the host decoder anyway
        __syncthreads();
        for (size_t i = tid; i < nwords_out; i += PT) out32[i] = 0u;
        __syncthreads();
        if (tid == 0) {
            st = jpg_decode_segment_sequential(words, avail, tab, B, (int)nm, out, iters);
            if (st) atomicOr(&status[f], st);
        }
    }
}

bool sizes_ok(int F, int H, int W) { return F >= 1 && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }
long long mcus_of(int S, int H, int W) { return jpg_mcus(S, H, W); }

template <int S>
int parallel_launch(const uint8_t* stream, long long stream_bytes, const int64_t* segments, int n_segments, const uint8_t* huffman, int F,
                    int mcus, int L, int16_t* coef_out, int32_t* status, void* workspace, hipStream_t st) {
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    const long long bytes_cap = ws_bytes_cap(stream_bytes, n_segments), slots = ws_slots_cap(stream_bytes, n_segments, L);
    DTK_LAUNCH("jpeg_parallel", jpeg_parallel_kernel<S>, dim3((unsigned)n_segments), dim3(PT), 0, st, stream, stream_bytes,
               reinterpret_cast<const long long*>(segments), n_segments, huffman, F, mcus, L, coef_out, status, ws,
               reinterpret_cast<unsigned long long*>(ws + bytes_cap), reinterpret_cast<int*>(ws + bytes_cap + slots * 8));
    return 0;
}

}  // namespace

extern "C" size_t dtk_jpeg_decode_parallel_workspace_bytes(int32_t sampling, int64_t stream_bytes, int32_t n_segments,
                                                           int32_t subseq_bytes) {
    const int L = subseq_bytes ? subseq_bytes : JPG_SUBSEQ_DEFAULT;
    if (!jpg_sampling_ok(sampling) || stream_bytes < 1 || n_segments < 1 || !jpg_subseq_ok(L)) return 0;
    return (size_t)(ws_bytes_cap(stream_bytes, n_segments) + ws_slots_cap(stream_bytes, n_segments, L) * 12);
}

extern "C" int dtk_jpeg_decode_coefficients_parallel(int32_t sampling, const uint8_t* stream, int64_t stream_bytes,
                                                     const int64_t* segments, const int64_t* segments_host, int32_t n_segments,
                                                     const uint8_t* huffman, int32_t F, int32_t H, int32_t W, int32_t subseq_bytes,
                                                     int16_t* coef_out, int32_t* status, void* workspace, void* stream_) {
    DTK_REQUIRE(jpg_sampling_ok(sampling),
                "jpeg_decode_coefficients_parallel: sampling must be DTK_JPEG_420, _422, _444 or _GRAY (0 .. 3), got %d", sampling);
    DTK_REQUIRE(sizes_ok(F, H, W), "jpeg_decode_coefficients_parallel: F >= 1 and 1 <= H, W <= 65535 are required, got F=%d %d x %d", F, H,
                W);
    const int L = subseq_bytes ? subseq_bytes : JPG_SUBSEQ_DEFAULT;
    DTK_REQUIRE(jpg_subseq_ok(L), "jpeg_decode_coefficients_parallel: subseq_bytes must be 0 or a multiple of 4 in %d .. %d, got %d",
                JPG_SUBSEQ_MIN, JPG_SUBSEQ_MAX, subseq_bytes);
    DTK_REQUIRE(stream && segments && segments_host && huffman && coef_out && status && workspace,
                "jpeg_decode_coefficients_parallel: null pointer (stream / segments / segments_host / huffman / coef_out / status / "
                "workspace)");
    DTK_REQUIRE(stream_bytes >= 1 && n_segments >= 1,
                "jpeg_decode_coefficients_parallel: stream_bytes and n_segments must be positive, got %lld, %d", (long long)stream_bytes,
                n_segments);
    const long long mcus = mcus_of(sampling, H, W);
    long long end = 0;
    for (int s = 0; s < n_segments; ++s) {
        const int64_t* g = segments_host + (size_t)s * SEG_FIELDS;
        DTK_REQUIRE(g[0] >= 0 && g[0] < F && g[1] >= 0 && g[2] >= 0 && g[2] <= SEG_MAX_BYTES && g[1] <= stream_bytes - g[2] && g[3] >= 0 &&
                        g[4] >= 1 && g[3] <= mcus - g[4],
                    "jpeg_decode_coefficients_parallel: segment %d (frame %lld, bytes %lld + %lld, MCUs %lld + %lld) does not fit %d "
                    "frames, %lld bytes, %lld MCUs",
                    s, (long long)g[0], (long long)g[1], (long long)g[2], (long long)g[3], (long long)g[4], F, (long long)stream_bytes,
                    mcus);
        // a segment's place in the workspace follows from its byte range: the ranges must not overlap and must rise with the index
        DTK_REQUIRE(g[1] >= end, "jpeg_decode_coefficients_parallel: segment %d starts at byte %lld, inside or before segment %d's bytes",
                    s, (long long)g[1], s - 1);
        end = g[1] + g[2];
    }
    hipStream_t st = dtk_stream(stream_);
    DTK_HIP(dtk_zero_async(status, (size_t)F * 4, st));
    switch (sampling) {
        case JPG_420:
            return parallel_launch<JPG_420>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, L, coef_out, status, workspace,
                                            st);
        case JPG_422:
            return parallel_launch<JPG_422>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, L, coef_out, status, workspace,
                                            st);
        case JPG_444:
            return parallel_launch<JPG_444>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, L, coef_out, status, workspace,
                                            st);
        default:
            return parallel_launch<JPG_GRAY>(stream, stream_bytes, segments, n_segments, huffman, F, (int)mcus, L, coef_out, status,
                                             workspace, st);
    }
}
