// anchors.hip -- anchor bookkeeping and occlusion (models/model_inference.py:130-200), device-side, no host sync.
//
//   dtk_build_anchor_sources : A_n = {a : cs[n][a] >= th}; pairs (n,a) numbered n-major (the layout of the
//                              reference's dict n -> [A_n, T, 2]); source list of the anchor stage sorted by
//                              anchor frame so that consecutive sources share their target feature frame.
//   dtk_occlusion            : d[k][t] = |G[k][t] - traj[a_k]|, lower median over anchors, threshold tau.
//   dtk_build_anchor_sources_needed / dtk_occlusion_needed : the same pairs and the same flags from the anchor maps the
//                              flags depend on.  occ = (med > tau) | low with tau = max of med over the anchor frames, so an
//                              anchor frame has med <= tau (occ = low) and a low frame is occluded whatever its median: only
//                              the UNDECIDED frames (neither anchor nor low) need a median, and they need tau, i.e. the
//                              anchor frames.  A query with no undecided frame (or no anchor) needs no anchor map at all.
#include "block_scan.h"

namespace {

__device__ __forceinline__ bool is_anchor(const float* cs, float th, int n, int T, int t) {
    return cs[(size_t)n * T + t] >= th;
}

// the frames of query n whose column of the anchor maps the flags can depend on: anchors (they set tau) and undecided frames
// (cs neither >= anchor_th nor < cos_th; a NaN cs is undecided).  The rest -- low and not an anchor -- is occluded by cs alone.
__device__ __forceinline__ bool is_undecided(float c, float anchor_th, float cos_th) { return !(c >= anchor_th) && !(c < cos_th); }
__device__ __forceinline__ bool is_needed(float c, float anchor_th, float cos_th) { return c >= anchor_th || !(c < cos_th); }

// n_anchors[n] as anchor_count_kernel; need_w[n] = needed columns of query n if it is OPEN (>= 1 anchor and >= 1 undecided
// frame), else 0: the sources every pair of the query emits
__global__ __launch_bounds__(256) void query_need_kernel(const float* __restrict__ cs, float anchor_th, float cos_th, int N, int T,
                                                         int32_t* __restrict__ n_anchors, int32_t* __restrict__ need_w) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int anchors = 0, undecided = 0, needed = 0;
    for (int t = 0; t < T; ++t) {
        const float c = cs[(size_t)n * T + t];
        anchors += c >= anchor_th ? 1 : 0;
        undecided += is_undecided(c, anchor_th, cos_th) ? 1 : 0;
        needed += is_needed(c, anchor_th, cos_th) ? 1 : 0;
    }
    n_anchors[n] = anchors;
    need_w[n] = (anchors > 0 && undecided > 0) ? needed : 0;
}

// frame_cnt[a] = sources of anchor frame a = sum of need_w[n] over the queries with anchor (n, a)
__global__ __launch_bounds__(256) void frame_weight_kernel(const float* __restrict__ cs, float th, int N, int T,
                                                           const int32_t* __restrict__ need_w, int32_t* __restrict__ frame_cnt) {
    const int a = blockIdx.x;
    int c = 0;
    for (int n = threadIdx.x; n < N; n += 256) c += is_anchor(cs, th, n, T, a) ? need_w[n] : 0;
    c = block_sum_i<4>(c);
    if (threadIdx.x == 0) frame_cnt[a] = c;
}

// one block: counts[0] = pairs, counts[1] = emitted sources, counts[3] = open queries
__global__ __launch_bounds__(256) void finalize_needed_counts_kernel(const int32_t* __restrict__ pair_off,
                                                                     const int32_t* __restrict__ frame_off,
                                                                     const int32_t* __restrict__ need_w, int N, int T,
                                                                     int32_t* __restrict__ counts) {
    int open = 0;
    for (int n = threadIdx.x; n < N; n += 256) open += need_w[n] > 0 ? 1 : 0;
    open = block_sum_i<4>(open);
    if (threadIdx.x == 0) {
        counts[0] = pair_off[N];
        counts[1] = frame_off[T];
        counts[3] = open;
    }
}

__global__ __launch_bounds__(256) void anchor_count_kernel(const float* __restrict__ cs, float th, int N, int T,
                                                           int32_t* __restrict__ n_anchors) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int c = 0;
    for (int t = 0; t < T; ++t) c += is_anchor(cs, th, n, T, t) ? 1 : 0;
    n_anchors[n] = c;
}

__global__ __launch_bounds__(256) void frame_count_kernel(const float* __restrict__ cs, float th, int N, int T,
                                                          int32_t* __restrict__ frame_cnt) {
    const int a = blockIdx.x;
    int c = 0;
    for (int n = threadIdx.x; n < N; n += 256) c += is_anchor(cs, th, n, T, a) ? 1 : 0;
    c = block_sum_i<4>(c);
    if (threadIdx.x == 0) frame_cnt[a] = c;
}

// single block: out[0..n] = exclusive scan of in[0..n-1]; optionally count zeros
__global__ __launch_bounds__(256) void exclusive_scan_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                             int n, int32_t* __restrict__ zero_count) {
    int carry = 0, zeros = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const int v = i < n ? in[i] : 0;
        if (i < n && v == 0) ++zeros;
        int total;
        const int excl = block_scan_excl<4>(v, total);
        if (i < n) out[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
    if (zero_count) {
        zeros = block_sum_i<4>(zeros);
        if (threadIdx.x == 0) *zero_count = zeros;
    }
}

__global__ void finalize_counts_kernel(const int32_t* __restrict__ pair_off, int N, int T, int32_t* __restrict__ counts) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        counts[0] = pair_off[N];
        counts[1] = pair_off[N] * T;
    }
}

// block a: walk the queries in order, place the pairs of frame a at frame_off[a] + (rank among queries)
__global__ __launch_bounds__(256) void emit_sources_kernel(const float* __restrict__ cs, float th, int N, int T,
                                                           const int32_t* __restrict__ pair_off,
                                                           const int32_t* __restrict__ frame_off,
                                                           int32_t* __restrict__ pair_frame,
                                                           int32_t* __restrict__ src_row, int32_t* __restrict__ tgt,
                                                           int32_t* __restrict__ out_idx) {
    const int a = blockIdx.x;
    int carry = frame_off[a];
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + threadIdx.x;
        const int flag = (n < N && is_anchor(cs, th, n, T, a)) ? 1 : 0;
        int total;
        const int excl = block_scan_excl<4>(flag, total);
        if (flag) {
            const int j = carry + excl;  // position among the pairs sorted by anchor frame
            int rank = 0;
            for (int t = 0; t < a; ++t) rank += is_anchor(cs, th, n, T, t) ? 1 : 0;
            const int p = pair_off[n] + rank;
            pair_frame[p] = a;
            const size_t mb = (size_t)j * T;
            for (int t = 0; t < T; ++t) {
                src_row[mb + t] = n * T + t;
                tgt[mb + t] = a;
                out_idx[mb + t] = p * T + t;
            }
        }
        carry += total;
    }
}

// block a as emit_sources_kernel, but pair (n, a) emits need_w[n] sources -- the needed columns of n in frame order, none for a
// closed query -- so the position of a pair is the scan of those weights; pair_frame is written for EVERY pair
__global__ __launch_bounds__(256) void emit_needed_sources_kernel(const float* __restrict__ cs, float anchor_th, float cos_th,
                                                                  int N, int T, const int32_t* __restrict__ pair_off,
                                                                  const int32_t* __restrict__ frame_off,
                                                                  const int32_t* __restrict__ need_w,
                                                                  int32_t* __restrict__ pair_frame,
                                                                  int32_t* __restrict__ src_row, int32_t* __restrict__ tgt,
                                                                  int32_t* __restrict__ out_idx) {
    const int a = blockIdx.x;
    int carry = frame_off[a];
    for (int n0 = 0; n0 < N; n0 += 256) {
        const int n = n0 + threadIdx.x;
        const bool anchor = n < N && is_anchor(cs, anchor_th, n, T, a);
        const int weight = anchor ? need_w[n] : 0;
        int total;
        const int excl = block_scan_excl<4>(weight, total);
        if (anchor) {
            int rank = 0;
            for (int t = 0; t < a; ++t) rank += is_anchor(cs, anchor_th, n, T, t) ? 1 : 0;
            const int p = pair_off[n] + rank;
            pair_frame[p] = a;
            if (weight > 0) {
                int m = carry + excl;  // first source of this pair among the sources sorted by anchor frame
                for (int t = 0; t < T; ++t) {
                    if (!is_needed(cs[(size_t)n * T + t], anchor_th, cos_th)) continue;
                    src_row[m] = n * T + t;
                    tgt[m] = a;
                    out_idx[m] = p * T + t;
                    ++m;
                }
            }
        }
        carry += total;
    }
}

// |G[p][t] - traj[a]| without fma contraction (the reference evaluates sqrt(dx*dx + dy*dy) with separate roundings)
__device__ __forceinline__ float anchor_dist(const float* __restrict__ green, const float* __restrict__ tr, int p, int a,
                                             int T, int t) {
    const float dx = green[((size_t)p * T + t) * 2] - tr[2 * a];
    const float dy = green[((size_t)p * T + t) * 2 + 1] - tr[2 * a + 1];
    return sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
}

// one block per query, one wave per frame t at a time: every anchor distance is computed ONCE into LDS (so the rank
// selection compares stored values: an element can never compare "less than itself"), then lane k ranks d[k] against
// all A values; the lane whose rank is the lower median's publishes it (torch.median semantics, ties by index).
// PRUNED (dtk_occlusion_needed): green holds only what dtk_build_anchor_sources_needed listed.  A closed query gets
// occ = low without a read of green; an open one skips the columns that are not needed (med[t] stays unwritten and unread).
template <bool PRUNED>
__global__ __launch_bounds__(256) void occlusion_kernel(const float* __restrict__ green,
                                                        const int32_t* __restrict__ pair_off,
                                                        const int32_t* __restrict__ pair_frame,
                                                        const float* __restrict__ traj, const float* __restrict__ cs,
                                                        float anchor_th, float cos_th, uint8_t* __restrict__ occ, int N,
                                                        int T) {
    extern __shared__ float smem_occ[];  // med[T] | d[4][T]
    float* med = smem_occ;
    __shared__ float red[4];
    const int n = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* d = smem_occ + T + w * T;
    const int p0 = pair_off[n], A = pair_off[n + 1] - p0;
    const float* tr = traj + (size_t)n * T * 2;
    if (A <= 0) {  // the reference raises here (torch.stack of an empty list); host reports it via counts[2]
        for (int t = threadIdx.x; t < T; t += 256) occ[(size_t)n * T + t] = 1;
        return;
    }
    if constexpr (PRUNED) {
        int undecided = 0;
        for (int t = threadIdx.x; t < T; t += 256) undecided |= is_undecided(cs[(size_t)n * T + t], anchor_th, cos_th) ? 1 : 0;
        if (!__syncthreads_or(undecided)) {  // closed: every frame is an anchor (med <= tau) or low
            for (int t = threadIdx.x; t < T; t += 256) occ[(size_t)n * T + t] = cs[(size_t)n * T + t] < cos_th ? 1 : 0;
            return;
        }
    }
    const int want = (A - 1) / 2;  // torch.median: lower median
    for (int t = w; t < T; t += 4) {
        if constexpr (PRUNED)
            if (!is_needed(cs[(size_t)n * T + t], anchor_th, cos_th)) continue;  // wave-uniform
        for (int k = lane; k < A; k += WAVE) d[k] = anchor_dist(green, tr, p0 + k, pair_frame[p0 + k], T, t);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < A; k += WAVE) {
            const float dk = d[k];
            int rank = 0;
            for (int k2 = 0; k2 < A; ++k2) {
                const float d2 = d[k2];
                rank += (d2 < dk || (d2 == dk && k2 < k)) ? 1 : 0;
            }
            if (rank == want) med[t] = dk;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // d is rewritten for the next frame
    }
    __syncthreads();
    float tau = -INFINITY;
    for (int t = threadIdx.x; t < T; t += 256)
        if (cs[(size_t)n * T + t] >= anchor_th) tau = fmaxf(tau, med[t]);
    tau = wave_max(tau);
    if (lane == 0) red[w] = tau;
    __syncthreads();
    tau = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int t = threadIdx.x; t < T; t += 256) {
        const float c = cs[(size_t)n * T + t];
        const bool far = (!PRUNED || is_needed(c, anchor_th, cos_th)) && med[t] > tau;
        occ[(size_t)n * T + t] = (far || c < cos_th) ? 1 : 0;
    }
}

}  // namespace

extern "C" int dtk_build_anchor_sources(const float* cs, float anchor_th, int N, int T, int32_t* n_anchors,
                                        int32_t* pair_off, int32_t* pair_frame, int32_t* src_row, int32_t* tgt,
                                        int32_t* out_idx, int32_t* counts, int32_t* scratch, void* stream) {
    DTK_REQUIRE(cs && n_anchors && pair_off && pair_frame && src_row && tgt && out_idx && counts && scratch,
                "dtk_build_anchor_sources: null pointer");
    DTK_REQUIRE(N > 0 && T > 0 && (long long)N * T * T < 2147483647LL, "dtk_build_anchor_sources: N*T*T out of range");
    hipStream_t st = dtk_stream(stream);
    int32_t* frame_cnt = scratch;          // [T]
    int32_t* frame_off = scratch + T;      // [T+1]
    DTK_LAUNCH("anchor_count", anchor_count_kernel, dim3(dtk_cdiv(N, 256)), dim3(256), 0, st, cs, anchor_th, N, T, n_anchors);
    DTK_LAUNCH("exclusive_scan", exclusive_scan_kernel, dim3(1), dim3(256), 0, st, n_anchors, pair_off, N, counts + 2);
    DTK_LAUNCH("frame_count", frame_count_kernel, dim3(T), dim3(256), 0, st, cs, anchor_th, N, T, frame_cnt);
    DTK_LAUNCH("exclusive_scan", exclusive_scan_kernel, dim3(1), dim3(256), 0, st, frame_cnt, frame_off, T, (int32_t*)nullptr);
    DTK_LAUNCH("finalize_counts", finalize_counts_kernel, dim3(1), dim3(64), 0, st, pair_off, N, T, counts);
    DTK_LAUNCH("emit_sources", emit_sources_kernel, dim3(T), dim3(256), 0, st, cs, anchor_th, N, T, pair_off, frame_off,
                       pair_frame, src_row, tgt, out_idx);
    return DTK_OK;
}

extern "C" int dtk_occlusion(const float* green, const int32_t* pair_off, const int32_t* pair_frame, const float* traj,
                             const float* cs, float anchor_th, float cos_th, uint8_t* occ, int N, int T, void* stream) {
    DTK_REQUIRE(green && pair_off && pair_frame && traj && cs && occ && N >= 0 && T > 0, "dtk_occlusion: bad args");
    DTK_REQUIRE((size_t)5 * T * sizeof(float) <= 60 * 1024, "dtk_occlusion: T=%d too large", T);
    if (N == 0) return DTK_OK;
    DTK_LAUNCH("occlusion", occlusion_kernel<false>, dim3(N), dim3(256), (size_t)5 * T * sizeof(float), dtk_stream(stream), green,
                       pair_off, pair_frame, traj, cs, anchor_th, cos_th, occ, N, T);
    return DTK_OK;
}

extern "C" int dtk_build_anchor_sources_needed(const float* cs, float anchor_th, float cos_th, int N, int T, int32_t* n_anchors,
                                               int32_t* pair_off, int32_t* pair_frame, int32_t* src_row, int32_t* tgt,
                                               int32_t* out_idx, int32_t* counts, int32_t* scratch, void* stream) {
    DTK_REQUIRE(cs && n_anchors && pair_off && pair_frame && src_row && tgt && out_idx && counts && scratch,
                "dtk_build_anchor_sources_needed: null pointer");
    DTK_REQUIRE(N > 0 && T > 0 && (long long)N * T * T < 2147483647LL, "dtk_build_anchor_sources_needed: N*T*T out of range");
    hipStream_t st = dtk_stream(stream);
    int32_t* frame_cnt = scratch;              // [T]
    int32_t* frame_off = scratch + T;          // [T+1]
    int32_t* need_w = scratch + 2 * T + 2;     // [N]
    DTK_LAUNCH("query_need", query_need_kernel, dim3(dtk_cdiv(N, 256)), dim3(256), 0, st, cs, anchor_th, cos_th, N, T, n_anchors,
               need_w);
    DTK_LAUNCH("exclusive_scan", exclusive_scan_kernel, dim3(1), dim3(256), 0, st, n_anchors, pair_off, N, counts + 2);
    DTK_LAUNCH("frame_weight", frame_weight_kernel, dim3(T), dim3(256), 0, st, cs, anchor_th, N, T, need_w, frame_cnt);
    DTK_LAUNCH("exclusive_scan", exclusive_scan_kernel, dim3(1), dim3(256), 0, st, frame_cnt, frame_off, T, (int32_t*)nullptr);
    DTK_LAUNCH("finalize_counts", finalize_needed_counts_kernel, dim3(1), dim3(256), 0, st, pair_off, frame_off, need_w, N, T,
               counts);
    DTK_LAUNCH("emit_sources", emit_needed_sources_kernel, dim3(T), dim3(256), 0, st, cs, anchor_th, cos_th, N, T, pair_off,
               frame_off, need_w, pair_frame, src_row, tgt, out_idx);
    return DTK_OK;
}

extern "C" int dtk_occlusion_needed(const float* green, const int32_t* pair_off, const int32_t* pair_frame, const float* traj,
                                    const float* cs, float anchor_th, float cos_th, uint8_t* occ, int N, int T, void* stream) {
    DTK_REQUIRE(green && pair_off && pair_frame && traj && cs && occ && N >= 0 && T > 0, "dtk_occlusion_needed: bad args");
    DTK_REQUIRE((size_t)5 * T * sizeof(float) <= 60 * 1024, "dtk_occlusion_needed: T=%d too large", T);
    if (N == 0) return DTK_OK;
    DTK_LAUNCH("occlusion", occlusion_kernel<true>, dim3(N), dim3(256), (size_t)5 * T * sizeof(float), dtk_stream(stream), green,
                       pair_off, pair_frame, traj, cs, anchor_th, cos_th, occ, N, T);
    return DTK_OK;
}


// ------------------------------------------------------------------------------------------------------------
// TAP-Vid metric counts on the device (eval/metrics.py:7-147, compute_tapvid_metrics for ONE video), so that the
// trajectories of inference_benchmark.py never have to leave the GPU as .npy files to be scored.
// One thread per (query, frame); counts[18] (uint64):
//   [0] evaluated points  [1] occlusion prediction == ground truth  [2] visible in the ground truth
//   [3+3i] within threshold 2^i px & visible  [4+3i] ... & predicted visible (true positives)  [5+3i] false positives
// all restricted to the evaluated frames of the query (strided: every frame but the query frame; first: later frames).
// The distance test replicates the float32 arithmetic of the numpy code: (px*sp - gx*sg)^2 summed, < thresh^2.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tapvid_counts_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ pred_occ,
                                                            const float* __restrict__ gt, const uint8_t* __restrict__ gt_occ,
                                                            const int32_t* __restrict__ qframe, float spx, float spy,
                                                            float sgx, float sgy, int first_mode, int N, int T,
                                                            unsigned long long* __restrict__ counts) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    int c[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) c[k] = 0;
    if (i < (long long)N * T) {
        const int n = (int)(i / T), t = (int)(i - (long long)n * T);
        const int qf = qframe[n];
        const bool ev = first_mode ? (t > qf) : (t != qf);
        if (ev) {
            const bool vis = gt_occ[i] == 0, pvis = pred_occ[i] == 0;
            const float dx = __fsub_rn(__fmul_rn(pred[2 * i], spx), __fmul_rn(gt[2 * i], sgx));
            const float dy = __fsub_rn(__fmul_rn(pred[2 * i + 1], spy), __fmul_rn(gt[2 * i + 1], sgy));
            const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
            c[0] = 1;
            c[1] = (pvis == vis);
            c[2] = vis;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const float th = (float)(1 << k);
                const bool within = d2 < th * th;
                c[3 + 3 * k] = within && vis;
                c[4 + 3 * k] = within && vis && pvis;
                c[5 + 3 * k] = ((!vis) && pvis) || ((!within) && pvis);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 18; ++k) {
        const int s = wave_sum_i(c[k]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&counts[k], (unsigned long long)s);
    }
}

extern "C" int dtk_tapvid_counts(const float* pred_tracks, const uint8_t* pred_occluded, const float* gt_tracks,
                                 const uint8_t* gt_occluded, const int32_t* query_frame, float pred_scale_x,
                                 float pred_scale_y, float gt_scale_x, float gt_scale_y, int first_mode, int N, int T,
                                 unsigned long long* counts18, void* stream) {
    DTK_REQUIRE(counts18, "dtk_tapvid_counts: null pointer");
    DTK_REQUIRE(N >= 0 && T > 0, "dtk_tapvid_counts: bad sizes");
    hipStream_t st = dtk_stream(stream);
    DTK_HIP(hipMemsetAsync(counts18, 0, 18 * sizeof(unsigned long long), st));
    if (N == 0) return DTK_OK;  // no query: eighteen zeros (the arrays are empty, and an empty device tensor has no address)
    DTK_REQUIRE(pred_tracks && pred_occluded && gt_tracks && gt_occluded && query_frame, "dtk_tapvid_counts: null pointer");
    DTK_LAUNCH("tapvid_counts", tapvid_counts_kernel, dim3(dtk_cdiv((long long)N * T, 256)), dim3(256), 0, st, pred_tracks,
               pred_occluded, gt_tracks, gt_occluded, query_frame, pred_scale_x, pred_scale_y, gt_scale_x, gt_scale_y,
               first_mode, N, T, counts18);
    return DTK_OK;
}


// ------------------------------------------------------------------------------------------------------------
// BADJA metric counts on the device (eval/metrics.py:226-287, compute_badja_metrics_for_video for ONE video).
//   area[t]  = number of segmentations[t] > 0 pixels (an integer; numpy's float32 sum of 0 / 1 flags is the same number while it
//              stays below 2^24, which the launcher guarantees by refusing H W >= 2^24)
//   thr[t]   = float32(0.2) * sqrtf(float32(area[t]))          (what numpy 2 computes: the python float 0.2 is a weak scalar)
//   for every point i and frame t in 1 .. T_seg - 1 with gt_occluded[i][t] == 0:
//     dist = sqrt((px - gx)^2 + (py - gy)^2) in float64, px = float32(pred * scale) promoted, gx the float64 ground truth,
//     the sum not contracted into an FMA
//   counts3 (uint64): [0] visible  [1] dist < thr[t]  [2] dist < 3.0
// Integer atomics only, so two calls give the same bits.
// ------------------------------------------------------------------------------------------------------------
template <typename M>
__global__ __launch_bounds__(256) void badja_area_kernel(const M* __restrict__ seg, long long HW,
                                                         unsigned long long* __restrict__ areas) {
    const M* frame = seg + (size_t)blockIdx.y * HW;
    int c = 0;   // at most HW / gridDim.x / 256 + 1 < 2^24 per thread
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) c += frame[p] > (M)0;
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&areas[blockIdx.y], (unsigned long long)c);
}

__global__ __launch_bounds__(256) void badja_counts_kernel(const float* __restrict__ pred, const double* __restrict__ gt,
                                                           const uint8_t* __restrict__ gt_occ,
                                                           const unsigned long long* __restrict__ areas, float spx, float spy,
                                                           int N, int T, int T_seg, unsigned long long* __restrict__ counts) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int per = T_seg - 1;   // frames 1 .. T_seg - 1
    int vis = 0, in_seg = 0, in_3px = 0;
    if (idx < (long long)N * per) {
        const int n = (int)(idx / per), t = 1 + (int)(idx - (long long)n * per);
        const size_t at = (size_t)n * T + t;
        if (gt_occ[at] == 0) {
            const float thr = __fmul_rn(0.2f, __fsqrt_rn((float)areas[t]));
            const double dx = __dsub_rn((double)__fmul_rn(pred[2 * at], spx), gt[2 * at]);
            const double dy = __dsub_rn((double)__fmul_rn(pred[2 * at + 1], spy), gt[2 * at + 1]);
            const double dist = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
            vis = 1;
            in_seg = dist < (double)thr;
            in_3px = dist < 3.0;
        }
    }
    vis = wave_sum_i(vis), in_seg = wave_sum_i(in_seg), in_3px = wave_sum_i(in_3px);
    if ((threadIdx.x & 63) == 0) {
        if (vis) atomicAdd(&counts[0], (unsigned long long)vis);
        if (in_seg) atomicAdd(&counts[1], (unsigned long long)in_seg);
        if (in_3px) atomicAdd(&counts[2], (unsigned long long)in_3px);
    }
}

extern "C" int dtk_badja_counts(const float* pred_tracks, const double* gt_tracks, const uint8_t* gt_occluded,
                                const void* segmentations, int32_t seg_is_float, float pred_scale_x, float pred_scale_y,
                                int32_t N, int32_t T, int32_t T_seg, int32_t H, int32_t W, unsigned long long* areas,
                                unsigned long long* counts3, void* stream) {
    DTK_REQUIRE(counts3 && areas && segmentations, "dtk_badja_counts: null pointer");
    DTK_REQUIRE(N >= 0 && T > 0 && T_seg > 0 && T_seg <= T && T_seg <= 65535 && H > 0 && W > 0,
                "dtk_badja_counts: bad sizes N=%d T=%d T_seg=%d (needs 1 <= T_seg <= T) masks %d x %d", N, T, T_seg, W, H);
    DTK_REQUIRE((long long)H * W < (1LL << 24),
                "dtk_badja_counts: a %d x %d mask can have an area of 2^24 or more, where numpy's float32 sum of the reference "
                "stops being the pixel count", W, H);
    DTK_REQUIRE(seg_is_float == 0 || seg_is_float == 1, "dtk_badja_counts: seg_is_float must be 0 (uint8) or 1 (float32)");
    hipStream_t st = dtk_stream(stream);
    DTK_HIP(hipMemsetAsync(counts3, 0, 3 * sizeof(unsigned long long), st));
    DTK_HIP(hipMemsetAsync(areas, 0, (size_t)T_seg * sizeof(unsigned long long), st));
    const long long HW = (long long)H * W;
    const int per_frame = dtk_cdiv(HW, 256 * 8);   // blocks per mask: about eight pixels per thread
    const dim3 grid(per_frame < 1024 ? per_frame : 1024, T_seg);
    if (seg_is_float) {
        DTK_LAUNCH("badja_area", badja_area_kernel<float>, grid, dim3(256), 0, st, (const float*)segmentations, HW, areas);
    } else {
        DTK_LAUNCH("badja_area", badja_area_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)segmentations, HW, areas);
    }
    if (N == 0 || T_seg == 1) return DTK_OK;   // nothing to score: three zeros
    DTK_REQUIRE(pred_tracks && gt_tracks && gt_occluded, "dtk_badja_counts: null pointer");
    DTK_LAUNCH("badja_counts", badja_counts_kernel, dim3(dtk_cdiv((long long)N * (T_seg - 1), 256)), dim3(256), 0, st, pred_tracks,
               gt_tracks, gt_occluded, areas, pred_scale_x, pred_scale_y, N, T, T_seg, counts3);
    return DTK_OK;
}
