// vit_patch_embed.h -- the patch embedding of the ViT encoder: tokens from ImageNet-normalised frames, exact to fp32 grade, on the
// f32-input MFMA (any patch / stride) or, for the 14 x 14 patches at stride 7 of DINOv2, on the split-fp16 MFMA; launch_patch_embed
// chooses.  Lives in the anonymous namespace of the one translation unit, vit.hip.
#pragma once
#include "vit_gemm_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// patch embedding: tokens[f][1 + R + r*pw + c][:] = W . patch(r,c) + b + pos[r*pw + c];  tokens[f][0] = cls_pos;
// tokens[f][1 .. R] = registers (DINOv2 with registers: no position encoding; R = 0 for the plain models), S = 1 + R + ph*pw
// 32 patches x 32 output features per wave (MFMA 32x32x2 f32), 4 waves = 64 patches x 64 features per workgroup
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_embed_kernel(const float* __restrict__ frames, const float* __restrict__ Wp,
                                                          const float* __restrict__ bp, const float* __restrict__ pos,
                                                          const float* __restrict__ cls_pos,
                                                          const float* __restrict__ mean_std, float* __restrict__ x,
                                                          int H, int W, int ph, int pw, int D, int patch, int stride,
                                                          int S, int R, const float* __restrict__ regs) {
    const int HW = ph * pw;
    const int K = 3 * patch * patch;
    const int frame = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int p0 = blockIdx.x * 64 + (w >> 1) * 32;
    const int n0 = blockIdx.y * 64 + (w & 1) * 32;
    const int li = lane & 31, lk = lane >> 5;
    const float* img = frames + (size_t)frame * 3 * H * W;
    const int p = min(p0 + li, HW - 1);
    const int pr = p / pw, pc = p % pw;
    const int n = min(n0 + li, D - 1);
    const float* wrow = Wp + (size_t)n * K;  // [D][3][patch][patch]
    f16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = lk; k < K; k += 2) {
        const int ch = k / (patch * patch), rem = k - ch * patch * patch;
        const int ky = rem / patch, kx = rem - ky * patch;
        const float px = img[((size_t)ch * H + pr * stride + ky) * W + pc * stride + kx];
        const float a = (px - mean_std[ch]) / mean_std[3 + ch];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wrow[k], acc, 0, 0, 0);
    }
    const int co = n0 + li;
    if (co < D) {
        const float b = bp[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * lk;
            const int pp = p0 + i;
            if (pp < HW) x[((size_t)frame * S + 1 + R + pp) * D + co] = acc[r] + b + pos[(size_t)pp * D + co];
        }
    }
    if (blockIdx.x == 0 && (w >> 1) == 0 && lk == 0 && co < D) {   // the prefix rows of this frame: once per feature
        x[(size_t)frame * S * D + co] = cls_pos[co];
        for (int r = 0; r < R; ++r) x[((size_t)frame * S + 1 + r) * D + co] = regs[(size_t)r * D + co];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// patch embedding on the split-fp16 MFMA (patch 14, stride 7): fp32-grade results from fp16 matrix instructions.
// Every fp32 operand is carried as hi + lo fp16 halves and a product is xh.wh + xh.wl + xl.wh accumulated in fp32 (each
// fp16 x fp16 product is exact in fp32; the dropped xl.wl term is 2^-22 relative).  The normalised frame is first
// rewritten as two NHWC planes with 4 channels per pixel (channel 3 = 0), so that with k = (ky * 14 + kx) * 4 + c an
// 8-wide A fragment is two neighbouring taps = two 8-byte LDS reads -- no im2col gather.  A workgroup owns 128
// consecutive tokens of one patch row (a wave 32 of them) x 96 output features and walks K = 784 in seven chunks of two
// kernel rows; per chunk the two pixel rows (903 px) and the 96 x 112 weight slab (both planes) are staged in LDS.
// ---------------------------------------------------------------------------------------------------------------
constexpr int PE_P = 14, PE_S = 7, PE_TOK = 128, PE_NF = 96;
constexpr int PE_ROWPX = (PE_TOK - 1) * PE_S + PE_P;  // 903 pixels of one kernel row for 128 tokens
constexpr int PE_K = PE_P * PE_P * 4;                 // 784
constexpr int PE_CK = 2 * PE_P * 4;                   // 112 k per chunk (two kernel rows)
constexpr int PE_WP = PE_CK + 8;                      // weight row pitch in halves (240 B: conflict-free fragments)
constexpr float PE_WSCALE = 256.f;                    // weights carry 2^8 so that their lo halves stay normal numbers

__global__ __launch_bounds__(256) void frame_split4_kernel(const float* __restrict__ frames, const float* __restrict__ mean_std,
                                                           h4v* __restrict__ hi_, h4v* __restrict__ lo_, int H, int W,
                                                           long long npix) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // over frames * H * W
    if (i >= npix) return;
    const long long f = i / ((long long)H * W), p = i - f * (long long)H * W;
    const float* fr = frames + f * 3 * (long long)H * W + p;
    h4v h, l;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = (fr[(long long)c * H * W] - mean_std[c]) / mean_std[3 + c];
        h[c] = (half_t)v;
        l[c] = (half_t)(v - (float)h[c]);
    }
    h[3] = (half_t)0.f;
    l[3] = (half_t)0.f;
    hi_[i] = h;
    lo_[i] = l;
}

// [D][3][14][14] fp32 -> split planes [D][784] of w * 2^8, k = (ky * 14 + kx) * 4 + c
__global__ void pack_patch_split_kernel(const float* __restrict__ w, int D, half_t* __restrict__ Wh, half_t* __restrict__ Wl) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)D * PE_K) return;
    const int n = (int)(idx / PE_K), k = (int)(idx - (long long)n * PE_K);
    const int tap = k >> 2, c = k & 3;
    const float v = c < 3 ? w[((size_t)n * 3 + c) * (PE_P * PE_P) + tap] * PE_WSCALE : 0.f;
    const half_t h = (half_t)v;
    Wh[idx] = h;
    Wl[idx] = (half_t)(v - (float)h);
}

__global__ __launch_bounds__(256) void patch_embed_split_kernel(const h4v* __restrict__ in_hi, const h4v* __restrict__ in_lo,
                                                                const half_t* __restrict__ Wh, const half_t* __restrict__ Wl,
                                                                const float* __restrict__ bp, const float* __restrict__ pos,
                                                                const float* __restrict__ cls_pos, float* __restrict__ x,
                                                                int H, int W, int ph, int pw, int D, int S, int groups_x,
                                                                int units, int slabs, int R, const float* __restrict__ regs) {
    __shared__ h4v Xh[2 * PE_ROWPX], Xl[2 * PE_ROWPX];
    __shared__ __attribute__((aligned(16))) half_t Wsh[PE_NF * PE_WP], Wsl[PE_NF * PE_WP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // Block -> (frame, patch row, token group, feature slab).  Workgroup b runs on XCD b % 8 and every XCD has its own L2:
    // the feature slabs of a token group re-read the same pixel rows, and so does the patch row below it (stride 7, kernel
    // 14), so each XCD gets a contiguous range of (frame, patch row, group) units and runs a unit's slabs back to back --
    // with the plain 3-D grid those blocks sat on different XCDs and every re-read went to HBM (PMC: 7.5 GB fetched per
    // 90-frame launch for 0.6 GB of split frames).
    const int per_xcd = (units + 7) / 8;
    const int within = blockIdx.x >> 3;
    const int unit = (blockIdx.x & 7) * per_xcd + within / slabs;
    if (within / slabs >= per_xcd || unit >= units) return;
    const int n0 = (within % slabs) * PE_NF;
    const int pc0 = (unit % groups_x) * PE_TOK, pr = (unit / groups_x) % ph;
    const size_t frame = unit / (groups_x * ph);
    const int li = lane & 31, hh = lane >> 5;
    const h4v* fh = in_hi + frame * (size_t)H * W;
    const h4v* fl = in_lo + frame * (size_t)H * W;
    const int tokl = w * 32 + li;  // this lane's token (row of the A operand) inside the group
    f16v acc[3];
#pragma unroll
    for (int n = 0; n < 3; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    for (int c = 0; c < PE_P / 2; ++c) {
        __syncthreads();
        for (int idx = tid; idx < 2 * PE_ROWPX; idx += 256) {
            const int r = idx / PE_ROWPX, px = idx - r * PE_ROWPX;
            const size_t g = (size_t)(pr * PE_S + 2 * c + r) * W + min(pc0 * PE_S + px, W - 1);
            Xh[idx] = fh[g];
            Xl[idx] = fl[g];
        }
        for (int idx = tid; idx < PE_NF * (PE_CK / 8); idx += 256) {
            const int f = idx / (PE_CK / 8), piece = idx - f * (PE_CK / 8);
            const size_t src = (size_t)min(n0 + f, D - 1) * PE_K + c * PE_CK + piece * 8;
            *reinterpret_cast<uint4*>(Wsh + f * PE_WP + piece * 8) = *reinterpret_cast<const uint4*>(Wh + src);
            *reinterpret_cast<uint4*>(Wsl + f * PE_WP + piece * 8) = *reinterpret_cast<const uint4*>(Wl + src);
        }
        __syncthreads();
#pragma unroll
        for (int ls = 0; ls < PE_CK / 16; ++ls) {
            const int t0 = 2 * (2 * ls + hh);  // first of this lane's two taps inside the chunk (kx even: same row)
            const int p0 = (t0 / PE_P) * PE_ROWPX + tokl * PE_S + t0 % PE_P;
            const h4v a0 = Xh[p0], a1 = Xh[p0 + 1], b0 = Xl[p0], b1 = Xl[p0 + 1];
            const h8 xh = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            const h8 xl = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int wo = (n * 32 + li) * PE_WP + ls * 16 + hh * 8;
                const h8 wh = *reinterpret_cast<const h8*>(Wsh + wo), wl = *reinterpret_cast<const h8*>(Wsl + wo);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl, acc[n], 0, 0, 0);
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh, acc[n], 0, 0, 0);
            }
        }
    }
    // D[i][j]: j = lane & 31 (feature), i = (r&3) + 8 (r>>2) + 4 hh (token of the wave's 32)
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        const int co = n0 + n * 32 + li;
        if (co >= D) continue;
        const float b = bp[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int pc = pc0 + w * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (pc < pw) {
                const int pp = pr * pw + pc;
                x[((size_t)frame * S + 1 + R + pp) * D + co] = acc[n][r] * (1.f / PE_WSCALE) + b + pos[(size_t)pp * D + co];
            }
        }
        if (pr == 0 && pc0 == 0 && w == 0 && hh == 0) {   // the prefix rows of this frame: once per feature
            x[(size_t)frame * S * D + co] = cls_pos[co];
            for (int r = 0; r < R; ++r) x[((size_t)frame * S + 1 + r) * D + co] = regs[(size_t)r * D + co];
        }
    }
}

// x [nf][S][D] = the tokens of `nf` frames, S = 1 + n_registers + ph * pw.
// The split-fp16 form runs for 14 x 14 patches at stride 7 when its inputs fit the two
// scratch regions the caller lends (vit_run: `hid` and `delta`, both unused until the first block): the split planes of the
// normalised frames go to `planes`, the split weights to `wsplit`.  Otherwise the generic kernel, which needs no scratch.
inline int launch_patch_embed(const dtk_vit_model* m, const float* frames, int nf, int H, int W, int ph, int pw, float* x, void* planes,
                              size_t planes_bytes, void* wsplit, size_t wsplit_bytes, hipStream_t st) {
    const int D = m->D, HW = ph * pw, R = m->n_registers, S = 1 + R + HW;
    const bool fits = (size_t)nf * H * W * 16 <= planes_bytes && (size_t)D * PE_K * 4 <= wsplit_bytes;
    if (m->patch == PE_P && m->stride == PE_S && fits) {
        h4v* fh = reinterpret_cast<h4v*>(planes);
        h4v* fl = fh + (size_t)nf * H * W;
        half_t* wh = reinterpret_cast<half_t*>(wsplit);
        half_t* wl = wh + (size_t)D * PE_K;
        const long long npix = (long long)nf * H * W;
        DTK_LAUNCH("vit_frame_split", frame_split4_kernel, dim3(dtk_cdiv(npix, 256)), dim3(256), 0, st, frames, m->mean_std, fh, fl, H, W,
                   npix);
        DTK_LAUNCH("vit_frame_split", pack_patch_split_kernel, dim3(dtk_cdiv((long long)D * PE_K, 256)), dim3(256), 0, st, m->patch_w, D,
                   wh, wl);
        const int groups_x = dtk_cdiv(pw, PE_TOK);
        const int units = groups_x * ph * nf, slabs = dtk_cdiv(D, PE_NF);
        DTK_LAUNCH("vit_patch_embed", patch_embed_split_kernel, dim3(8 * dtk_cdiv(units, 8) * slabs), dim3(256), 0, st, fh, fl, wh, wl,
                   m->patch_b, m->pos, m->cls_pos, x, H, W, ph, pw, D, S, groups_x, units, slabs, R, m->registers);
    } else {
        DTK_LAUNCH("vit_patch_embed", patch_embed_kernel, dim3(dtk_cdiv(HW, 64), dtk_cdiv(D, 64), nf), dim3(256), 0, st, frames,
                   m->patch_w, m->patch_b, m->pos, m->cls_pos, m->mean_std, x, H, W, ph, pw, D, m->patch, m->stride, S, R, m->registers);
    }
    return DTK_OK;
}

}  // namespace
