// raft_stages.h -- the RAFT kernels around the convolutions: image layout, instance norm, pyramid pooling, the correlation lookup
// and the convex upsampling.  All activations are NHWC fp32.  No atomics anywhere: every output element is written by one thread
// from sums taken in a fixed order, so two runs give the same bits whatever the launch order.
#pragma once
#include "common.h"

namespace {

// image1 / image2 [N][3][hw] -> [2 N][hw][3] (image1's batch first)
__global__ void raft_images_nhwc_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int N, int hw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)2 * N * hw) return;
    const int n = (int)(i / hw), px = (int)(i - (long long)n * hw);
    const float* src = n < N ? a + (size_t)n * 3 * hw : b + (size_t)(n - N) * 3 * hw;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = src[(size_t)c * hw + px];
}

__global__ void raft_zero_flow_kernel(float* __restrict__ flow, long long stride, long long M) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) { flow[i * stride] = 0.f; flow[i * stride + 1] = 0.f; }
}

// ---- instance norm, two launches.
// Statistics: block (chunk, n), thread (channel c, sub s) with blockDim = C * subs.  The pixels of the chunk are dealt to the subs
// round robin; each thread sums its pixels in order, the subs are added in order (the chunk's mean), then the squared deviations
// from THAT mean the same way (no cancellation), and the block writes (count, mean, M2) per channel.
// Apply: every block combines the chunks of its image in chunk order with Chan's update in float64 -- the same sequence in every
// block, hence the same mean and variance -- and normalises its own chunk:  y = (x - mean) / sqrt(M2 / count + eps);
// relu: y = max(y, 0);  res: y = max(res + y, 0).
__global__ __launch_bounds__(256) void raft_in_stats_kernel(const float* __restrict__ x, float* __restrict__ ws, int hw, int C, int chunks) {
    __shared__ float red[256];
    __shared__ float mean_s[256];
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int c = threadIdx.x % C, s = threadIdx.x / C, subs = blockDim.x / C;
    const int per = (hw + chunks - 1) / chunks;
    const int p0 = chunk * per, p1 = min(hw, p0 + per);
    const float* xi = x + (size_t)n * hw * C;
    float sum = 0.f;
    for (int px = p0 + s; px < p1; px += subs) sum += xi[(size_t)px * C + c];
    red[threadIdx.x] = sum;
    __syncthreads();
    const int cnt = max(p1 - p0, 0);
    if (s == 0) {
        float t = 0.f;
        for (int k = 0; k < subs; ++k) t += red[k * C + c];
        mean_s[c] = cnt > 0 ? t / (float)cnt : 0.f;
    }
    __syncthreads();
    const float mu = mean_s[c];
    float m2 = 0.f;
    for (int px = p0 + s; px < p1; px += subs) {
        const float d = xi[(size_t)px * C + c] - mu;
        m2 += d * d;
    }
    __syncthreads();
    red[threadIdx.x] = m2;
    __syncthreads();
    if (s == 0) {
        float t = 0.f;
        for (int k = 0; k < subs; ++k) t += red[k * C + c];
        float* o = ws + ((size_t)(n * chunks + chunk) * C + c) * 3;
        o[0] = (float)cnt;
        o[1] = mu;
        o[2] = t;
    }
}

__global__ __launch_bounds__(256) void raft_in_apply_kernel(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ out,
                                                            const float* __restrict__ ws, int hw, int C, int chunks, float eps, int relu) {
    __shared__ float mean_s[256];
    __shared__ float rstd_s[256];
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int c = threadIdx.x % C, s = threadIdx.x / C, subs = blockDim.x / C;
    if (s == 0) {
        double cnt = 0.0, mean = 0.0, m2 = 0.0;
        for (int k = 0; k < chunks; ++k) {
            const float* o = ws + ((size_t)(n * chunks + k) * C + c) * 3;
            const double nb = o[0], mb = o[1], sb = o[2];
            if (nb <= 0.0) continue;
            const double tot = cnt + nb, d = mb - mean;
            mean += d * nb / tot;
            m2 += sb + d * d * cnt * nb / tot;
            cnt = tot;
        }
        mean_s[c] = (float)mean;
        rstd_s[c] = (float)(1.0 / sqrt(m2 / cnt + (double)eps));
    }
    __syncthreads();
    const int per = (hw + chunks - 1) / chunks;
    const int p0 = chunk * per, p1 = min(hw, p0 + per);
    const float mu = mean_s[c], rs = rstd_s[c];
    const size_t base = (size_t)n * hw * C;
    for (int px = p0 + s; px < p1; px += subs) {
        const size_t i = base + (size_t)px * C + c;
        float y = (x[i] - mu) * rs;
        if (relu) y = fmaxf(y, 0.f);
        if (res) y = fmaxf(res[i] + y, 0.f);
        out[i] = y;
    }
}

// ---- pyramid level l from level l - 1: 2 x 2 average of the j map, odd last row / column dropped: ((a + b) + (c + d)) / 4
__global__ void raft_corr_pool_kernel(const float* __restrict__ prev, float* __restrict__ cur, long long total, int hp, int wp, int hc, int wc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % wc), y = (int)((i / wc) % hc);
    const long long map = i / ((long long)wc * hc);
    const float* q = prev + map * hp * wp + (size_t)(2 * y) * wp + 2 * x;
    cur[i] = ((q[0] + q[1]) + (q[wp] + q[wp + 1])) * 0.25f;
}

// ---- lookup.  Thread (cell i, level l, slow window index a) writes the 9 channels 81 l + 9 a + b, b = 0 .. 8, of cell i.
// x = (col + flow_x) / 2^l, y = (row + flow_y) / 2^l (exact scalings);  x0 = floor(x), fx = x - x0 (exact), y alike.  Channel
// (a, b) reads at (x + a - 4, y + b - 4): the corners (X, Y), (X + 1, Y), (X, Y + 1), (X + 1, Y + 1) with X = x0 + a - 4,
// Y = y0 + b - 4 and the weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy, the four products summed in that order from
// zero; a corner outside the level's map contributes zero.
__global__ void raft_lookup_kernel(const float* __restrict__ pyr, const float* __restrict__ flow, long long flow_stride, int N, int h, int w,
                                   float* __restrict__ out, long long out_stride) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long M = (long long)N * h * w;
    if (t >= M * 36) return;
    const long long cell = t / 36;
    const int la = (int)(t - cell * 36), l = la / 9, a = la - 9 * l;
    const int hw = h * w;
    const int n = (int)(cell / hw), i = (int)(cell - (long long)n * hw);
    const int row = i / w, col = i - row * w;
    int hl = h, wl = w;
    size_t off = 0;
    for (int k = 0; k < l; ++k) { off += (size_t)N * hw * hl * wl; hl >>= 1; wl >>= 1; }
    const float* map = pyr + off + ((size_t)n * hw + i) * hl * wl;
    const float inv = 1.0f / (float)(1 << l);
    const float x = ((float)col + flow[cell * flow_stride]) * inv, y = ((float)row + flow[cell * flow_stride + 1]) * inv;
    float* o = out + cell * out_stride + 81 * l + 9 * a;
    // beyond +-2^24 the position is far outside every map: all zeros (also keeps the int conversions defined); NaN alike
    if (!(fabsf(x) < 16777216.f && fabsf(y) < 16777216.f)) {
#pragma unroll
        for (int b = 0; b < 9; ++b) o[b] = 0.f;
        return;
    }
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int X = (int)xf + a - 4, Y0 = (int)yf - 4;
    const bool in0 = X >= 0 && X < wl, in1 = X + 1 >= 0 && X + 1 < wl;
    float v0[10], v1[10];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const int Y = Y0 + r;
        const bool iny = Y >= 0 && Y < hl;
        v0[r] = iny && in0 ? map[(size_t)Y * wl + X] : 0.f;
        v1[r] = iny && in1 ? map[(size_t)Y * wl + X + 1] : 0.f;
    }
    const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        float acc = 0.f;
        acc += w00 * v0[b];
        acc += w10 * v1[b];
        acc += w01 * v0[b + 1];
        acc += w11 * v1[b + 1];
        o[b] = acc;
    }
}

// ---- convex upsampling x 8.  mask [N h w][576], channel 64 k + 8 dy + dx; flow cell slices [2] (x, y).  Thread -> one output pixel
// (n, 8 y + dy, 8 x + dx):  m = max_k mask_k;  e_k = expf(mask_k - m);  out_c = (sum_k e_k * 8 flow_c(y + k / 3 - 1, x + k % 3 - 1))
// / (sum_k e_k), both sums over k = 0 .. 8 in order, zero flow outside the map.  out [N][2][8 h][8 w].
__global__ void raft_upsample_kernel(const float* __restrict__ flow, long long flow_stride, const float* __restrict__ mask, int N, int h, int w,
                                     float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H8 = 8 * h, W8 = 8 * w;
    if (t >= (long long)N * H8 * W8) return;
    const int X = (int)(t % W8), Y = (int)((t / W8) % H8), n = (int)(t / ((long long)W8 * H8));
    const int x = X >> 3, dx = X & 7, y = Y >> 3, dy = Y & 7;
    const long long cell = ((long long)n * h + y) * w + x;
    const float* mk = mask + cell * 576 + 8 * dy + dx;
    float mv[9], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) { mv[k] = mk[64 * k]; mx = fmaxf(mx, mv[k]); }
    float den = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float e = expf(mv[k] - mx);
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        float fx = 0.f, fy = 0.f;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            const float* f = flow + (((long long)n * h + yy) * w + xx) * flow_stride;
            fx = 8.0f * f[0];
            fy = 8.0f * f[1];
        }
        den += e;
        sx += e * fx;
        sy += e * fy;
    }
    const size_t plane = (size_t)H8 * W8;
    float* o = out + (size_t)n * 2 * plane + (size_t)Y * W8 + X;
    o[0] = sx / den;
    o[plane] = sy / den;
}

}  // namespace
