// raft.hip -- RAFT-large optical flow (torchvision's raft_large) for the trajectory preprocessing: the dtk_raft_* entries of
// include/dtk.h.  The kernels are in raft_conv.h (the implicit-GEMM convolution and the correlation GEMM on the matrix cores)
// and raft_stages.h (instance norm, pyramid pooling, lookup, convex upsampling); this file checks arguments, lays out the
// workspace and launches.
#include "raft_conv.h"
#include "raft_stages.h"

namespace {

bool on_device(const void* p) {
    if (p == nullptr) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

size_t conv_cin_pad(int cin) { return (size_t)((cin + RC_K - 1) / RC_K) * RC_K; }
size_t conv_cout_pad(int cout) { return (size_t)((cout + 63) / 64) * 64; }

int check_conv_desc(const dtk_raft_conv_desc& d, const char* what) {
    DTK_REQUIRE(d.w_hi != nullptr && d.bias != nullptr, "%s: null weights", what);
    DTK_REQUIRE(d.cin >= 1 && d.cout >= 1 && d.kh >= 1 && d.kw >= 1 && d.kh <= 7 && d.kw <= 7, "%s: bad kernel %d x %d, %d -> %d", what,
                d.kh, d.kw, d.cin, d.cout);
    DTK_REQUIRE(d.stride == 1 || d.stride == 2, "%s: stride %d", what, d.stride);
    DTK_REQUIRE(d.pad_h >= 0 && d.pad_w >= 0 && d.pad_h < d.kh && d.pad_w < d.kw, "%s: bad padding", what);
    DTK_REQUIRE(d.inv_wscale > 0.f, "%s: inv_wscale must be positive", what);
    return DTK_OK;
}

// One convolution.  `in2` (with in_split) is the second source of the input channels; out / res / mul / gate are channel slices.
struct ConvIO {
    const float* in; int64_t in_stride; const float* in2; int64_t in2_stride; int in_split;
    float* out; int64_t out_stride;
    int act; const float* res; int64_t res_stride; int res_relu; const float* mul; int64_t mul_stride; const float* gate;
    int64_t gate_stride;
};

int launch_conv(const dtk_raft_conv_desc& d, const ConvIO& io, int N, int H, int W, int mode, hipStream_t st) {
    ConvP p;
    p.in = io.in; p.in_stride = io.in_stride; p.in2 = io.in2; p.in2_stride = io.in2_stride; p.split = io.in2 ? io.in_split : d.cin;
    p.N = N; p.H = H; p.W = W; p.Cin = d.cin;
    p.Ho = (H + 2 * d.pad_h - d.kh) / d.stride + 1;
    p.Wo = (W + 2 * d.pad_w - d.kw) / d.stride + 1;
    p.KH = d.kh; p.KW = d.kw; p.stride = d.stride; p.ph = d.pad_h; p.pw = d.pad_w;
    p.CinPad = (int)conv_cin_pad(d.cin);
    p.Kpad = d.kh * d.kw * p.CinPad;
    p.w_hi = (const _Float16*)d.w_hi; p.w_lo = (const _Float16*)d.w_lo; p.bias = d.bias; p.inv_ws = d.inv_wscale;
    p.out = io.out; p.out_stride = io.out_stride; p.Cout = d.cout;
    p.act = io.act; p.res = io.res; p.res_stride = io.res_stride; p.res_relu = io.res_relu; p.mul = io.mul; p.mul_stride = io.mul_stride;
    p.gate = io.gate; p.gate_stride = io.gate_stride;
    p.M = (long long)N * p.Ho * p.Wo;
    DTK_REQUIRE(p.Ho >= 1 && p.Wo >= 1 && p.M >= 1 && p.M < (1ll << 31), "raft conv: bad output size %d x %d x %d", N, p.Ho, p.Wo);
    DTK_REQUIRE((long long)N * H * W < (1ll << 31), "raft conv: more than 2^31 input pixels");
    DTK_REQUIRE(mode == DTK_RAFT_SPLIT || mode == DTK_RAFT_FP16, "raft conv: unknown operand mode %d", mode);
    DTK_REQUIRE(mode == DTK_RAFT_FP16 || d.w_lo != nullptr, "raft conv: the split mode needs the lo weight plane");
    DTK_REQUIRE(io.in2 == nullptr || (io.in_split % RC_K == 0 && io.in_split > 0 && io.in_split < d.cin),
                "raft conv: the second input must start at a multiple of %d channels", RC_K);
    // 16-byte loads need every 4-channel group aligned; anything else (Cin = 2, 3, a slice at an odd offset) loads by element
    auto al = [](const float* q, int64_t s) { return q == nullptr || (((uintptr_t)q & 15) == 0 && s % 4 == 0); };
    p.vec_in = d.cin % 4 == 0 && p.split % 4 == 0 && al(io.in, io.in_stride) && al(io.in2, io.in2_stride);
    p.vec_out = al(io.out, io.out_stride) && al(io.res, io.res_stride) && al(io.mul, io.mul_stride) && al(io.gate, io.gate_stride);
    const dim3 block(256);
    const int gm = dtk_cdiv(p.M, RC_M);
    if (d.cout <= 16) {
        const dim3 grid(gm, 1);
        if (mode == DTK_RAFT_SPLIT) DTK_LAUNCH("raft_conv_split_n16", (raft_conv_kernel<true, 1>), grid, block, 0, st, p);
        else DTK_LAUNCH("raft_conv_fp16_n16", (raft_conv_kernel<false, 1>), grid, block, 0, st, p);
    } else {
        const dim3 grid(gm, dtk_cdiv(d.cout, 64));
        if (mode == DTK_RAFT_SPLIT) DTK_LAUNCH("raft_conv_split", (raft_conv_kernel<true, 4>), grid, block, 0, st, p);
        else DTK_LAUNCH("raft_conv_fp16", (raft_conv_kernel<false, 4>), grid, block, 0, st, p);
    }
    return DTK_OK;
}

int in_chunks(long long hw) {
    long long c = (hw + 511) / 512;
    return (int)(c < 1 ? 1 : (c > 128 ? 128 : c));
}

int launch_instance_norm(const float* x, const float* res, float* out, int N, int H, int W, int C, float eps, int relu,
                         float* ws, hipStream_t st) {
    const long long hw = (long long)H * W;
    const int chunks = in_chunks(hw);
    const int subs = 256 / C;
    DTK_LAUNCH("raft_in_stats", raft_in_stats_kernel, dim3(chunks, N), dim3(C * subs), 0, st, x, ws, (int)hw, C, chunks);
    DTK_LAUNCH("raft_in_apply", raft_in_apply_kernel, dim3(chunks, N), dim3(C * subs), 0, st, x, res, out, ws, (int)hw, C, chunks, eps,
               relu);
    return DTK_OK;
}

void level_sizes(int h, int w, int* hl, int* wl) {
    hl[0] = h; wl[0] = w;
    for (int l = 1; l < 4; ++l) { hl[l] = hl[l - 1] / 2; wl[l] = wl[l - 1] / 2; }
}

int launch_pyramid(const float* f1, const float* f2, int N, int h, int w, int C, int mode, float* pyr, hipStream_t st) {
    int hl[4], wl[4];
    level_sizes(h, w, hl, wl);
    const int hw = h * w;
    CorrP p;
    p.f1 = f1; p.f2 = f2; p.out = pyr; p.hw = hw; p.C = C; p.scale = 1.0f / sqrtf((float)C);
    const dim3 grid(dtk_cdiv(hw, RC_M), dtk_cdiv(hw, 64), N);
    if (mode == DTK_RAFT_SPLIT) DTK_LAUNCH("raft_corr_split", (raft_corr_kernel<true>), grid, dim3(256), 0, st, p);
    else DTK_LAUNCH("raft_corr_fp16", (raft_corr_kernel<false>), grid, dim3(256), 0, st, p);
    float* prev = pyr;
    for (int l = 1; l < 4; ++l) {
        float* cur = prev + (size_t)N * hw * hl[l - 1] * wl[l - 1];
        const long long total = (long long)N * hw * hl[l] * wl[l];
        DTK_LAUNCH("raft_corr_pool", raft_corr_pool_kernel, dim3(dtk_cdiv(total, 256)), dim3(256), 0, st, prev, cur, total, hl[l - 1],
                   wl[l - 1], hl[l], wl[l]);
        prev = cur;
    }
    return DTK_OK;
}

int launch_lookup(const float* pyr, const float* flow, int64_t flow_stride, int N, int h, int w, float* out, int64_t out_stride,
                  hipStream_t st) {
    const long long total = (long long)N * h * w * 36;
    DTK_LAUNCH("raft_lookup", raft_lookup_kernel, dim3(dtk_cdiv(total, 256)), dim3(256), 0, st, pyr, flow, (long long)flow_stride, N, h, w,
               out, (long long)out_stride);
    return DTK_OK;
}

int launch_upsample(const float* flow, int64_t flow_stride, const float* mask, int N, int h, int w, float* out, hipStream_t st) {
    const long long total = (long long)N * h * w * 64;
    DTK_LAUNCH("raft_upsample", raft_upsample_kernel, dim3(dtk_cdiv(total, 256)), dim3(256), 0, st, flow, (long long)flow_stride, mask, N,
               h, w, out);
    return DTK_OK;
}

// the workspace of dtk_raft_forward, in floats
struct Layout {
    size_t img, e[3], ds, fmap, hx, corr, t256, t128, cf, z, rh, mask, pyr, in_ws, total;
};

bool raft_sizes_ok(int N, int H, int W) {
    return N >= 1 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && H / 8 >= 16 && W / 8 >= 16 &&
           (long long)2 * N * (H / 2) * (W / 2) < (1ll << 31) && (long long)N * H * W < (1ll << 31);
}

Layout make_layout(int N, int H, int W) {
    Layout L;
    const size_t P2 = (size_t)(H / 2) * (W / 2), P4 = (size_t)(H / 4) * (W / 4), P8 = (size_t)(H / 8) * (W / 8);
    const size_t M = (size_t)N * P8;
    int hl[4], wl[4];
    level_sizes(H / 8, W / 8, hl, wl);
    size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 63) / 64 * 64; return at; };
    L.img = take((size_t)2 * N * H * W * 3);
    for (int k = 0; k < 3; ++k) L.e[k] = take((size_t)2 * N * P2 * 64);
    L.ds = take((size_t)2 * N * P4 * 96);
    L.fmap = take((size_t)2 * N * P8 * 256);
    L.hx = take(M * 384);
    L.corr = take(M * 324);
    L.t256 = take(M * 256);
    L.t128 = take(M * 128);
    L.cf = take(M * 256);
    L.z = take(M * 128);
    L.rh = take(M * 128);
    L.mask = take(M * 576);
    size_t cells = 0;
    for (int l = 0; l < 4; ++l) cells += (size_t)hl[l] * wl[l];
    L.pyr = take(M * cells);
    L.in_ws = take((size_t)2 * N * 128 * 128 * 3);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

size_t dtk_raft_conv_packed_halves(int32_t cout, int32_t cin, int32_t kh, int32_t kw) {
    if (cout < 1 || cin < 1 || kh < 1 || kw < 1 || kh > 7 || kw > 7) return 0;
    return conv_cout_pad(cout) * (size_t)kh * kw * conv_cin_pad(cin);
}

int dtk_raft_conv_pack(const float* w, int32_t cout, int32_t cin, int32_t kh, int32_t kw, float wscale, void* w_hi, void* w_lo,
                       void* stream) {
    const size_t n = dtk_raft_conv_packed_halves(cout, cin, kh, kw);
    DTK_REQUIRE(n > 0, "dtk_raft_conv_pack: bad shape %d x %d x %d x %d", cout, cin, kh, kw);
    DTK_REQUIRE(on_device(w) && on_device(w_hi) && on_device(w_lo), "dtk_raft_conv_pack: host or null pointer");
    DTK_REQUIRE(wscale > 0.f, "dtk_raft_conv_pack: wscale must be positive");
    hipStream_t st = dtk_stream(stream);
    DTK_LAUNCH("raft_conv_pack", raft_conv_pack_kernel, dim3(dtk_cdiv((long long)n, 256)), dim3(256), 0, st, w, cout, cin, kh, kw,
               (int)conv_cin_pad(cin), (long long)n, wscale, (_Float16*)w_hi, (_Float16*)w_lo);
    return DTK_OK;
}

int dtk_raft_conv(const dtk_raft_conv_args* a, void* stream) {
    DTK_REQUIRE(a != nullptr, "dtk_raft_conv: null arguments");
    if (int rc = check_conv_desc(a->conv, "dtk_raft_conv")) return rc;
    DTK_REQUIRE(a->N >= 1 && a->H >= 1 && a->W >= 1, "dtk_raft_conv: bad input size");
    DTK_REQUIRE(on_device(a->in) && on_device(a->out) && on_device(a->conv.w_hi) && on_device(a->conv.bias) &&
                    (a->in2 == nullptr || on_device(a->in2)) && (a->res == nullptr || on_device(a->res)) &&
                    (a->mul == nullptr || on_device(a->mul)) && (a->gate == nullptr || on_device(a->gate)) &&
                    (a->conv.w_lo == nullptr || on_device(a->conv.w_lo)),
                "dtk_raft_conv: host or null pointer");
    DTK_REQUIRE(a->act >= DTK_RAFT_ACT_NONE && a->act <= DTK_RAFT_ACT_TANH, "dtk_raft_conv: unknown activation %d", a->act);
    const int c1 = a->in2 ? a->in_split : a->conv.cin;
    DTK_REQUIRE(a->in_stride >= c1 && (a->in2 == nullptr || a->in2_stride >= a->conv.cin - c1) && a->out_stride >= a->conv.cout &&
                    (a->res == nullptr || a->res_stride >= a->conv.cout) && (a->mul == nullptr || a->mul_stride >= a->conv.cout) &&
                    (a->gate == nullptr || a->gate_stride >= a->conv.cout),
                "dtk_raft_conv: a channel stride is smaller than its slice");
    ConvIO io{a->in, a->in_stride, a->in2, a->in2_stride, a->in_split, a->out, a->out_stride, a->act, a->res, a->res_stride,
              a->res_relu, a->mul, a->mul_stride, a->gate, a->gate_stride};
    return launch_conv(a->conv, io, a->N, a->H, a->W, a->mode, dtk_stream(stream));
}

size_t dtk_raft_instance_norm_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
    if (N < 1 || H < 1 || W < 1 || C < 1 || C > 256) return 0;
    return (size_t)N * in_chunks((long long)H * W) * C * 3 * sizeof(float);
}

int dtk_raft_instance_norm(const float* x, const float* res, float* out, int32_t N, int32_t H, int32_t W, int32_t C, float eps,
                           int32_t relu, void* workspace, size_t workspace_bytes, void* stream) {
    const size_t need = dtk_raft_instance_norm_workspace_bytes(N, H, W, C);
    DTK_REQUIRE(need > 0 && (long long)N * H * W < (1ll << 31) && N < 65536, "dtk_raft_instance_norm: bad size %d x %d x %d x %d", N, H, W,
                C);
    DTK_REQUIRE(on_device(x) && on_device(out) && on_device(workspace) && (res == nullptr || on_device(res)),
                "dtk_raft_instance_norm: host or null pointer");
    if (workspace_bytes < need) {
        dtk_set_error("dtk_raft_instance_norm: workspace %zu < %zu bytes", workspace_bytes, need);
        return DTK_E_WORKSPACE;
    }
    return launch_instance_norm(x, res, out, N, H, W, C, eps, relu, (float*)workspace, dtk_stream(stream));
}

size_t dtk_raft_pyramid_floats(int32_t N, int32_t h, int32_t w) {
    if (N < 1 || h < 16 || w < 16) return 0;
    int hl[4], wl[4];
    level_sizes(h, w, hl, wl);
    size_t cells = 0;
    for (int l = 0; l < 4; ++l) cells += (size_t)hl[l] * wl[l];
    return (size_t)N * h * w * cells;
}

int dtk_raft_corr_pyramid(const float* f1, const float* f2, int32_t N, int32_t h, int32_t w, int32_t C, int32_t mode, float* pyramid,
                          void* stream) {
    DTK_REQUIRE(N >= 1 && N < 65536 && h >= 16 && w >= 16 && (long long)h * w < 65536 * 64, "dtk_raft_corr_pyramid: the feature map must "
                "be at least 16 x 16 (got %d x %d, batch %d)", h, w, N);
    DTK_REQUIRE(C >= RC_K && C % RC_K == 0, "dtk_raft_corr_pyramid: C must be a multiple of %d", RC_K);
    DTK_REQUIRE(mode == DTK_RAFT_SPLIT || mode == DTK_RAFT_FP16, "dtk_raft_corr_pyramid: unknown operand mode %d", mode);
    DTK_REQUIRE(on_device(f1) && on_device(f2) && on_device(pyramid), "dtk_raft_corr_pyramid: host or null pointer");
    return launch_pyramid(f1, f2, N, h, w, C, mode, pyramid, dtk_stream(stream));
}

int dtk_raft_lookup(const float* pyramid, const float* flow, int64_t flow_stride, int32_t N, int32_t h, int32_t w, float* out,
                    int64_t out_stride, void* stream) {
    DTK_REQUIRE(N >= 1 && h >= 16 && w >= 16 && (long long)N * h * w * 36 < (1ll << 31), "dtk_raft_lookup: bad size %d x %d x %d", N, h, w);
    DTK_REQUIRE(flow_stride >= 2 && out_stride >= 324, "dtk_raft_lookup: a channel stride is smaller than its slice");
    DTK_REQUIRE(on_device(pyramid) && on_device(flow) && on_device(out), "dtk_raft_lookup: host or null pointer");
    return launch_lookup(pyramid, flow, flow_stride, N, h, w, out, out_stride, dtk_stream(stream));
}

int dtk_raft_upsample(const float* flow, int64_t flow_stride, const float* mask, int32_t N, int32_t h, int32_t w, float* out,
                      void* stream) {
    DTK_REQUIRE(N >= 1 && h >= 1 && w >= 1 && (long long)N * h * w * 64 < (1ll << 31), "dtk_raft_upsample: bad size %d x %d x %d", N, h, w);
    DTK_REQUIRE(flow_stride >= 2, "dtk_raft_upsample: flow_stride below 2");
    DTK_REQUIRE(on_device(flow) && on_device(mask) && on_device(out), "dtk_raft_upsample: host or null pointer");
    return launch_upsample(flow, flow_stride, mask, N, h, w, out, dtk_stream(stream));
}

size_t dtk_raft_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    if (!raft_sizes_ok(N, H, W)) return 0;
    return make_layout(N, H, W).total * sizeof(float);
}

int dtk_raft_forward(const dtk_raft_model* m, const float* image1, const float* image2, int32_t N, int32_t H, int32_t W,
                     int32_t num_flow_updates, int32_t mode, float* flow_out, void* workspace, size_t workspace_bytes, void* stream) {
    DTK_REQUIRE(m != nullptr, "dtk_raft_forward: null model");
    DTK_REQUIRE(N >= 1 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0, "dtk_raft_forward: the image size must be divisible by 8, got "
                "%d x %d (batch %d)", H, W, N);
    DTK_REQUIRE(H / 8 >= 16 && W / 8 >= 16, "dtk_raft_forward: the feature map must be at least 16 x 16 (images of 128 x 128), got "
                "%d x %d", H / 8, W / 8);
    DTK_REQUIRE(raft_sizes_ok(N, H, W), "dtk_raft_forward: batch %d of %d x %d is too large for 32-bit pixel indices", N, H, W);
    DTK_REQUIRE(num_flow_updates >= 1, "dtk_raft_forward: num_flow_updates %d", num_flow_updates);
    DTK_REQUIRE(mode == DTK_RAFT_SPLIT || mode == DTK_RAFT_FP16, "dtk_raft_forward: unknown operand mode %d", mode);
    DTK_REQUIRE(on_device(image1) && on_device(image2) && on_device(flow_out) && on_device(workspace),
                "dtk_raft_forward: host or null pointer");
    for (int k = 0; k < DTK_RAFT_NUM_CONVS; ++k) {
        if (int rc = check_conv_desc(m->conv[k], "dtk_raft_forward")) return rc;
        DTK_REQUIRE(on_device(m->conv[k].w_hi) && on_device(m->conv[k].bias) && (mode == DTK_RAFT_FP16 || on_device(m->conv[k].w_lo)),
                    "dtk_raft_forward: convolution %d has host or null weights", k);
    }
    const Layout L = make_layout(N, H, W);
    if (workspace_bytes < L.total * sizeof(float)) {
        dtk_set_error("dtk_raft_forward: workspace %zu < %zu bytes", workspace_bytes, L.total * sizeof(float));
        return DTK_E_WORKSPACE;
    }
    hipStream_t st = dtk_stream(stream);
    float* ws = (float*)workspace;
    const int h = H / 8, w = W / 8;
    const long long M = (long long)N * h * w;

    auto conv = [&](int k, const float* in, int64_t is, float* out, int64_t os, int n, int hh, int ww, int act, const float* res = nullptr,
                    int64_t rs = 0, int res_relu = 0) {
        ConvIO io{in, is, nullptr, 0, 0, out, os, act, res, rs, res_relu, nullptr, 0, nullptr, 0};
        return launch_conv(m->conv[k], io, n, hh, ww, mode, st);
    };
#define RAFT_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

    // images: [N][3][H][W] x 2 -> [2N][H][W][3]
    {
        const long long total = (long long)2 * N * H * W;
        DTK_LAUNCH("raft_images_nhwc", raft_images_nhwc_kernel, dim3(dtk_cdiv(total, 256)), dim3(256), 0, st, image1, image2, ws + L.img, N,
                   H * W);
    }
    float* inws = ws + L.in_ws;
    // ---- the two encoders: base 0 = feature (instance norm, both images), base 16 = context (BatchNorm folded, image 1)
    for (int enc = 0; enc < 2; ++enc) {
        const int base = enc == 0 ? DTK_RAFT_FEATURE : DTK_RAFT_CONTEXT;
        const int n = enc == 0 ? 2 * N : N;
        const bool inorm = enc == 0;
        float *x = ws + L.e[0], *t1 = ws + L.e[1], *t2 = ws + L.e[2], *ds = ws + L.ds;
        int hh = H / 2, ww = W / 2, c = 64;
        RAFT_TRY(conv(base, ws + L.img, 3, x, 64, n, H, W, inorm ? DTK_RAFT_ACT_NONE : DTK_RAFT_ACT_RELU));
        if (inorm) RAFT_TRY(launch_instance_norm(x, nullptr, x, n, hh, ww, c, 1e-5f, 1, inws, st));
        int k = base + 1;
        for (int layer = 0; layer < 3; ++layer) {
            for (int blk = 0; blk < 2; ++blk) {
                const bool down = layer > 0 && blk == 0;
                const int cin = c, ih = hh, iw = ww;
                if (down) { c = layer == 1 ? 96 : 128; hh /= 2; ww /= 2; }
                const int k1 = k, k2 = k + 1, kd = k + 2;
                k += down ? 3 : 2;
                if (inorm) {
                    RAFT_TRY(conv(k1, x, cin, t1, c, n, ih, iw, DTK_RAFT_ACT_NONE));
                    RAFT_TRY(launch_instance_norm(t1, nullptr, t1, n, hh, ww, c, 1e-5f, 1, inws, st));
                    RAFT_TRY(conv(k2, t1, c, t2, c, n, hh, ww, DTK_RAFT_ACT_NONE));
                    const float* skip = x;
                    if (down) {
                        RAFT_TRY(conv(kd, x, cin, ds, c, n, ih, iw, DTK_RAFT_ACT_NONE));
                        RAFT_TRY(launch_instance_norm(ds, nullptr, ds, n, hh, ww, c, 1e-5f, 0, inws, st));
                        skip = ds;
                    }
                    RAFT_TRY(launch_instance_norm(t2, skip, x, n, hh, ww, c, 1e-5f, 1, inws, st));   // x = relu(skip + relu(norm(t2)))
                } else {
                    RAFT_TRY(conv(k1, x, cin, t1, c, n, ih, iw, DTK_RAFT_ACT_RELU));
                    const float* skip = x;
                    if (down) {
                        RAFT_TRY(conv(kd, x, cin, ds, c, n, ih, iw, DTK_RAFT_ACT_NONE));
                        skip = ds;
                    }
                    RAFT_TRY(conv(k2, t1, c, t2, c, n, hh, ww, DTK_RAFT_ACT_RELU, skip, c, 1));   // t2 = relu(skip + relu(conv))
                    float* sw = x; x = t2; t2 = sw;
                }
            }
        }
        if (enc == 0) {
            RAFT_TRY(conv(base + 15, x, 128, ws + L.fmap, 256, n, h, w, DTK_RAFT_ACT_NONE));
        } else {
            RAFT_TRY(conv(DTK_RAFT_CONTEXT_HIDDEN, x, 128, ws + L.hx, 384, n, h, w, DTK_RAFT_ACT_TANH));
            RAFT_TRY(conv(DTK_RAFT_CONTEXT_CONTEXT, x, 128, ws + L.hx + 128, 384, n, h, w, DTK_RAFT_ACT_RELU));
        }
    }
    RAFT_TRY(launch_pyramid(ws + L.fmap, ws + L.fmap + (size_t)M * 256, N, h, w, 256, mode, ws + L.pyr, st));
    float* hx = ws + L.hx;
    float* flow = hx + 382;
    DTK_LAUNCH("raft_zero_flow", raft_zero_flow_kernel, dim3(dtk_cdiv(M, 256)), dim3(256), 0, st, flow, 384ll, M);

    for (int it = 0; it < num_flow_updates; ++it) {
        RAFT_TRY(launch_lookup(ws + L.pyr, flow, 384, N, h, w, ws + L.corr, 324, st));
        RAFT_TRY(conv(DTK_RAFT_MOTION + 0, ws + L.corr, 324, ws + L.t256, 256, N, h, w, DTK_RAFT_ACT_RELU));
        RAFT_TRY(conv(DTK_RAFT_MOTION + 1, ws + L.t256, 256, ws + L.cf, 256, N, h, w, DTK_RAFT_ACT_RELU));
        RAFT_TRY(conv(DTK_RAFT_MOTION + 2, flow, 384, ws + L.t128, 128, N, h, w, DTK_RAFT_ACT_RELU));
        RAFT_TRY(conv(DTK_RAFT_MOTION + 3, ws + L.t128, 128, ws + L.cf + 192, 256, N, h, w, DTK_RAFT_ACT_RELU));
        RAFT_TRY(conv(DTK_RAFT_MOTION + 4, ws + L.cf, 256, hx + 256, 384, N, h, w, DTK_RAFT_ACT_RELU));
        for (int g = 0; g < 2; ++g) {
            const int kz = DTK_RAFT_GRU + 3 * g;
            RAFT_TRY(conv(kz, hx, 384, ws + L.z, 128, N, h, w, DTK_RAFT_ACT_SIGMOID));
            {   // rh = sigmoid(convr([h, x])) * h
                ConvIO io{hx, 384, nullptr, 0, 0, ws + L.rh, 128, DTK_RAFT_ACT_SIGMOID, nullptr, 0, 0, hx, 384, nullptr, 0};
                RAFT_TRY(launch_conv(m->conv[kz + 1], io, N, h, w, mode, st));
            }
            {   // h = (1 - z) h + z tanh(convq([rh, x])), in place: the convolution does not read h
                ConvIO io{ws + L.rh, 128, hx + 128, 384, 128, hx, 384, DTK_RAFT_ACT_TANH, nullptr, 0, 0, nullptr, 0, ws + L.z, 128};
                RAFT_TRY(launch_conv(m->conv[kz + 2], io, N, h, w, mode, st));
            }
        }
        RAFT_TRY(conv(DTK_RAFT_FLOW_HEAD, hx, 384, ws + L.t256, 256, N, h, w, DTK_RAFT_ACT_RELU));
        RAFT_TRY(conv(DTK_RAFT_FLOW_HEAD + 1, ws + L.t256, 256, flow, 384, N, h, w, DTK_RAFT_ACT_NONE, flow, 384, 0));   // flow += delta
    }
    RAFT_TRY(conv(DTK_RAFT_MASK, hx, 384, ws + L.t256, 256, N, h, w, DTK_RAFT_ACT_RELU));
    RAFT_TRY(conv(DTK_RAFT_MASK + 1, ws + L.t256, 256, ws + L.mask, 576, N, h, w, DTK_RAFT_ACT_NONE));
    RAFT_TRY(launch_upsample(flow, 384, ws + L.mask, N, h, w, flow_out, st));
#undef RAFT_TRY
    return DTK_OK;
}

}  // extern "C"
