// elementwise.hip -- token-row operations: pos-embed row adds (me_add_rows), window partition / merge (me_window_rows), dropout /
// drop-path with the residual add (me_dropout_add), pos-embed table resize (me_resize_rows), token pooling (me_pool_tokens / _bwd).
// All of these are bandwidth-bound integer/index or element-wise work: coalesced 16-byte accesses, grid-stride
// loops, no LDS.
#include "common.h"

namespace {

__global__ __launch_bounds__(EW_THREADS) void add_rows_kernel(const void* __restrict__ x, int xdt,
                                                              const void* __restrict__ pos, int pdt, void* __restrict__ y,
                                                              int ydt, int64_t rows, int64_t pos_rows, int cols) {
    const int c4 = cols / 4;
    const int64_t total = rows * c4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t r = i / c4;
        const int c = (int)(i % c4) * 4;
        f32x4 v = load4_as_f32(x, xdt, r * cols + c);
        v += load4_as_f32(pos, pdt, (r % pos_rows) * cols + c);
        store4_from_f32(y, ydt, r * cols + c, v);
    }
}

}  // namespace

extern "C" int me_add_rows(const void* x, int x_dtype, const void* pos, int pos_dtype, void* y, int y_dtype, int64_t rows,
                           int64_t pos_rows, int cols, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && pos && y && rows > 0 && pos_rows > 0 && cols > 0 && cols % 4 == 0, "me_add_rows: bad args");
    ME_CHECK_ARG(me_dtype_ok(x_dtype) && me_dtype_ok(pos_dtype) && me_dtype_ok(y_dtype), "me_add_rows: bad dtype");
    ME_CHECK_ARG(aligned4(x, x_dtype) && aligned4(pos, pos_dtype) && aligned4(y, y_dtype),
                 "me_add_rows: x, pos and y must be aligned to four elements of their type");
    hipLaunchKernelGGL(add_rows_kernel, dim3(grid_blocks(rows * (cols / 4))), dim3(EW_THREADS), 0, stream, x, x_dtype, pos,
                       pos_dtype, y, y_dtype, rows, pos_rows, cols);
    ME_CHECK_LAUNCH("me_add_rows");
    return ME_OK;
}

namespace {

// ---- window partition / merge of token rows (windowed attention, Image/detection/.../base/vit.py:160-190).
// Tokens of one image are rows (y, x) of an H x W grid; windows of ws x ws tile the grid padded up to multiples of ws.
// partition: win[(b, wy, wx), (iy, ix)] = tok[b, wy*ws + iy, wx*ws + ix]  or 0 outside the grid (the reference zero-pads
// q, k, v AFTER the qkv Linear, so padded keys take part in the softmax with score 0 and value 0); merge is the inverse
// gather (padded rows are dropped).  Same-dtype 16-byte row-chunk copies; pure integer index arithmetic (bit-exact).
__global__ __launch_bounds__(EW_THREADS) void window_rows_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int B,
                                                                 int H, int W, int ws, int chunks, int merge) {
    const int gh = (H + ws - 1) / ws, gw = (W + ws - 1) / ws;
    const int64_t win_rows = (int64_t)B * gh * gw * ws * ws, tok_rows = (int64_t)B * H * W;
    const int64_t total = (merge ? tok_rows : win_rows) * chunks;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t r = i / chunks;
        const int c = (int)(i % chunks);
        if (merge) {
            const int x = (int)(r % W), y = (int)((r / W) % H);
            const int64_t b = r / ((int64_t)W * H);
            const int64_t wr = (((b * gh + y / ws) * gw + x / ws) * ws + y % ws) * ws + x % ws;
            dst[i] = src[wr * chunks + c];
        } else {
            const int ix = (int)(r % ws), iy = (int)((r / ws) % ws);
            const int64_t w = r / ((int64_t)ws * ws);
            const int wx = (int)(w % gw), wy = (int)((w / gw) % gh);
            const int64_t b = w / ((int64_t)gw * gh);
            const int y = wy * ws + iy, x = wx * ws + ix;
            dst[i] = (y < H && x < W) ? src[((b * H + y) * W + x) * chunks + c] : u32x4{0u, 0u, 0u, 0u};
        }
    }
}

}  // namespace

extern "C" int me_window_rows(const void* src, void* dst, int dtype, int B, int H, int W, int window, int cols, int merge,
                              void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(src && dst && B > 0 && H > 0 && W > 0 && window > 0 && cols > 0, "me_window_rows: bad args");
    ME_CHECK_ARG(me_dtype_ok(dtype), "me_window_rows: bad dtype");
    const int64_t row_bytes = (int64_t)cols * (int64_t)me_dtype_size(dtype);
    ME_CHECK_ARG(row_bytes % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0,
                 "me_window_rows: rows must be multiples of 16 bytes, 16-byte aligned");
    const int chunks = (int)(row_bytes / 16);
    const int gh = (H + window - 1) / window, gw = (W + window - 1) / window;
    const int64_t rows = merge ? (int64_t)B * H * W : (int64_t)B * gh * gw * window * window;
    hipLaunchKernelGGL(window_rows_kernel, dim3(grid_blocks(rows * chunks)), dim3(EW_THREADS), 0, stream,
                       reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), B, H, W, window, chunks, merge);
    ME_CHECK_LAUNCH("me_window_rows");
    return ME_OK;
}

namespace {

// ---- dropout / drop-path with residual add.  Counter-based RNG (splitmix64 of seed + element index): the same
// (seed, index) regenerates the same mask in backward, nothing is stored.
__global__ __launch_bounds__(EW_THREADS) void dropout_add_kernel(const void* __restrict__ v, int vdt,
                                                                 const void* __restrict__ res, int rdt,
                                                                 void* __restrict__ out, int odt, int64_t rows, int cols,
                                                                 int64_t rows_per_sample, float p_drop, float p_path,
                                                                 uint64_t seed, const float* __restrict__ colscale) {
    const int c4 = cols / 4;
    const int64_t total = rows * c4;
    const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const float inv_path = p_path > 0.f ? 1.0f / (1.0f - p_path) : 1.0f;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t r = i / c4;
        const int c = (int)(i % c4) * 4;
        float rowscale = 1.0f;
        if (p_path > 0.f) {
            const uint64_t sample = (uint64_t)(r / rows_per_sample);
            rowscale = u01_hash(seed ^ 0xD1B54A32D192ED03ull, sample) >= p_path ? inv_path : 0.0f;
        }
        f32x4 x = load4_as_f32(v, vdt, r * cols + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float k = rowscale;
            if (p_drop > 0.f) k = u01_hash(seed, (uint64_t)(r * cols + c + e)) >= p_drop ? k * inv_keep : 0.0f;
            x[e] *= k;
        }
        if (colscale) x *= *reinterpret_cast<const f32x4*>(colscale + c);
        if (res) x += load4_as_f32(res, rdt, r * cols + c);
        store4_from_f32(out, odt, r * cols + c, x);
    }
}

}  // namespace

extern "C" int me_dropout_add(const void* v, int v_dtype, const void* res, int res_dtype, void* out, int out_dtype,
                              int64_t rows, int cols, int64_t rows_per_sample, float p_drop, float p_path, uint64_t seed, const float* colscale,
                              void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(v && out && rows > 0 && cols > 0 && cols % 4 == 0 && rows_per_sample > 0, "me_dropout_add: bad args");
    ME_CHECK_ARG(me_dtype_ok(v_dtype) && me_dtype_ok(out_dtype) && (!res || me_dtype_ok(res_dtype)), "me_dropout_add: bad dtype");
    ME_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f && p_path >= 0.f && p_path < 1.f, "me_dropout_add: probabilities must be in [0, 1)");
    ME_CHECK_ARG(aligned4(v, v_dtype) && (!res || aligned4(res, res_dtype)) && aligned4(out, out_dtype) && aligned4(colscale, ME_F32),
                 "me_dropout_add: v, res, out and colscale must be aligned to four elements of their type");
    hipLaunchKernelGGL(dropout_add_kernel, dim3(grid_blocks(rows * (cols / 4))), dim3(EW_THREADS), 0, stream, v, v_dtype, res,
                       res_dtype, out, out_dtype, rows, cols, rows_per_sample, p_drop, p_path, seed, colscale);
    ME_CHECK_LAUNCH("me_dropout_add");
    return ME_OK;
}

namespace {

// ---- position-embedding table resize (cls/pos-embed glue).
// Replaces TIMMVisionTransformer.resize_pos_embed (Image/detection/mmdet_custom/models/backbones/base/vit.py:459-486:
// reshape the [h*w, C] table to [1, C, h, w], F.interpolate(size=(H, W), mode, align_corners=False), flatten back) on the
// token-major layout directly: rows are grid positions, channels contiguous -- no permutes.  The sampling arithmetic is
// ATen's upsample_bicubic2d / upsample_bilinear2d, written out: source coordinate s = (in/out) * (d + 0.5) - 0.5 (bilinear
// clamps it at 0, bicubic does not), cubic-convolution weights with A = -0.75, taps clamped to the table edge, fp32.
__device__ __forceinline__ float cubic1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cubic2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
__global__ __launch_bounds__(EW_THREADS) void resize_rows_kernel(const void* __restrict__ src, int src_dtype, void* __restrict__ dst,
                                                                 int dst_dtype, int h, int w, int H, int W, int C, int mode) {
    const int cq = C / 4;
    const int64_t total = (int64_t)H * W * cq;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int ox = (int)((i / cq) % W), oy = (int)(i / ((int64_t)cq * W));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (mode == 1) {                 // bicubic
            const float fy = sy * ((float)oy + 0.5f) - 0.5f, fx = sx * ((float)ox + 0.5f) - 0.5f;
            const float fly = floorf(fy), flx = floorf(fx);
            const int iy = (int)fly, ix = (int)flx;
            const float ty = fy - fly, tx = fx - flx;
            const float A = -0.75f;
            const float wy[4] = {cubic2(ty + 1.f, A), cubic1(ty, A), cubic1(1.f - ty, A), cubic2(2.f - ty, A)};
            const float wx[4] = {cubic2(tx + 1.f, A), cubic1(tx, A), cubic1(1.f - tx, A), cubic2(2.f - tx, A)};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                int yy = iy - 1 + a;
                yy = yy < 0 ? 0 : (yy > h - 1 ? h - 1 : yy);
                f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    int xx = ix - 1 + b;
                    xx = xx < 0 ? 0 : (xx > w - 1 ? w - 1 : xx);
                    row += wx[b] * load4_as_f32(src, src_dtype, ((int64_t)yy * w + xx) * C + c);
                }
                acc += wy[a] * row;
            }
        } else {                         // bilinear
            float fy = sy * ((float)oy + 0.5f) - 0.5f, fx = sx * ((float)ox + 0.5f) - 0.5f;
            fy = fy < 0.f ? 0.f : fy;
            fx = fx < 0.f ? 0.f : fx;
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 < h - 1 ? y0 + 1 : y0, x1 = x0 < w - 1 ? x0 + 1 : x0;
            const float ly = fy - (float)y0, lx = fx - (float)x0;
            const f32x4 v00 = load4_as_f32(src, src_dtype, ((int64_t)y0 * w + x0) * C + c);
            const f32x4 v01 = load4_as_f32(src, src_dtype, ((int64_t)y0 * w + x1) * C + c);
            const f32x4 v10 = load4_as_f32(src, src_dtype, ((int64_t)y1 * w + x0) * C + c);
            const f32x4 v11 = load4_as_f32(src, src_dtype, ((int64_t)y1 * w + x1) * C + c);
            acc = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
        }
        store4_from_f32(dst, dst_dtype, ((int64_t)oy * W + ox) * C + c, acc);
    }
}

}  // namespace

extern "C" int me_resize_rows(const void* src, int src_dtype, void* dst, int dst_dtype, int h, int w, int H, int W, int cols,
                              int mode, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(src && dst && h > 0 && w > 0 && H > 0 && W > 0 && cols > 0 && cols % 4 == 0, "me_resize_rows: bad args");
    ME_CHECK_ARG(me_dtype_ok(src_dtype) && me_dtype_ok(dst_dtype), "me_resize_rows: bad dtype");
    ME_CHECK_ARG(mode == ME_RESIZE_BILINEAR || mode == ME_RESIZE_BICUBIC, "me_resize_rows: mode %d (bilinear / bicubic only)", mode);
    ME_CHECK_ARG(aligned4(src, src_dtype) && aligned4(dst, dst_dtype), "me_resize_rows: src and dst must be aligned to four elements of their type");
    hipLaunchKernelGGL(resize_rows_kernel, dim3(grid_blocks((int64_t)H * W * (cols / 4))), dim3(EW_THREADS), 0, stream, src,
                       src_dtype, dst, dst_dtype, h, w, H, W, cols, mode);
    ME_CHECK_LAUNCH("me_resize_rows");
    return ME_OK;
}

namespace {

// ---- token pooling in front of the task heads: [B, N, C] tokens -> [B, C] features.
// Replaces x.mean(1) ahead of fc_norm (Video/models/modeling_finetune.py:445-454), x[:, 0] (cls token, same lines) and
// the 'max' / 'avg' global features of the PointCloud ClsHead (openpoints/models/classification/cls_base.py:126-133).
// One pass over the tokens, 4 channels per thread (coalesced along C), fp32 accumulation; max also records the arg-max
// token per channel (first index on ties, as torch.max) for the backward.
__global__ __launch_bounds__(EW_THREADS) void pool_tokens_kernel(const void* __restrict__ x, int x_dtype, float* __restrict__ out,
                                                                 int32_t* __restrict__ arg, int B, int N, int C, int mode) {
    const int cq = C / 4;
    const int64_t total = (int64_t)B * cq;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int c = (int)(i % cq) * 4, b = (int)(i / cq);
        const int64_t base = (int64_t)b * N * C + c;
        f32x4 acc = load4_as_f32(x, x_dtype, base);
        if (mode == ME_POOL_MEAN) {
            for (int n = 1; n < N; ++n) acc += load4_as_f32(x, x_dtype, base + (int64_t)n * C);
            acc *= 1.0f / (float)N;
        } else if (mode == ME_POOL_MAX) {
            int a[4] = {0, 0, 0, 0};
            for (int n = 1; n < N; ++n) {
                const f32x4 v = load4_as_f32(x, x_dtype, base + (int64_t)n * C);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > acc[e]) { acc[e] = v[e]; a[e] = n; }
            }
            if (arg) {
#pragma unroll
                for (int e = 0; e < 4; ++e) arg[(int64_t)b * C + c + e] = a[e];
            }
        }
        *reinterpret_cast<f32x4*>(out + (int64_t)b * C + c) = acc;
    }
}
__global__ __launch_bounds__(EW_THREADS) void pool_tokens_bwd_kernel(const float* __restrict__ dy, const int32_t* __restrict__ arg,
                                                                     void* __restrict__ dx, int dx_dtype, int B, int N, int C, int mode) {
    const int cq = C / 4;
    const int64_t total = (int64_t)B * N * cq;
    const float inv = 1.0f / (float)N;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int n = (int)((i / cq) % N), b = (int)(i / ((int64_t)cq * N));
        const f32x4 g = *reinterpret_cast<const f32x4*>(dy + (int64_t)b * C + c);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (mode == ME_POOL_MEAN) v = g * inv;
        else if (mode == ME_POOL_MAX) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = arg[(int64_t)b * C + c + e] == n ? g[e] : 0.f;
        } else if (n == 0) v = g;
        store4_from_f32(dx, dx_dtype, ((int64_t)b * N + n) * C + c, v);
    }
}

}  // namespace

extern "C" int me_pool_tokens(const void* x, int x_dtype, float* out, int32_t* argmax, int B, int N, int C, int mode, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && out && B > 0 && N > 0 && C > 0 && C % 4 == 0, "me_pool_tokens: bad args");
    ME_CHECK_ARG(me_dtype_ok(x_dtype), "me_pool_tokens: bad dtype");
    ME_CHECK_ARG(mode == ME_POOL_MEAN || mode == ME_POOL_MAX || mode == ME_POOL_FIRST, "me_pool_tokens: bad mode %d", mode);
    ME_CHECK_ARG(aligned4(x, x_dtype) && aligned4(out, ME_F32), "me_pool_tokens: x and out must be aligned to four elements of their type");
    hipLaunchKernelGGL(pool_tokens_kernel, dim3(grid_blocks((int64_t)B * (C / 4))), dim3(EW_THREADS), 0, stream, x, x_dtype, out,
                       argmax, B, N, C, mode);
    ME_CHECK_LAUNCH("me_pool_tokens");
    return ME_OK;
}

extern "C" int me_pool_tokens_bwd(const float* dy, const int32_t* argmax, void* dx, int dx_dtype, int B, int N, int C, int mode,
                                  void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(dy && dx && B > 0 && N > 0 && C > 0 && C % 4 == 0, "me_pool_tokens_bwd: bad args");
    ME_CHECK_ARG(me_dtype_ok(dx_dtype), "me_pool_tokens_bwd: bad dtype");
    ME_CHECK_ARG(mode == ME_POOL_MEAN || mode == ME_POOL_FIRST || (mode == ME_POOL_MAX && argmax),
                 "me_pool_tokens_bwd: bad mode %d (max needs the forward's argmax)", mode);
    ME_CHECK_ARG(aligned4(dy, ME_F32) && aligned4(dx, dx_dtype), "me_pool_tokens_bwd: dy and dx must be aligned to four elements of their type");
    hipLaunchKernelGGL(pool_tokens_bwd_kernel, dim3(grid_blocks((int64_t)B * N * (C / 4))), dim3(EW_THREADS), 0, stream, dy, argmax, dx,
                       dx_dtype, B, N, C, mode);
    ME_CHECK_LAUNCH("me_pool_tokens_bwd");
    return ME_OK;
}
