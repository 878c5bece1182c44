// conv_rows.hip -- the image-side glue of the ViT-Adapter backbone (SpatialPriorModule and the tail of ViTAdapter:
// Image/{detection,segmentation}/.../backbones/adapter_modules.py:194-246, vit_adapter.py:110-132) on token rows: an image
// tensor is [B*H*W, C] with C contiguous and rows in (b, y, x) order, the layout every other kernel of the library works on.
//   * me_conv3x3_gather / me_conv3x3_scatter: the unfold of a dense 3x3 convolution (padding 1, stride 1 or 2) and its
//     adjoint; the contraction itself is me_gemm (NT forward, TN weight gradient).
//   * me_maxpool3x3s2_rows / _bwd: MaxPool2d(3, 2, 1) with the winning tap per element.
//   * me_resize_rows_batched / _bwd: bilinear F.interpolate(align_corners=False) with the source scale as an argument.
//   * me_upsample2x_rows / _bwd: the row permutation behind ConvTranspose2d(C, C, 2, 2).
// All of them are memory-bound gathers: one thread per output quad of channels (16 bytes of fp32, 8 of bf16), consecutive
// threads on consecutive channels of a row, one 256-thread workgroup shape and a grid-stride loop for every pyramid size.
// Every backward is written as a gather too -- each output element sums its few contributions in a fixed order, no float
// atomics -- so two runs are bit-identical (the rule of deform.hip and point.hip).
#include "common.h"

namespace {

constexpr int CR_THREADS = 256;
inline unsigned cr_blocks(int64_t items) {
    int64_t b = (items + CR_THREADS - 1) / CR_THREADS;
    if (b > (1 << 20)) b = 1 << 20;
    return (unsigned)(b < 1 ? 1 : b);
}
bool cr_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int conv_out(int n, int s) { return (n - 1) / s + 1; }

// cols[(b, oy, ox), (dy * 3 + dx) * Cin + c] = x[(b, oy s + dy - 1, ox s + dx - 1), c], zero outside the image and in the
// columns past 9 Cin.  VEC: Cin % 4 == 0, so a quad of columns lies inside one tap (or wholly in the padding).
template <bool VEC>
__global__ __launch_bounds__(CR_THREADS) void conv3x3_gather_kernel(const void* __restrict__ x, void* __restrict__ cols, int dt, int H,
                                                                    int W, int Cin, int s, int Ho, int Wo, int Kpad, int64_t total) {
    const int kq = Kpad / 4, K9 = 9 * Cin;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int k = (int)(i % kq) * 4;
        const int64_t row = i / kq;
        const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
        const int64_t b = row / ((int64_t)Wo * Ho);
        const int y0 = oy * s - 1, x0 = ox * s - 1;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            if (k < K9) {
                const int tap = k / Cin, c = k - tap * Cin;
                const int yy = y0 + tap / 3, xx = x0 + tap % 3;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = load4_as_f32(x, dt, ((b * H + yy) * W + xx) * Cin + c);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = k + e;
                if (ke < K9) {
                    const int tap = ke / Cin, c = ke - tap * Cin;
                    const int yy = y0 + tap / 3, xx = x0 + tap % 3;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) v[e] = load1_as_f32(x, dt, ((b * H + yy) * W + xx) * Cin + c);
                }
            }
        }
        store4_from_f32(cols, dt, row * Kpad + k, v);
    }
}

// dx[(b, y, x), c] = sum over the taps (dy, dx), in that order, of dcols[(b, oy, ox), (dy * 3 + dx) * Cin + c] with
// oy s + dy - 1 = y and ox s + dx - 1 = x: the output pixels whose window holds this input pixel.  E = channels per thread.
template <int E>
__global__ __launch_bounds__(CR_THREADS) void conv3x3_scatter_kernel(const void* __restrict__ dcols, int dt, void* __restrict__ dx, int dxt,
                                                                     int H, int W, int Cin, int s, int Ho, int Wo, int Kpad,
                                                                     int64_t total) {
    const int cq = Cin / E;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * E;
        const int64_t pix = i / cq;
        const int px = (int)(pix % W), py = (int)((pix / W) % H);
        const int64_t b = pix / ((int64_t)W * H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int ty = py + 1 - dy;
            if (ty < 0 || ty % s != 0 || ty / s >= Ho) continue;
#pragma unroll
            for (int dxx = 0; dxx < 3; ++dxx) {
                const int tx = px + 1 - dxx;
                if (tx < 0 || tx % s != 0 || tx / s >= Wo) continue;
                const int64_t at = ((b * Ho + ty / s) * Wo + tx / s) * Kpad + (dy * 3 + dxx) * Cin + c;
                if (E == 4) acc += load4_as_f32(dcols, dt, at);
                else acc[0] += load1_as_f32(dcols, dt, at);
            }
        }
        if (E == 4) store4_from_f32(dx, dxt, pix * Cin + c, acc);
        else store1_from_f32(dx, dxt, pix * Cin + c, acc[0]);
    }
}

// MaxPool2d(3, 2, 1): per output element the maximum over the window's taps inside the image, scanned in (dy, dx) order with
// ATen's update rule (a later tap wins only if it is larger, or a NaN), and the winning tap dy * 3 + dx.
__global__ __launch_bounds__(CR_THREADS) void maxpool3x3s2_kernel(const void* __restrict__ x, int xt, void* __restrict__ y, int yt,
                                                                  int8_t* __restrict__ idx, int H, int W, int C, int Ho, int Wo,
                                                                  int64_t total) {
    const int cq = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int64_t row = i / cq;
        const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho);
        const int64_t b = row / ((int64_t)Wo * Ho);
        f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int tap[4] = {-1, -1, -1, -1};
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = oy * 2 - 1 + t / 3, xx = ox * 2 - 1 + t % 3;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const f32x4 v = load4_as_f32(x, xt, ((b * H + yy) * W + xx) * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (tap[e] < 0 || v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; tap[e] = t; }
        }
        store4_from_f32(y, yt, row * C + c, best);
        const uint32_t packed = (uint32_t)(tap[0] & 0xff) | ((uint32_t)(tap[1] & 0xff) << 8) | ((uint32_t)(tap[2] & 0xff) << 16) |
                                ((uint32_t)(tap[3] & 0xff) << 24);
        *reinterpret_cast<uint32_t*>(idx + row * C + c) = packed;
    }
}

// dx[(b, y, x), c] = sum over the at most four windows (oy, ox) that hold (y, x), in (oy, ox) order, of dy[(b, oy, ox), c]
// where that window's winner is this pixel
__global__ __launch_bounds__(CR_THREADS) void maxpool3x3s2_bwd_kernel(const void* __restrict__ dy, int dyt, const int8_t* __restrict__ idx,
                                                                      void* __restrict__ dx, int dxt, int H, int W, int C, int Ho, int Wo,
                                                                      int64_t total) {
    const int cq = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int64_t pix = i / cq;
        const int px = (int)(pix % W), py = (int)((pix / W) % H);
        const int64_t b = pix / ((int64_t)W * H);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        // tap dy of window oy sits at row 2 oy - 1 + dy: an even row is tap 1 of window y / 2, an odd one tap 2 of (y - 1) / 2
        // and tap 0 of (y + 1) / 2
        const int oy0 = py / 2, ny = (py & 1) ? 2 : 1;
        const int ox0 = px / 2, nx = (px & 1) ? 2 : 1;
        for (int a = 0; a < ny; ++a) {
            const int oy = oy0 + a;
            if (oy >= Ho) continue;
            const int ty = py - (2 * oy - 1);
            for (int e2 = 0; e2 < nx; ++e2) {
                const int ox = ox0 + e2;
                if (ox >= Wo) continue;
                const int t = ty * 3 + (px - (2 * ox - 1));
                const int64_t at = ((b * Ho + oy) * Wo + ox) * C + c;
                const uint32_t packed = *reinterpret_cast<const uint32_t*>(idx + at);
                const f32x4 g = load4_as_f32(dy, dyt, at);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((int)((packed >> (8 * e)) & 0xff) == t) acc[e] += g[e];
            }
        }
        store4_from_f32(dx, dxt, pix * C + c, acc);
    }
}

// ATen's bilinear source position of output index o (align_corners = False): s = scale (o + 0.5) - 0.5 clamped at 0, the lower
// tap min((int)s, n - 1), the upper one a step on where there is one, the fraction clamped to [0, 1]
struct LinTap {
    int i0, i1;
    float l;
};
__device__ __forceinline__ LinTap lin_tap(int o, float scale, int n) {
    float f = scale * ((float)o + 0.5f) - 0.5f;
    f = f < 0.f ? 0.f : f;
    LinTap t;
    t.i0 = (int)f;
    t.i0 = t.i0 > n - 1 ? n - 1 : t.i0;
    t.i1 = t.i0 < n - 1 ? t.i0 + 1 : t.i0;
    t.l = f - (float)t.i0;
    t.l = t.l < 0.f ? 0.f : (t.l > 1.f ? 1.f : t.l);
    return t;
}

__global__ __launch_bounds__(CR_THREADS) void resize_rows_batched_kernel(const void* __restrict__ src, int st, void* __restrict__ dst, int dt,
                                                                         int h, int w, int H, int W, int C, float sy, float sx,
                                                                         int64_t total) {
    const int cq = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int64_t row = i / cq;
        const int ox = (int)(row % W), oy = (int)((row / W) % H);
        const int64_t base = (row / ((int64_t)W * H)) * h * w;
        const LinTap ty = lin_tap(oy, sy, h), tx = lin_tap(ox, sx, w);
        const f32x4 v00 = load4_as_f32(src, st, (base + (int64_t)ty.i0 * w + tx.i0) * C + c);
        const f32x4 v01 = load4_as_f32(src, st, (base + (int64_t)ty.i0 * w + tx.i1) * C + c);
        const f32x4 v10 = load4_as_f32(src, st, (base + (int64_t)ty.i1 * w + tx.i0) * C + c);
        const f32x4 v11 = load4_as_f32(src, st, (base + (int64_t)ty.i1 * w + tx.i1) * C + c);
        const f32x4 acc = (1.f - ty.l) * ((1.f - tx.l) * v00 + tx.l * v01) + ty.l * ((1.f - tx.l) * v10 + tx.l * v11);
        store4_from_f32(dst, dt, row * C + c, acc);
    }
}

// candidate outputs of source index i: every o whose unclamped position lies in (i - 1, i + 1), widened by two on either side
// (the kernel recomputes the forward's own taps for each candidate, so a generous range costs time, never correctness); the
// first and last source index also take the clamped outputs at their end
__device__ __forceinline__ void lin_range(int i, float scale, int n, int N, int* lo, int* hi) {
    const float inv = 1.f / scale;
    int a = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 2;
    int b = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 2;
    if (i == 0 || a < 0) a = 0;
    if (i == n - 1 || b > N - 1) b = N - 1;
    *lo = a;
    *hi = b;
}
__device__ __forceinline__ float lin_weight(const LinTap& t, int i) { return (t.i0 == i ? 1.f - t.l : 0.f) + (t.i1 == i ? t.l : 0.f); }

// dsrc[(b, y, x), c] = sum over the outputs (oy, ox), ascending, of wy(oy -> y) wx(ox -> x) ddst[(b, oy, ox), c]
__global__ __launch_bounds__(CR_THREADS) void resize_rows_batched_bwd_kernel(const void* __restrict__ ddst, int dt, void* __restrict__ dsrc,
                                                                             int st, int h, int w, int H, int W, int C, float sy, float sx,
                                                                             int64_t total) {
    const int cq = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int64_t pix = i / cq;
        const int px = (int)(pix % w), py = (int)((pix / w) % h);
        const int64_t base = (pix / ((int64_t)w * h)) * H * W;
        int ylo, yhi, xlo, xhi;
        lin_range(py, sy, h, H, &ylo, &yhi);
        lin_range(px, sx, w, W, &xlo, &xhi);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int oy = ylo; oy <= yhi; ++oy) {
            const float wy = lin_weight(lin_tap(oy, sy, h), py);
            if (wy == 0.f) continue;
            for (int ox = xlo; ox <= xhi; ++ox) {
                const float wx = lin_weight(lin_tap(ox, sx, w), px);
                if (wx == 0.f) continue;
                acc += (wy * wx) * load4_as_f32(ddst, dt, (base + (int64_t)oy * W + ox) * C + c);
            }
        }
        store4_from_f32(dsrc, st, pix * C + c, acc);
    }
}

// out[(b, 2 y + ky, 2 x + kx), c] = y4[(b, y, x), (ky * 2 + kx) * C + c] + bias[c] + add[(b, 2 y + ky, 2 x + kx), c]
__global__ __launch_bounds__(CR_THREADS) void upsample2x_rows_kernel(const void* __restrict__ y4, int yt, const float* __restrict__ bias,
                                                                     const void* __restrict__ add, int at, void* __restrict__ out, int ot,
                                                                     int h, int w, int C, int64_t total) {
    const int cq = C / 4;
    const int W = 2 * w, H = 2 * h;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int64_t row = i / cq;
        const int ox = (int)(row % W), oy = (int)((row / W) % H);
        const int64_t b = row / ((int64_t)W * H);
        const int k = (oy & 1) * 2 + (ox & 1);
        f32x4 v = load4_as_f32(y4, yt, (((b * h + oy / 2) * w + ox / 2) * 4 + k) * C + c);
        if (bias) v += *reinterpret_cast<const f32x4*>(bias + c);
        if (add) v += load4_as_f32(add, at, row * C + c);
        store4_from_f32(out, ot, row * C + c, v);
    }
}

// dy4[(b, y, x), (ky * 2 + kx) * C + c] = dout[(b, 2 y + ky, 2 x + kx), c]
__global__ __launch_bounds__(CR_THREADS) void upsample2x_rows_bwd_kernel(const void* __restrict__ dout, int dt, void* __restrict__ dy4, int yt,
                                                                         int h, int w, int C, int64_t total) {
    const int cq = C / 4;
    for (int64_t i = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CR_THREADS) {
        const int c = (int)(i % cq) * 4;
        const int k = (int)((i / cq) % 4);
        const int64_t row = i / ((int64_t)cq * 4);
        const int x = (int)(row % w), y = (int)((row / w) % h);
        const int64_t b = row / ((int64_t)w * h);
        const f32x4 v = load4_as_f32(dout, dt, ((b * 2 * h + 2 * y + (k >> 1)) * 2 * w + 2 * x + (k & 1)) * C + c);
        store4_from_f32(dy4, yt, (row * 4 + k) * C + c, v);
    }
}

int conv_check(const char* who, const void* a, const void* b, int dt, int B, int H, int W, int Cin, int stride, int Kpad) {
    ME_CHECK_ARG(B >= 0 && H > 0 && W > 0 && Cin > 0, "%s: bad sizes B=%d H=%d W=%d Cin=%d", who, B, H, W, Cin);
    ME_CHECK_ARG(stride == 1 || stride == 2, "%s: stride %d (1 or 2)", who, stride);
    ME_CHECK_ARG(me_dtype_ok(dt), "%s: bad dtype %d", who, dt);
    ME_CHECK_ARG(Kpad >= 9 * Cin && Kpad % 8 == 0, "%s: Kpad=%d must be a multiple of 8 that holds 9 Cin = %d columns", who, Kpad, 9 * Cin);
    ME_CHECK_ARG((int64_t)B * H * W * (int64_t)Kpad < (1ll << 40), "%s: problem too large", who);
    if (B == 0) return ME_OK;
    ME_CHECK_ARG(a && b, "%s: NULL tensor", who);
    return ME_OK;
}

int rows_check(const char* who, const void* a, const void* b, int adt, int bdt, int B, int h, int w, int C) {
    ME_CHECK_ARG(B >= 0 && h > 0 && w > 0 && C > 0, "%s: bad sizes B=%d h=%d w=%d C=%d", who, B, h, w, C);
    ME_CHECK_ARG(C % 4 == 0, "%s: C=%d must be a multiple of 4", who, C);
    ME_CHECK_ARG(me_dtype_ok(adt) && me_dtype_ok(bdt), "%s: bad dtype", who);
    ME_CHECK_ARG((int64_t)B * h * w * (int64_t)C < (1ll << 40), "%s: problem too large", who);
    if (B == 0) return ME_OK;
    ME_CHECK_ARG(a && b, "%s: NULL tensor", who);
    ME_CHECK_ARG(cr_aligned(a, 16) && cr_aligned(b, 16), "%s: tensors must be 16-byte aligned", who);
    return ME_OK;
}

}  // namespace

extern "C" int me_conv3x3_gather(const void* x, int dtype, void* cols, int B, int H, int W, int Cin, int stride, int Kpad, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = conv_check("me_conv3x3_gather", x, cols, dtype, B, H, W, Cin, stride, Kpad);
    if (rc != ME_OK || B == 0) return rc;
    ME_CHECK_ARG(cr_aligned(cols, 16) && cr_aligned(x, Cin % 4 == 0 ? 16 : me_dtype_size(dtype)), "me_conv3x3_gather: misaligned tensor");
    const int Ho = conv_out(H, stride), Wo = conv_out(W, stride);
    const int64_t total = (int64_t)B * Ho * Wo * (Kpad / 4);
    if (Cin % 4 == 0)
        hipLaunchKernelGGL(conv3x3_gather_kernel<true>, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, x, cols, dtype, H, W, Cin, stride,
                           Ho, Wo, Kpad, total);
    else
        hipLaunchKernelGGL(conv3x3_gather_kernel<false>, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, x, cols, dtype, H, W, Cin,
                           stride, Ho, Wo, Kpad, total);
    ME_CHECK_LAUNCH("me_conv3x3_gather");
    return ME_OK;
}

extern "C" int me_conv3x3_scatter(const void* dcols, int dtype, void* dx, int dx_dtype, int B, int H, int W, int Cin, int stride, int Kpad,
                                  void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = conv_check("me_conv3x3_scatter", dcols, dx, dtype, B, H, W, Cin, stride, Kpad);
    if (rc != ME_OK || B == 0) return rc;
    ME_CHECK_ARG(me_dtype_ok(dx_dtype), "me_conv3x3_scatter: bad dx dtype %d", dx_dtype);
    ME_CHECK_ARG(cr_aligned(dcols, 16) && cr_aligned(dx, Cin % 4 == 0 ? 16 : me_dtype_size(dx_dtype)), "me_conv3x3_scatter: misaligned tensor");
    const int Ho = conv_out(H, stride), Wo = conv_out(W, stride);
    if (Cin % 4 == 0) {
        const int64_t total = (int64_t)B * H * W * (Cin / 4);
        hipLaunchKernelGGL(conv3x3_scatter_kernel<4>, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, dcols, dtype, dx, dx_dtype, H, W,
                           Cin, stride, Ho, Wo, Kpad, total);
    } else {
        const int64_t total = (int64_t)B * H * W * Cin;
        hipLaunchKernelGGL(conv3x3_scatter_kernel<1>, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, dcols, dtype, dx, dx_dtype, H, W,
                           Cin, stride, Ho, Wo, Kpad, total);
    }
    ME_CHECK_LAUNCH("me_conv3x3_scatter");
    return ME_OK;
}

extern "C" int me_maxpool3x3s2_rows(const void* x, int x_dtype, void* y, int y_dtype, int8_t* idx, int B, int H, int W, int C,
                                    void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = rows_check("me_maxpool3x3s2_rows", x, y, x_dtype, y_dtype, B, H, W, C);
    if (rc != ME_OK || B == 0) return rc;
    ME_CHECK_ARG(idx && cr_aligned(idx, 4), "me_maxpool3x3s2_rows: idx must be a 4-byte aligned int8 buffer");
    const int Ho = conv_out(H, 2), Wo = conv_out(W, 2);
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, x, x_dtype, y, y_dtype, idx, H, W, C, Ho, Wo,
                       total);
    ME_CHECK_LAUNCH("me_maxpool3x3s2_rows");
    return ME_OK;
}

extern "C" int me_maxpool3x3s2_rows_bwd(const void* dy, int dy_dtype, const int8_t* idx, void* dx, int dx_dtype, int B, int H, int W, int C,
                                        void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = rows_check("me_maxpool3x3s2_rows_bwd", dy, dx, dy_dtype, dx_dtype, B, H, W, C);
    if (rc != ME_OK || B == 0) return rc;
    ME_CHECK_ARG(idx && cr_aligned(idx, 4), "me_maxpool3x3s2_rows_bwd: idx must be a 4-byte aligned int8 buffer");
    const int Ho = conv_out(H, 2), Wo = conv_out(W, 2);
    const int64_t total = (int64_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, dy, dy_dtype, idx, dx, dx_dtype, H, W, C,
                       Ho, Wo, total);
    ME_CHECK_LAUNCH("me_maxpool3x3s2_rows_bwd");
    return ME_OK;
}

extern "C" int me_resize_rows_batched(const void* src, int src_dtype, void* dst, int dst_dtype, int B, int h, int w, int H, int W, int cols,
                                      float scale_y, float scale_x, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = rows_check("me_resize_rows_batched", src, dst, src_dtype, dst_dtype, B, h, w, cols);
    if (rc != ME_OK) return rc;
    ME_CHECK_ARG(H > 0 && W > 0 && scale_y > 0.f && scale_x > 0.f, "me_resize_rows_batched: bad output size %d x %d or scale", H, W);
    if (B == 0) return ME_OK;
    const int64_t total = (int64_t)B * H * W * (cols / 4);
    hipLaunchKernelGGL(resize_rows_batched_kernel, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, src, src_dtype, dst, dst_dtype, h, w, H,
                       W, cols, scale_y, scale_x, total);
    ME_CHECK_LAUNCH("me_resize_rows_batched");
    return ME_OK;
}

extern "C" int me_resize_rows_batched_bwd(const void* ddst, int ddst_dtype, void* dsrc, int dsrc_dtype, int B, int h, int w, int H, int W,
                                          int cols, float scale_y, float scale_x, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = rows_check("me_resize_rows_batched_bwd", ddst, dsrc, ddst_dtype, dsrc_dtype, B, h, w, cols);
    if (rc != ME_OK) return rc;
    ME_CHECK_ARG(H > 0 && W > 0 && scale_y > 0.f && scale_x > 0.f, "me_resize_rows_batched_bwd: bad output size %d x %d or scale", H, W);
    if (B == 0) return ME_OK;
    const int64_t total = (int64_t)B * h * w * (cols / 4);
    hipLaunchKernelGGL(resize_rows_batched_bwd_kernel, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, ddst, ddst_dtype, dsrc, dsrc_dtype,
                       h, w, H, W, cols, scale_y, scale_x, total);
    ME_CHECK_LAUNCH("me_resize_rows_batched_bwd");
    return ME_OK;
}

extern "C" int me_upsample2x_rows(const void* y4, int y4_dtype, const float* bias, const void* add, int add_dtype, void* out, int out_dtype,
                                  int B, int h, int w, int C, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = rows_check("me_upsample2x_rows", y4, out, y4_dtype, out_dtype, B, h, w, C);
    if (rc != ME_OK || B == 0) return rc;
    ME_CHECK_ARG((!bias || cr_aligned(bias, 16)) && (!add || (cr_aligned(add, 16) && me_dtype_ok(add_dtype))),
                 "me_upsample2x_rows: bias / add must be 16-byte aligned, add fp32 or bf16");
    const int64_t total = (int64_t)B * h * w * 4 * (C / 4);
    hipLaunchKernelGGL(upsample2x_rows_kernel, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, y4, y4_dtype, bias, add, add_dtype, out,
                       out_dtype, h, w, C, total);
    ME_CHECK_LAUNCH("me_upsample2x_rows");
    return ME_OK;
}

extern "C" int me_upsample2x_rows_bwd(const void* dout, int dout_dtype, void* dy4, int dy4_dtype, int B, int h, int w, int C, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = rows_check("me_upsample2x_rows_bwd", dout, dy4, dout_dtype, dy4_dtype, B, h, w, C);
    if (rc != ME_OK || B == 0) return rc;
    const int64_t total = (int64_t)B * h * w * 4 * (C / 4);
    hipLaunchKernelGGL(upsample2x_rows_bwd_kernel, dim3(cr_blocks(total)), dim3(CR_THREADS), 0, stream, dout, dout_dtype, dy4, dy4_dtype, h, w,
                       C, total);
    ME_CHECK_LAUNCH("me_upsample2x_rows_bwd");
    return ME_OK;
}
