// patchify.hip -- the Data2Seq patch gather and its adjoint: me_patchify, me_unpatchify_add (the exact-fp32 and
// odd-kernel-size route of the patch embed; integer index math, bit-exact).
#include "common.h"

namespace {

// ---- patch gather: cols[(b, pt, py, px), (c, dt, dy, dx)] = x[b, c, pt*st+dt, py*sh+dy, px*sw+dx]
struct PatchGeom {
    int B, Cin, T, H, W, kt, kh, kw, st, sh, sw, gt, gh, gw;
};
// element offset in x of index i of the gathered matrix, whose rows hold feat = Cin * kt * kh * kwx entries: kwx steps of dxs pixels
// along a patch row (kw steps of 1; the quad kernels: kw / 4 steps of 4)
__device__ __forceinline__ int64_t patch_offset(const PatchGeom& g, int64_t i, int64_t feat, int kwx, int dxs) {
    int64_t t = i / feat, f = i - t * feat;
    const int dx = (int)(f % kwx) * dxs; f /= kwx;
    const int dy = (int)(f % g.kh); f /= g.kh;
    const int dt = (int)(f % g.kt); f /= g.kt;
    const int c = (int)f;
    const int px = (int)(t % g.gw); t /= g.gw;
    const int py = (int)(t % g.gh); t /= g.gh;
    const int pt = (int)(t % g.gt); t /= g.gt;
    const int b = (int)t;
    return ((((int64_t)b * g.Cin + c) * g.T + (pt * g.st + dt)) * g.H + (py * g.sh + dy)) * g.W + (px * g.sw + dx);
}
__global__ __launch_bounds__(EW_THREADS) void patchify_kernel(const void* __restrict__ x, int xdt, void* __restrict__ out,
                                                              int odt, PatchGeom g) {
    const int64_t feat = (int64_t)g.Cin * g.kt * g.kh * g.kw;
    const int64_t ntok = (int64_t)g.B * g.gt * g.gh * g.gw;
    const int64_t total = ntok * feat;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS)
        store1_from_f32(out, odt, i, load1_as_f32(x, xdt, patch_offset(g, i, feat, g.kw, 1)));
}
// The same gather four features at a time (kw % 4 == 0: four consecutive dx of one patch row are four consecutive pixels): one index
// decomposition per quad, one 8 / 16-byte store per thread -- consecutive threads write consecutive bytes of the gathered matrix -- and a
// vector load where the source quad is aligned (x, W and sw multiples of 4 elements: the image / tubelet embeds), four scalar loads
// otherwise (the spectrogram's stride 10).  The scalar kernel above: 225 us for 256 images (0.7 TB/s); this one: see DESIGN.md.
__global__ __launch_bounds__(EW_THREADS) void patchify4_kernel(const void* __restrict__ x, int xdt, void* __restrict__ out, int odt, PatchGeom g,
                                                               int aligned) {
    const int64_t feat4 = (int64_t)g.Cin * g.kt * g.kh * (g.kw / 4);
    const int64_t ntok = (int64_t)g.B * g.gt * g.gh * g.gw;
    const int64_t total = ntok * feat4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t src = patch_offset(g, i, feat4, g.kw / 4, 4);
        f32x4 v;
        if (aligned) {
            v = load4_as_f32(x, xdt, src);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = load1_as_f32(x, xdt, src + e);
        }
        store4_from_f32(out, odt, i * 4, v);
    }
}
__global__ __launch_bounds__(EW_THREADS) void unpatchify_add_kernel(const void* __restrict__ dcols, int ddt,
                                                                    float* __restrict__ dx_out, PatchGeom g) {
    const int64_t feat = (int64_t)g.Cin * g.kt * g.kh * g.kw;
    const int64_t ntok = (int64_t)g.B * g.gt * g.gh * g.gw;
    const int64_t total = ntok * feat;
    const bool overlap = g.st < g.kt || g.sh < g.kh || g.sw < g.kw;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t dst = patch_offset(g, i, feat, g.kw, 1);
        const float v = load1_as_f32(dcols, ddt, i);
        if (overlap) atomicAdd(dx_out + dst, v);
        else dx_out[dst] += v;
    }
}
int make_geom(PatchGeom& g, int B, int Cin, int T, int H, int W, int kt, int kh, int kw, int st, int sh, int sw) {
    ME_CHECK_ARG(B > 0 && Cin > 0 && T > 0 && H > 0 && W > 0 && kt > 0 && kh > 0 && kw > 0 && st > 0 && sh > 0 && sw > 0,
                 "patchify: bad geometry");
    ME_CHECK_ARG(T >= kt && H >= kh && W >= kw, "patchify: kernel larger than input");
    g = PatchGeom{B, Cin, T, H, W, kt, kh, kw, st, sh, sw, (T - kt) / st + 1, (H - kh) / sh + 1, (W - kw) / sw + 1};
    return ME_OK;
}

}  // namespace

// non-overlapping patches (stride >= kernel on every axis), kw % 4 == 0, aligned quads: the scatter four pixels at a time
__global__ __launch_bounds__(EW_THREADS) void unpatchify_add4_kernel(const void* __restrict__ dcols, int ddt, float* __restrict__ dx_out, PatchGeom g) {
    const int64_t feat4 = (int64_t)g.Cin * g.kt * g.kh * (g.kw / 4);
    const int64_t ntok = (int64_t)g.B * g.gt * g.gh * g.gw;
    const int64_t total = ntok * feat4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * EW_THREADS) {
        f32x4* q = reinterpret_cast<f32x4*>(dx_out + patch_offset(g, i, feat4, g.kw / 4, 4));
        *q = *q + load4_as_f32(dcols, ddt, i * 4);
    }
}

extern "C" int me_patchify(const void* x, int x_dtype, void* cols, int cols_dtype, int B, int Cin, int T, int H, int W,
                           int kt, int kh, int kw, int st, int sh, int sw, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && cols, "me_patchify: null pointer");
    ME_CHECK_ARG(me_dtype_ok(x_dtype) && me_dtype_ok(cols_dtype), "me_patchify: bad dtype");
    PatchGeom g;
    int rc = make_geom(g, B, Cin, T, H, W, kt, kh, kw, st, sh, sw);
    if (rc) return rc;
    const int64_t total = (int64_t)B * g.gt * g.gh * g.gw * Cin * kt * kh * kw;
    if (kw % 4 == 0 && (uintptr_t)cols % 16 == 0) {
        // (source quads aligned: every row start and every patch column offset a multiple of 4 elements, the base 16-byte aligned)
        const int aligned = (W % 4 == 0 && sw % 4 == 0 && (uintptr_t)x % 16 == 0) ? 1 : 0;
        hipLaunchKernelGGL(patchify4_kernel, dim3(grid_blocks(total / 4)), dim3(EW_THREADS), 0, stream, x, x_dtype, cols, cols_dtype, g, aligned);
    } else {
        hipLaunchKernelGGL(patchify_kernel, dim3(grid_blocks(total)), dim3(EW_THREADS), 0, stream, x, x_dtype, cols, cols_dtype, g);
    }
    ME_CHECK_LAUNCH("me_patchify");
    return ME_OK;
}

extern "C" int me_unpatchify_add(const void* dcols, int dcols_dtype, float* dx, int B, int Cin, int T, int H, int W, int kt,
                                 int kh, int kw, int st, int sh, int sw, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(dcols && dx, "me_unpatchify_add: null pointer");
    ME_CHECK_ARG(me_dtype_ok(dcols_dtype), "me_unpatchify_add: bad dtype");
    PatchGeom g;
    int rc = make_geom(g, B, Cin, T, H, W, kt, kh, kw, st, sh, sw);
    if (rc) return rc;
    const int64_t total = (int64_t)B * g.gt * g.gh * g.gw * Cin * kt * kh * kw;
    const bool overlap = st < kt || sh < kh || sw < kw;
    if (!overlap && kw % 4 == 0 && W % 4 == 0 && sw % 4 == 0 && (uintptr_t)dx % 16 == 0 && (uintptr_t)dcols % 16 == 0) {
        hipLaunchKernelGGL(unpatchify_add4_kernel, dim3(grid_blocks(total / 4)), dim3(EW_THREADS), 0, stream, dcols, dcols_dtype, dx, g);
        ME_CHECK_LAUNCH("me_unpatchify_add");
        return ME_OK;
    }
    hipLaunchKernelGGL(unpatchify_add_kernel, dim3(grid_blocks(total)), dim3(EW_THREADS), 0, stream, dcols, dcols_dtype, dx, g);
    ME_CHECK_LAUNCH("me_unpatchify_add");
    return ME_OK;
}
