// colsum.hip -- column sums of a [rows, cols] matrix in two stages (bias gradients: me_colsum; layer-scale gradients, the
// column sums of an element-wise product: me_colsum_mul).  HBM-bound: coalesced reads, fp32 partial sums, a fixed fold order.
#include "common.h"

namespace {

// ---- column sums (bias gradients): stage 1: grid (col blocks of 256, row splits); each thread owns 4 columns? no:
// lanes own single columns (coalesced 2/4-byte reads across the wave are fine for this size); 4 waves x splits rows.
constexpr int CS_SPLITS = 128;
// rows [rb, re) of the row split blockIdx.y
__device__ __forceinline__ void cs_row_range(int64_t rows, int64_t& rb, int64_t& re) {
    const int64_t rows_per = (rows + CS_SPLITS - 1) / CS_SPLITS;
    rb = (int64_t)blockIdx.y * rows_per;
    re = rb + rows_per < rows ? rb + rows_per : rows;
}
// the four waves' sums (a: this wave's; V = f32x4 for a lane's four columns, float for one) meet in LDS; wave 0 stores the block's
// partial at column c
template <typename V>
__device__ __forceinline__ void cs_fold_store(V (*sh)[64], V a, int w, int lane, int64_t c, int64_t cols, float* __restrict__ partial) {
    sh[w][lane] = a;
    __syncthreads();
    if (w == 0 && c < cols)
        *reinterpret_cast<V*>(partial + (int64_t)blockIdx.y * cols + c) = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}
// vector path (cols % 4 == 0): a lane owns 4 consecutive columns (8/16-byte loads), a wave covers 256 columns of a
// row, the 4 waves of a block and blockIdx.y split the rows; 4 rows in flight per wave.
// (dtype is a template parameter: a runtime switch around each load would put a vmcnt(0) at every branch join and
// serialise the four rows in flight)
template <typename T> __device__ __forceinline__ f32x4 cs_ld4(const void* base, int64_t idx);
template <> __device__ __forceinline__ f32x4 cs_ld4<float>(const void* base, int64_t idx) {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + idx);
}
template <> __device__ __forceinline__ f32x4 cs_ld4<bf16_t>(const void* base, int64_t idx) {
    const u32x2 raw = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(base) + idx);
    return f32x4{__uint_as_float(raw[0] << 16), __uint_as_float(raw[0] & 0xffff0000u), __uint_as_float(raw[1] << 16),
                 __uint_as_float(raw[1] & 0xffff0000u)};
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_vec_kernel(const void* __restrict__ x, int64_t ldx,
                                                                 int64_t rows, int64_t cols, float* __restrict__ partial) {
    __shared__ f32x4 sh[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * 4;
    int64_t rb, re;
    cs_row_range(rows, rb, re);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    if (c < cols) {
        int64_t r = rb + w;
        for (; r + 28 < re; r += 32) {
            const f32x4 v0 = cs_ld4<T>(x, r * ldx + c), v1 = cs_ld4<T>(x, (r + 4) * ldx + c);
            const f32x4 v2 = cs_ld4<T>(x, (r + 8) * ldx + c), v3 = cs_ld4<T>(x, (r + 12) * ldx + c);
            const f32x4 v4 = cs_ld4<T>(x, (r + 16) * ldx + c), v5 = cs_ld4<T>(x, (r + 20) * ldx + c);
            const f32x4 v6 = cs_ld4<T>(x, (r + 24) * ldx + c), v7 = cs_ld4<T>(x, (r + 28) * ldx + c);
            a0 += v0 + v4; a1 += v1 + v5; a2 += v2 + v6; a3 += v3 + v7;
        }
        for (; r < re; r += 4) a0 += cs_ld4<T>(x, r * ldx + c);
    }
    cs_fold_store(sh, (a0 + a1) + (a2 + a3), w, lane, c, cols, partial);
}
__global__ __launch_bounds__(256) void colsum_partial_kernel(const void* __restrict__ x, int xdt, int64_t ldx, int64_t rows,
                                                             int64_t cols, float* __restrict__ partial) {
    // scalar fallback.  block: 64 columns x 4 row-lanes; blockIdx.y = row split
    __shared__ float sh[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + lane;
    int64_t rb, re;
    cs_row_range(rows, rb, re);
    float a = 0.f;
    if (c < cols)
        for (int64_t r = rb + w; r < re; r += 4) a += load1_as_f32(x, xdt, r * ldx + c);
    cs_fold_store(sh, a, w, lane, c, cols, partial);
}
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, int64_t cols,
                                                           float* __restrict__ out, int accumulate) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float a = 0.f;
    for (int s = 0; s < CS_SPLITS; ++s) a += partial[(int64_t)s * cols + c];
    out[c] = accumulate ? out[c] + a : a;
}

// out[c] = sum_r x[r,c] * y[r,c]  (layer-scale gradients: d gamma = colsum(dy * branch)); same split / fold as colsum
__global__ __launch_bounds__(256) void colsum_mul_partial_kernel(const void* __restrict__ x, int xdt, int64_t ldx,
                                                                 const void* __restrict__ y, int ydt, int64_t ldy,
                                                                 int64_t rows, int64_t cols, float* __restrict__ partial) {
    __shared__ f32x4 sh[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * 4;
    int64_t rb, re;
    cs_row_range(rows, rb, re);
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c < cols)
        for (int64_t r = rb + w; r < re; r += 4) a += load4_as_f32(x, xdt, r * ldx + c) * load4_as_f32(y, ydt, r * ldy + c);
    cs_fold_store(sh, a, w, lane, c, cols, partial);
}

}  // namespace

extern "C" size_t me_colsum_workspace(int64_t cols) { return (size_t)CS_SPLITS * (size_t)cols * sizeof(float); }

extern "C" int me_colsum(const void* x, int x_dtype, int64_t ldx, int64_t rows, int64_t cols, float* out, int accumulate,
                         void* workspace, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && out && workspace && rows > 0 && cols > 0, "me_colsum: bad args");
    ME_CHECK_ARG(me_dtype_ok(x_dtype), "me_colsum: bad dtype");
    float* partial = reinterpret_cast<float*>(workspace);
    if (cols % 4 == 0 && ldx % 4 == 0 && (uintptr_t)x % 16 == 0) {
        dim3 grid((unsigned)((cols + 255) / 256), CS_SPLITS);
        if (x_dtype == ME_BF16)
            hipLaunchKernelGGL(colsum_partial_vec_kernel<bf16_t>, grid, dim3(256), 0, stream, x, ldx, rows, cols, partial);
        else
            hipLaunchKernelGGL(colsum_partial_vec_kernel<float>, grid, dim3(256), 0, stream, x, ldx, rows, cols, partial);
    } else {
        dim3 grid((unsigned)((cols + 63) / 64), CS_SPLITS);
        hipLaunchKernelGGL(colsum_partial_kernel, grid, dim3(256), 0, stream, x, x_dtype, ldx, rows, cols, partial);
    }
    ME_CHECK_LAUNCH("me_colsum(partial)");
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, partial, cols, out,
                       accumulate);
    ME_CHECK_LAUNCH("me_colsum(final)");
    return ME_OK;
}

extern "C" int me_colsum_mul(const void* x, int x_dtype, int64_t ldx, const void* y, int y_dtype, int64_t ldy, int64_t rows,
                             int64_t cols, float* out, int accumulate, void* workspace, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && y && out && workspace && rows > 0 && cols > 0, "me_colsum_mul: bad args");
    ME_CHECK_ARG(me_dtype_ok(x_dtype) && me_dtype_ok(y_dtype), "me_colsum_mul: bad dtype");
    ME_CHECK_ARG(cols % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, "me_colsum_mul: cols and row strides must be multiples of 4");
    ME_CHECK_ARG(aligned4(x, x_dtype) && aligned4(y, y_dtype) && aligned4(workspace, ME_F32),
                 "me_colsum_mul: x and y must be aligned to four elements of their type, the workspace to 16 bytes");
    float* partial = reinterpret_cast<float*>(workspace);
    dim3 grid((unsigned)((cols + 255) / 256), CS_SPLITS);
    hipLaunchKernelGGL(colsum_mul_partial_kernel, grid, dim3(256), 0, stream, x, x_dtype, ldx, y, y_dtype, ldy, rows, cols, partial);
    ME_CHECK_LAUNCH("me_colsum_mul(partial)");
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, partial, cols, out,
                       accumulate);
    ME_CHECK_LAUNCH("me_colsum_mul(final)");
    return ME_OK;
}
