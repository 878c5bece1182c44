// optim.hip -- the fused optimizer on the flat parameter bucket: AdamW (me_adamw_step) and the fine-tune recipe around it
// (me_grad_stats, me_adamw_prepare, me_adamw_step_segments).  HBM-bound element-wise passes over the four fp32 streams.
#include "common.h"

namespace {

__device__ __forceinline__ float adamw_update(float& pi, float gi, float& mi, float& vi, float lr, float b1, float b2, float eps, float wd,
                                              float bc1, float bc2_sqrt) {
    pi *= (1.0f - lr * wd);
    mi = b1 * mi + (1.0f - b1) * gi;
    vi = b2 * vi + (1.0f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    return pi;
}
// element i of the bucket: load, update, the three stores and the bf16 mirror
__device__ __forceinline__ void adamw_element(float* p, const float* g, float* m, float* v, int64_t i, float gscale, float lr, float b1,
                                              float b2, float eps, float wd, float bc1, float bc2_sqrt, bf16_t* mirror) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_update(pi, g[i] * gscale, mi, vi, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
    if (mirror) mirror[i] = (bf16_t)pi;
}
// VEC: four elements per lane (16-byte accesses on the four fp32 streams, 8 bytes on the bf16 mirror); the launcher takes it when the
// slice's addresses allow it, the n % 4 tail goes through block 0's first lanes.  Same arithmetic per element either way.
template <bool VEC>
__global__ __launch_bounds__(EW_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                           float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                           float gscale, bf16_t* __restrict__ mirror) {
    if (VEC) {
        const int64_t n4 = n / 4;
        for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS) {
            f32x4 pv = *reinterpret_cast<const f32x4*>(p + i * 4), mv = *reinterpret_cast<const f32x4*>(m + i * 4),
                  vv = *reinterpret_cast<const f32x4*>(v + i * 4);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pi = pv[e], mi = mv[e], vi = vv[e];
                adamw_update(pi, gv[e] * gscale, mi, vi, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
                pv[e] = pi; mv[e] = mi; vv[e] = vi;
            }
            *reinterpret_cast<f32x4*>(m + i * 4) = mv;
            *reinterpret_cast<f32x4*>(v + i * 4) = vv;
            *reinterpret_cast<f32x4*>(p + i * 4) = pv;
            if (mirror) {
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (bf16_t)pv[e];
                *reinterpret_cast<bf16x4*>(mirror + i * 4) = o;
            }
        }
        if (blockIdx.x != 0 || (int64_t)threadIdx.x >= n - n4 * 4) return;
        adamw_element(p, g, m, v, n4 * 4 + threadIdx.x, gscale, lr, b1, b2, eps, wd, bc1, bc2_sqrt, mirror);
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * EW_THREADS)
        adamw_element(p, g, m, v, i, gscale, lr, b1, b2, eps, wd, bc1, bc2_sqrt, mirror);
}

}  // namespace

extern "C" int me_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             void* bf16_mirror, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1, "me_adamw_step: bad args");
    if (n == 0) return ME_OK;
    const float bc1 = 1.0f - powf(beta1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    const bool vec = n >= 4 && (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 &&
                     ((uintptr_t)bf16_mirror & 7) == 0;
    if (vec)
        hipLaunchKernelGGL(adamw_kernel<true>, dim3(grid_blocks(n / 4)), dim3(EW_THREADS), 0, stream, param, grad, exp_avg, exp_avg_sq, n, lr,
                           beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, reinterpret_cast<bf16_t*>(bf16_mirror));
    else
        hipLaunchKernelGGL(adamw_kernel<false>, dim3(grid_blocks(n)), dim3(EW_THREADS), 0, stream, param, grad, exp_avg, exp_avg_sq, n, lr,
                           beta1, beta2, eps, weight_decay, bc1, bc2_sqrt, grad_scale, reinterpret_cast<bf16_t*>(bf16_mirror));
    ME_CHECK_LAUNCH("me_adamw_step");
    return ME_OK;
}

namespace {

// ---- fine-tune recipe of the fused optimizer: what the reference's training loops wrap around AdamW --
// layer-wise lr decay / no-decay parameter groups (Video/optim_factory.py:28-41, 56-95;
// Image/segmentation/mmcv_custom/layer_decay_optimizer_constructor.py:17-41), GradScaler.unscale_ + clip_grad_norm_ and the
// skipped step on a non-finite gradient (Video/utils.py:376-404) -- on the flat bucket, with the decisions taken ON THE
// DEVICE: no host round trip between backward and the optimizer step.
//   grad_stats_kernel + grad_stats_fold_kernel : L2 norm and number of non-finite values of the bucket (deterministic
//                                                two-level sum of squares in double)
//   adamw_prepare_kernel                       : one thread: total norm, clip coefficient, found-inf, the step counter and its
//                                                bias corrections -> me_adamw_ctl
//   adamw_seg_kernel                           : the AdamW pass with a per-segment (lr scale, weight decay) table in LDS
constexpr int GS_BLOCKS = 1024;
__global__ __launch_bounds__(EW_THREADS) void grad_stats_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
    // the squares are formed and summed in DOUBLE: the gradients are still multiplied by the loss scale here (the unscale is
    // part of adamw_prepare), and a finite gradient whose scaled square leaves the fp32 range must not read as non-finite --
    // GradScaler.unscale_ divides first and only then looks for inf (Video/utils.py:388-392).  HBM-bound either way.
    double ss = 0.0;
    float bad = 0.f;
    auto take = [&](float x) {
        const bool nf = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;                  // inf or nan
        const double d = nf ? 0.0 : (double)x;                                              // (counted, not summed)
        ss = __builtin_fma(d, d, ss);
        bad += nf ? 1.f : 0.f;
    };
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) take(v[e]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) take(g[n4 * 4 + threadIdx.x]);
    __shared__ double sh[2][EW_THREADS / 64];
    double dss = ss, dbad = bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { dss += __shfl_xor(dss, o, 64); dbad += __shfl_xor(dbad, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = dss; sh[1][threadIdx.x >> 6] = dbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, b = 0;
        for (int w = 0; w < EW_THREADS / 64; ++w) { a += sh[0][w]; b += sh[1][w]; }
        part[blockIdx.x * 2] = a;
        part[blockIdx.x * 2 + 1] = b;
    }
}
__global__ __launch_bounds__(64) void grad_stats_fold_kernel(const double* __restrict__ part, int nb, float* __restrict__ stats) {
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nb; i += 64) { a += part[i * 2]; b += part[i * 2 + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
    // stats[0] is the L2 NORM (not its square): representable in fp32 for any finite fp32 gradient buffer of < 2^64 elements
    if (threadIdx.x == 0) { stats[0] = (float)sqrt(a); stats[1] = (float)b; }
}

}  // namespace

extern "C" size_t me_grad_stats_workspace(void) { return (size_t)GS_BLOCKS * 2 * sizeof(double); }

extern "C" int me_grad_stats(const float* grad, int64_t n, float* stats, void* workspace, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(grad && stats && workspace && n > 0, "me_grad_stats: bad args");
    ME_CHECK_ARG((uintptr_t)grad % 16 == 0, "me_grad_stats: the gradient buffer must be 16-byte aligned");
    int nb = grid_blocks(n / 4 + 1);
    nb = nb < GS_BLOCKS ? nb : GS_BLOCKS;
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)nb), dim3(EW_THREADS), 0, stream, grad, n, part);
    hipLaunchKernelGGL(grad_stats_fold_kernel, dim3(1), dim3(64), 0, stream, part, nb, stats);
    ME_CHECK_LAUNCH("me_grad_stats");
    return ME_OK;
}

namespace {

__global__ void adamw_prepare_kernel(me_adamw_ctl* __restrict__ ctl, const float* __restrict__ stats, const float* __restrict__ loss_scale,
                                     float grad_scale, float max_norm, float b1, float b2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float mul = grad_scale;
    if (loss_scale) mul /= *loss_scale;                               // GradScaler.unscale_: grads were computed on loss * scale
    float norm = 0.f, bad = 0.f;
    if (stats) {
        norm = stats[0] * fabsf(mul);                                 // norm of the UNSCALED, averaged gradient
        bad = (stats[1] > 0.f || !(norm == norm) || norm > 3.0e38f) ? 1.f : 0.f;
        if (max_norm > 0.f) {
            // torch.nn.utils.clip_grad_norm_: coef = max_norm / (total_norm + 1e-6), clamped at 1
            const float coef = max_norm / (norm + 1e-6f);
            mul *= coef < 1.f ? coef : 1.f;
        }
    }
    int step = ctl->step;
    if (bad == 0.f) ++step;                                           // GradScaler.step skips optimizer.step(): no state moves
    ctl->step = step;
    ctl->grad_mul = mul;
    ctl->skip = bad;
    ctl->bc1 = 1.0f - powf(b1, (float)step);
    ctl->bc2_sqrt = sqrtf(1.0f - powf(b2, (float)step));
    ctl->total_norm = norm;
    ctl->found_inf = bad;
}

}  // namespace

extern "C" int me_adamw_prepare(me_adamw_ctl* ctl, const float* stats, const float* loss_scale, float grad_scale, float max_norm,
                                float beta1, float beta2, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(ctl != nullptr, "me_adamw_prepare: null control block");
    hipLaunchKernelGGL(adamw_prepare_kernel, dim3(1), dim3(1), 0, stream, ctl, stats, loss_scale, grad_scale, max_norm, beta1, beta2);
    ME_CHECK_LAUNCH("me_adamw_prepare");
    return ME_OK;
}

namespace {

constexpr int ADAMW_MAX_SEG = 512;
__global__ __launch_bounds__(EW_THREADS) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, int64_t n, const me_adamw_segment* __restrict__ seg,
                                                               int ns, float lr, float b1, float b2, float eps,
                                                               const me_adamw_ctl* __restrict__ ctl, bf16_t* __restrict__ mirror) {
    __shared__ int64_t s_end[ADAMW_MAX_SEG];
    __shared__ float s_lr[ADAMW_MAX_SEG], s_wd[ADAMW_MAX_SEG];
    for (int k = threadIdx.x; k < ns; k += EW_THREADS) { s_end[k] = seg[k].end; s_lr[k] = lr * seg[k].lr_scale; s_wd[k] = seg[k].weight_decay; }
    __syncthreads();
    const float gscale = ctl->grad_mul, bc1 = ctl->bc1, bc2_sqrt = ctl->bc2_sqrt;
    if (ctl->skip != 0.f) return;                                     // (uniform) non-finite gradient: parameters and moments stay
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * EW_THREADS) {
        int lo = 0, hi = ns - 1;                                      // the segment that holds i: first k with i < end[k]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (i < s_end[mid]) hi = mid; else lo = mid + 1;
        }
        adamw_element(p, g, m, v, i, gscale, s_lr[lo], b1, b2, eps, s_wd[lo], bc1, bc2_sqrt, mirror);
    }
}

}  // namespace

extern "C" int me_adamw_step_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                      const me_adamw_segment* segments, int n_segments, float lr, float beta1, float beta2, float eps,
                                      const me_adamw_ctl* ctl, void* bf16_mirror, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && segments && ctl && n >= 0, "me_adamw_step_segments: bad args");
    ME_CHECK_ARG(n_segments >= 1 && n_segments <= ADAMW_MAX_SEG, "me_adamw_step_segments: 1 .. %d segments (got %d)", ADAMW_MAX_SEG, n_segments);
    if (n == 0) return ME_OK;
    hipLaunchKernelGGL(adamw_seg_kernel, dim3(grid_blocks(n)), dim3(EW_THREADS), 0, stream, param, grad, exp_avg, exp_avg_sq, n, segments,
                       n_segments, lr, beta1, beta2, eps, ctl, reinterpret_cast<bf16_t*>(bf16_mirror));
    ME_CHECK_LAUNCH("me_adamw_step_segments");
    return ME_OK;
}
