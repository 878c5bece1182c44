// video_mae.hip -- the glue of VideoMAE pre-training around the Blocks (Video/models/modeling_pretrain.py:124-139, 340-360 and the target /
// loss of Video/engine_for_pretraining.py:66-105) on the device: me_tubelet_gather writes the tubelets of the VISIBLE tokens only as
// GEMM rows, me_take_rows gathers position rows, me_mae_assemble_fwd / _bwd join the visible tokens with the mask tokens, me_mae_loss
// forms the per-patch normalised pixel target of the decoded tokens and the masked mean-squared error against it in one pass.
// Semantics and summation orders: include/metaenc.h.  Gathers, element-wise work and fixed-order reductions only.
// Every index read from a list is clamped into its range before it addresses memory (values out of range are a precondition failure).
#include "common.h"

namespace {

constexpr int VM_THREADS = 256;
constexpr int VM_WAVES = VM_THREADS / ME_WAVE;
constexpr int VM_RUNS = 256;                 // me_mae_assemble_bwd cuts the B Ndec mask-token rows into at most this many runs
constexpr int VM_MAX_CIN = 16;               // channels of a clip me_mae_loss keeps statistics for
constexpr int VM_MAX_COLS = 16320;           // kt kh kw Cin values of one patch in LDS: with the kernel's static 144 bytes within 64 KiB
constexpr int VM_MAX_BLOCKS = 1 << 20;

__device__ __forceinline__ int vm_clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the clip geometry: token n of a sample is (t', h', w') row-major over the [T / kt, H / kh, W / kw] tubelet grid
struct VmGeom {
    int Cin, T, H, W, kt, kh, kw, Hp, Wp, tokens;
};

// element offset of pixel (c, dt, dh, dw) of token n inside one sample [Cin, T, H, W]
__device__ __forceinline__ int64_t vm_pixel(const VmGeom& g, int n, int c, int dt, int dh, int dw) {
    const int tp = n / (g.Hp * g.Wp), r = n - tp * g.Hp * g.Wp, hp = r / g.Wp, wp = r - hp * g.Wp;
    return (((int64_t)c * g.T + tp * g.kt + dt) * g.H + hp * g.kh + dh) * g.W + wp * g.kw + dw;
}

// out[(b, j), k] = video[b, c, t' kt + dt, h' kh + dh, w' kw + dw], k = ((c kt + dt) kh + dh) kw + dw, token idx[b, j].
// V = 4: four consecutive dw per thread (kw, W, ld_out multiples of 4, both pointers aligned: the host decides)
template <int V>
__global__ __launch_bounds__(VM_THREADS) void tubelet_gather_kernel(const void* __restrict__ video, int vdt, const int32_t* __restrict__ idx,
                                                                    void* __restrict__ out, int odt, int64_t ld_out, VmGeom g, int B, int Nsel) {
    const int K = g.Cin * g.kt * g.kh * g.kw, KV = K / V;
    const int64_t total = (int64_t)B * Nsel * KV, sample = (int64_t)g.Cin * g.T * g.H * g.W;
    for (int64_t i = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VM_THREADS) {
        const int64_t row = i / KV;
        const int k = (int)(i - row * KV) * V;
        const int b = (int)(row / Nsel);
        const int n = vm_clampi(idx[row], g.tokens);
        const int dw = k % g.kw, q = k / g.kw, dh = q % g.kh, q2 = q / g.kh, dt = q2 % g.kt, c = q2 / g.kt;
        const int64_t src = (int64_t)b * sample + vm_pixel(g, n, c, dt, dh, dw);
        if (V == 4) store4_from_f32(out, odt, row * ld_out + k, load4_as_f32(video, vdt, src));
        else store1_from_f32(out, odt, row * ld_out + k, load1_as_f32(video, vdt, src));
    }
}

// out[(b, j), c] = table[idx[b, j], c] (+ add[c])
__global__ __launch_bounds__(VM_THREADS) void take_rows_kernel(const void* __restrict__ table, int tdt, int64_t ld_table, int rows,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ add,
                                                               void* __restrict__ out, int odt, int64_t ld_out, int64_t nrows, int C) {
    const int64_t total = nrows * C;
    for (int64_t i = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VM_THREADS) {
        const int64_t row = i / C;
        const int c = (int)(i - row * C);
        float v = load1_as_f32(table, tdt, (int64_t)vm_clampi(idx[row], rows) * ld_table + c);
        if (add) v += add[c];
        store1_from_f32(out, odt, row * ld_out + c, v);
    }
}

// out[b, j] = xv[b, j] + pos[vis_idx[b, j]] for j < Nvis, mask_token + pos[dec_idx[b, j - Nvis]] behind
__global__ __launch_bounds__(VM_THREADS) void mae_assemble_kernel(const void* __restrict__ xv, int xdt, int64_t ld_xv, const float* __restrict__ pos,
                                                                  int64_t ld_pos, int rows, const int32_t* __restrict__ vis_idx,
                                                                  const int32_t* __restrict__ dec_idx, const float* __restrict__ mask_token,
                                                                  void* __restrict__ out, int odt, int64_t ld_out, int B, int Nvis, int Ndec, int Cd) {
    const int Nf = Nvis + Ndec;
    const int64_t total = (int64_t)B * Nf * Cd;
    for (int64_t i = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VM_THREADS) {
        const int64_t row = i / Cd;
        const int c = (int)(i - row * Cd);
        const int b = (int)(row / Nf), j = (int)(row - (int64_t)b * Nf);
        float v;
        if (j < Nvis) {
            const int64_t r = (int64_t)b * Nvis + j;
            v = load1_as_f32(xv, xdt, r * ld_xv + c) + pos[(int64_t)vm_clampi(vis_idx[r], rows) * ld_pos + c];
        } else {
            v = mask_token[c] + pos[(int64_t)vm_clampi(dec_idx[(int64_t)b * Ndec + j - Nvis], rows) * ld_pos + c];
        }
        store1_from_f32(out, odt, row * ld_out + c, v);
    }
}

// dxv[b, j] = dx_full[b, j], j < Nvis
__global__ __launch_bounds__(VM_THREADS) void mae_dxv_kernel(const void* __restrict__ dx, int ddt, int64_t ld_dx, void* __restrict__ dxv, int odt,
                                                             int64_t ld_dxv, int B, int Nvis, int Nf, int Cd) {
    const int64_t total = (int64_t)B * Nvis * Cd;
    for (int64_t i = (int64_t)blockIdx.x * VM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * VM_THREADS) {
        const int64_t row = i / Cd;
        const int c = (int)(i - row * Cd);
        const int b = (int)(row / Nvis), j = (int)(row - (int64_t)b * Nvis);
        store1_from_f32(dxv, odt, row * ld_dxv + c, load1_as_f32(dx, ddt, ((int64_t)b * Nf + j) * ld_dx + c));
    }
}

// part[run, c] = the sum over the run's mask-token rows (m = b Ndec + j in [run M / runs, (run + 1) M / runs)), m ascending
__global__ __launch_bounds__(VM_THREADS) void mae_dmask_part_kernel(const void* __restrict__ dx, int ddt, int64_t ld_dx, int Nvis, int Ndec, int Cd,
                                                                    int64_t M, int runs, float* __restrict__ part) {
    const int c = blockIdx.x * VM_THREADS + threadIdx.x, run = blockIdx.y;
    if (c >= Cd) return;
    const int64_t m0 = run * M / runs, m1 = (run + 1) * M / runs;
    float s = 0.f;
    for (int64_t m = m0; m < m1; ++m) {
        const int64_t b = m / Ndec, j = m - b * Ndec;
        s += load1_as_f32(dx, ddt, (b * (Nvis + Ndec) + Nvis + j) * ld_dx + c);
    }
    part[(int64_t)run * Cd + c] = s;
}

// dmask_token[c] = the sum of the runs, ascending (zero when there are none)
__global__ __launch_bounds__(VM_THREADS) void mae_dmask_sum_kernel(const float* __restrict__ part, int runs, int Cd, float* __restrict__ dmask) {
    const int c = blockIdx.x * VM_THREADS + threadIdx.x;
    if (c >= Cd) return;
    float s = 0.f;
    for (int r = 0; r < runs; ++r) s += part[(int64_t)r * Cd + c];
    dmask[c] = s;
}

// the sum of one value per thread over the workgroup, the same in every thread: the xor-shuffle tree inside a wave, then the waves in
// ascending order.  red: VM_WAVES floats of LDS.  Fixed order, so two runs agree bit for bit.
__device__ __forceinline__ float vm_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                                      // the previous use of red is over
    if ((threadIdx.x & (ME_WAVE - 1)) == 0) red[threadIdx.x / ME_WAVE] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < VM_WAVES; ++w) s += red[w];
    return s;
}

// scalars[1] = sum of w[0 .. n), by one workgroup: thread t sums elements t, t + 256, ... ascending, then vm_block_sum
__global__ __launch_bounds__(VM_THREADS) void mae_wsum_kernel(const float* __restrict__ w, int64_t n, float* __restrict__ scalars) {
    __shared__ float red[VM_WAVES];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += VM_THREADS) s += w[i];
    s = vm_block_sum(s, red);
    if (threadIdx.x == 0) scalars[1] = s;
}

// scalars[0] = sum w l / sum w (0 when sum w == 0), same order as above; sum w is read from scalars[1]
__global__ __launch_bounds__(VM_THREADS) void mae_loss_sum_kernel(const float* __restrict__ w, const float* __restrict__ tok, int64_t n,
                                                                  float* __restrict__ scalars) {
    __shared__ float red[VM_WAVES];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += VM_THREADS) s += w[i] * tok[i];
    s = vm_block_sum(s, red);
    if (threadIdx.x == 0) {
        const float sw = scalars[1];
        scalars[0] = sw != 0.f ? s / sw : 0.f;
    }
}

// workgroup = one decoded token (b, j).  The patch's kt kh kw Cin pixel values u = x std + mean are staged in LDS in the label's column
// order ((dt kh + dh) kw + dw) Cin + c; per channel the mean, then the sum of squared deviations from it (two passes over LDS), the label
// (u - mean) / (sqrt(M2 / (n - 1)) + 1e-6); then the squared error against pred, the optional label and dpred rows.
__global__ __launch_bounds__(VM_THREADS) void mae_loss_kernel(const void* __restrict__ video, int vdt, VmGeom g, const float* __restrict__ mean,
                                                              const float* __restrict__ stdv, const int32_t* __restrict__ dec_idx,
                                                              const float* __restrict__ w, const void* __restrict__ pred, int pdt, int64_t ld_pred,
                                                              int normalize, const float* __restrict__ gscale, int Ndec,
                                                              float* __restrict__ tok_loss, float* __restrict__ labels, int64_t ld_labels,
                                                              void* __restrict__ dpred, int64_t ld_dpred, const float* __restrict__ scalars) {
    extern __shared__ __align__(16) unsigned char vm_smem[];
    float* u = reinterpret_cast<float*>(vm_smem);                         // [cols]
    __shared__ float red[VM_WAVES];
    __shared__ float st_mean[VM_MAX_CIN], st_inv[VM_MAX_CIN];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int b = (int)(row / Ndec);
    const int n = vm_clampi(dec_idx[row], g.tokens);
    const int npix = g.kt * g.kh * g.kw, cols = npix * g.Cin;
    const int64_t sample = (int64_t)g.Cin * g.T * g.H * g.W;
    for (int i = tid; i < cols; i += VM_THREADS) {                        // i in the clip's own order (c, dt, dh, dw): dw runs along a line
        const int dw = i % g.kw, q = i / g.kw, dh = q % g.kh, q2 = q / g.kh, dt = q2 % g.kt, c = q2 / g.kt;
        const float x = load1_as_f32(video, vdt, (int64_t)b * sample + vm_pixel(g, n, c, dt, dh, dw));
        u[((dt * g.kh + dh) * g.kw + dw) * g.Cin + c] = x * stdv[c] + mean[c];
    }
    __syncthreads();
    if (normalize) {
        for (int c = 0; c < g.Cin; ++c) {
            float s = 0.f;
            for (int p = tid; p < npix; p += VM_THREADS) s += u[p * g.Cin + c];
            const float m = vm_block_sum(s, red) / (float)npix;
            float s2 = 0.f;
            for (int p = tid; p < npix; p += VM_THREADS) {
                const float d = u[p * g.Cin + c] - m;
                s2 += d * d;
            }
            const float var = vm_block_sum(s2, red) / (float)(npix - 1);
            if (tid == 0) {
                st_mean[c] = m;
                st_inv[c] = 1.0f / (sqrtf(var) + 1e-6f);
            }
        }
        __syncthreads();
    }
    const float wt = w[row];
    float scale = 0.f;                                                    // g 2 w / (cols sum w)
    if (dpred) {
        const float sw = scalars[1];
        scale = sw != 0.f ? (gscale ? gscale[0] : 1.0f) * 2.0f * wt / ((float)cols * sw) : 0.f;
    }
    float acc = 0.f;
    for (int i = tid; i < cols; i += VM_THREADS) {
        float lab = u[i];
        if (normalize) {
            const int c = i % g.Cin;
            lab = (lab - st_mean[c]) * st_inv[c];
        }
        const float d = load1_as_f32(pred, pdt, row * ld_pred + i) - lab;
        acc += d * d;
        if (labels) labels[row * ld_labels + i] = lab;
        if (dpred) store1_from_f32(dpred, pdt, row * ld_dpred + i, scale != 0.f ? scale * d : 0.f);
    }
    acc = vm_block_sum(acc, red);
    if (tid == 0 && tok_loss) tok_loss[row] = acc / (float)cols;
}

unsigned vm_blocks(int64_t total) {
    const int64_t blocks = (total + VM_THREADS - 1) / VM_THREADS;
    return (unsigned)(blocks < VM_MAX_BLOCKS ? blocks : VM_MAX_BLOCKS);
}
bool vm_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
int vm_runs(int64_t M) { return (int)(M < VM_RUNS ? M : VM_RUNS); }

int vm_geometry(const char* who, int B, int Cin, int T, int H, int W, int kt, int kh, int kw, VmGeom* g) {
    ME_CHECK_ARG(B >= 0 && Cin > 0 && T > 0 && H > 0 && W > 0 && kt > 0 && kh > 0 && kw > 0, "%s: bad sizes B=%d Cin=%d T=%d H=%d W=%d k=(%d, %d, %d)", who,
                 B, Cin, T, H, W, kt, kh, kw);
    ME_CHECK_ARG(kt <= T && kh <= H && kw <= W, "%s: tubelet (%d, %d, %d) larger than the clip (%d, %d, %d)", who, kt, kh, kw, T, H, W);
    ME_CHECK_ARG((int64_t)Cin * kt * kh * kw < (1 << 24) && (int64_t)(T / kt) * (H / kh) * (W / kw) < (1 << 30),
                 "%s: tubelet of %lld values / %lld tokens per sample (too large)", who, (long long)Cin * kt * kh * kw,
                 (long long)(T / kt) * (H / kh) * (W / kw));
    g->Cin = Cin, g->T = T, g->H = H, g->W = W, g->kt = kt, g->kh = kh, g->kw = kw;
    g->Hp = H / kh, g->Wp = W / kw, g->tokens = (T / kt) * g->Hp * g->Wp;
    return ME_OK;
}

}  // namespace

extern "C" int me_tubelet_gather(const void* video, int video_dtype, const int32_t* idx, void* out, int out_dtype, int64_t ld_out, int B, int Cin,
                                 int T, int H, int W, int kt, int kh, int kw, int Nsel, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_tubelet_gather";
    VmGeom g;
    const int rc = vm_geometry(who, B, Cin, T, H, W, kt, kh, kw, &g);
    if (rc != ME_OK) return rc;
    const int K = Cin * kt * kh * kw;
    ME_CHECK_ARG(me_dtype_ok(video_dtype) && me_dtype_ok(out_dtype), "%s: video_dtype %d / out_dtype %d (ME_F32 or ME_BF16)", who, video_dtype, out_dtype);
    ME_CHECK_ARG(Nsel >= 0 && ld_out >= K, "%s: Nsel=%d, ld_out=%lld (>= K=%d)", who, Nsel, (long long)ld_out, K);
    if (B == 0 || Nsel == 0) return ME_OK;
    ME_CHECK_ARG(video && idx && out, "%s: NULL video / idx / out", who);
    const size_t va = 4 * me_dtype_size(video_dtype), oa = 4 * me_dtype_size(out_dtype);
    if (kw % 4 == 0 && W % 4 == 0 && ld_out % 4 == 0 && vm_aligned(video, va) && vm_aligned(out, oa))
        hipLaunchKernelGGL(tubelet_gather_kernel<4>, dim3(vm_blocks((int64_t)B * Nsel * (K / 4))), dim3(VM_THREADS), 0, stream, video, video_dtype, idx, out,
                           out_dtype, ld_out, g, B, Nsel);
    else
        hipLaunchKernelGGL(tubelet_gather_kernel<1>, dim3(vm_blocks((int64_t)B * Nsel * K)), dim3(VM_THREADS), 0, stream, video, video_dtype, idx, out,
                           out_dtype, ld_out, g, B, Nsel);
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}

extern "C" int me_take_rows(const void* table, int table_dtype, int64_t ld_table, int rows, const int32_t* idx, const float* add, void* out,
                            int out_dtype, int64_t ld_out, int B, int Nsel, int C, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_take_rows";
    ME_CHECK_ARG(me_dtype_ok(table_dtype) && me_dtype_ok(out_dtype), "%s: table_dtype %d / out_dtype %d (ME_F32 or ME_BF16)", who, table_dtype, out_dtype);
    ME_CHECK_ARG(B >= 0 && Nsel >= 0 && C > 0 && rows > 0 && ld_table >= C && ld_out >= C, "%s: B=%d Nsel=%d C=%d rows=%d ld_table=%lld ld_out=%lld", who, B,
                 Nsel, C, rows, (long long)ld_table, (long long)ld_out);
    if (B == 0 || Nsel == 0) return ME_OK;
    ME_CHECK_ARG(table && idx && out, "%s: NULL table / idx / out", who);
    const int64_t nrows = (int64_t)B * Nsel;
    hipLaunchKernelGGL(take_rows_kernel, dim3(vm_blocks(nrows * C)), dim3(VM_THREADS), 0, stream, table, table_dtype, ld_table, rows, idx, add, out,
                       out_dtype, ld_out, nrows, C);
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}

extern "C" int me_mae_assemble_fwd(const void* xv, int xv_dtype, int64_t ld_xv, const float* pos, int64_t ld_pos, int rows, const int32_t* vis_idx,
                                   const int32_t* dec_idx, const float* mask_token, void* out, int out_dtype, int64_t ld_out, int B, int Nvis,
                                   int Ndec, int Cd, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_mae_assemble_fwd";
    ME_CHECK_ARG(me_dtype_ok(xv_dtype) && me_dtype_ok(out_dtype), "%s: xv_dtype %d / out_dtype %d (ME_F32 or ME_BF16)", who, xv_dtype, out_dtype);
    ME_CHECK_ARG(B >= 0 && Nvis >= 0 && Ndec >= 0 && Cd > 0 && rows > 0 && ld_xv >= Cd && ld_pos >= Cd && ld_out >= Cd,
                 "%s: B=%d Nvis=%d Ndec=%d Cd=%d rows=%d ld_xv=%lld ld_pos=%lld ld_out=%lld", who, B, Nvis, Ndec, Cd, rows, (long long)ld_xv,
                 (long long)ld_pos, (long long)ld_out);
    if (B == 0 || Nvis + Ndec == 0) return ME_OK;
    ME_CHECK_ARG(pos && out && (Nvis == 0 || (xv && vis_idx)) && (Ndec == 0 || (dec_idx && mask_token)), "%s: NULL pointer", who);
    hipLaunchKernelGGL(mae_assemble_kernel, dim3(vm_blocks((int64_t)B * (Nvis + Ndec) * Cd)), dim3(VM_THREADS), 0, stream, xv, xv_dtype, ld_xv, pos, ld_pos,
                       rows, vis_idx, dec_idx, mask_token, out, out_dtype, ld_out, B, Nvis, Ndec, Cd);
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}

extern "C" size_t me_mae_assemble_bwd_workspace(int B, int Ndec, int Cd) {
    if (B <= 0 || Ndec <= 0 || Cd <= 0) return 0;
    return (size_t)vm_runs((int64_t)B * Ndec) * Cd * sizeof(float);
}

extern "C" int me_mae_assemble_bwd(const void* dx_full, int dx_dtype, int64_t ld_dx, void* dxv, int dxv_dtype, int64_t ld_dxv, float* dmask_token,
                                   int B, int Nvis, int Ndec, int Cd, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_mae_assemble_bwd";
    ME_CHECK_ARG(me_dtype_ok(dx_dtype) && (!dxv || me_dtype_ok(dxv_dtype)), "%s: dx_dtype %d / dxv_dtype %d (ME_F32 or ME_BF16)", who, dx_dtype, dxv_dtype);
    ME_CHECK_ARG(B >= 0 && Nvis >= 0 && Ndec >= 0 && Cd > 0 && ld_dx >= Cd && (!dxv || ld_dxv >= Cd), "%s: B=%d Nvis=%d Ndec=%d Cd=%d ld_dx=%lld ld_dxv=%lld",
                 who, B, Nvis, Ndec, Cd, (long long)ld_dx, (long long)ld_dxv);
    const int64_t M = (int64_t)B * Ndec;
    ME_CHECK_ARG(dx_full || (int64_t)B * (Nvis + Ndec) == 0, "%s: NULL dx_full", who);
    const int runs = vm_runs(M);
    if (dmask_token && runs > 0) {                                        // every check before the first launch
        const size_t need = me_mae_assemble_bwd_workspace(B, Ndec, Cd);
        if (!workspace || workspace_bytes < need) {
            me_set_error("%s: workspace of %zu bytes needed", who, need);
            return ME_ERR_WORKSPACE;
        }
    }
    if (dxv && B > 0 && Nvis > 0)
        hipLaunchKernelGGL(mae_dxv_kernel, dim3(vm_blocks((int64_t)B * Nvis * Cd)), dim3(VM_THREADS), 0, stream, dx_full, dx_dtype, ld_dx, dxv, dxv_dtype,
                           ld_dxv, B, Nvis, Nvis + Ndec, Cd);
    if (dmask_token) {
        float* part = static_cast<float*>(workspace);
        const unsigned cb = (unsigned)((Cd + VM_THREADS - 1) / VM_THREADS);
        if (runs > 0)
            hipLaunchKernelGGL(mae_dmask_part_kernel, dim3(cb, runs), dim3(VM_THREADS), 0, stream, dx_full, dx_dtype, ld_dx, Nvis, Ndec, Cd, M, runs, part);
        hipLaunchKernelGGL(mae_dmask_sum_kernel, dim3(cb), dim3(VM_THREADS), 0, stream, part, runs, Cd, dmask_token);
    }
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}

extern "C" int me_mae_loss(const void* video, int video_dtype, int B, int Cin, int T, int H, int W, int kt, int kh, int kw, const float* mean,
                           const float* stdv, const int32_t* dec_idx, const float* w, int Ndec, const void* pred, int pred_dtype, int64_t ld_pred,
                           int normalize_target, const float* grad_scale, float* tok_loss, float* scalars, float* labels, int64_t ld_labels,
                           void* dpred, int64_t ld_dpred, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_mae_loss";
    VmGeom g;
    const int rc = vm_geometry(who, B, Cin, T, H, W, kt, kh, kw, &g);
    if (rc != ME_OK) return rc;
    const int npix = kt * kh * kw, cols = npix * Cin;
    ME_CHECK_ARG(me_dtype_ok(video_dtype) && me_dtype_ok(pred_dtype), "%s: video_dtype %d / pred_dtype %d (ME_F32 or ME_BF16)", who, video_dtype, pred_dtype);
    ME_CHECK_ARG(Ndec >= 0 && ld_pred >= cols && (!labels || ld_labels >= cols) && (!dpred || ld_dpred >= cols),
                 "%s: Ndec=%d, ld_pred=%lld ld_labels=%lld ld_dpred=%lld (>= kt kh kw Cin = %d)", who, Ndec, (long long)ld_pred, (long long)ld_labels,
                 (long long)ld_dpred, cols);
    ME_CHECK_ARG(!normalize_target || npix >= 2, "%s: the unbiased variance needs at least two pixels per patch (kt kh kw = %d)", who, npix);
    ME_CHECK_ARG(scalars != nullptr, "%s: NULL scalars (fp32 [2]: loss, sum of w)", who);
    if (Cin > VM_MAX_CIN || cols > VM_MAX_COLS) {
        me_set_error("%s: Cin=%d (at most %d), kt kh kw Cin = %d values per patch (at most %d)", who, Cin, VM_MAX_CIN, cols, VM_MAX_COLS);
        return ME_ERR_UNSUPPORTED;
    }
    const int64_t M = (int64_t)B * Ndec;
    ME_CHECK_ARG(M == 0 || (video && mean && stdv && dec_idx && w && pred), "%s: NULL video / mean / std / dec_idx / w / pred", who);
    ME_CHECK_ARG(M < (1ll << 31), "%s: B Ndec = %lld decoded tokens (too many)", who, (long long)M);
    hipLaunchKernelGGL(mae_wsum_kernel, dim3(1), dim3(VM_THREADS), 0, stream, w, M, scalars);
    if (M > 0) {
        const size_t lds = (size_t)cols * sizeof(float);
        static OncePerDevice once;
        if (once.need() && hipFuncSetAttribute(reinterpret_cast<const void*>(mae_loss_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(VM_MAX_COLS * sizeof(float))) != hipSuccess) {
            (void)hipGetLastError();
            me_set_error("%s: the device refuses %zu bytes of dynamic LDS", who, (size_t)VM_MAX_COLS * sizeof(float));
            return ME_ERR_UNSUPPORTED;
        }
        hipLaunchKernelGGL(mae_loss_kernel, dim3((unsigned)M), dim3(VM_THREADS), lds, stream, video, video_dtype, g, mean, stdv, dec_idx, w, pred, pred_dtype,
                           ld_pred, normalize_target, grad_scale, Ndec, tok_loss, labels, ld_labels, dpred, ld_dpred, scalars);
    }
    if (tok_loss || M == 0) hipLaunchKernelGGL(mae_loss_sum_kernel, dim3(1), dim3(VM_THREADS), 0, stream, w, tok_loss, M, scalars);
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}
