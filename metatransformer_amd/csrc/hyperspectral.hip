// hyperspectral.hip -- the SpectralFormer band-neighbourhood tokenizer (Hyper-spectrum/train.py:80-125 + the embedding half of
// Hyper-spectrum/metatransformer.py:146-159) on the device: me_hsi_gather writes the reference's [B, bands, p p bp] tensor,
// me_hsi_embed_fwd projects it without ever writing it, me_hsi_embed_wgrad regenerates it for the parameter gradients.
// Semantics and summation orders: include/metaenc.h.  Every token of one pixel reads the same p p x bands neighbourhood, so a
// workgroup stages that neighbourhood (reflection applied) in LDS once and forms token features by index: feature k of token j is
// nb[q(k)][(j + s(k)) mod bands], with q and s from a K-entry table.
#include "common.h"

namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_CS = 64;                    // channels per workgroup of the forward kernels (bf16: four 16-wide MFMA tiles)
constexpr int HS_CF = 32;                    // channels per workgroup of the weight gradient: a thread's accumulators
constexpr int HS_RUNS = 32;                  // the weight gradient cuts the pixels into min(B, HS_RUNS) runs
constexpr size_t HS_LDS_MAX = 160 * 1024;    // LDS of one gfx950 CU
typedef __attribute__((ext_vector_type(8))) uint16_t u16x8;

__device__ __forceinline__ int hs_clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// np.pad(mode="symmetric") for one reflection (p / 2 <= n), clamped so that no argument can leave the cube
__device__ __forceinline__ int hs_refl(int i, int n) { return hs_clampi(i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i), n); }
// band shift of group g (train.py:111-124): the lower groups of a p > 1 window come in reversed order
__device__ __forceinline__ int hs_shift(int g, int nn, int p) { return (p == 1 || g >= nn) ? g - nn : -(g + 1); }
// (j + s) mod bands for |s| < bands, 0 <= j < bands
__device__ __forceinline__ int hs_wrap(int j, int bands) { return j < 0 ? j + bands : (j >= bands ? j - bands : j); }
__device__ __forceinline__ int2 hs_entry(int k, int K, const me_hsi_desc& d) {
    if (k >= K) return make_int2(-1, 0);
    const int pp = d.patch * d.patch, g = k / pp;
    return make_int2((k - g * pp) * d.bands, hs_shift(g, d.band_patch / 2, d.patch));
}

// nb[q][band] = cube[refl(r + dy - p / 2), refl(c + dx - p / 2), band], q = dy p + dx, as T (whole workgroup; no barrier inside)
template <typename T> __device__ __forceinline__ void hs_stage(const me_hsi_desc& d, int b, T* __restrict__ nb) {
    const int p = d.patch, half = p / 2, bands = d.bands;
    const int r = hs_clampi(d.points[2 * (int64_t)b], d.H), c = hs_clampi(d.points[2 * (int64_t)b + 1], d.W);
    const int total = p * p * bands;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int q = i / bands, band = i - q * bands;
        const int dy = q / p, dx = q - dy * p;
        const int y = hs_refl(r + dy - half, d.H), x = hs_refl(c + dx - half, d.W);
        nb[i] = (T)load1_as_f32(d.cube, d.cube_dtype, (int64_t)y * d.row_stride + (int64_t)x * d.pix_stride + band);
    }
}

__global__ __launch_bounds__(HS_THREADS) void hsi_gather_kernel(me_hsi_desc d, void* __restrict__ out, int out_dtype, int64_t ld_out, int K) {
    const int p = d.patch, pp = p * p, half = p / 2, nn = d.band_patch / 2, bands = d.bands;
    const int64_t total = (int64_t)d.B * bands * K;
    for (int64_t idx = (int64_t)blockIdx.x * HS_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * HS_THREADS) {
        const int64_t row = idx / K;
        const int k = (int)(idx - row * K);
        const int64_t b = row / bands;
        const int j = (int)(row - b * bands);
        const int g = k / pp, q = k - g * pp, dy = q / p, dx = q - dy * p;
        const int r = hs_clampi(d.points[2 * b], d.H), c = hs_clampi(d.points[2 * b + 1], d.W);
        const int y = hs_refl(r + dy - half, d.H), x = hs_refl(c + dx - half, d.W);
        const int band = hs_wrap(j + hs_shift(g, nn, p), bands);
        store1_from_f32(out, out_dtype, row * ld_out + k, load1_as_f32(d.cube, d.cube_dtype, (int64_t)y * d.row_stride + (int64_t)x * d.pix_stride + band));
    }
}

// row (b, 0) = cls + pos[0] for the channels c0 .. c0 + n of the workgroup
__device__ __forceinline__ void hs_cls_row(int b, int bands, int c0, int n, int C, const float* __restrict__ cls, const float* __restrict__ pos,
                                           void* __restrict__ out, int out_dtype, int64_t ld_out) {
    const int c = c0 + (int)threadIdx.x * 4;
    if ((int)threadIdx.x < n / 4 && c < C) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(cls + c) + *reinterpret_cast<const f32x4*>(pos + c);
        store4_from_f32(out, out_dtype, (int64_t)b * (bands + 1) * ld_out + c, v);
    }
}

// bf16: workgroup = (pixel, 64 channels).  D[c][token] = W[c][k] tok[token][k]: A = the weight slice (LDS, K zero-padded to Kp), B = token
// fragments formed from the staged neighbourhood; a wave takes every fourth 16-token tile and holds four 16 x 16 accumulators.
__global__ __launch_bounds__(HS_THREADS) void hsi_fwd_bf16_kernel(me_hsi_desc d, const uint16_t* __restrict__ W, int64_t ld_w,
                                                                  const float* __restrict__ bias, const float* __restrict__ cls,
                                                                  const float* __restrict__ pos, int64_t ld_pos, void* __restrict__ out,
                                                                  int out_dtype, int64_t ld_out, int C, int K, int Kp) {
    extern __shared__ __align__(16) unsigned char hs_smem[];
    const int lds_w = Kp + 8;                                             // staged weight row in elements (16 B of padding)
    uint16_t* Ws = reinterpret_cast<uint16_t*>(hs_smem);                  // [HS_CS][lds_w]
    int2* ktab = reinterpret_cast<int2*>(hs_smem + (size_t)HS_CS * lds_w * 2);      // [Kp]
    uint16_t* nb = reinterpret_cast<uint16_t*>(ktab + Kp);                // [p p][bands] bf16 bits
    const int tid = threadIdx.x, b = blockIdx.x, c0 = blockIdx.y * HS_CS, bands = d.bands;
    for (int i = tid; i < HS_CS * Kp; i += HS_THREADS) {
        const int row = i / Kp, k = i - row * Kp, c = c0 + row;
        Ws[row * lds_w + k] = (c < C && k < K) ? W[(int64_t)c * ld_w + k] : (uint16_t)0;
    }
    for (int k = tid; k < Kp; k += HS_THREADS) ktab[k] = hs_entry(k, K, d);
    hs_stage<bf16_t>(d, b, reinterpret_cast<bf16_t*>(nb));
    hs_cls_row(b, bands, c0, HS_CS, C, cls, pos, out, out_dtype, ld_out);
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, kg = lane >> 4;
    const int tiles = (bands + 15) / 16;
    for (int tt = wave; tt < tiles; tt += HS_THREADS / 64) {
        const int token = tt * 16 + l15;
        const int j = token < bands ? token : bands - 1;
        f32x4 acc[HS_CS / 16];
#pragma unroll
        for (int ct = 0; ct < HS_CS / 16; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < Kp; ks += 32) {
            const int kb = ks + kg * 8;
            u16x8 tok;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int2 t = ktab[kb + e];
                tok[e] = t.x >= 0 ? nb[t.x + hs_wrap(j + t.y, bands)] : (uint16_t)0;
            }
            const bf16x8 bfrag = __builtin_bit_cast(bf16x8, tok);
#pragma unroll
            for (int ct = 0; ct < HS_CS / 16; ++ct) {
                const bf16x8 afrag = *reinterpret_cast<const bf16x8*>(Ws + (ct * 16 + l15) * lds_w + kb);
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc[ct], 0, 0, 0);
            }
        }
        if (token < bands) {
            const int64_t orow = (int64_t)b * (bands + 1) + 1 + token;
#pragma unroll
            for (int ct = 0; ct < HS_CS / 16; ++ct) {
                const int c = c0 + ct * 16 + kg * 4;                       // acc[ct][r] = D[c + r][token]
                if (c < C) {
                    f32x4 v = acc[ct] + *reinterpret_cast<const f32x4*>(pos + (int64_t)(token + 1) * ld_pos + c);
                    if (bias) v += *reinterpret_cast<const f32x4*>(bias + c);
                    store4_from_f32(out, out_dtype, orow * ld_out + c, v);
                }
            }
        }
    }
}

// fp32: workgroup = (pixel, 64 channels); a thread owns 8 channels of 4 tokens (32 tokens apart) and runs one FMA chain in ascending k.
// The weight slice lies in LDS as Wt[k][64] in float4 slots, slot (c / 4) ^ (k & 15): the staging writes (consecutive k for one channel)
// spread over the banks, the reads (one k, a thread's two slots) stay conflict-free.
__device__ __forceinline__ int hs_wslot(int k, int s4) { return k * HS_CS + ((s4 ^ (k & 15)) << 2); }

__global__ __launch_bounds__(HS_THREADS) void hsi_fwd_f32_kernel(me_hsi_desc d, const float* __restrict__ W, int64_t ld_w,
                                                                 const float* __restrict__ bias, const float* __restrict__ cls,
                                                                 const float* __restrict__ pos, int64_t ld_pos, void* __restrict__ out,
                                                                 int out_dtype, int64_t ld_out, int C, int K) {
    extern __shared__ __align__(16) unsigned char hs_smem[];
    float* Wt = reinterpret_cast<float*>(hs_smem);                        // [K][HS_CS], swizzled
    int2* ktab = reinterpret_cast<int2*>(Wt + (size_t)K * HS_CS);         // [K]
    float* nb = reinterpret_cast<float*>(ktab + K);                       // [p p][bands]
    const int tid = threadIdx.x, b = blockIdx.x, c0 = blockIdx.y * HS_CS, bands = d.bands;
    for (int i = tid; i < HS_CS * K; i += HS_THREADS) {
        const int cc = i / K, k = i - cc * K, c = c0 + cc;
        Wt[hs_wslot(k, cc >> 2) + (cc & 3)] = c < C ? W[(int64_t)c * ld_w + k] : 0.f;
    }
    for (int k = tid; k < K; k += HS_THREADS) ktab[k] = hs_entry(k, K, d);
    hs_stage<float>(d, b, nb);
    hs_cls_row(b, bands, c0, HS_CS, C, cls, pos, out, out_dtype, ld_out);
    __syncthreads();
    const int cg = tid & 7, tl = tid >> 3, c = c0 + cg * 8;
    for (int j0 = 0; j0 < bands; j0 += 128) {
        int jr[4];
        f32x4 acc[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int jt = j0 + tl + 32 * t;
            jr[t] = jt < bands ? jt : bands - 1;
            acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int k = 0; k < K; ++k) {
            const int2 tk = ktab[k];
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wt + hs_wslot(k, cg * 2));
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(Wt + hs_wslot(k, cg * 2 + 1));
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float v = nb[tk.x + hs_wrap(jr[t] + tk.y, bands)];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[t][0][e] = fmaf(v, w0[e], acc[t][0][e]);
                    acc[t][1][e] = fmaf(v, w1[e], acc[t][1][e]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int jt = j0 + tl + 32 * t;
            if (jt >= bands) continue;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = c + 4 * h;
                if (ch < C) {
                    f32x4 v = acc[t][h] + *reinterpret_cast<const f32x4*>(pos + (int64_t)(jt + 1) * ld_pos + ch);
                    if (bias) v += *reinterpret_cast<const f32x4*>(bias + ch);
                    store4_from_f32(out, out_dtype, ((int64_t)b * (bands + 1) + 1 + jt) * ld_out + ch, v);
                }
            }
        }
    }
}

// weight gradient: workgroup = (32 channels, run of pixels, up to 256 features); thread = one feature k, 32 channel sums in registers.
// Per pixel the neighbourhood and the dy slice are staged; the token loop reads one neighbourhood value and the 32 dy values (LDS
// broadcast).  (The dy values through wave-uniform scalar loads instead of LDS were measured slower: DESIGN.md 7g.)
__global__ __launch_bounds__(HS_THREADS) void hsi_wgrad_kernel(me_hsi_desc d, const void* __restrict__ dy, int dy_dtype, int64_t ld_dy, int C,
                                                               int K, int runs, float* __restrict__ part) {
    extern __shared__ __align__(16) unsigned char hs_smem[];
    const int bands = d.bands;
    float* dys = reinterpret_cast<float*>(hs_smem);                       // [bands][HS_CF]
    float* nb = dys + (size_t)bands * HS_CF;                              // [p p][bands]
    const int tid = threadIdx.x, c0 = blockIdx.x * HS_CF, run = blockIdx.y, k = blockIdx.z * blockDim.x + tid;
    const int2 tk = hs_entry(k, K, d);
    const int b0 = (int)((int64_t)run * d.B / runs), b1 = (int)((int64_t)(run + 1) * d.B / runs);
    float acc[HS_CF];
#pragma unroll
    for (int i = 0; i < HS_CF; ++i) acc[i] = 0.f;
    for (int b = b0; b < b1; ++b) {
        __syncthreads();                                                  // the previous pixel's readers are done
        hs_stage<float>(d, b, nb);
        for (int i = tid; i < bands * HS_CF; i += blockDim.x) {
            const int j = i / HS_CF, c = c0 + (i - j * HS_CF);
            dys[i] = c < C ? load1_as_f32(dy, dy_dtype, ((int64_t)b * (bands + 1) + 1 + j) * ld_dy + c) : 0.f;
        }
        __syncthreads();
        if (tk.x >= 0) {
            for (int j = 0; j < bands; ++j) {
                const float v = nb[tk.x + hs_wrap(j + tk.y, bands)];
                const f32x4* g4 = reinterpret_cast<const f32x4*>(dys + j * HS_CF);
#pragma unroll
                for (int q = 0; q < HS_CF / 4; ++q) {
                    const f32x4 g = g4[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[q * 4 + e] = fmaf(g[e], v, acc[q * 4 + e]);
                }
            }
        }
    }
    if (tk.x >= 0) {
#pragma unroll
        for (int cc = 0; cc < HS_CF; ++cc)
            if (c0 + cc < C) part[((int64_t)run * C + c0 + cc) * K + k] = acc[cc];
    }
}

__device__ __forceinline__ float hs_update(float old_or_unused, float sum, float beta) { return beta == 0.f ? sum : beta * old_or_unused + sum; }

__global__ __launch_bounds__(HS_THREADS) void hsi_wsum_kernel(const float* __restrict__ part, int runs, int C, int K, float* __restrict__ dw,
                                                              int64_t ld_dw, float beta) {
    const int64_t i = (int64_t)blockIdx.x * HS_THREADS + threadIdx.x;
    if (i >= (int64_t)C * K) return;
    const int c = (int)(i / K), k = (int)(i - (int64_t)c * K);
    float s = 0.f;
    for (int r = 0; r < runs; ++r) s += part[(int64_t)r * C * K + i];
    float* dst = dw + (int64_t)c * ld_dw + k;
    *dst = hs_update(beta == 0.f ? 0.f : *dst, s, beta);
}

// tmp[j, c] = sum_b dy[b, j, c], b ascending (4 channels per thread)
__global__ __launch_bounds__(HS_THREADS) void hsi_dpos_kernel(const void* __restrict__ dy, int dy_dtype, int64_t ld_dy, int B, int rows, int C,
                                                              float* __restrict__ tmp) {
    const int64_t i = (int64_t)blockIdx.x * HS_THREADS + threadIdx.x;
    const int c4n = C / 4;
    if (i >= (int64_t)rows * c4n) return;
    const int j = (int)(i / c4n), c = (int)(i - (int64_t)j * c4n) * 4;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) s += load4_as_f32(dy, dy_dtype, ((int64_t)b * rows + j) * ld_dy + c);
    *reinterpret_cast<f32x4*>(tmp + (int64_t)j * C + c) = s;
}

__global__ __launch_bounds__(HS_THREADS) void hsi_vec_kernel(const float* __restrict__ tmp, int rows, int C, float* __restrict__ dbias,
                                                             float* __restrict__ dcls, float* __restrict__ dpos, int64_t ld_dpos, float beta) {
    const int c = blockIdx.x * HS_THREADS + threadIdx.x;
    if (c >= C) return;
    if (dcls) dcls[c] = hs_update(beta == 0.f ? 0.f : dcls[c], tmp[c], beta);
    float s = 0.f;
    for (int j = 0; j < rows; ++j) {
        const float v = tmp[(int64_t)j * C + c];
        if (j >= 1) s += v;
        if (dpos) {
            float* dst = dpos + (int64_t)j * ld_dpos + c;
            *dst = hs_update(beta == 0.f ? 0.f : *dst, v, beta);
        }
    }
    if (dbias) dbias[c] = hs_update(beta == 0.f ? 0.f : dbias[c], s, beta);
}

bool hs_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int hs_K(const me_hsi_desc* d) { return d->patch * d->patch * d->band_patch; }
int hs_runs(const me_hsi_desc* d) { return d->B < HS_RUNS ? d->B : HS_RUNS; }
size_t hs_round(size_t n) { return (n + 255) / 256 * 256; }

int hs_check(const char* who, const me_hsi_desc* d) {
    ME_CHECK_ARG(d != nullptr, "%s: NULL descriptor", who);
    ME_CHECK_ARG(d->H > 0 && d->W > 0 && d->bands > 0 && d->B >= 0, "%s: bad sizes H=%d W=%d bands=%d B=%d", who, d->H, d->W, d->bands, d->B);
    ME_CHECK_ARG(d->patch >= 1 && d->patch <= 63 && d->patch % 2 == 1, "%s: patch=%d (odd, 1 .. 63)", who, d->patch);
    ME_CHECK_ARG(d->band_patch >= 1 && d->band_patch % 2 == 1, "%s: band_patch=%d (odd)", who, d->band_patch);
    ME_CHECK_ARG(d->patch / 2 <= (d->H < d->W ? d->H : d->W), "%s: patch=%d needs patch / 2 <= min(H, W) = min(%d, %d) (one reflection)", who, d->patch,
                 d->H, d->W);
    ME_CHECK_ARG(d->band_patch <= d->bands, "%s: band_patch=%d exceeds bands=%d", who, d->band_patch, d->bands);
    ME_CHECK_ARG((int64_t)d->patch * d->patch * d->band_patch <= (1 << 16), "%s: patch^2 band_patch = %lld features (at most 65536)", who,
                 (long long)d->patch * d->patch * d->band_patch);
    ME_CHECK_ARG(me_dtype_ok(d->cube_dtype), "%s: cube_dtype %d (ME_F32 or ME_BF16)", who, d->cube_dtype);
    ME_CHECK_ARG(d->pix_stride >= d->bands && d->row_stride >= (int64_t)(d->W - 1) * d->pix_stride + d->bands,
                 "%s: strides row=%lld pix=%lld too small for W=%d bands=%d", who, (long long)d->row_stride, (long long)d->pix_stride, d->W, d->bands);
    if (d->B == 0) return ME_OK;
    ME_CHECK_ARG(d->cube && d->points, "%s: NULL cube / points", who);
    return ME_OK;
}

int hs_check_C(const char* who, int C) {
    if (C <= 0 || C % 8 != 0) {
        me_set_error("%s: C=%d channels (a positive multiple of 8)", who, C);
        return ME_ERR_UNSUPPORTED;
    }
    return ME_OK;
}

template <typename Kern> int hs_lds(const char* who, Kern kern, OncePerDevice& once, size_t bytes) {
    if (bytes > HS_LDS_MAX) {
        me_set_error("%s: the patch x patch x bands neighbourhood and the weight slice need %zu bytes of LDS (at most %zu)", who, bytes, HS_LDS_MAX);
        return ME_ERR_UNSUPPORTED;
    }
    if (once.need()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)HS_LDS_MAX);
    return ME_OK;
}

}  // namespace

extern "C" int me_hsi_gather(const me_hsi_desc* d, void* out, int out_dtype, int64_t ld_out, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_hsi_gather";
    const int rc = hs_check(who, d);
    if (rc != ME_OK) return rc;
    const int K = hs_K(d);
    ME_CHECK_ARG(me_dtype_ok(out_dtype), "%s: out_dtype %d (ME_F32 or ME_BF16)", who, out_dtype);
    ME_CHECK_ARG(ld_out >= K, "%s: ld_out=%lld < K=%d", who, (long long)ld_out, K);
    if (d->B == 0) return ME_OK;
    ME_CHECK_ARG(out != nullptr, "%s: NULL output", who);
    const int64_t total = (int64_t)d->B * d->bands * K;
    const int64_t blocks = (total + HS_THREADS - 1) / HS_THREADS;
    hipLaunchKernelGGL(hsi_gather_kernel, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(HS_THREADS), 0, stream, *d, out, out_dtype,
                       ld_out, K);
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}

extern "C" int me_hsi_embed_fwd(const me_hsi_desc* d, const void* weight, int w_dtype, int64_t ld_w, const float* bias, const float* cls,
                                const float* pos, int64_t ld_pos, void* out, int out_dtype, int64_t ld_out, int C, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_hsi_embed_fwd";
    int rc = hs_check(who, d);
    if (rc != ME_OK) return rc;
    if ((rc = hs_check_C(who, C)) != ME_OK) return rc;
    const int K = hs_K(d);
    ME_CHECK_ARG(me_dtype_ok(w_dtype) && me_dtype_ok(out_dtype), "%s: w_dtype %d / out_dtype %d (ME_F32 or ME_BF16)", who, w_dtype, out_dtype);
    ME_CHECK_ARG(ld_w >= K && ld_out >= C && ld_pos >= C && ld_out % 4 == 0 && ld_pos % 4 == 0,
                 "%s: ld_w=%lld (>= K=%d), ld_out=%lld, ld_pos=%lld (>= C=%d, multiples of 4)", who, (long long)ld_w, K, (long long)ld_out,
                 (long long)ld_pos, C);
    if (d->B == 0) return ME_OK;
    ME_CHECK_ARG(weight && cls && pos && out, "%s: NULL weight / cls / pos / out", who);
    ME_CHECK_ARG(hs_aligned(bias) && hs_aligned(cls) && hs_aligned(pos) && hs_aligned(out), "%s: bias, cls, pos and out must be 16-byte aligned", who);
    const size_t nb_elems = (size_t)d->patch * d->patch * d->bands;
    if (w_dtype == ME_BF16) {
        static OncePerDevice once;
        const int Kp = (K + 31) / 32 * 32;
        const size_t lds = (size_t)HS_CS * (Kp + 8) * 2 + (size_t)Kp * sizeof(int2) + nb_elems * 2;
        if ((rc = hs_lds(who, hsi_fwd_bf16_kernel, once, lds)) != ME_OK) return rc;
        hipLaunchKernelGGL(hsi_fwd_bf16_kernel, dim3(d->B, (C + HS_CS - 1) / HS_CS), dim3(HS_THREADS), lds, stream, *d,
                           static_cast<const uint16_t*>(weight), ld_w, bias, cls, pos, ld_pos, out, out_dtype, ld_out, C, K, Kp);
    } else {
        static OncePerDevice once;
        const size_t lds = (size_t)K * HS_CS * 4 + (size_t)K * sizeof(int2) + nb_elems * 4;
        if ((rc = hs_lds(who, hsi_fwd_f32_kernel, once, lds)) != ME_OK) return rc;
        hipLaunchKernelGGL(hsi_fwd_f32_kernel, dim3(d->B, (C + HS_CS - 1) / HS_CS), dim3(HS_THREADS), lds, stream, *d,
                           static_cast<const float*>(weight), ld_w, bias, cls, pos, ld_pos, out, out_dtype, ld_out, C, K);
    }
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}

extern "C" size_t me_hsi_embed_wgrad_workspace(const me_hsi_desc* d, int C) {
    if (!d || d->B <= 0 || C <= 0 || d->bands <= 0 || d->patch <= 0 || d->band_patch <= 0 || d->patch > 63 ||
        (int64_t)d->patch * d->patch * d->band_patch > (1 << 16))
        return 0;
    return hs_round((size_t)hs_runs(d) * C * hs_K(d) * 4) + hs_round((size_t)(d->bands + 1) * C * 4);
}

extern "C" int me_hsi_embed_wgrad(const me_hsi_desc* d, const void* dy, int dy_dtype, int64_t ld_dy, int C, float* dw, int64_t ld_dw,
                                  float* dbias, float* dcls, float* dpos, int64_t ld_dpos, float beta, void* workspace,
                                  size_t workspace_bytes, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_hsi_embed_wgrad";
    int rc = hs_check(who, d);
    if (rc != ME_OK) return rc;
    if ((rc = hs_check_C(who, C)) != ME_OK) return rc;
    const int K = hs_K(d), rows = d->bands + 1;
    ME_CHECK_ARG(me_dtype_ok(dy_dtype), "%s: dy_dtype %d (ME_F32 or ME_BF16)", who, dy_dtype);
    ME_CHECK_ARG(ld_dy >= C && ld_dy % 4 == 0 && (!dw || ld_dw >= K) && (!dpos || ld_dpos >= C),
                 "%s: ld_dy=%lld (>= C=%d, a multiple of 4), ld_dw=%lld (>= K=%d), ld_dpos=%lld (>= C)", who, (long long)ld_dy, C, (long long)ld_dw, K,
                 (long long)ld_dpos);
    if (d->B == 0 || (!dw && !dbias && !dcls && !dpos)) return ME_OK;
    ME_CHECK_ARG(dy != nullptr && hs_aligned(dy), "%s: dy NULL or not 16-byte aligned", who);
    const size_t need = me_hsi_embed_wgrad_workspace(d, C);
    if (!workspace || workspace_bytes < need) {
        me_set_error("%s: workspace of %zu bytes needed", who, need);
        return ME_ERR_WORKSPACE;
    }
    ME_CHECK_ARG(hs_aligned(workspace), "%s: workspace must be 16-byte aligned", who);
    const int runs = hs_runs(d);
    float* part = static_cast<float*>(workspace);
    float* tmp = reinterpret_cast<float*>(static_cast<char*>(workspace) + hs_round((size_t)runs * C * K * 4));
    if (dw) {
        static OncePerDevice once;
        const size_t lds = (size_t)d->bands * HS_CF * 4 + (size_t)d->patch * d->patch * d->bands * 4;
        const int threads = K >= HS_THREADS ? HS_THREADS : (K + 63) / 64 * 64;      // one thread per feature, whole waves
        if ((rc = hs_lds(who, hsi_wgrad_kernel, once, lds)) != ME_OK) return rc;
        hipLaunchKernelGGL(hsi_wgrad_kernel, dim3((C + HS_CF - 1) / HS_CF, runs, (K + threads - 1) / threads), dim3(threads), lds, stream, *d, dy,
                           dy_dtype, ld_dy, C, K, runs, part);
        hipLaunchKernelGGL(hsi_wsum_kernel, dim3((unsigned)(((int64_t)C * K + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS), 0, stream, part, runs,
                           C, K, dw, ld_dw, beta);
    }
    if (dbias || dcls || dpos) {
        hipLaunchKernelGGL(hsi_dpos_kernel, dim3((unsigned)(((int64_t)rows * (C / 4) + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS), 0, stream, dy,
                           dy_dtype, ld_dy, d->B, rows, C, tmp);
        hipLaunchKernelGGL(hsi_vec_kernel, dim3((C + HS_THREADS - 1) / HS_THREADS), dim3(HS_THREADS), 0, stream, tmp, rows, C, dbias, dcls, dpos, ld_dpos,
                           beta);
    }
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}
