// fbank.hip -- waveform -> Kaldi log-mel filterbank for a batch of clips (Audio/src/dataloader.py:98-205: torchaudio's
// compliance.kaldi.fbank with the reference's settings, mix-up, cut / pad, SpecAug bands, normalisation).  Semantics: include/metaenc.h.
// A workgroup owns ME_FBANK_RUN consecutive output rows of one clip: frames overlap 2.5x, so their span of samples is staged in LDS
// once (mean removal and mix-up applied on the way in) and every frame is cut from there.  A wave transforms one frame at a time: the
// `padded` real samples as a padded / 2 point complex FFT (Stockham, radix 4 with one radix-2 pass when padded / 2 is no power of 4)
// between two LDS buffers of its own, the real-input split, the triangular filters from their (first bin, count) ranges, the log.
// Twiddles, window and filter weights are the caller's tables, copied to LDS: no sincosf on the device.
#include "common.h"

namespace {

constexpr int FB_THREADS = 512;
constexpr int FB_WAVES = FB_THREADS / 64;
constexpr int FB_SUM_THREADS = 256;         // fbank_sum_kernel: four wave sums per chunk, added in order
constexpr int FB_RUN = ME_FBANK_RUN;
constexpr int FB_CHUNK = 4096;                 // samples per partial sum of the means
constexpr int FB_MAX_MEL = 256;
constexpr int FB_MAX_WEIGHTS = 8192;           // n_mel * mel_ld floats in LDS
constexpr size_t FB_LDS_MAX = 160 * 1024;      // LDS of one gfx950 CU
constexpr float FB_EPS = 1.1920929e-07f;
constexpr float FB_PREEMPH = 0.97f;

__device__ __forceinline__ int fb_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int fb_len(const me_fbank_desc& d, int b) { return d.lengths ? fb_clampi(d.lengths[b], 0, d.n_samples) : d.n_samples; }
__device__ __forceinline__ int fb_len2(const me_fbank_desc& d, int b) {
    if (!d.wave2) return 0;
    return d.lengths2 ? fb_clampi(d.lengths2[b], 0, d.n_samples2) : d.n_samples2;
}
// mean from the chunk sums of one clip (whole waves call this): a lane adds the chunks lane, lane + 64, ... in ascending order, wave_sum's
// fixed tree adds the lanes -- the same value in every lane, wave and kernel, from one load per lane instead of a chain of them
__device__ __forceinline__ float fb_mean(const float* __restrict__ part, int len, int lane) {
    const int used = len > 0 ? (len + FB_CHUNK - 1) / FB_CHUNK : 0;
    float s = 0.f;
    for (int c = lane; c < used; c += 64) s += part[c];
    s = wave_sum(s);
    return len > 0 ? s / (float)len : 0.f;
}
// sample i < len of the clip after step 1, before the mix's own mean is removed
__device__ __forceinline__ float fb_sample(const me_fbank_desc& d, int b, int i, int len2, float lam, float m1, float m2) {
    const float a = d.wave[(int64_t)b * d.ld_wave + i] - m1;
    if (!d.wave2) return a;
    const float c = i < len2 ? d.wave2[(int64_t)b * d.ld_wave2 + i] - m2 : 0.f;
    return lam * a + (1.f - lam) * c;
}

// part[(which B + b) nch + chunk]: which = 0 the wave, 1 the mix-up partner (pass 0), 2 the mixed wave (pass 1: needs both means)
__global__ __launch_bounds__(FB_SUM_THREADS) void fbank_sum_kernel(me_fbank_desc d, int nch, int pass, float* __restrict__ part) {
    __shared__ float red[FB_SUM_THREADS / 64];
    const int tid = threadIdx.x, chunk = blockIdx.x, b = blockIdx.y, which = pass ? 2 : (int)blockIdx.z;
    const int len = fb_len(d, b), len2 = fb_len2(d, b);
    const int n = which == 1 ? len2 : len;
    float m1 = 0.f, m2 = 0.f, lam = 0.f;
    if (pass) {
        m1 = fb_mean(part + (int64_t)b * nch, len, tid & 63);
        m2 = fb_mean(part + ((int64_t)d.B + b) * nch, len2, tid & 63);
        lam = d.lam[b];
    }
    const int i0 = chunk * FB_CHUNK, i1 = n - i0 < FB_CHUNK ? n : i0 + FB_CHUNK;
    float s = 0.f;
    for (int i = i0 + tid; i < i1; i += FB_SUM_THREADS)
        s += pass ? fb_sample(d, b, i, len2, lam, m1, m2) : (which ? d.wave2[(int64_t)b * d.ld_wave2 + i] : d.wave[(int64_t)b * d.ld_wave + i]);
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) part[((int64_t)which * d.B + b) * nch + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float2 fb_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// one Stockham pass of radix R over M points: Ns = the product of the radices before it, tw[n] = exp(-2 pi i n / padded)
template <int R>
__device__ __forceinline__ void fb_pass(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw, int M, int Ns,
                                        int padded, int lane) {
    const int q = M / R, step = padded / (Ns * R);
    for (int j = lane; j < q; j += 64) {
        const int k = j & (Ns - 1);
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = in[j + r * q];
        if (Ns > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) v[r] = fb_cmul(v[r], tw[r * k * step]);
        }
        float2* o = out + (j - k) * R + k;
        if constexpr (R == 4) {
            const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
            const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
            const float2 a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);            // -i (v1 - v3)
            o[0] = make_float2(a0.x + a2.x, a0.y + a2.y);
            o[Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
            o[2 * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
            o[3 * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
        } else {
            o[0] = make_float2(v[0].x + v[R - 1].x, v[0].y + v[R - 1].y);
            o[Ns] = make_float2(v[0].x - v[R - 1].x, v[0].y - v[R - 1].y);
        }
    }
}

// LDS written by one lane of a wave and read by another lane of the SAME wave: the wave's LDS instructions execute in order, so what
// is needed is that the compiler keeps them in order (what __syncwarp is on this target); no workgroup barrier
__device__ __forceinline__ void fb_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// step 3 for sample i of the frame f (mean mu): mean removal, pre-emphasis, window; zero behind the window
__device__ __forceinline__ float fb_prepared(const float* __restrict__ f, float mu, const float* __restrict__ wnd, int win, int i) {
    return i < win ? ((f[i] - mu) - FB_PREEMPH * (f[i > 0 ? i - 1 : 0] - mu)) * wnd[i] : 0.f;
}

// the first radix-4 pass (Ns = 1: no twiddles) takes its points z[n] = (y[2n], y[2n + 1]) straight from the prepared frame; a lane's four
// results are consecutive: two 16-byte stores
__device__ __forceinline__ void fb_first_pass(const float* __restrict__ f, float mu, const float* __restrict__ wnd, int win, float2* __restrict__ out,
                                              int M, int lane) {
    const int q = M / 4;
    for (int j = lane; j < q; j += 64) {
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = j + r * q;
            v[r] = make_float2(fb_prepared(f, mu, wnd, win, 2 * n), fb_prepared(f, mu, wnd, win, 2 * n + 1));
        }
        const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
        const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
        const float2 a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);                // -i (v1 - v3)
        f32x4* o = reinterpret_cast<f32x4*>(out + 4 * j);
        o[0] = f32x4{a0.x + a2.x, a0.y + a2.y, a1.x + a3.x, a1.y + a3.y};
        o[1] = f32x4{a0.x - a2.x, a0.y - a2.y, a1.x - a3.x, a1.y - a3.y};
    }
}

struct FbCell {              // steps 8 and 9 for one clip
    int f0, f1, t0, t1, normalize;
    float mean, den;
    __device__ __forceinline__ float operator()(float raw, int t, int m) const {
        if ((m >= f0 && m < f1) || (t >= t0 && t < t1)) raw = 0.f;
        return normalize ? (raw - mean) / den : raw;
    }
};

// one output row by one wave; row = the n_mel raw values in LDS, or NULL for a padded row
__device__ __forceinline__ void fb_store_row(const me_fbank_desc& d, const FbCell& cell, int b, int t, const float* row, int vec, int lane) {
    const int64_t base = ((int64_t)b * d.target_length + t) * d.ld_out;
    if (vec) {
        for (int m = lane * 4; m < d.n_mel; m += 256) {
            const f32x4 r = row ? *reinterpret_cast<const f32x4*>(row + m) : f32x4{0.f, 0.f, 0.f, 0.f};
            store4_from_f32(d.out, d.out_dtype, base + m, f32x4{cell(r[0], t, m), cell(r[1], t, m + 1), cell(r[2], t, m + 2), cell(r[3], t, m + 3)});
        }
    } else {
        for (int m = lane; m < d.n_mel; m += 64) store1_from_f32(d.out, d.out_dtype, base + m, cell(row ? row[m] : 0.f, t, m));
    }
}

// workgroup = (run of FB_RUN output rows, clip).  LDS, in floats: twiddle [2 padded] | window [win4] | mel_weight [n_mel mel_ld] |
// mel_range [2 n_mel] | span [FB_RUN - 1) shift + win] | per wave: bufA [padded] | bufB [padded] | row [FB_MAX_MEL]
// PADDED is a template parameter so that the transform's sizes, strides and twiddle steps are constants: its passes unroll into
// straight-line code with immediate offsets (index arithmetic was most of the instructions otherwise)
template <int PADDED>
__global__ __launch_bounds__(FB_THREADS) void fbank_kernel(me_fbank_desc d, int nch, int vec, const float* __restrict__ part) {
    extern __shared__ __align__(16) unsigned char fb_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y, r0 = blockIdx.x * FB_RUN;
    constexpr int padded = PADDED, M = padded / 2;
    const int win = d.win, shift = d.shift, n_mel = d.n_mel;
    const int len = fb_len(d, b), len2 = fb_len2(d, b);
    const int T = len >= win ? 1 + (len - win) / shift : 0;
    const int rows = d.target_length - r0 < FB_RUN ? d.target_length - r0 : FB_RUN;            // output rows of this workgroup
    const int nf = fb_clampi(T - r0, 0, rows);                                                  // of them, frames
    FbCell cell;
    cell.f0 = d.freq_mask ? d.freq_mask[2 * b] : 0;
    cell.f1 = d.freq_mask ? d.freq_mask[2 * b + 1] : 0;
    cell.t0 = d.time_mask ? d.time_mask[2 * b] : 0;
    cell.t1 = d.time_mask ? d.time_mask[2 * b + 1] : 0;
    cell.normalize = d.normalize;
    cell.mean = d.norm_mean;
    cell.den = 2.f * d.norm_std;
    for (int i = nf + wv; i < rows; i += FB_WAVES) fb_store_row(d, cell, b, r0 + i, nullptr, vec, lane);
    if (nf == 0) return;                                                                        // (the same for the whole workgroup)

    const int win4 = (win + 3) & ~3, nw = n_mel * d.mel_ld, nw4 = (nw + 3) & ~3, nr4 = (2 * n_mel + 3) & ~3;
    const int span_n = (FB_RUN - 1) * shift + win, span4 = (span_n + 3) & ~3;
    float* lds = reinterpret_cast<float*>(fb_smem);
    float2* tw = reinterpret_cast<float2*>(lds);
    float* wnd = lds + 2 * padded;
    float* melw = wnd + win4;
    int* range = reinterpret_cast<int*>(melw + nw4);
    float* span = melw + nw4 + nr4;
    float* mine = span + span4 + wv * (2 * padded + FB_MAX_MEL);
    float2* bufA = reinterpret_cast<float2*>(mine);
    float2* bufB = reinterpret_cast<float2*>(mine + padded);
    float* row = mine + 2 * padded;

    for (int i = tid; i < 2 * padded; i += FB_THREADS) lds[i] = d.twiddle[i];
    for (int i = tid; i < win; i += FB_THREADS) wnd[i] = d.window[i];
    for (int i = tid; i < nw; i += FB_THREADS) melw[i] = d.mel_weight[i];
    for (int m = tid; m < n_mel; m += FB_THREADS) {
        const int cnt = fb_clampi(d.mel_range[2 * m + 1], 0, d.mel_ld < M ? d.mel_ld : M);
        range[2 * m] = fb_clampi(d.mel_range[2 * m], 0, M - cnt);
        range[2 * m + 1] = cnt;
    }
    {
        const float m1 = fb_mean(part + (int64_t)b * nch, len, lane);
        float m2 = 0.f, mx = 0.f, lam = 0.f;
        if (d.wave2) {
            m2 = fb_mean(part + ((int64_t)d.B + b) * nch, len2, lane);
            mx = fb_mean(part + (2 * (int64_t)d.B + b) * nch, len, lane);
            lam = d.lam[b];
        }
        const int s0 = r0 * shift, cnt = (nf - 1) * shift + win;                                // s0 + cnt <= len: frame nf - 1 ends inside the clip
        for (int i0 = tid; i0 < cnt; i0 += 4 * FB_THREADS) {                                    // four loads in flight per thread
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = i0 + u * FB_THREADS < cnt ? fb_sample(d, b, s0 + i0 + u * FB_THREADS, len2, lam, m1, m2) - mx : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * FB_THREADS < cnt) span[i0 + u * FB_THREADS] = v[u];
        }
    }
    __syncthreads();

    // from here on the waves go their own way: a frame's buffers belong to its wave, which orders its LDS traffic with fb_wave_sync
    for (int fi = wv; fi < nf; fi += FB_WAVES) {
        const float* f = span + fi * shift;
        float s = 0.f;
        for (int i = lane; i < win; i += 64) s += f[i];
        const float mu = wave_sum(s) / (float)win;
        // M = 4^a or 2 * 4^a: radix-4 passes A -> B -> A ..., then one radix-2 pass when M is no power of 4; padded 512 and 256 both take four
        fb_first_pass(f, mu, wnd, win, bufA, M, lane);
        fb_wave_sync();
        int Ns = 4;
        float2 *src = bufA, *dst = bufB;
#pragma unroll
        for (; Ns * 4 <= M; Ns *= 4) {
            fb_pass<4>(src, dst, tw, M, Ns, padded, lane);
            fb_wave_sync();
            float2* t_ = src; src = dst; dst = t_;
        }
        if (Ns < M) {
            fb_pass<2>(src, dst, tw, M, Ns, padded, lane);
            fb_wave_sync();
            float2* t_ = src; src = dst; dst = t_;
        }
        // real-input split: X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[M - k]) / 2, O = -i (Z[k] - conj Z[M - k]) / 2; power into dst
        float* P = reinterpret_cast<float*>(dst);
        for (int k = lane; k < M; k += 64) {
            const float2 zk = src[k], zm = src[(M - k) & (M - 1)];
            const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            const float2 o = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
            const float2 wo = fb_cmul(o, tw[k]);
            const float xr = e.x + wo.x, xi = e.y + wo.y;
            P[k] = xr * xr + xi * xi;
        }
        fb_wave_sync();
        for (int m = lane; m < n_mel; m += 64) {
            const int first = range[2 * m], cnt = range[2 * m + 1];
            const float* w = melw + m * d.mel_ld;
            float e = 0.f;
            for (int i = 0; i < cnt; ++i) e = fmaf(w[i], P[first + i], e);
            row[m] = logf(fmaxf(e, FB_EPS));
        }
        fb_wave_sync();
        fb_store_row(d, cell, b, r0 + fi, row, vec, lane);
        fb_wave_sync();                                                  // the row and both buffers are free for the next frame
    }
}

int fb_nch(const me_fbank_desc* d) {
    const int n = d->n_samples > d->n_samples2 ? d->n_samples : d->n_samples2;
    return n > 0 ? (n + FB_CHUNK - 1) / FB_CHUNK : 1;
}

size_t fb_lds_bytes(const me_fbank_desc* d) {
    const size_t win4 = (d->win + 3) & ~3, nw4 = ((size_t)d->n_mel * d->mel_ld + 3) & ~(size_t)3, nr4 = (2 * d->n_mel + 3) & ~3;
    const size_t span4 = ((size_t)(FB_RUN - 1) * d->shift + d->win + 3) & ~(size_t)3;
    return 4 * (2 * (size_t)d->padded + win4 + nw4 + nr4 + span4 + (size_t)FB_WAVES * (2 * d->padded + FB_MAX_MEL));
}

int fb_check(const char* who, const me_fbank_desc* d) {
    ME_CHECK_ARG(d != nullptr, "%s: NULL descriptor", who);
    ME_CHECK_ARG(d->B >= 0 && d->B <= 65535 && d->n_samples >= 0 && d->n_samples <= (1 << 30) && d->target_length >= 0 && d->target_length <= (1 << 24),
                 "%s: bad sizes B=%d (at most 65535) n_samples=%d target_length=%d", who, d->B, d->n_samples, d->target_length);
    ME_CHECK_ARG(d->win >= 1 && d->shift >= 1 && d->n_mel >= 1 && d->mel_ld >= 1, "%s: win=%d shift=%d n_mel=%d mel_ld=%d must be positive", who,
                 d->win, d->shift, d->n_mel, d->mel_ld);
    if ((d->padded != 512 && d->padded != 256) || d->win > d->padded || d->n_mel > FB_MAX_MEL || (int64_t)d->n_mel * d->mel_ld > FB_MAX_WEIGHTS ||
        d->shift > d->padded) {
        me_set_error("%s: unsupported geometry padded=%d win=%d shift=%d n_mel=%d mel_ld=%d (padded 512 or 256, win and shift <= padded, "
                     "n_mel <= %d, n_mel * mel_ld <= %d)", who, d->padded, d->win, d->shift, d->n_mel, d->mel_ld, FB_MAX_MEL, FB_MAX_WEIGHTS);
        return ME_ERR_UNSUPPORTED;
    }
    ME_CHECK_ARG(d->ld_wave >= d->n_samples && d->ld_out >= d->n_mel, "%s: ld_wave=%lld (>= n_samples=%d), ld_out=%lld (>= n_mel=%d)", who,
                 (long long)d->ld_wave, d->n_samples, (long long)d->ld_out, d->n_mel);
    ME_CHECK_ARG(me_dtype_ok(d->out_dtype), "%s: out_dtype %d (ME_F32 or ME_BF16)", who, d->out_dtype);
    if (d->wave2)
        ME_CHECK_ARG(d->lam && d->n_samples2 >= 0 && d->n_samples2 <= (1 << 30) && d->ld_wave2 >= d->n_samples2,
                     "%s: the mix-up partner needs lam, 0 <= n_samples2=%d and ld_wave2=%lld >= n_samples2", who, d->n_samples2, (long long)d->ld_wave2);
    ME_CHECK_ARG(!d->normalize || d->norm_std != 0.f, "%s: norm_std = 0", who);
    if (d->B == 0 || d->target_length == 0) return ME_OK;
    ME_CHECK_ARG((d->wave || d->n_samples == 0) && d->out && d->window && d->twiddle && d->mel_range && d->mel_weight,
                 "%s: NULL wave / out / window / twiddle / mel_range / mel_weight", who);
    return ME_OK;
}

}  // namespace

extern "C" size_t me_fbank_workspace_bytes(const me_fbank_desc* d) {
    if (!d || d->B <= 0 || d->n_samples < 0 || d->n_samples > (1 << 30) || (d->wave2 && (d->n_samples2 < 0 || d->n_samples2 > (1 << 30)))) return 0;
    me_fbank_desc e = *d;
    if (!e.wave2) e.n_samples2 = 0;
    return (size_t)3 * d->B * fb_nch(&e) * sizeof(float);
}

extern "C" int me_fbank(const me_fbank_desc* d_, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_fbank";
    const int rc = fb_check(who, d_);
    if (rc != ME_OK) return rc;
    if (d_->B == 0 || d_->target_length == 0) return ME_OK;
    me_fbank_desc d = *d_;
    if (!d.wave2) d.n_samples2 = 0, d.lengths2 = nullptr, d.lam = nullptr;
    const size_t need = me_fbank_workspace_bytes(&d);
    if (!workspace || workspace_bytes < need) {
        me_set_error("%s: workspace of %zu bytes needed", who, need);
        return ME_ERR_WORKSPACE;
    }
    ME_CHECK_ARG((uintptr_t)workspace % 4 == 0, "%s: workspace must be 4-byte aligned", who);
    const size_t lds = fb_lds_bytes(&d);
    if (lds > FB_LDS_MAX) {
        me_set_error("%s: unsupported geometry: %zu bytes of LDS needed (at most %zu)", who, lds, FB_LDS_MAX);
        return ME_ERR_UNSUPPORTED;
    }
    static OncePerDevice once;
    if (once.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fbank_kernel<512>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS_MAX);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fbank_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FB_LDS_MAX);
    }
    const int nch = fb_nch(&d);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(fbank_sum_kernel, dim3(nch, d.B, d.wave2 ? 2 : 1), dim3(FB_SUM_THREADS), 0, stream, d, nch, 0, part);
    if (d.wave2) hipLaunchKernelGGL(fbank_sum_kernel, dim3(nch, d.B, 1), dim3(FB_SUM_THREADS), 0, stream, d, nch, 1, part);
    // whole rows as 16-byte (fp32) / 8-byte (bf16) stores when every row starts on such a boundary
    const size_t esz = me_dtype_size(d.out_dtype);
    const int vec = d.n_mel % 4 == 0 && d.ld_out % 4 == 0 && (uintptr_t)d.out % (4 * esz) == 0;
    const dim3 grid((d.target_length + FB_RUN - 1) / FB_RUN, d.B);
    if (d.padded == 512) hipLaunchKernelGGL(fbank_kernel<512>, grid, dim3(FB_THREADS), lds, stream, d, nch, vec, part);
    else hipLaunchKernelGGL(fbank_kernel<256>, grid, dim3(FB_THREADS), lds, stream, d, nch, vec, part);
    ME_CHECK_LAUNCH(who);
    return ME_OK;
}
