// deform.hip -- multi-scale deformable attention (Deformable DETR's MSDeformAttn, the sampling core of the ViT-Adapter's
// Injector / Extractor: Image/{detection,segmentation}/ops), forward and backward, fp32:
//   out[n, q, m D + d] = sum_{l, p} w[n, q, m, l, p] * bilinear(value_l[n, :, m, d]; x W_l - 0.5, y H_l - 0.5)
// with value [N, S, M, D] (level l = rows level_start[l] .. + H_l W_l, row-major H_l x W_l), (x, y) = loc[n, q, m, l, p, :] in [0, 1]
// over the level, and corners outside the level contributing zero (grid_sample, zeros padding, align_corners = False).
//   * me_ms_deform_attn_fwd: a group of lanes per (query, head), one float4 of the head's D channels per lane, so a corner fetch
//     is one contiguous 4 D-byte segment (D = 32: 8 lanes, 8 pairs per wave); the pairs run in memory order, so neighbouring
//     queries meet the same value rows in L2.
//   * me_ms_deform_attn_bwd: dloc / dattn in the same layout (the sum over a head's channels by DPP inside the lane group);
//     dvalue by inverting the (sample, corner) -> value-row map with the counting sort of inv_lists.h and one gather pass per
//     value row that recomputes the corner weight -- no float atomics, every element written, two runs bit-identical.
#include "common.h"
#include "inv_lists.h"

namespace {

constexpr int MSDA_MAX_LEVELS = 8;
constexpr int MSDA_MAX_D = 128;
constexpr int MSDA_THREADS = 256;

struct MsdaLevels {
    int H[MSDA_MAX_LEVELS], W[MSDA_MAX_LEVELS], start[MSDA_MAX_LEVELS];
};

// pixel-space sample position of a normalised location: (x0, y0) = its upper-left corner, (fx, fy) the fractions towards the
// lower-right one.  ok = the sample touches the level at all (x in (-1, W), y in (-1, H); a NaN location touches nothing).
struct MsdaTap {
    int x0, y0;
    float fx, fy;
    bool ok;
};
__device__ __forceinline__ MsdaTap msda_tap(float lx, float ly, int H, int W) {
    const float x = __builtin_fmaf(lx, (float)W, -0.5f), y = __builtin_fmaf(ly, (float)H, -0.5f);
    MsdaTap t;
    t.ok = x > -1.f && x < (float)W && y > -1.f && y < (float)H;
    const float xf = __builtin_floorf(x), yf = __builtin_floorf(y);
    t.x0 = t.ok ? (int)xf : -2;
    t.y0 = t.ok ? (int)yf : -2;
    t.fx = x - xf;
    t.fy = y - yf;
    return t;
}

__device__ __forceinline__ float4 msda_row4(const float* __restrict__ base, int64_t row_stride, int y, int x, int H, int W) {
    if (y < 0 || y >= H || x < 0 || x >= W) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4*>(base + ((int64_t)y * W + x) * row_stride);
}
__device__ __forceinline__ float4 fma4(float w, float4 v, float4 a) {
    a.x = __builtin_fmaf(w, v.x, a.x); a.y = __builtin_fmaf(w, v.y, a.y);
    a.z = __builtin_fmaf(w, v.z, a.z); a.w = __builtin_fmaf(w, v.w, a.w);
    return a;
}
__device__ __forceinline__ float dot4(float4 a, float4 b) {
    return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)));
}

// One group of 2^lg lanes per (n, q, m) pair, lane j of the group on channels 4 j .. 4 j + 3 (lanes past D idle).  The levels
// are unrolled so that their shapes are read from the kernel arguments by constant index.
__global__ __launch_bounds__(MSDA_THREADS) void msda_fwd_kernel(const float* __restrict__ value, const float* __restrict__ loc,
                                                                const float* __restrict__ attn, float* __restrict__ out,
                                                                MsdaLevels lv, int L, int S, int Lq, int M, int D, int P, int lg,
                                                                int64_t pairs) {
    const int64_t pair = ((int64_t)blockIdx.x * MSDA_THREADS + threadIdx.x) >> lg;
    const int c = (threadIdx.x & ((1 << lg) - 1)) * 4;
    if (pair >= pairs || c >= D) return;
    const int m = (int)(pair % M);
    const int64_t n = pair / M / Lq;
    const int64_t rs = (int64_t)M * D;
    const float* vb = value + (n * S * M + m) * D + c;
    const float* lp = loc + pair * L * P * 2;
    const float* wp = attn + pair * L * P;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int l = 0; l < MSDA_MAX_LEVELS; ++l) {
        if (l < L) {
            const int H = lv.H[l], W = lv.W[l];
            const float* vl = vb + (int64_t)lv.start[l] * rs;
            for (int p = 0; p < P; ++p) {
                const int i = l * P + p;
                const float2 xy = *reinterpret_cast<const float2*>(lp + 2 * i);
                const float a = wp[i];
                const MsdaTap t = msda_tap(xy.x, xy.y, H, W);
                if (!t.ok) continue;
                const float4 v00 = msda_row4(vl, rs, t.y0, t.x0, H, W), v01 = msda_row4(vl, rs, t.y0, t.x0 + 1, H, W);
                const float4 v10 = msda_row4(vl, rs, t.y0 + 1, t.x0, H, W), v11 = msda_row4(vl, rs, t.y0 + 1, t.x0 + 1, H, W);
                const float hx = 1.f - t.fx, hy = 1.f - t.fy;
                acc = fma4(a * (hy * hx), v00, acc);
                acc = fma4(a * (hy * t.fx), v01, acc);
                acc = fma4(a * (t.fy * hx), v10, acc);
                acc = fma4(a * (t.fy * t.fx), v11, acc);
            }
        }
    }
    *reinterpret_cast<float4*>(out + pair * D + c) = acc;
}

// sum over the 2^lg lanes of a group (lg <= 5), the result in every lane of the group: DPP inside a row of 16 (quad
// permutes, then the mirrored half row and the mirrored row: after the quad steps every lane of a quad holds its quad's sum),
// one bpermute for the groups of 32.  Groups are aligned to their size and a wave's lanes all arrive here.
__device__ __forceinline__ float group_sum(float x, int lg) {
    if (lg >= 1) x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0xB1, 0xf, 0xf, true));    // quad_perm [1, 0, 3, 2]
    if (lg >= 2) x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x4E, 0xf, 0xf, true));    // quad_perm [2, 3, 0, 1]
    if (lg >= 3) x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x141, 0xf, 0xf, true));   // row_half_mirror
    if (lg >= 4) x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x140, 0xf, 0xf, true));   // row_mirror
    if (lg >= 5) x += __shfl_xor(x, 16, 64);
    return x;
}

// dattn[sample] = sum_d dout[d] * bilinear(value)[d];  dloc[sample] = w * (W_l d/dx, H_l d/dy) of the same sum.  Same lane
// layout as the forward; every lane of a wave stays in step (idle lanes contribute zeros), lane 0 of a group writes.
__global__ __launch_bounds__(MSDA_THREADS) void msda_bwd_query_kernel(const float* __restrict__ value, const float* __restrict__ loc,
                                                                      const float* __restrict__ attn, const float* __restrict__ dout,
                                                                      float* __restrict__ dloc, float* __restrict__ dattn,
                                                                      MsdaLevels lv, int L, int S, int Lq, int M, int D, int P, int lg,
                                                                      int64_t pairs) {
    const int64_t pair_raw = ((int64_t)blockIdx.x * MSDA_THREADS + threadIdx.x) >> lg;
    const int sub = threadIdx.x & ((1 << lg) - 1);
    const int c = sub * 4;
    const bool pair_on = pair_raw < pairs;
    const bool on = pair_on && c < D;
    const int64_t pair = pair_on ? pair_raw : pairs - 1;
    const int m = (int)(pair % M);
    const int64_t n = pair / M / Lq;
    const int64_t rs = (int64_t)M * D;
    const float* vb = value + (n * S * M + m) * D + (on ? c : 0);
    const float* lp = loc + pair * L * P * 2;
    const float* wp = attn + pair * L * P;
    const float4 g = on ? *reinterpret_cast<const float4*>(dout + pair * D + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int l = 0; l < MSDA_MAX_LEVELS; ++l) {
        if (l < L) {
            const int H = lv.H[l], W = lv.W[l];
            const float* vl = vb + (int64_t)lv.start[l] * rs;
            for (int p = 0; p < P; ++p) {
                const int i = l * P + p;
                const float2 xy = *reinterpret_cast<const float2*>(lp + 2 * i);
                const float a = wp[i];
                const MsdaTap t = msda_tap(xy.x, xy.y, H, W);
                float d00 = 0.f, d01 = 0.f, d10 = 0.f, d11 = 0.f;
                if (on && t.ok) {
                    d00 = dot4(g, msda_row4(vl, rs, t.y0, t.x0, H, W));
                    d01 = dot4(g, msda_row4(vl, rs, t.y0, t.x0 + 1, H, W));
                    d10 = dot4(g, msda_row4(vl, rs, t.y0 + 1, t.x0, H, W));
                    d11 = dot4(g, msda_row4(vl, rs, t.y0 + 1, t.x0 + 1, H, W));
                }
                const float hx = 1.f - t.fx, hy = 1.f - t.fy;
                // the sample = hy (hx v00 + fx v01) + fy (hx v10 + fx v11)
                float s = hy * __builtin_fmaf(hx, d00, t.fx * d01) + t.fy * __builtin_fmaf(hx, d10, t.fx * d11);
                float gx = __builtin_fmaf(hy, d01 - d00, t.fy * (d11 - d10));
                float gy = __builtin_fmaf(hx, d10 - d00, t.fx * (d11 - d01));
                s = group_sum(s, lg);
                gx = group_sum(gx, lg);
                gy = group_sum(gy, lg);
                if (pair_on && sub == 0) {
                    const int64_t si = pair * L * P + i;
                    dattn[si] = t.ok ? s : 0.f;
                    dloc[2 * si] = t.ok ? a * (float)W * gx : 0.f;
                    dloc[2 * si + 1] = t.ok ? a * (float)H * gy : 0.f;
                }
            }
        }
    }
}

// idx[sample * 4 + corner] = the value row (within batch item n: (level_start + y W + x) * M + m) that corner of the sample
// reads, or -1 for a corner outside the level.  corner = 2 dy + dx.
__global__ __launch_bounds__(MSDA_THREADS) void msda_corner_rows_kernel(const float* __restrict__ loc, int32_t* __restrict__ idx,
                                                                        MsdaLevels lv, int L, int M, int P, int64_t samples) {
    for (int64_t s = (int64_t)blockIdx.x * MSDA_THREADS + threadIdx.x; s < samples; s += (int64_t)gridDim.x * MSDA_THREADS) {
        const int LP = L * P;
        const int64_t pair = s / LP;
        const int l = (int)(s - pair * LP) / P;
        const int m = (int)(pair % M);
        int H = 1, W = 1, start = 0;
#pragma unroll
        for (int k = 0; k < MSDA_MAX_LEVELS; ++k)
            if (k == l) { H = lv.H[k]; W = lv.W[k]; start = lv.start[k]; }
        const float2 xy = *reinterpret_cast<const float2*>(loc + 2 * s);
        const MsdaTap t = msda_tap(xy.x, xy.y, H, W);
        int4 r;
        int* rp = &r.x;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = t.y0 + (k >> 1), x = t.x0 + (k & 1);
            const bool in = t.ok && y >= 0 && y < H && x >= 0 && x < W;
            rp[k] = in ? (start + y * W + x) * M + m : -1;
        }
        *reinterpret_cast<int4*>(idx + 4 * s) = r;
    }
}

// dvalue[row, c] = sum over the row's list (ascending flat position (sample, corner)) of w[sample] * corner weight * dout[pair, c];
// a group of 2^lg lanes per value row (n, s, m), a float4 of its D channels per lane.  Rows with an empty list get zeros.
__global__ __launch_bounds__(MSDA_THREADS) void msda_bwd_value_kernel(const float* __restrict__ loc, const float* __restrict__ attn,
                                                                      const float* __restrict__ dout, const int32_t* __restrict__ off,
                                                                      const int32_t* __restrict__ srt, float* __restrict__ dvalue,
                                                                      MsdaLevels lv, int L, int D, int P, int lg, int64_t rows) {
    const int64_t row = ((int64_t)blockIdx.x * MSDA_THREADS + threadIdx.x) >> lg;
    const int c = (threadIdx.x & ((1 << lg) - 1)) * 4;
    if (row >= rows || c >= D) return;
    const int LP = L * P;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = off[row], e1 = off[row + 1]; e < e1; ++e) {
        const int fe = srt[e];
        const int corner = fe & 3;
        const int s = fe >> 2;
        const int pair = s / LP;
        const int l = (s - pair * LP) / P;
        int H = 1, W = 1;
#pragma unroll
        for (int k = 0; k < MSDA_MAX_LEVELS; ++k)
            if (k == l) { H = lv.H[k]; W = lv.W[k]; }
        const float2 xy = *reinterpret_cast<const float2*>(loc + 2 * (int64_t)s);
        const MsdaTap t = msda_tap(xy.x, xy.y, H, W);
        const float wx = (corner & 1) ? t.fx : 1.f - t.fx, wy = (corner & 2) ? t.fy : 1.f - t.fy;
        const float4 g = *reinterpret_cast<const float4*>(dout + (int64_t)pair * D + c);
        acc = fma4(attn[s] * (wy * wx), g, acc);
    }
    *reinterpret_cast<float4*>(dvalue + row * D + c) = acc;
}

int group_log2(int D) {
    int lg = 0;
    while ((4 << lg) < D) ++lg;
    return lg;
}
unsigned group_blocks(int64_t groups, int lg) {
    const int per = MSDA_THREADS >> lg;
    return (unsigned)((groups + per - 1) / per);
}
bool msda_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// argument checks shared by the three entry points; fills lv.  Returns ME_OK, or the error with me_last_error set.
int msda_check(const char* who, const int32_t* shapes, const int32_t* level_start, int N, int S, int M, int D, int Lq, int L, int P,
               bool inverted_index, MsdaLevels* lv) {
    ME_CHECK_ARG(N >= 0 && S >= 0 && Lq >= 0 && M > 0 && D > 0 && L > 0 && P > 0, "%s: bad sizes N=%d S=%d M=%d D=%d Lq=%d L=%d P=%d", who, N, S,
                 M, D, Lq, L, P);
    if (L > MSDA_MAX_LEVELS) {
        me_set_error("%s: L=%d levels (at most %d)", who, L, MSDA_MAX_LEVELS);
        return ME_ERR_UNSUPPORTED;
    }
    if (D % 4 != 0 || D > MSDA_MAX_D) {
        me_set_error("%s: D=%d channels per head (a multiple of 4, at most %d)", who, D, MSDA_MAX_D);
        return ME_ERR_UNSUPPORTED;
    }
    for (int l = 0; l < MSDA_MAX_LEVELS; ++l) {
        lv->H[l] = lv->W[l] = 1;
        lv->start[l] = 0;
    }
    if (S == 0) return ME_OK;                                // an empty problem: nothing is read, the levels stay unset
    ME_CHECK_ARG(shapes && level_start, "%s: spatial_shapes / level_start_index are host arrays and may not be NULL", who);
    int64_t sum = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t H = shapes[2 * l], W = shapes[2 * l + 1], st = level_start[l];
        ME_CHECK_ARG(H > 0 && W > 0 && st == sum && st + H * W <= S,
                     "%s: level %d: shape (%d, %d) at level_start_index %d: levels must follow one another from row 0 within S=%d value rows",
                     who, l, (int)H, (int)W, (int)st, S);
        lv->H[l] = (int)H; lv->W[l] = (int)W; lv->start[l] = (int)st;
        sum += H * W;
    }
    ME_CHECK_ARG(sum == S, "%s: spatial_shapes cover %lld rows, value has S=%d", who, (long long)sum, S);
    ME_CHECK_ARG((int64_t)N * Lq * M < (1ll << 33), "%s: too many (query, head) pairs for one launch", who);
    ME_CHECK_ARG(!inverted_index || ((int64_t)N * S * M < (1ll << 31) && (int64_t)N * Lq * M * L * P * 4 < (1ll << 31)),
                 "%s: too many value rows or (sample, corner) entries for the int32 inverted index", who);
    return ME_OK;
}

struct MsdaWs {
    size_t idx, off, cur, ent, srt, total;
};
MsdaWs msda_ws(int N, int S, int M, int Lq, int L, int P) {
    MsdaWs w;
    const size_t R = (size_t)N * S * M, E = (size_t)N * Lq * M * L * P * 4;
    size_t o = 0;
    auto take = [&](size_t elems) { const size_t at = o; o += (elems * 4 + 255) / 256 * 256; return at; };
    w.idx = take(E); w.off = take(R + 1); w.cur = take(R); w.ent = take(E); w.srt = take(E);
    w.total = o;
    return w;
}

}  // namespace

extern "C" int me_ms_deform_attn_fwd(const float* value, const int32_t* spatial_shapes, const int32_t* level_start, const float* loc,
                                     const float* attn, float* out, int N, int S, int M, int D, int Lq, int L, int P, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    MsdaLevels lv;
    const int rc = msda_check("me_ms_deform_attn_fwd", spatial_shapes, level_start, N, S, M, D, Lq, L, P, false, &lv);
    if (rc != ME_OK) return rc;
    if (N == 0 || Lq == 0 || S == 0) return ME_OK;
    ME_CHECK_ARG(value && loc && attn && out, "me_ms_deform_attn_fwd: NULL tensor");
    ME_CHECK_ARG(msda_aligned(value, 16) && msda_aligned(out, 16) && msda_aligned(loc, 8),
                 "me_ms_deform_attn_fwd: value / out must be 16-byte aligned, sampling_locations 8-byte aligned");
    const int64_t pairs = (int64_t)N * Lq * M;
    const int lg = group_log2(D);
    hipLaunchKernelGGL(msda_fwd_kernel, dim3(group_blocks(pairs, lg)), dim3(MSDA_THREADS), 0, stream, value, loc, attn, out, lv, L, S, Lq,
                       M, D, P, lg, pairs);
    ME_CHECK_LAUNCH("me_ms_deform_attn_fwd");
    return ME_OK;
}

extern "C" size_t me_ms_deform_attn_bwd_workspace(int N, int S, int M, int Lq, int L, int P) {
    if (N <= 0 || S <= 0 || M <= 0 || Lq <= 0 || L <= 0 || P <= 0) return 0;
    return msda_ws(N, S, M, Lq, L, P).total;
}

extern "C" int me_ms_deform_attn_bwd(const float* value, const int32_t* spatial_shapes, const int32_t* level_start, const float* loc,
                                     const float* attn, const float* dout, float* dvalue, float* dloc, float* dattn, int N, int S, int M,
                                     int D, int Lq, int L, int P, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    MsdaLevels lv;
    const int rc0 = msda_check("me_ms_deform_attn_bwd", spatial_shapes, level_start, N, S, M, D, Lq, L, P, dvalue != nullptr, &lv);
    if (rc0 != ME_OK) return rc0;
    ME_CHECK_ARG((dloc != nullptr) == (dattn != nullptr), "me_ms_deform_attn_bwd: dloc and dattn come together (both or neither)");
    ME_CHECK_ARG(dvalue || dloc, "me_ms_deform_attn_bwd: no gradient asked for");
    if (N == 0 || S == 0) return ME_OK;
    if (Lq == 0) {                                           // no sample touches value
        if (dvalue && hipMemsetAsync(dvalue, 0, (size_t)N * S * M * D * 4, stream) != hipSuccess) {
            me_set_error("me_ms_deform_attn_bwd: memset failed");
            return ME_ERR_HIP;
        }
        return ME_OK;
    }
    ME_CHECK_ARG(value && loc && attn && dout, "me_ms_deform_attn_bwd: NULL tensor");
    ME_CHECK_ARG(msda_aligned(value, 16) && msda_aligned(dout, 16) && msda_aligned(loc, 8) && (!dvalue || msda_aligned(dvalue, 16)),
                 "me_ms_deform_attn_bwd: value / dout / dvalue must be 16-byte aligned, sampling_locations 8-byte aligned");
    const int lg = group_log2(D);
    const int64_t pairs = (int64_t)N * Lq * M;
    if (dloc) {
        hipLaunchKernelGGL(msda_bwd_query_kernel, dim3(group_blocks(pairs, lg)), dim3(MSDA_THREADS), 0, stream, value, loc, attn, dout, dloc,
                           dattn, lv, L, S, Lq, M, D, P, lg, pairs);
        ME_CHECK_LAUNCH("me_ms_deform_attn_bwd (dloc / dattn)");
    }
    if (dvalue) {
        const MsdaWs w = msda_ws(N, S, M, Lq, L, P);
        if (!workspace || workspace_bytes < w.total) {
            me_set_error("me_ms_deform_attn_bwd: workspace of %zu bytes needed", w.total);
            return ME_ERR_WORKSPACE;
        }
        ME_CHECK_ARG(msda_aligned(workspace, 16), "me_ms_deform_attn_bwd: workspace must be 16-byte aligned");
        char* ws = static_cast<char*>(workspace);
        auto I = [&](size_t at) { return reinterpret_cast<int32_t*>(ws + at); };
        const int64_t samples = pairs * L * P;
        hipLaunchKernelGGL(msda_corner_rows_kernel, dim3(grid_blocks(samples)), dim3(MSDA_THREADS), 0, stream, loc, I(w.idx), lv, L, M, P,
                           samples);
        const int rc = invert_lists(I(w.idx), N, (int64_t)Lq * M * L * P * 4, S * M, I(w.off), I(w.cur), I(w.ent), I(w.srt), stream,
                                    "me_ms_deform_attn_bwd (inverted lists)");
        if (rc != ME_OK) return rc;
        const int64_t rows = (int64_t)N * S * M;
        hipLaunchKernelGGL(msda_bwd_value_kernel, dim3(group_blocks(rows, lg)), dim3(MSDA_THREADS), 0, stream, loc, attn, dout, I(w.off),
                           I(w.srt), dvalue, lv, L, D, P, lg, rows);
        ME_CHECK_LAUNCH("me_ms_deform_attn_bwd (dvalue)");
    }
    return ME_OK;
}
