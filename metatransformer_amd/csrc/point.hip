// point.hip -- the point-cloud grouping of P3Embed (openpoints group_embed.py:176-286) at room scale:
//   * me_knn_stream: k nearest support points for clouds of any size (me_knn's LDS-resident form holds n <= 10 240);
//   * me_group_features / me_group_features_bwd: the grouped GEMM operand rows [dp | f-part | 0 ...] and their
//     deterministic backward onto the token-major features.
#include "common.h"

namespace {

constexpr int PT_THREADS = 256;
inline unsigned pt_blocks(int64_t work_items) {
    int64_t b = (work_items + PT_THREADS - 1) / PT_THREADS;
    const int64_t cap = 256 * 8;   // 256 CUs x 8 blocks, grid-stride the rest
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---------------------------------------------------------------------------------------------------- streaming KNN
// A workgroup of 4 waves takes 4 x KNN_QPW queries of one cloud and streams the support points through LDS in tiles of
// KNN_TILE, shared by all its queries.  Each query keeps its running top-k as ONE 64-bit key per lane, sorted ascending
// across lanes 0..k-1 of the wave:  key = distance bits << 32 | index  (a non-negative float is monotone as an integer, so
// the unsigned order of the keys is the lexicographic (distance, index) order: ties go to the lower index, as in knn_kernel).
// Per tile step every lane computes the distance of one candidate; a ballot keeps the candidates below the current k-th key
// (usually none once the list has filled: ~k ln(n / k) insertions per query on an unordered cloud) and each survivor is
// inserted in one shift of the list across the lanes.  The distance is knn_kernel's expression, so both forms rank alike.
constexpr int KNN_TILE = 2048;       // support points per LDS tile (24 KB, SoA)
constexpr int KNN_QPW = 4;           // queries per wave

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void knn_stream_kernel(const float* __restrict__ support, const float* __restrict__ query,
                                                         int32_t* __restrict__ idx, int n, int m, int k) {
    __shared__ float sx[KNN_TILE], sy[KNN_TILE], sz[KNN_TILE];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int q0 = (blockIdx.x * 4 + wave) * KNN_QPW;
    support += (int64_t)b * n * 3;
    float qx[KNN_QPW], qy[KNN_QPW], qz[KNN_QPW];
    unsigned long long list[KNN_QPW], thr[KNN_QPW];
#pragma unroll
    for (int t = 0; t < KNN_QPW; ++t) {
        const int q = q0 + t < m ? q0 + t : m - 1;           // (a wave past the end still joins the barriers; it writes nothing)
        const float* qp = query + ((int64_t)b * m + q) * 3;
        qx[t] = qp[0]; qy[t] = qp[1]; qz[t] = qp[2];
        list[t] = ~0ull;
        thr[t] = ~0ull;
    }
    for (int t0 = 0; t0 < n; t0 += KNN_TILE) {
        const int cnt = n - t0 < KNN_TILE ? n - t0 : KNN_TILE;
        __syncthreads();                                     // the previous tile is consumed
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const float* sp = support + (int64_t)(t0 + i) * 3;
            sx[i] = sp[0]; sy[i] = sp[1]; sz[i] = sp[2];
        }
        __syncthreads();
        for (int i0 = 0; i0 < cnt; i0 += 64) {
            const int i = i0 + lane;
            const bool on = i < cnt;
            const float x = on ? sx[i] : 0.f, y = on ? sy[i] : 0.f, z = on ? sz[i] : 0.f;
#pragma unroll
            for (int t = 0; t < KNN_QPW; ++t) {
                const float dx = x - qx[t], dy = y - qy[t], dz = z - qz[t];
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                const unsigned long long key = on ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(t0 + i)) : ~0ull;
                unsigned long long surv = __ballot(key < thr[t]);
                while (surv) {
                    const int l = __builtin_ctzll(surv);
                    surv &= surv - 1;
                    const unsigned long long v = readlane64(key, l);
                    if (v < thr[t]) {                        // (an earlier survivor of this step may have lowered the bar)
                        const unsigned long long cur = list[t];
                        const unsigned plo = (unsigned)__shfl_up((int)(unsigned)cur, 1, 64);
                        const unsigned phi = (unsigned)__shfl_up((int)(unsigned)(cur >> 32), 1, 64);
                        const unsigned long long prev = ((unsigned long long)phi << 32) | plo;
                        list[t] = cur < v ? cur : ((lane == 0 || prev < v) ? v : prev);
                        thr[t] = readlane64(list[t], k - 1);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < KNN_QPW; ++t) {
        const int q = q0 + t;
        if (q < m && lane < k) idx[((int64_t)b * m + q) * k + lane] = (int32_t)(unsigned)list[t];
    }
}

// ---------------------------------------------------------------------------------------------------- grouped rows
// rows[(b, s, j), :] = [ p[nbr] - p[ctr] (3) | mode part | 0 ... ] with nbr = nbr_idx[b, s, j], ctr = ctr_idx[b, s]:
//   ME_GROUP_DP       nothing            ME_GROUP_DP_FJ     f[nbr] (C)
//   ME_GROUP_DP_DF    f[nbr] - f[ctr]    ME_GROUP_DP_FJ_DF  f[nbr] (C) | f[nbr] - f[ctr] (C)
// One thread per output element, consecutive threads along a row (coalesced stores, row-contiguous gathers).  An index
// outside [0, n) yields a NaN row instead of a read out of bounds.
__global__ __launch_bounds__(PT_THREADS) void group_features_kernel(const float* __restrict__ pts, const void* __restrict__ feats,
                                                                    int fdt, const int32_t* __restrict__ ctr,
                                                                    const int32_t* __restrict__ nbr, float* __restrict__ rows,
                                                                    int n, int m, int k, int C, int cols, int mode, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PT_THREADS) {
        const int64_t row = e / cols;
        const int c = (int)(e - row * cols);
        const int64_t bs = row / k;
        const int64_t b = bs / m;
        const int ni = nbr[row], ci = ctr[bs];
        float v = 0.f;
        if (ni < 0 || ni >= n || ci < 0 || ci >= n) {
            v = __builtin_nanf("");
        } else if (c < 3) {
            v = pts[(b * n + ni) * 3 + c] - pts[(b * n + ci) * 3 + c];
        } else {
            const int cf = c - 3;
            const int64_t fn = (b * n + ni) * C, fc = (b * n + ci) * C;
            if (mode == ME_GROUP_DP_FJ) {
                if (cf < C) v = load1_as_f32(feats, fdt, fn + cf);
            } else if (mode == ME_GROUP_DP_DF) {
                if (cf < C) v = load1_as_f32(feats, fdt, fn + cf) - load1_as_f32(feats, fdt, fc + cf);
            } else if (mode == ME_GROUP_DP_FJ_DF) {
                if (cf < C) v = load1_as_f32(feats, fdt, fn + cf);
                else if (cf < 2 * C) v = load1_as_f32(feats, fdt, fn + cf - C) - load1_as_f32(feats, fdt, fc + cf - C);
            }
        }
        rows[e] = v;
    }
}

// ---- backward: the index lists inverted by a counting sort, each support point's list put in ascending order, then
// gathered in that order -- a fixed summation order, so two runs are bit-identical (no float atomics).
// cnt[b * n + v] = occurrences of v in idx[b, :] (integer atomics: exact)
__global__ __launch_bounds__(PT_THREADS) void inv_count_kernel(const int32_t* __restrict__ idx, int64_t L, int64_t total, int n,
                                                               int32_t* __restrict__ cnt) {
    for (int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PT_THREADS) {
        const int v = idx[e];
        if (v >= 0 && v < n) atomicAdd(&cnt[(e / L) * n + v], 1);
    }
}

// off[0..N] = exclusive prefix sum of cnt[0..N-1] (one workgroup of 1024: a contiguous chunk per thread, an LDS scan of the
// chunk sums); cnt is zeroed behind it for use as the fill cursor
__global__ __launch_bounds__(1024) void inv_scan_kernel(int32_t* __restrict__ cnt, int32_t* __restrict__ off, int64_t N) {
    __shared__ int32_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (N + 1023) / 1024;
    const int64_t lo = t * per < N ? t * per : N, hi = lo + per < N ? lo + per : N;
    int32_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int32_t add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int32_t run = part[t] - s;                               // exclusive
    for (int64_t i = lo; i < hi; ++i) {
        off[i] = run;
        run += cnt[i];
        cnt[i] = 0;
    }
    if (t == 1023) off[N] = part[1023];
}

__global__ __launch_bounds__(PT_THREADS) void inv_fill_kernel(const int32_t* __restrict__ idx, int64_t L, int64_t total, int n,
                                                              const int32_t* __restrict__ off, int32_t* __restrict__ cur,
                                                              int32_t* __restrict__ ent) {
    for (int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PT_THREADS) {
        const int v = idx[e];
        if (v < 0 || v >= n) continue;
        const int64_t slot = (e / L) * n + v;
        ent[off[slot] + atomicAdd(&cur[slot], 1)] = (int32_t)e;
    }
}

// one wave per list: every entry's rank = number of smaller entries of the list (entries are distinct row ids)
__global__ __launch_bounds__(PT_THREADS) void inv_sort_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ ent,
                                                              int32_t* __restrict__ srt, int64_t N) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * PT_THREADS + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * PT_THREADS) >> 6;
    for (int64_t s = wave0; s < N; s += nw) {
        const int o = off[s], c = off[s + 1] - o;
        for (int p = lane; p < c; p += 64) {
            const int32_t v = ent[o + p];
            int r = 0;
            for (int q = 0; q < c; ++q) r += ent[o + q] < v;
            srt[o + r] = v;
        }
    }
}

// dcs[bs, c] = sum_j drow[(bs, j), col0 + c]: the gradient every centre receives from its own group
__global__ __launch_bounds__(PT_THREADS) void group_centre_sum_kernel(const float* __restrict__ drow, float* __restrict__ dcs, int k,
                                                                      int C, int cols, int col0, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PT_THREADS) {
        const int64_t bs = e / C;
        const int c = (int)(e - bs * C);
        const float* r = drow + bs * k * cols + col0 + c;
        float s = 0.f;
        for (int j = 0; j < k; ++j) s += r[(int64_t)j * cols];
        dcs[e] = s;
    }
}

// df[b, i, c] = sum over the rows that gathered i as a neighbour (ascending row id) of their feature-part gradients
//             - sum over the centres at i (ascending) of dcs
__global__ __launch_bounds__(PT_THREADS) void group_features_bwd_kernel(const float* __restrict__ drow, const float* __restrict__ dcs,
                                                                        const int32_t* __restrict__ noff, const int32_t* __restrict__ nsrt,
                                                                        const int32_t* __restrict__ coff, const int32_t* __restrict__ csrt,
                                                                        void* __restrict__ df, int dfdt, int C, int cols, int fj_col,
                                                                        int df_col, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * PT_THREADS) {
        const int64_t bi = e / C;
        const int c = (int)(e - bi * C);
        float s = 0.f;
        for (int q = noff[bi], qe = noff[bi + 1]; q < qe; ++q) {
            const float* r = drow + (int64_t)nsrt[q] * cols;
            if (fj_col >= 0) s += r[fj_col + c];
            if (df_col >= 0) s += r[df_col + c];
        }
        if (df_col >= 0) {
            float cs = 0.f;
            for (int q = coff[bi], qe = coff[bi + 1]; q < qe; ++q) cs += dcs[(int64_t)csrt[q] * C + c];
            s -= cs;
        }
        store1_from_f32(df, dfdt, e, s);
    }
}

// byte offsets of the backward's workspace pieces (4-byte elements throughout)
struct GroupWs {
    size_t noff, ncur, nent, nsrt, coff, ccur, cent, csrt, dcs, total;
};
GroupWs group_ws(int B, int n, int m, int k, int C) {
    GroupWs w;
    const size_t N = (size_t)B * n, R = (size_t)B * m * k, S = (size_t)B * m;
    size_t o = 0;
    auto take = [&](size_t elems) { const size_t at = o; o += (elems * 4 + 255) / 256 * 256; return at; };
    w.noff = take(N + 1); w.ncur = take(N); w.nent = take(R); w.nsrt = take(R);
    w.coff = take(N + 1); w.ccur = take(N); w.cent = take(S); w.csrt = take(S);
    w.dcs = take((size_t)B * m * C);
    w.total = o;
    return w;
}

// inverts idx [B, L] (values in [0, n)) into ascending per-point lists of flat positions b * L + l: off [B n + 1], srt
int invert_lists(const int32_t* idx, int B, int64_t L, int n, int32_t* off, int32_t* cur, int32_t* ent, int32_t* srt,
                 hipStream_t stream) {
    const int64_t N = (int64_t)B * n, total = (int64_t)B * L;
    if (hipMemsetAsync(cur, 0, (size_t)N * 4, stream) != hipSuccess) { me_set_error("me_group_features_bwd: memset failed"); return ME_ERR_HIP; }
    hipLaunchKernelGGL(inv_count_kernel, dim3(pt_blocks(total)), dim3(PT_THREADS), 0, stream, idx, L, total, n, cur);
    hipLaunchKernelGGL(inv_scan_kernel, dim3(1), dim3(1024), 0, stream, cur, off, N);
    hipLaunchKernelGGL(inv_fill_kernel, dim3(pt_blocks(total)), dim3(PT_THREADS), 0, stream, idx, L, total, n, off, cur, ent);
    hipLaunchKernelGGL(inv_sort_kernel, dim3(pt_blocks(N * 64)), dim3(PT_THREADS), 0, stream, off, ent, srt, N);
    ME_CHECK_LAUNCH("me_group_features_bwd (inverted lists)");
    return ME_OK;
}

bool group_mode_ok(int mode) {
    return mode == ME_GROUP_DP || mode == ME_GROUP_DP_FJ || mode == ME_GROUP_DP_DF || mode == ME_GROUP_DP_FJ_DF;
}
int group_width(int mode, int C) { return 3 + (mode == ME_GROUP_DP ? 0 : mode == ME_GROUP_DP_FJ_DF ? 2 * C : C); }

}  // namespace

extern "C" int me_knn_stream(const float* support, const float* query, int32_t* idx, int B, int n, int m, int k, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(support && query && idx && B > 0 && n > 0 && m > 0 && k > 0 && k <= n, "me_knn_stream: bad args");
    ME_CHECK_ARG(B <= 65535, "me_knn_stream: B=%d exceeds the grid's y dimension", B);
    if (k > 64) {
        me_set_error("me_knn_stream: k=%d (at most 64: one list entry per lane of a wave)", k);
        return ME_ERR_UNSUPPORTED;
    }
    const int per_block = 4 * KNN_QPW;
    hipLaunchKernelGGL(knn_stream_kernel, dim3((unsigned)((m + per_block - 1) / per_block), (unsigned)B), dim3(256), 0, stream,
                       support, query, idx, n, m, k);
    ME_CHECK_LAUNCH("me_knn_stream");
    return ME_OK;
}

extern "C" int me_group_features(const float* points, const void* feats, int feats_dtype, const int32_t* ctr_idx,
                                 const int32_t* nbr_idx, float* rows, int B, int n, int m, int k, int C, int cols, int mode,
                                 void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(group_mode_ok(mode), "me_group_features: mode %d", mode);
    ME_CHECK_ARG(points && ctr_idx && nbr_idx && rows && B > 0 && n > 0 && m > 0 && k > 0 && C >= 0 && cols > 0,
                 "me_group_features: bad args");
    ME_CHECK_ARG(mode == ME_GROUP_DP || (feats && C > 0 && me_dtype_ok(feats_dtype)), "me_group_features: features / dtype required");
    ME_CHECK_ARG(cols % 8 == 0 && cols >= group_width(mode, C), "me_group_features: cols %d (a multiple of 8 >= %d)", cols,
                 group_width(mode, C));
    const int64_t total = (int64_t)B * m * k * cols;
    hipLaunchKernelGGL(group_features_kernel, dim3(pt_blocks(total)), dim3(PT_THREADS), 0, stream, points, feats, feats_dtype,
                       ctr_idx, nbr_idx, rows, n, m, k, C, cols, mode, total);
    ME_CHECK_LAUNCH("me_group_features");
    return ME_OK;
}

extern "C" size_t me_group_features_bwd_workspace(int B, int n, int m, int k, int C) {
    if (B <= 0 || n <= 0 || m <= 0 || k <= 0 || C <= 0) return 0;
    return group_ws(B, n, m, k, C).total;
}

extern "C" int me_group_features_bwd(const float* drows, const int32_t* ctr_idx, const int32_t* nbr_idx, void* df, int df_dtype,
                                     int B, int n, int m, int k, int C, int cols, int mode, void* workspace,
                                     size_t workspace_bytes, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(group_mode_ok(mode), "me_group_features_bwd: mode %d", mode);
    ME_CHECK_ARG(drows && ctr_idx && nbr_idx && df && B > 0 && n > 0 && m > 0 && k > 0 && C > 0 && me_dtype_ok(df_dtype),
                 "me_group_features_bwd: bad args");
    ME_CHECK_ARG(cols >= group_width(mode, C), "me_group_features_bwd: cols %d < %d", cols, group_width(mode, C));
    ME_CHECK_ARG((int64_t)B * m * k < (1ll << 31) && (int64_t)B * n < (1ll << 31), "me_group_features_bwd: too many rows for int32 lists");
    const int64_t total = (int64_t)B * n * C;
    if (mode == ME_GROUP_DP) {                               // the features feed nothing
        if (hipMemsetAsync(df, 0, (size_t)total * me_dtype_size(df_dtype), stream) != hipSuccess) {
            me_set_error("me_group_features_bwd: memset failed");
            return ME_ERR_HIP;
        }
        return ME_OK;
    }
    const GroupWs w = group_ws(B, n, m, k, C);
    if (!workspace || workspace_bytes < w.total) {
        me_set_error("me_group_features_bwd: workspace of %zu bytes needed", w.total);
        return ME_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    auto I = [&](size_t at) { return reinterpret_cast<int32_t*>(ws + at); };
    int rc = invert_lists(nbr_idx, B, (int64_t)m * k, n, I(w.noff), I(w.ncur), I(w.nent), I(w.nsrt), stream);
    if (rc != ME_OK) return rc;
    const int fj_col = (mode == ME_GROUP_DP_FJ || mode == ME_GROUP_DP_FJ_DF) ? 3 : -1;
    const int df_col = mode == ME_GROUP_DP_DF ? 3 : mode == ME_GROUP_DP_FJ_DF ? 3 + C : -1;
    float* dcs = reinterpret_cast<float*>(ws + w.dcs);
    if (df_col >= 0) {
        rc = invert_lists(ctr_idx, B, m, n, I(w.coff), I(w.ccur), I(w.cent), I(w.csrt), stream);
        if (rc != ME_OK) return rc;
        const int64_t ctot = (int64_t)B * m * C;
        hipLaunchKernelGGL(group_centre_sum_kernel, dim3(pt_blocks(ctot)), dim3(PT_THREADS), 0, stream, drows, dcs, k, C, cols,
                           df_col, ctot);
    }
    hipLaunchKernelGGL(group_features_bwd_kernel, dim3(pt_blocks(total)), dim3(PT_THREADS), 0, stream, drows, dcs, I(w.noff),
                       I(w.nsrt), I(w.coff), I(w.csrt), df, df_dtype, C, cols, fj_col, df_col, total);
    ME_CHECK_LAUNCH("me_group_features_bwd");
    return ME_OK;
}
