// point.hip -- the point-cloud grouping of P3Embed (openpoints group_embed.py:176-286) at room scale, and the feature
// propagation of the point segmentation decoders (PointNet++ three_nn + three_interpolate, layers/upsampling.py):
//   * me_fps / me_knn / me_group_relative: the tokenizer front end of PointPatchEmbed -- farthest point sampling, the k nearest
//     neighbours with the distances resident in LDS (n <= 10 240) and the relative-xyz neighbourhood rows;
//   * me_knn_stream: k nearest support points for clouds of any size (me_knn's LDS-resident form holds n <= 10 240);
//   * me_group_features / me_group_features_bwd: the grouped GEMM operand rows [dp | f-part | 0 ...] and their
//     deterministic backward onto the token-major features;
//   * me_three_nn / me_three_interpolate / me_three_interpolate_bwd: inverse-distance interpolation from the 3 nearest known
//     points onto token-major rows, and its deterministic backward.
#include "common.h"
#include "inv_lists.h"

namespace {

// ---- point-cloud tokenizer front end: farthest point sampling, k nearest neighbours, neighbourhood gather.
// Replaces, for PointPatchEmbed (PointCloud/openpoints/models/layers/group_embed.py:138-172):
//   furthest_point_sample  -> furthest_point_sampling_kernel (openpoints/cpp/pointnet2_batch/src/sampling_gpu.cu:101-210)
//   KNNGroup / KNN         -> torch.cdist + topk(largest=False) (openpoints/models/layers/group.py:12-28, 297-320)
//   grouping_operation + "relative_xyz"  (group.py:310-313)
// Index arithmetic is integer; the sampled / neighbour INDICES are what the parity tests compare bit-exactly.
//
// FPS.  What the reference kernel computes per round -- the next sample is the point that maximises min(d(p, last sample),
// temp[p]) -- is an arg-max with a SPECIFIC order among equal values, fixed by its thread-strided scan and its shared-memory
// tree (thread t = k mod T walks k = t, t + T, ... keeping the first strict maximum; partners (t, t + s), s = T/2 .. 1, fold
// with `v2 > v1 ? i2 : i1`): the winner is the candidate with the largest value, then the smallest BIT-REVERSED thread id,
// then the smallest k.  That is a total order, so here it is one 64-bit key per candidate
//     key = value bits (a non-negative float: monotone as an integer) << 32 | ~(bitrev(t) << ibits | k / T)
// and the arg-max is an unsigned maximum, taken in any association:
//   * one workgroup per cloud, T = the reference's thread count (opt_n_threads: largest power of two <= n, <= 1024), thread t
//     owns the same points k = t + i T as there -- but holds them, and their running minimum distances, in REGISTERS for all
//     m rounds (x, y, z, temp: 4 registers per point, up to 24 points per lane = 24 576 points; the reference re-reads
//     12 n bytes and read-modify-writes 4 n bytes of global memory every round);
//   * a lane's own scan is the reference's (first strict maximum in slot order); across the lanes of a wave the keys meet in
//     four DPP steps (quad_perm, row_half_mirror, row_mirror) + four v_readlane + scalar maxima, across the <= 16 waves in
//     one LDS word pair per wave and ONE barrier per round (slots alternate by round parity), against log2(T) + 1 barriers;
//   * larger clouds (n > 24 576) run the same rounds with the points and temp left in memory (FPS_MEM).
// The distance is evaluated exactly as hipcc evaluates the reference's expression (x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) +
// (z2-z1)*(z2-z1) on gfx950 -- fma(dy, dy, dx*dx) + dz*dz, read off the ISA of the reference kernel built for this GPU -- so that the indices
// agree with the reference kernel built for this GPU bit for bit, not only on tie-rich lattices (tests/test_gpu_pointcloud_ref.py).
__device__ __forceinline__ float fps_dist(float dx, float dy, float dz) {
#pragma clang fp contract(off)
    const float xx = dx * dx, zz = dz * dz;
    const float xy = __builtin_fmaf(dy, dy, xx);
    return xy + zz;
}
template <int CTRL> __device__ __forceinline__ unsigned long long fps_dpp_max(unsigned long long v) {
    const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, 0xf, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, 0xf, 0xf, false);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o > v ? o : v;
}
// maximum over the wave, wave-uniform result
__device__ __forceinline__ unsigned long long fps_wave_max(unsigned long long v) {
    v = fps_dpp_max<0xB1>(v);       // quad_perm [1,0,3,2]
    v = fps_dpp_max<0x4E>(v);       // quad_perm [2,3,0,1]
    v = fps_dpp_max<0x141>(v);      // row_half_mirror
    v = fps_dpp_max<0x140>(v);      // row_mirror: every lane of a row of 16 holds the row's maximum
    unsigned long long r = 0;
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        const unsigned long long x = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), row * 16) << 32) |
                                     (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, row * 16);
        r = x > r ? x : r;
    }
    return r;
}
// R > 0: register-resident, R points per lane.  R == 0 (FPS_MEM): points and temp stay in memory.
template <int R>
__global__ __launch_bounds__(1024) void fps_kernel(const float* __restrict__ pts, float* __restrict__ temp, int32_t* __restrict__ idxs,
                                                   int n, int m, int logT, int ibits) {
    __shared__ unsigned long long wave_key[2][16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = 1 << logT, nwaves = (int)(blockDim.x >> 6);
    pts += (int64_t)b * n * 3;
    temp += (int64_t)b * n;
    idxs += (int64_t)b * m;
    // ~(bitrev(t) << ibits): the thread part of the tie order (threads past T, in a wave that T does not fill, own nothing)
    const bool lane_on = tid < T;
    const unsigned rev = logT ? (__builtin_bitreverse32((unsigned)tid) >> (32 - logT)) : 0u;
    const unsigned tie_hi = ~(rev << ibits);
    constexpr int RR = R > 0 ? R : 1;
    float px[RR], py[RR], pz[RR], tmin[RR];
    if (R > 0) {
#pragma unroll
        for (int i = 0; i < RR; ++i) {
            // slots past the end of the cloud repeat point 0: their distance is 0 from the first round on, and a lane's scan keeps
            // the FIRST maximum, so they never displace a real point
            const int k = tid + i * T;
            const int kk = (lane_on && k < n) ? k : 0;
            px[i] = pts[kk * 3 + 0]; py[i] = pts[kk * 3 + 1]; pz[i] = pts[kk * 3 + 2];
            tmin[i] = 1e10f;          // the reference's caller fills temp with 1e10 (subsample.py: fill_(1e10))
        }
    } else {
        for (int k = tid; k < n; k += T) if (lane_on) temp[k] = 1e10f;
    }
    int old = 0;
    if (tid == 0) idxs[0] = 0;
    for (int j = 1; j < m; ++j) {
        const float x1 = pts[old * 3 + 0], y1 = pts[old * 3 + 1], z1 = pts[old * 3 + 2];      // (wave-uniform address)
        float best = -1.f;
        unsigned bi = 0;
        if (R > 0) {
#pragma unroll
            for (int i = 0; i < RR; ++i) {
                const float d2 = fminf(fps_dist(px[i] - x1, py[i] - y1, pz[i] - z1), tmin[i]);
                tmin[i] = d2;
                bi = d2 > best ? (unsigned)i : bi;
                best = d2 > best ? d2 : best;
            }
        } else if (lane_on) {
            unsigned i = 0;
            for (int k = tid; k < n; k += T, ++i) {
                const float d2 = fminf(fps_dist(pts[k * 3 + 0] - x1, pts[k * 3 + 1] - y1, pts[k * 3 + 2] - z1), temp[k]);
                temp[k] = d2;
                bi = d2 > best ? i : bi;
                best = d2 > best ? d2 : best;
            }
        }
        unsigned long long key = lane_on ? (((unsigned long long)__float_as_uint(best) << 32) | (tie_hi - bi)) : 0ull;
        key = fps_wave_max(key);
        if (nwaves > 1) {
            if (lane == 0) wave_key[j & 1][wave] = key;
            __syncthreads();
            key = fps_wave_max(lane < nwaves ? wave_key[j & 1][lane] : 0ull);
        }
        const unsigned tie = ~(unsigned)key;                              // bitrev(t) << ibits | slot
        const unsigned t = logT ? (__builtin_bitreverse32(tie >> ibits) >> (32 - logT)) : 0u;
        old = (int)(((tie & ((1u << ibits) - 1u)) << logT) | t);
        old = __builtin_amdgcn_readfirstlane(old);
        if (tid == 0) idxs[j] = old;
    }
}

// ---------------------------------------------------------------------------------------------------- resident KNN
// k nearest support points of every query, ascending by squared distance, ties by lower index: one wave per query.
// Each lane scans its strided share keeping a sorted private top-k list is too register-hungry for k = 32; instead the
// wave selects the k winners one at a time (k rounds of a wave-wide arg-min over the distances held in LDS).
__global__ __launch_bounds__(256) void knn_kernel(const float* __restrict__ support, const float* __restrict__ query,
                                                  int32_t* __restrict__ idx, int n, int m, int k) {
    extern __shared__ __attribute__((aligned(16))) char knn_smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* dist = reinterpret_cast<float*>(knn_smem) + (int64_t)wave * n;      // this wave's [n] distances
    const int b = blockIdx.y;
    const int q = blockIdx.x * 4 + wave;
    if (q >= m) return;                                                         // (whole wave)
    support += (int64_t)b * n * 3;
    const float qx = query[((int64_t)b * m + q) * 3 + 0], qy = query[((int64_t)b * m + q) * 3 + 1], qz = query[((int64_t)b * m + q) * 3 + 2];
    for (int i = lane; i < n; i += 64) {
        const float dx = support[i * 3 + 0] - qx, dy = support[i * 3 + 1] - qy, dz = support[i * 3 + 2] - qz;
        dist[i] = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    }
    __builtin_amdgcn_wave_barrier();
    int32_t* out = idx + ((int64_t)b * m + q) * k;
    for (int r = 0; r < k; ++r) {
        float best = 3.0e38f;
        int besti = 0x7fffffff;
        for (int i = lane; i < n; i += 64) {
            const float d = dist[i];
            if (d < best) { best = d; besti = i; }                              // first (lowest index) of equal values per lane
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(besti, o, 64);
            if (ob < best || (ob == best && oi < besti)) { best = ob; besti = oi; }
        }
        if (lane == 0) { out[r] = besti; dist[besti] = 3.0e38f; }
        __builtin_amdgcn_wave_barrier();
    }
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
// rows[(b, s, j), 0..2] = pts[b, idx[b, s, j]] - centers[b, s] (relative_xyz), columns 3 .. cols-1 zero: the first MLP layer's
// GEMM operand (reduction dimension padded to the GEMM's 16-byte granule).
__global__ __launch_bounds__(PT_THREADS) void group_rel_kernel(const float* __restrict__ pts, const float* __restrict__ centers,
                                                               const int32_t* __restrict__ idx, float* __restrict__ rows, int B, int n,
                                                               int m, int k, int cols) {
    const int64_t total = (int64_t)B * m * k;
    for (int64_t i = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * PT_THREADS) {
        const int64_t bs = i / k;
        const int b = (int)(bs / m);
        const int id = idx[i];
        const float* p = pts + ((int64_t)b * n + id) * 3;
        const float* c = centers + bs * 3;
        float* r = rows + i * cols;
        r[0] = p[0] - c[0]; r[1] = p[1] - c[1]; r[2] = p[2] - c[2];
        for (int j = 3; j < cols; ++j) r[j] = 0.f;
    }
}

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

// ---- backward: the index lists inverted by a counting sort (inv_lists.h), each support point's list put in ascending order, then
// gathered in that order -- a fixed summation order, so two runs are bit-identical (no float atomics).

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

bool group_mode_ok(int mode) {
    return mode == ME_GROUP_DP || mode == ME_GROUP_DP_FJ || mode == ME_GROUP_DP_DF || mode == ME_GROUP_DP_FJ_DF;
}
int group_width(int mode, int C) { return 3 + (mode == ME_GROUP_DP ? 0 : mode == ME_GROUP_DP_FJ_DF ? 2 * C : C); }

// ---------------------------------------------------------------------------------------------------- three-NN interpolation
// One unknown point per lane.  A workgroup of TNN_THREADS queries of one cloud streams the known points through LDS in SoA
// tiles; every lane reads the same tile entry (a broadcast), four points per float4 read of each coordinate array.  Each lane
// keeps its 3 nearest in registers with three_nn_kernel_fast's strict-< insertion over the points in index order, so ties
// keep the lower index: the (squared distance, index) order.  The distance is me_knn's expression.  A tile's tail is padded
// with +inf coordinates, whose distance is never below a running best.  Unused slots (m < 3) keep index 0 and dist2 = +inf
// (the reference's 1e40 stored as fp32), so their weight is exactly 0.
constexpr int TNN_THREADS = 128;
constexpr int TNN_TILE = 1024;       // known points per LDS tile (12 KB, SoA)

// knn_stream_kernel's distance expression
__device__ __forceinline__ float tnn_dist(float x, float y, float z, float qx, float qy, float qz) {
    const float dx = x - qx, dy = y - qy, dz = z - qz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

__device__ __forceinline__ void tnn_insert(float d, int k, float& b1, float& b2, float& b3, int& i1, int& i2, int& i3) {
    if (d < b3) {                                            // rare once the list has filled; the shift itself is selects
        const bool c1 = d < b1, c2 = d < b2;
        b3 = c2 ? b2 : d;            i3 = c2 ? i2 : k;
        b2 = c1 ? b1 : (c2 ? d : b2); i2 = c1 ? i1 : (c2 ? k : i2);
        b1 = c1 ? d : b1;            i1 = c1 ? k : i1;
    }
}

__global__ __launch_bounds__(TNN_THREADS) void three_nn_kernel(const float* __restrict__ unknown, const float* __restrict__ known,
                                                               int32_t* __restrict__ idx, float* __restrict__ weight,
                                                               float* __restrict__ dist, int n, int m) {
    __shared__ __attribute__((aligned(16))) float sx[TNN_TILE];
    __shared__ __attribute__((aligned(16))) float sy[TNN_TILE];
    __shared__ __attribute__((aligned(16))) float sz[TNN_TILE];
    const int b = blockIdx.y;
    const int q = blockIdx.x * TNN_THREADS + threadIdx.x;
    const int qc = q < n ? q : n - 1;                        // (a lane past the end still joins the barriers; it writes nothing)
    const float* up = unknown + ((int64_t)b * n + qc) * 3;
    const float qx = up[0], qy = up[1], qz = up[2];
    known += (int64_t)b * m * 3;
    float b1 = __builtin_inff(), b2 = __builtin_inff(), b3 = __builtin_inff();
    int i1 = 0, i2 = 0, i3 = 0;
    for (int t0 = 0; t0 < m; t0 += TNN_TILE) {
        const int cnt = m - t0 < TNN_TILE ? m - t0 : TNN_TILE;
        const int cnt4 = (cnt + 3) & ~3;
        __syncthreads();                                     // the previous tile is consumed
        for (int i = threadIdx.x; i < cnt4; i += TNN_THREADS) {
            if (i < cnt) {
                const float* kp = known + (int64_t)(t0 + i) * 3;
                sx[i] = kp[0]; sy[i] = kp[1]; sz[i] = kp[2];
            } else {
                sx[i] = sy[i] = sz[i] = __builtin_inff();
            }
        }
        __syncthreads();
        const float4* X = reinterpret_cast<const float4*>(sx);
        const float4* Y = reinterpret_cast<const float4*>(sy);
        const float4* Z = reinterpret_cast<const float4*>(sz);
        for (int j = 0; j < cnt4 / 4; ++j) {
            const float4 x = X[j], y = Y[j], z = Z[j];
            const int k = t0 + 4 * j;
            tnn_insert(tnn_dist(x.x, y.x, z.x, qx, qy, qz), k, b1, b2, b3, i1, i2, i3);
            tnn_insert(tnn_dist(x.y, y.y, z.y, qx, qy, qz), k + 1, b1, b2, b3, i1, i2, i3);
            tnn_insert(tnn_dist(x.z, y.z, z.z, qx, qy, qz), k + 2, b1, b2, b3, i1, i2, i3);
            tnn_insert(tnn_dist(x.w, y.w, z.w, qx, qy, qz), k + 3, b1, b2, b3, i1, i2, i3);
        }
    }
    if (q >= n) return;
    const int64_t o = ((int64_t)b * n + q) * 3;
    const float d1 = __builtin_sqrtf(b1), d2 = __builtin_sqrtf(b2), d3 = __builtin_sqrtf(b3);
    // three_interpolation's weights: r = 1 / (dist + 1e-8), w = r / sum(r), fp32
    const float r1 = 1.f / (d1 + 1e-8f), r2 = 1.f / (d2 + 1e-8f), r3 = 1.f / (d3 + 1e-8f);
    const float s = (r1 + r2) + r3;
    idx[o] = i1; idx[o + 1] = i2; idx[o + 2] = i3;
    weight[o] = r1 / s; weight[o + 1] = r2 / s; weight[o + 2] = r3 / s;
    if (dist) { dist[o] = d1; dist[o + 1] = d2; dist[o + 2] = d3; }
}

// out[r, col0 + c] (= or +=) w0 f[i0, c] + w1 f[i1, c] + w2 f[i2, c] for the rows r = b * n + q, i_j = b * m + idx[r, j].  A wave
// takes 64 / lpr rows at once (lpr = lanes per row, a power of two covering the row's VEC-wide chunks); consecutive lanes read
// consecutive chunks of the gathered rows.  An index outside [0, m) gives a NaN row instead of a read out of bounds.
template <int VEC>
__global__ __launch_bounds__(PT_THREADS) void three_interp_kernel(const float* __restrict__ feats, int64_t ldf,
                                                                  const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                                  float* __restrict__ out, int64_t ldo, int col0, int n, int m,
                                                                  int C, int accumulate, int lpr_log2, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int lpr = 1 << lpr_log2;
    const int sub = lane >> lpr_log2, l = lane & (lpr - 1);
    const int rpw = 64 >> lpr_log2;
    const int64_t wave0 = ((int64_t)blockIdx.x * PT_THREADS + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * PT_THREADS) >> 6;
    for (int64_t r = wave0 * rpw + sub; r < rows; r += nw * rpw) {
        const int64_t base = (r / n) * m;
        const int k0 = idx[r * 3], k1 = idx[r * 3 + 1], k2 = idx[r * 3 + 2];
        const float w0 = weight[r * 3], w1 = weight[r * 3 + 1], w2 = weight[r * 3 + 2];
        const bool bad = k0 < 0 || k0 >= m || k1 < 0 || k1 >= m || k2 < 0 || k2 >= m;
        const float* f0 = feats + (base + (bad ? 0 : k0)) * ldf;
        const float* f1 = feats + (base + (bad ? 0 : k1)) * ldf;
        const float* f2 = feats + (base + (bad ? 0 : k2)) * ldf;
        float* o = out + r * ldo + col0;
        for (int c = l * VEC; c < C; c += lpr * VEC) {
            if constexpr (VEC == 4) {
                const float4 a = *reinterpret_cast<const float4*>(f0 + c), e = *reinterpret_cast<const float4*>(f1 + c),
                             g = *reinterpret_cast<const float4*>(f2 + c);
                float4 v;
                v.x = __builtin_fmaf(w2, g.x, __builtin_fmaf(w1, e.x, w0 * a.x));
                v.y = __builtin_fmaf(w2, g.y, __builtin_fmaf(w1, e.y, w0 * a.y));
                v.z = __builtin_fmaf(w2, g.z, __builtin_fmaf(w1, e.z, w0 * a.z));
                v.w = __builtin_fmaf(w2, g.w, __builtin_fmaf(w1, e.w, w0 * a.w));
                if (bad) v.x = v.y = v.z = v.w = __builtin_nanf("");
                float4* op = reinterpret_cast<float4*>(o + c);
                if (accumulate) {
                    const float4 p = *op;
                    v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
                }
                *op = v;
            } else {
                float v = __builtin_fmaf(w2, f2[c], __builtin_fmaf(w1, f1[c], w0 * f0[c]));
                if (bad) v = __builtin_nanf("");
                o[c] = accumulate ? o[c] + v : v;
            }
        }
    }
}

// dfeats[v, c] = sum over the (q, j) with idx[q, j] = v, in ascending order of q * 3 + j, of w[q, j] dout[q, col0 + c]; rows that
// no query references get 0.  The lists come from invert_lists (flat positions (b * n + q) * 3 + j, ascending).
template <int VEC>
__global__ __launch_bounds__(PT_THREADS) void three_interp_bwd_kernel(const float* __restrict__ dout, int64_t ldo, int col0,
                                                                      const float* __restrict__ weight, const int32_t* __restrict__ off,
                                                                      const int32_t* __restrict__ srt, float* __restrict__ df,
                                                                      int64_t ldf, int C, int lpr_log2, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int lpr = 1 << lpr_log2;
    const int sub = lane >> lpr_log2, l = lane & (lpr - 1);
    const int rpw = 64 >> lpr_log2;
    const int64_t wave0 = ((int64_t)blockIdx.x * PT_THREADS + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * PT_THREADS) >> 6;
    for (int64_t v = wave0 * rpw + sub; v < rows; v += nw * rpw) {
        const int e0 = off[v], e1 = off[v + 1];
        float* o = df + v * ldf;
        for (int c = l * VEC; c < C; c += lpr * VEC) {
            if constexpr (VEC == 4) {
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int e = e0; e < e1; ++e) {
                    const int fe = srt[e];
                    const float w = weight[fe];
                    const float4 d = *reinterpret_cast<const float4*>(dout + (int64_t)(fe / 3) * ldo + col0 + c);
                    s.x = __builtin_fmaf(w, d.x, s.x); s.y = __builtin_fmaf(w, d.y, s.y);
                    s.z = __builtin_fmaf(w, d.z, s.z); s.w = __builtin_fmaf(w, d.w, s.w);
                }
                *reinterpret_cast<float4*>(o + c) = s;
            } else {
                float s = 0.f;
                for (int e = e0; e < e1; ++e) {
                    const int fe = srt[e];
                    s = __builtin_fmaf(weight[fe], dout[(int64_t)(fe / 3) * ldo + col0 + c], s);
                }
                o[c] = s;
            }
        }
    }
}

// lanes per row (log2) for rows of C floats read VEC at a time: the smallest power of two covering the row, at most a wave
int lanes_log2(int C, int vec) {
    const int chunks = (C + vec - 1) / vec;
    int lg = 0;
    while ((1 << lg) < chunks && lg < 6) ++lg;
    return lg;
}
unsigned row_blocks(int64_t rows, int lpr_log2) {
    const int64_t waves = (rows + (64 >> lpr_log2) - 1) / (64 >> lpr_log2);
    int64_t b = (waves + PT_THREADS / 64 - 1) / (PT_THREADS / 64);
    const int64_t cap = 256 * 16;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct InterpWs {
    size_t off, cur, ent, srt, total;
};
InterpWs interp_ws(int B, int n, int m) {
    InterpWs w;
    const size_t N = (size_t)B * m, R = (size_t)B * n * 3;
    size_t o = 0;
    auto take = [&](size_t elems) { const size_t at = o; o += (elems * 4 + 255) / 256 * 256; return at; };
    w.off = take(N + 1); w.cur = take(N); w.ent = take(R); w.srt = take(R);
    w.total = o;
    return w;
}

}  // namespace

extern "C" int me_fps(const float* points, int32_t* idx, float* temp, int B, int n, int m, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(points && idx && temp && B > 0 && n > 0 && m > 0 && m <= n, "me_fps: bad args (B=%d n=%d m=%d)", B, n, m);
    int logT = 0;
    while ((2 << logT) <= n && logT < 10) ++logT;          // opt_n_threads(n) of the reference launcher: T = 1 << logT
    const int T = 1 << logT, threads = T < 64 ? 64 : T;
    const int per_lane = (n + T - 1) / T;                   // points per reference thread
    int ibits = 1;
    while ((1 << ibits) < per_lane) ++ibits;
#define ME_FPS_CASE(RR) hipLaunchKernelGGL(fps_kernel<RR>, dim3((unsigned)B), dim3((unsigned)threads), 0, stream, points, temp, idx, n, m, logT, ibits)
    if (per_lane <= 1) ME_FPS_CASE(1);
    else if (per_lane <= 2) ME_FPS_CASE(2);
    else if (per_lane <= 4) ME_FPS_CASE(4);
    else if (per_lane <= 8) ME_FPS_CASE(8);
    else if (per_lane <= 16) ME_FPS_CASE(16);
    else if (per_lane <= 24) ME_FPS_CASE(24);
    else ME_FPS_CASE(0);
#undef ME_FPS_CASE
    ME_CHECK_LAUNCH("me_fps");
    return ME_OK;
}

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

extern "C" int me_knn(const float* support, const float* query, int32_t* idx, int B, int n, int m, int k, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(support && query && idx && B > 0 && n > 0 && m > 0 && k > 0 && k <= n, "me_knn: bad args");
    if (n > 10240) return me_knn_stream(support, query, idx, B, n, m, k, stream_);      // beyond the LDS-resident form
    const size_t lds = (size_t)4 * n * sizeof(float);
    return launch_kernel<knn_kernel>("me_knn", dim3((unsigned)((m + 3) / 4), (unsigned)B), 256, lds, 160 * 1024, stream, support, query, idx, n, m, k);
}

extern "C" int me_group_relative(const float* points, const float* centers, const int32_t* idx, float* rows, int B, int n, int m,
                                 int k, int cols, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(points && centers && idx && rows && B > 0 && n > 0 && m > 0 && k > 0 && cols >= 3, "me_group_relative: bad args");
    hipLaunchKernelGGL(group_rel_kernel, dim3(grid_blocks((int64_t)B * m * k)), dim3(PT_THREADS), 0, stream, points, centers, idx,
                       rows, B, n, m, k, cols);
    ME_CHECK_LAUNCH("me_group_relative");
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
    hipLaunchKernelGGL(group_features_kernel, dim3(grid_blocks(total)), dim3(PT_THREADS), 0, stream, points, feats, feats_dtype,
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
        hipLaunchKernelGGL(group_centre_sum_kernel, dim3(grid_blocks(ctot)), dim3(PT_THREADS), 0, stream, drows, dcs, k, C, cols,
                           df_col, ctot);
    }
    hipLaunchKernelGGL(group_features_bwd_kernel, dim3(grid_blocks(total)), dim3(PT_THREADS), 0, stream, drows, dcs, I(w.noff),
                       I(w.nsrt), I(w.coff), I(w.csrt), df, df_dtype, C, cols, fj_col, df_col, total);
    ME_CHECK_LAUNCH("me_group_features_bwd");
    return ME_OK;
}

extern "C" int me_three_nn(const float* unknown, const float* known, int32_t* idx, float* weight, float* dist, int B, int n, int m,
                           void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(unknown && known && idx && weight && B > 0 && n >= 0, "me_three_nn: bad args");
    ME_CHECK_ARG(m > 0, "me_three_nn: m=%d known points (at least 1 required)", m);
    ME_CHECK_ARG(B <= 65535, "me_three_nn: B=%d exceeds the grid's y dimension", B);
    ME_CHECK_ARG((int64_t)B * n * 3 < (1ll << 31), "me_three_nn: B * n * 3 exceeds int32 row indexing");
    if (n == 0) return ME_OK;
    hipLaunchKernelGGL(three_nn_kernel, dim3((unsigned)((n + TNN_THREADS - 1) / TNN_THREADS), (unsigned)B), dim3(TNN_THREADS), 0, stream,
                       unknown, known, idx, weight, dist, n, m);
    ME_CHECK_LAUNCH("me_three_nn");
    return ME_OK;
}

extern "C" int me_three_interpolate(const float* feats, int ldf, const int32_t* idx, const float* weight, float* out, int ldo,
                                    int col0, int B, int n, int m, int C, int accumulate, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(feats && idx && weight && out && B > 0 && n >= 0 && m > 0 && C > 0, "me_three_interpolate: bad args");
    ME_CHECK_ARG(ldf >= C && col0 >= 0 && ldo >= col0 + C, "me_three_interpolate: ldf %d / ldo %d / col0 %d for C %d", ldf, ldo,
                 col0, C);
    const int64_t rows = (int64_t)B * n;
    if (rows == 0) return ME_OK;
    const bool vec = C % 4 == 0 && ldf % 4 == 0 && ldo % 4 == 0 && col0 % 4 == 0 && aligned16(feats) && aligned16(out);
    const int lg = lanes_log2(C, vec ? 4 : 1);
    if (vec)
        hipLaunchKernelGGL(three_interp_kernel<4>, dim3(row_blocks(rows, lg)), dim3(PT_THREADS), 0, stream, feats, (int64_t)ldf, idx,
                           weight, out, (int64_t)ldo, col0, n, m, C, accumulate, lg, rows);
    else
        hipLaunchKernelGGL(three_interp_kernel<1>, dim3(row_blocks(rows, lg)), dim3(PT_THREADS), 0, stream, feats, (int64_t)ldf, idx,
                           weight, out, (int64_t)ldo, col0, n, m, C, accumulate, lg, rows);
    ME_CHECK_LAUNCH("me_three_interpolate");
    return ME_OK;
}

extern "C" size_t me_three_interpolate_bwd_workspace(int B, int n, int m) {
    if (B <= 0 || n < 0 || m <= 0) return 0;
    return interp_ws(B, n, m).total;
}

extern "C" int me_three_interpolate_bwd(const float* dout, int ldo, int col0, const int32_t* idx, const float* weight, float* dfeats,
                                        int ldf, int B, int n, int m, int C, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(dfeats && B > 0 && n >= 0 && m > 0 && C > 0 && (n == 0 || (dout && idx && weight)), "me_three_interpolate_bwd: bad args");
    ME_CHECK_ARG(ldf >= C && col0 >= 0 && ldo >= col0 + C, "me_three_interpolate_bwd: ldf %d / ldo %d / col0 %d for C %d", ldf, ldo,
                 col0, C);
    ME_CHECK_ARG((int64_t)B * n * 3 < (1ll << 31) && (int64_t)B * m < (1ll << 31), "me_three_interpolate_bwd: too many rows for int32 lists");
    const InterpWs w = interp_ws(B, n, m);
    if (!workspace || workspace_bytes < w.total) {
        me_set_error("me_three_interpolate_bwd: workspace of %zu bytes needed", w.total);
        return ME_ERR_WORKSPACE;
    }
    char* ws = static_cast<char*>(workspace);
    auto I = [&](size_t at) { return reinterpret_cast<int32_t*>(ws + at); };
    int rc = invert_lists(idx, B, (int64_t)n * 3, m, I(w.off), I(w.cur), I(w.ent), I(w.srt), stream,
                          "me_three_interpolate_bwd (inverted lists)");
    if (rc != ME_OK) return rc;
    const int64_t rows = (int64_t)B * m;
    const bool vec = C % 4 == 0 && ldf % 4 == 0 && ldo % 4 == 0 && col0 % 4 == 0 && aligned16(dout) && aligned16(dfeats);
    const int lg = lanes_log2(C, vec ? 4 : 1);
    if (vec)
        hipLaunchKernelGGL(three_interp_bwd_kernel<4>, dim3(row_blocks(rows, lg)), dim3(PT_THREADS), 0, stream, dout, (int64_t)ldo, col0,
                           weight, I(w.off), I(w.srt), dfeats, (int64_t)ldf, C, lg, rows);
    else
        hipLaunchKernelGGL(three_interp_bwd_kernel<1>, dim3(row_blocks(rows, lg)), dim3(PT_THREADS), 0, stream, dout, (int64_t)ldo, col0,
                           weight, I(w.off), I(w.srt), dfeats, (int64_t)ldf, C, lg, rows);
    ME_CHECK_LAUNCH("me_three_interpolate_bwd");
    return ME_OK;
}
