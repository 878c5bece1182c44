// graph.hip -- the TokenGT graph tokenizer (Data2Seq/Graph.py:43-305) behind its node-identifier Linears: me_graph_tokens_fwd
// assembles padded_feature / padded_index / padding_mask in one launch, me_graph_tokens_bwd forms every parameter gradient as a
// gather along inverted index lists (inv_lists.h), so no float atomic is used and two runs are bit-identical.  Semantics and the
// summation orders: include/metaenc.h.  One wave owns one output row throughout (a float4 of the C channels per lane and step).
#include "common.h"
#include "inv_lists.h"

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_CHUNK = 512;      // positions per chunk of the table index lists: the longest list the rank sort ever sees
constexpr int GT_SEG = 64;         // entries per partial sum of a table row (= one wave: a lane holds one entry's row number)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ int clamp_index(int64_t v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : (int)v); }

// largest b in [0, B) with off[b] <= x (off ascending, off[0] = 0 <= x < off[B])
__device__ __forceinline__ int gt_find(const int32_t* __restrict__ off, int B, int x) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(GT_THREADS) void graph_fwd_kernel(me_graph_desc d, void* __restrict__ out, int out_dtype,
                                                               int64_t* __restrict__ pidx, uint8_t* __restrict__ pmask) {
    const int lane = threadIdx.x & 63;
    const int64_t row = ((int64_t)blockIdx.x * GT_THREADS + threadIdx.x) >> 6;
    const int R = d.T + 2, C = d.C;
    if (row >= (int64_t)d.B * R) return;
    const int b = (int)(row / R), r = (int)(row - (int64_t)b * R), t = r - 2;
    const int n0 = d.offsets[b], n = d.offsets[b + 1] - n0;
    const int e0 = d.offsets[d.B + 1 + b], ne = d.offsets[d.B + 2 + b] - e0;
    const bool node = r >= 2 && t < n, edge = r >= 2 && !node && t < n + ne, pad = r >= 2 && !node && !edge;
    int64_t u = 0, v = 0;
    const int64_t* feat = nullptr;
    const float* tab = nullptr;
    const float* pert = nullptr;
    int F = 0, tab_rows = 1;
    if (node) {
        u = v = t;
        feat = d.node_data + (int64_t)(n0 + t) * d.Fn; F = d.Fn; tab = d.atom; tab_rows = d.atom_rows;
        if (d.perturb) pert = d.perturb + ((int64_t)b * d.max_n + t) * C;
    } else if (edge) {
        const int64_t e = e0 + (t - n);
        u = d.edge_index[e]; v = d.edge_index[d.Se + e];
        feat = d.edge_data + e * d.Fe; F = d.Fe; tab = d.edge; tab_rows = d.edge_rows;
    }
    if (lane == 0) {
        pmask[row] = pad ? 1 : 0;
        if (r >= 2) {
            int64_t* p = pidx + ((int64_t)b * d.T + t) * 2;
            p[0] = u; p[1] = v;
        }
    }
    const bool has_z = d.Z != nullptr && n > 0 && (node || edge);
    const float* za = has_z ? d.Z + (int64_t)(n0 + clamp_index(u, n)) * 2 * C : nullptr;
    const float* zb = has_z ? d.Z + (int64_t)(n0 + clamp_index(v, n)) * 2 * C + C : nullptr;
    const float* ord = (d.order && (node || edge)) ? d.order + (u == v ? C : 0) : nullptr;
    for (int c = lane * 4; c < C; c += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r == 0) acc = ld4(d.graph_token + c);
        else if (r == 1) acc = ld4(d.null_token + c);
        else if (!pad) {
            for (int f = 0; f < F; ++f) add4(acc, ld4(tab + (int64_t)clamp_index(feat[f], tab_rows) * C + c));
            if (pert) add4(acc, ld4(pert + c));
            if (has_z) { add4(acc, ld4(za + c)); add4(acc, ld4(zb + c)); }
            if (ord) add4(acc, ld4(ord + c));
        }
        store4_from_f32(out, out_dtype, row * C + c, f32x4{acc.x, acc.y, acc.z, acc.w});
    }
}

// Layout of the index space the backward inverts (one invert_lists call):
//   positions  [0, Se) edge e as a source, [Se, 2 Se) as a target, then the Sn Fn entries of node_data, then the Se Fe of edge_data;
//   slots      [0, 2 Sn): 2 i + half = the Z_a / Z_b half of node i; then (table row r, chunk k) at 2 Sn + r NC + k, r over the atom
//              rows followed by the edge rows, k = (position within its own data array) / GT_CHUNK.  A table row's slots are
//              adjacent and its chunks ascend, so the row's whole list is one ascending run of srt.
struct GtPlan {
    int64_t L, SnF, SeF, N, maxseg;
    int NC, Rt;
    size_t nrow, erow, idx, off, cur, ent, srt, nseg, segoff, part, part2, total;
};
GtPlan gt_plan(const me_graph_desc& d) {
    GtPlan p;
    p.SnF = (int64_t)d.Sn * d.Fn; p.SeF = (int64_t)d.Se * d.Fe;
    p.L = 2 * (int64_t)d.Se + p.SnF + p.SeF;
    const int64_t longest = p.SnF > p.SeF ? p.SnF : p.SeF;
    p.NC = (int)((longest + GT_CHUNK - 1) / GT_CHUNK);
    if (p.NC < 1) p.NC = 1;
    p.Rt = d.atom_rows + d.edge_rows;
    p.N = 2 * (int64_t)d.Sn + (int64_t)p.Rt * p.NC;
    const int64_t tab = p.SnF + p.SeF;
    p.maxseg = tab / GT_SEG + (tab < p.Rt ? tab : p.Rt) + 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    p.nrow = take((size_t)d.Sn * 4); p.erow = take((size_t)d.Se * 4); p.idx = take((size_t)p.L * 4);
    p.off = take((size_t)(p.N + 1) * 4); p.cur = take((size_t)p.N * 4); p.ent = take((size_t)p.L * 4); p.srt = take((size_t)p.L * 4);
    p.nseg = take((size_t)p.Rt * 4); p.segoff = take((size_t)(p.Rt + 1) * 4);
    p.part = take((size_t)p.maxseg * d.C * 4); p.part2 = take((size_t)d.B * 2 * d.C * 4);
    p.total = o;
    return p;
}

__global__ __launch_bounds__(GT_THREADS) void gt_index_kernel(me_graph_desc d, int NC, int32_t* __restrict__ nrow,
                                                              int32_t* __restrict__ erow, int32_t* __restrict__ idx) {
    const int64_t Sn = d.Sn, Se = d.Se, SnF = Sn * d.Fn, SeF = Se * d.Fe, total = Sn + Se + SnF + SeF;
    const int R = d.T + 2;
    const int last_row = d.B * R - 1;
    const int32_t* noff = d.offsets;
    const int32_t* eoff = d.offsets + d.B + 1;
    for (int64_t w = (int64_t)blockIdx.x * GT_THREADS + threadIdx.x; w < total; w += (int64_t)gridDim.x * GT_THREADS) {
        if (w < Sn) {
            const int i = (int)w, b = gt_find(noff, d.B, i);
            const int row = b * R + 2 + (i - noff[b]);
            nrow[i] = row < last_row ? row : last_row;
        } else if (w < Sn + Se) {
            const int e = (int)(w - Sn), b = gt_find(eoff, d.B, e);
            const int n0 = noff[b], n = noff[b + 1] - n0;
            const int row = b * R + 2 + n + (e - eoff[b]);
            erow[e] = row < last_row ? row : last_row;
            const int64_t u = d.edge_index[e], v = d.edge_index[Se + e];
            idx[e] = (u >= 0 && u < n) ? 2 * (n0 + (int)u) : -1;
            idx[Se + e] = (v >= 0 && v < n) ? 2 * (n0 + (int)v) + 1 : -1;
        } else if (w < Sn + Se + SnF) {
            const int64_t p = w - Sn - Se, val = d.node_data[p];
            idx[2 * Se + p] = (val >= 1 && val < d.atom_rows) ? (int32_t)(2 * Sn + val * NC + p / GT_CHUNK) : -1;
        } else {
            const int64_t p = w - Sn - Se - SnF, val = d.edge_data[p];
            idx[2 * Se + SnF + p] = (val >= 1 && val < d.edge_rows) ? (int32_t)(2 * Sn + (d.atom_rows + val) * NC + p / GT_CHUNK) : -1;
        }
    }
}

__global__ __launch_bounds__(GT_THREADS) void gt_nseg_kernel(const int32_t* __restrict__ off, int64_t base, int NC, int Rt,
                                                             int32_t* __restrict__ nseg) {
    const int r = blockIdx.x * GT_THREADS + threadIdx.x;
    if (r >= Rt) return;
    const int len = off[base + (int64_t)(r + 1) * NC] - off[base + (int64_t)r * NC];
    nseg[r] = (len + GT_SEG - 1) / GT_SEG;
}

// dZ[i, half C + c] = dout[node token i] + the edge tokens that name node i as source (half 0) / target (half 1), ascending
__global__ __launch_bounds__(GT_THREADS) void gt_dz_kernel(const float* __restrict__ dout, const int32_t* __restrict__ nrow,
                                                           const int32_t* __restrict__ erow, const int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ srt, float* __restrict__ dZ, int Sn, int Se, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t s = ((int64_t)blockIdx.x * GT_THREADS + threadIdx.x) >> 6;
    if (s >= 2 * (int64_t)Sn) return;
    const int i = (int)(s >> 1), half = (int)(s & 1);
    const int k0 = off[s], k1 = off[s + 1];
    const float* own = dout + (int64_t)nrow[i] * C;
    for (int c = lane * 4; c < C; c += 256) {
        float4 acc = ld4(own + c);
        for (int k = k0; k < k1; ++k) add4(acc, ld4(dout + (int64_t)erow[srt[k] - half * Se] * C + c));
        *reinterpret_cast<float4*>(dZ + ((int64_t)i * 2 + half) * C + c) = acc;
    }
}

// part[g] = the sum of segment g (GT_SEG consecutive entries of one table row's list) of the token rows its entries name
__global__ __launch_bounds__(GT_THREADS) void gt_table_seg_kernel(const float* __restrict__ dout, const int32_t* __restrict__ nrow,
                                                                  const int32_t* __restrict__ erow, const int32_t* __restrict__ off,
                                                                  const int32_t* __restrict__ srt, const int32_t* __restrict__ segoff,
                                                                  float* __restrict__ part, int64_t base, int NC, int Rt, int64_t Se2,
                                                                  int64_t SnF, int Fn, int Fe, int C, int64_t maxseg) {
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * GT_THREADS + threadIdx.x) >> 6;
    if (g >= maxseg || g >= segoff[Rt]) return;
    const int r = gt_find(segoff, Rt, (int)g);
    const int k0 = off[base + (int64_t)r * NC] + (int)(g - segoff[r]) * GT_SEG;
    const int end = off[base + (int64_t)(r + 1) * NC];
    const int cnt = end - k0 < GT_SEG ? end - k0 : GT_SEG;
    int mine = 0;
    if (lane < cnt) {
        const int64_t p = srt[k0 + lane] - Se2;
        mine = p < SnF ? nrow[p / Fn] : erow[(p - SnF) / Fe];
    }
    for (int c0 = 0; c0 < C; c0 += 256) {              // (wave-uniform trip counts: every lane takes part in the shuffles)
        const int c = c0 + lane * 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < cnt; ++j) {
            const int64_t row = __shfl(mine, j, 64);
            if (c < C) add4(acc, ld4(dout + row * C + c));
        }
        if (c < C) *reinterpret_cast<float4*>(part + g * C + c) = acc;
    }
}

__global__ __launch_bounds__(GT_THREADS) void gt_table_sum_kernel(const float* __restrict__ part, const int32_t* __restrict__ segoff,
                                                                  float* __restrict__ d_atom, float* __restrict__ d_edge, int atom_rows,
                                                                  int Rt, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t r = ((int64_t)blockIdx.x * GT_THREADS + threadIdx.x) >> 6;
    if (r >= Rt) return;
    float* dst = r < atom_rows ? d_atom : d_edge;
    if (!dst) return;
    dst += (r < atom_rows ? r : r - atom_rows) * C;
    const int g0 = segoff[r], g1 = segoff[r + 1];
    for (int c = lane * 4; c < C; c += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int g = g0; g < g1; ++g) add4(acc, ld4(part + (int64_t)g * C + c));
        *reinterpret_cast<float4*>(dst + c) = acc;
    }
}

// part2[b, o] = the sum over graph b's tokens of type id o (order[1]: nodes and self-loops; order[0]: the other edges), in token order
__global__ __launch_bounds__(GT_THREADS) void gt_order_graph_kernel(me_graph_desc d, const float* __restrict__ dout,
                                                                    float* __restrict__ part2) {
    const int b = blockIdx.x, R = d.T + 2, C = d.C;
    const int n = d.offsets[b + 1] - d.offsets[b];
    const int e0 = d.offsets[d.B + 1 + b], ne = d.offsets[d.B + 2 + b] - e0;
    const float* rows = dout + ((int64_t)b * R + 2) * C;
    for (int c = threadIdx.x * 4; c < C; c += GT_THREADS * 4) {
        float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
        for (int t = 0; t < n; ++t) add4(a1, ld4(rows + (int64_t)t * C + c));
        for (int t = 0; t < ne; ++t) {
            const float4 g = ld4(rows + (int64_t)(n + t) * C + c);
            if (d.edge_index[e0 + t] == d.edge_index[d.Se + e0 + t]) add4(a1, g); else add4(a0, g);
        }
        *reinterpret_cast<float4*>(part2 + ((int64_t)b * 2) * C + c) = a0;
        *reinterpret_cast<float4*>(part2 + ((int64_t)b * 2 + 1) * C + c) = a1;
    }
}

// block o: 0 d_graph, 1 d_null (rows 0 / 1 of every graph), 2 / 3 d_order[0 / 1] (part2), each summed over the graphs in order
__global__ __launch_bounds__(GT_THREADS) void gt_colsum_kernel(const float* __restrict__ dout, const float* __restrict__ part2,
                                                               float* __restrict__ d_graph, float* __restrict__ d_null,
                                                               float* __restrict__ d_order, int B, int R, int C) {
    const int o = blockIdx.x;
    float* dst = o == 0 ? d_graph : o == 1 ? d_null : d_order ? d_order + (o - 2) * C : nullptr;
    if (!dst) return;
    const float* src = o < 2 ? dout + (int64_t)o * C : part2 + (int64_t)(o - 2) * C;
    const int64_t step = o < 2 ? (int64_t)R * C : 2 * (int64_t)C;
    for (int c = threadIdx.x * 4; c < C; c += GT_THREADS * 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = 0; b < B; ++b) add4(acc, ld4(src + b * step + c));
        *reinterpret_cast<float4*>(dst + c) = acc;
    }
}

__global__ __launch_bounds__(GT_THREADS) void gt_perturb_kernel(me_graph_desc d, const float* __restrict__ dout,
                                                                float* __restrict__ d_perturb) {
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * GT_THREADS + threadIdx.x) >> 6;
    if (w >= (int64_t)d.B * d.max_n) return;
    const int b = (int)(w / d.max_n), i = (int)(w - (int64_t)b * d.max_n), C = d.C;
    const bool live = i < d.offsets[b + 1] - d.offsets[b];
    const float* src = dout + ((int64_t)b * (d.T + 2) + 2 + i) * C;
    for (int c = lane * 4; c < C; c += 256)
        *reinterpret_cast<float4*>(d_perturb + w * C + c) = live ? ld4(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
}

bool gt_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
unsigned gt_wave_blocks(int64_t waves) { return (unsigned)((waves * 64 + GT_THREADS - 1) / GT_THREADS); }

int gt_check(const char* who, const me_graph_desc* d) {
    ME_CHECK_ARG(d != nullptr, "%s: NULL descriptor", who);
    ME_CHECK_ARG(d->B >= 0 && d->T >= 0 && d->Sn >= 0 && d->Se >= 0 && d->Fn >= 0 && d->Fe >= 0 && d->max_n >= 0 && d->max_n <= d->T &&
                     d->atom_rows > 0 && d->edge_rows > 0,
                 "%s: bad sizes B=%d T=%d Sn=%d Se=%d Fn=%d Fe=%d max_n=%d atom_rows=%d edge_rows=%d", who, d->B, d->T, d->Sn, d->Se, d->Fn,
                 d->Fe, d->max_n, d->atom_rows, d->edge_rows);
    if (d->C <= 0 || d->C % 4 != 0) {
        me_set_error("%s: C=%d channels (a positive multiple of 4)", who, d->C);
        return ME_ERR_UNSUPPORTED;
    }
    if (d->B == 0) return ME_OK;
    ME_CHECK_ARG(d->offsets && d->atom && d->edge && d->graph_token && d->null_token, "%s: NULL offsets / atom / edge / graph_token / null_token",
                 who);
    ME_CHECK_ARG((d->Sn == 0 || d->node_data) && (d->Se == 0 || (d->edge_data && d->edge_index)), "%s: NULL node_data / edge_data / edge_index",
                 who);
    ME_CHECK_ARG(gt_aligned(d->atom) && gt_aligned(d->edge) && gt_aligned(d->graph_token) && gt_aligned(d->null_token) && gt_aligned(d->order) &&
                     gt_aligned(d->Z) && gt_aligned(d->perturb),
                 "%s: tables, token rows, Z and perturb must be 16-byte aligned", who);
    ME_CHECK_ARG((int64_t)d->B * (d->T + 2) < (1ll << 31), "%s: too many token rows for int32 row numbers", who);
    return ME_OK;
}

}  // namespace

extern "C" int me_graph_tokens_fwd(const me_graph_desc* d, void* padded_feature, int out_dtype, int64_t* padded_index,
                                   uint8_t* padding_mask, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int rc = gt_check("me_graph_tokens_fwd", d);
    if (rc != ME_OK) return rc;
    ME_CHECK_ARG(me_dtype_ok(out_dtype), "me_graph_tokens_fwd: out_dtype %d (ME_F32 or ME_BF16)", out_dtype);
    if (d->B == 0) return ME_OK;
    ME_CHECK_ARG(padded_feature && padding_mask && (d->T == 0 || padded_index), "me_graph_tokens_fwd: NULL output");
    ME_CHECK_ARG(gt_aligned(padded_feature) && gt_aligned(padded_index), "me_graph_tokens_fwd: outputs must be 16-byte aligned");
    const int64_t rows = (int64_t)d->B * (d->T + 2);
    hipLaunchKernelGGL(graph_fwd_kernel, dim3(gt_wave_blocks(rows)), dim3(GT_THREADS), 0, stream, *d, padded_feature, out_dtype, padded_index,
                       padding_mask);
    ME_CHECK_LAUNCH("me_graph_tokens_fwd");
    return ME_OK;
}

extern "C" size_t me_graph_tokens_bwd_workspace(const me_graph_desc* d) {
    if (!d || d->B <= 0 || d->C <= 0 || d->Sn < 0 || d->Se < 0 || d->Fn < 0 || d->Fe < 0 || d->atom_rows <= 0 || d->edge_rows <= 0) return 0;
    return gt_plan(*d).total;
}

extern "C" int me_graph_tokens_bwd(const me_graph_desc* d, const float* dout, float* d_atom, float* d_edge, float* d_graph, float* d_null,
                                   float* d_order, float* dZ, float* d_perturb, int parts, void* workspace, size_t workspace_bytes,
                                   void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const char* who = "me_graph_tokens_bwd";
    const int rc0 = gt_check(who, d);
    if (rc0 != ME_OK) return rc0;
    ME_CHECK_ARG(parts != 0 && (parts & ~(ME_GRAPH_BWD_INDEX | ME_GRAPH_BWD_GATHER)) == 0, "%s: parts=%d (ME_GRAPH_BWD_INDEX | ME_GRAPH_BWD_GATHER)", who,
                 parts);
    if (d->B == 0) return ME_OK;
    const GtPlan p = gt_plan(*d);
    ME_CHECK_ARG(p.N < (1ll << 31) && p.L < (1ll << 31), "%s: too many index entries (%lld) or list slots (%lld) for the int32 inverted index", who,
                 (long long)p.L, (long long)p.N);
    if (!workspace || workspace_bytes < p.total) {
        me_set_error("%s: workspace of %zu bytes needed", who, p.total);
        return ME_ERR_WORKSPACE;
    }
    ME_CHECK_ARG(gt_aligned(workspace), "%s: workspace must be 16-byte aligned", who);
    char* ws = static_cast<char*>(workspace);
    auto I = [&](size_t at) { return reinterpret_cast<int32_t*>(ws + at); };
    auto Fp = [&](size_t at) { return reinterpret_cast<float*>(ws + at); };
    const int64_t base = 2 * (int64_t)d->Sn;
    if (parts & ME_GRAPH_BWD_INDEX) {
        const int64_t work = (int64_t)d->Sn + d->Se + p.SnF + p.SeF;
        if (work > 0)
            hipLaunchKernelGGL(gt_index_kernel, dim3(grid_blocks(work)), dim3(GT_THREADS), 0, stream, *d, p.NC, I(p.nrow), I(p.erow), I(p.idx));
        const int rc = invert_lists(I(p.idx), 1, p.L, (int)p.N, I(p.off), I(p.cur), I(p.ent), I(p.srt), stream, "me_graph_tokens_bwd (inverted lists)");
        if (rc != ME_OK) return rc;
        hipLaunchKernelGGL(gt_nseg_kernel, dim3((p.Rt + GT_THREADS - 1) / GT_THREADS), dim3(GT_THREADS), 0, stream, I(p.off), base, p.NC, p.Rt,
                           I(p.nseg));
        hipLaunchKernelGGL(inv_scan_kernel, dim3(1), dim3(1024), 0, stream, I(p.nseg), I(p.segoff), (int64_t)p.Rt);
        ME_CHECK_LAUNCH("me_graph_tokens_bwd (index)");
    }
    if (!(parts & ME_GRAPH_BWD_GATHER)) return ME_OK;
    ME_CHECK_ARG(dout != nullptr && gt_aligned(dout), "%s: dout NULL or not 16-byte aligned", who);
    ME_CHECK_ARG(gt_aligned(d_atom) && gt_aligned(d_edge) && gt_aligned(d_graph) && gt_aligned(d_null) && gt_aligned(d_order) && gt_aligned(dZ) &&
                     gt_aligned(d_perturb),
                 "%s: gradients must be 16-byte aligned", who);
    const int R = d->T + 2;
    if (dZ && d->Sn > 0)
        hipLaunchKernelGGL(gt_dz_kernel, dim3(gt_wave_blocks(base)), dim3(GT_THREADS), 0, stream, dout, I(p.nrow), I(p.erow), I(p.off), I(p.srt), dZ,
                           d->Sn, d->Se, d->C);
    if (d_atom || d_edge) {
        hipLaunchKernelGGL(gt_table_seg_kernel, dim3(gt_wave_blocks(p.maxseg)), dim3(GT_THREADS), 0, stream, dout, I(p.nrow), I(p.erow), I(p.off),
                           I(p.srt), I(p.segoff), Fp(p.part), base, p.NC, p.Rt, 2 * (int64_t)d->Se, p.SnF, d->Fn > 0 ? d->Fn : 1, d->Fe > 0 ? d->Fe : 1,
                           d->C, p.maxseg);
        hipLaunchKernelGGL(gt_table_sum_kernel, dim3(gt_wave_blocks(p.Rt)), dim3(GT_THREADS), 0, stream, Fp(p.part), I(p.segoff), d_atom, d_edge,
                           d->atom_rows, p.Rt, d->C);
    }
    if (d_order) hipLaunchKernelGGL(gt_order_graph_kernel, dim3(d->B), dim3(GT_THREADS), 0, stream, *d, dout, Fp(p.part2));
    if (d_graph || d_null || d_order)
        hipLaunchKernelGGL(gt_colsum_kernel, dim3(4), dim3(GT_THREADS), 0, stream, dout, Fp(p.part2), d_graph, d_null, d_order, d->B, R, d->C);
    if (d_perturb && d->max_n > 0)
        hipLaunchKernelGGL(gt_perturb_kernel, dim3(gt_wave_blocks((int64_t)d->B * d->max_n)), dim3(GT_THREADS), 0, stream, *d, dout, d_perturb);
    ME_CHECK_LAUNCH("me_graph_tokens_bwd");
    return ME_OK;
}
