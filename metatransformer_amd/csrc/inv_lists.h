// inv_lists.h -- inversion of an index map by a counting sort, shared by the deterministic scatter backwards (point.hip:
// me_group_features_bwd, me_three_interpolate_bwd; deform.hip: me_ms_deform_attn_bwd).  idx [B, L] holds, per flat position, the
// destination it contributes to (a value in [0, n); anything else contributes nowhere).  invert_lists turns it into, per destination
// b * n + v, the list of the flat positions b * L + l that name it, in ascending order: a fixed summation order for whoever gathers
// along the lists, so two runs are bit-identical (no float atomics).
#pragma once
#include "common.h"

namespace {

constexpr int PT_THREADS = 256;

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

// inverts idx [B, L] (values in [0, n)) into ascending per-point lists of flat positions b * L + l: off [B n + 1], srt
int invert_lists(const int32_t* idx, int B, int64_t L, int n, int32_t* off, int32_t* cur, int32_t* ent, int32_t* srt,
                 hipStream_t stream, const char* what = "me_group_features_bwd (inverted lists)") {
    const int64_t N = (int64_t)B * n, total = (int64_t)B * L;
    if (hipMemsetAsync(cur, 0, (size_t)N * 4, stream) != hipSuccess) { me_set_error("%s: memset failed", what); return ME_ERR_HIP; }
    hipLaunchKernelGGL(inv_count_kernel, dim3(grid_blocks(total)), dim3(PT_THREADS), 0, stream, idx, L, total, n, cur);
    hipLaunchKernelGGL(inv_scan_kernel, dim3(1), dim3(1024), 0, stream, cur, off, N);
    hipLaunchKernelGGL(inv_fill_kernel, dim3(grid_blocks(total)), dim3(PT_THREADS), 0, stream, idx, L, total, n, off, cur, ent);
    hipLaunchKernelGGL(inv_sort_kernel, dim3(grid_blocks(N * 64)), dim3(PT_THREADS), 0, stream, off, ent, srt, N);
    ME_CHECK_LAUNCH(what);
    return ME_OK;
}

}  // namespace
