// timeseries.hip -- the time-series tokenizer: DataEmbedding in one kernel (me_timeseries_embed) and the circular unfold
// behind its Conv1d weight gradient (me_timeseries_unfold).
#include "common.h"

namespace {

// ---- time-series DataEmbedding
constexpr int TS_MAX_MARK = 8;
struct TsTables {
    const float* tab[TS_MAX_MARK];
    int rows[TS_MAX_MARK];
};
__global__ __launch_bounds__(EW_THREADS) void ts_embed_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const int32_t* __restrict__ marks, int n_mark, TsTables tt,
                                                              const float* __restrict__ pe, void* __restrict__ out, int odt,
                                                              int B, int L, int cin, int C, int32_t* __restrict__ err) {
    // one block per (b, l) token; threads over channels.  Reference summation order (Data2Seq/Time_Series.py:93,123):
    // value + (hour + weekday + day + month [+ minute]) + pos, i.e. mark columns 3,2,1,0[,4].
    const int64_t tok = blockIdx.x;
    const int b = (int)(tok / L), l = (int)(tok % L);
    const int lm = (l - 1 + L) % L, lp = (l + 1) % L;
    const float* x0 = x + ((int64_t)b * L + lm) * cin;
    const float* x1 = x + ((int64_t)b * L + l) * cin;
    const float* x2 = x + ((int64_t)b * L + lp) * cin;
    for (int c = threadIdx.x; c < C; c += EW_THREADS) {
        const float* wc = w + (int64_t)c * cin * 3;
        float v = 0.f;
        for (int i = 0; i < cin; ++i) v += wc[i * 3 + 0] * x0[i];
        float v1 = 0.f;
        for (int i = 0; i < cin; ++i) v1 += wc[i * 3 + 1] * x1[i];
        float v2 = 0.f;
        for (int i = 0; i < cin; ++i) v2 += wc[i * 3 + 2] * x2[i];
        v = (v + v1) + v2;
        if (marks) {
            float t = 0.f;
            const int order[5] = {3, 2, 1, 0, 4};
            bool first = true;
            for (int k = 0; k < 5; ++k) {
                const int f = order[k];
                if (f >= n_mark) continue;
                int idx = marks[tok * n_mark + f];
                if (idx < 0 || idx >= tt.rows[f]) {
                    if (err) atomicExch(err, 1);
                    idx = 0;
                }
                const float e = tt.tab[f][(int64_t)idx * C + c];
                t = first ? e : t + e;
                first = false;
            }
            v += t;
        }
        if (pe) v += pe[(int64_t)l * C + c];
        store1_from_f32(out, odt, tok * C + c, v);
    }
}

}  // namespace

extern "C" int me_timeseries_embed(const float* x, const float* conv_w, const int32_t* marks, int n_mark,
                                   const float* const* tables, const int32_t* table_rows, const float* pe, void* out,
                                   int out_dtype, int B, int L, int cin, int C, int32_t* err_flag, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && conv_w && out && B > 0 && L > 0 && cin > 0 && C > 0, "me_timeseries_embed: bad args");
    ME_CHECK_ARG(me_dtype_ok(out_dtype), "me_timeseries_embed: bad dtype");
    ME_CHECK_ARG(n_mark >= 0 && n_mark <= 5, "me_timeseries_embed: n_mark must be 0..5");
    ME_CHECK_ARG(n_mark == 0 || (marks && tables && table_rows), "me_timeseries_embed: marks given without tables");
    TsTables tt;
    for (int f = 0; f < TS_MAX_MARK; ++f) { tt.tab[f] = nullptr; tt.rows[f] = 0; }
    for (int f = 0; f < n_mark; ++f) {   // `tables` / `table_rows` are HOST arrays of device pointers / sizes
        tt.tab[f] = tables[f];
        tt.rows[f] = table_rows[f];
        ME_CHECK_ARG(tt.tab[f] && tt.rows[f] > 0, "me_timeseries_embed: bad table %d", f);
    }
    hipLaunchKernelGGL(ts_embed_kernel, dim3((unsigned)((int64_t)B * L)), dim3(EW_THREADS), 0, stream, x, conv_w,
                       n_mark ? marks : nullptr, n_mark, tt, pe, out, out_dtype, B, L, cin, C, err_flag);
    ME_CHECK_LAUNCH("me_timeseries_embed");
    return ME_OK;
}

// circular unfold for the Conv1d weight gradient: out[(b,l), i*3 + k] = x[b, (l + k - 1) mod L, i], zero in the pad columns
__global__ __launch_bounds__(EW_THREADS) void ts_unfold_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int L,
                                                               int cin, int ncols) {
    const int64_t total = (int64_t)B * L * ncols;
    for (int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * EW_THREADS) {
        const int col = (int)(t % ncols);
        const int64_t row = t / ncols;
        float v = 0.f;
        if (col < 3 * cin) {
            const int i = col / 3, k = col % 3;
            const int l = (int)(row % L);
            const int64_t b = row / L;
            int ls = l + k - 1;
            ls = ls < 0 ? ls + L : (ls >= L ? ls - L : ls);
            v = x[(b * L + ls) * cin + i];
        }
        out[t] = v;
    }
}

extern "C" int me_timeseries_unfold(const float* x, float* out, int B, int L, int cin, int ncols, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(x && out && B > 0 && L > 0 && cin > 0 && ncols >= 3 * cin, "me_timeseries_unfold: bad args");
    hipLaunchKernelGGL(ts_unfold_kernel, dim3(grid_blocks((int64_t)B * L * ncols)), dim3(EW_THREADS), 0, stream, x, out, B, L, cin,
                       ncols);
    ME_CHECK_LAUNCH("me_timeseries_unfold");
    return ME_OK;
}
