// attention.hip -- fused multi-head self-attention core (forward + backward), flash-style.
//
// Replaces PointCloud/openpoints/models/layers/attention.py:28-35: the qkv reshape/permute, (q @ k^T) * scale,
// softmax(-1), attn @ v and the transpose back to [B,N,C].  The [B,H,N,N] score matrix is never written: K/V
// tiles of 64 keys are staged in LDS, the softmax runs online in registers, heads are addressed in place in
// the [tokens, 3C] Linear output (no permute copy) and O is written head-major straight into [tokens, C].
//
// This file: the entry points, the route (attn_route) and the kernel forms special to bf16 without dropout at head_dim <= 64.  What none
// of them takes (ME_ATTN_GENERIC) runs on the tiled kernels of attention_qkv.hip, which also has the MFMA formulation all forms share.
#include "attention_host.h"
#include "attention_tile.h"
#include <math.h>
#include <stdlib.h>

namespace {

// =====================================================================================================
// small-sequence kernels (bf16, head_dim <= 64, N <= 256): ONE workgroup of 8 waves per (batch, head), the whole
// sequence resident in LDS.  At the encoder's N = 197 the tiled kernels (attention_qkv.hip) are bound by staging, not math: two
// query blocks per head re-fetch K/V through different XCD L2s, every 64-key tile costs two barriers, and the
// 128-query / 64-key tiling pads 197 to 256 both ways.  Here each array is fetched exactly once with all loads in
// flight together, rows are padded only to a multiple of 32, and the per-wave loops over key (query) sub-tiles run
// without any barrier.  The backward is ONE kernel: phase A (a wave owns 32 queries) computes delta = rowsum(dO*O)
// and dQ, phase B (a wave owns 32 keys) computes dK and dV from the same resident tiles -- no delta kernel, no second
// pass over HBM.  Both phases recompute S and dP (7 MFMA products instead of the minimal 5); results are
// deterministic (no atomics).
//
// The per-wave pieces below (rows32_* and Rows32Stage: a wave owns 32 rows, 8 waves to a workgroup) are shared by seven
// kernels: attn_fwd_small / attn_bwd_small here, attn_fwd_mid / attn_bwd_mid (N <= 512) and attn_fwd_chunk /
// attn_bwd_dq_chunk / attn_bwd_dkdv_chunk (N > 512) further down.  Those differ only in what is resident in LDS and when.
// acc_zero, row_frags_load and acc_store_row / acc_store_row_pair, which they share with the tiled kernels, are in attention_tile.h.
// =====================================================================================================
// developer instrumentation (tools/attn_trace.hip defines ME_ATTN_TRACE and includes this file): per-workgroup
// s_memtime stamps at the phase boundaries; compiled out of libmetaenc.so
#ifdef ME_ATTN_TRACE
__device__ long long g_trace[1 << 19];      // [item slot < 4096][wave < 16][stamp < 8]
#define TRACE_STAMP(slot, k) do { if ((threadIdx.x & 63) == 0 && (slot) < (1 << 12)) g_trace[((slot) * 16 + (threadIdx.x >> 6)) * 8 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define TRACE_STAMP(slot, k) do { } while (0)
#endif

constexpr int SM_THREADS = 512;
constexpr int SM_MAXN = 256;
constexpr int SM_MINN = 64;      // at or below one 64-key tile the tiled kernels (more workgroups per CU) win
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

template <int HD, int NARR, int MAXN = SM_MAXN, int NTHR = SM_THREADS> struct Rows32Stage {
    static constexpr int CPR = HD / 8;
    static constexpr int ITEMS = (MAXN * CPR) / NTHR;
    u32x4 v[NARR][ITEMS];
    // branch-free: out-of-range rows / chunks read a clamped (valid) address; they are zeroed when the values are WRITTEN to
    // LDS (store), not here -- a select on a loaded value right behind the load makes the wave wait for the data, which
    // is exactly what a prefetch must not do (measured: ~4 k of 15.7 k clocks per item in the persistent forward)
    __device__ __forceinline__ void load(const bf16_t* const (&base)[NARR], const int64_t (&ld)[NARR], int N, int hd, int tid) {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int it = tid + NTHR * i;
            const int chunk = it % CPR, row = it / CPR;
            const bool ok = (row < N) && (chunk * 8 < hd);
            const int rc = ok ? row : 0, cc = ok ? chunk : 0;
#pragma unroll
            for (int a = 0; a < NARR; ++a) v[a][i] = *reinterpret_cast<const u32x4*>(base[a] + (int64_t)rc * ld[a] + cc * 8);
        }
    }
    // N / hd: the bounds the matching load() was given (rows >= N and chunks past hd are written as zeros)
    __device__ __forceinline__ void store(char* const (&lds)[NARR], int NR, int tid, int N, int hd) const {
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int it = tid + NTHR * i;
            const int chunk = it % CPR, row = it / CPR;
            const bool ok = (row < N) && (chunk * 8 < hd);
            if (row < NR) {
#pragma unroll
                for (int a = 0; a < NARR; ++a)
                    *reinterpret_cast<u32x4*>(lds[a] + row * Cfg<bf16_t, HD>::RROW + chunk * 16) = ok ? v[a][i] : zero4();
            }
        }
    }
    // load + store back to back (no prefetch distance): rows [0, N) of every array into NR rows of its tile
    __device__ __forceinline__ void fill(const bf16_t* const (&base)[NARR], const int64_t (&ld)[NARR], char* const (&lds)[NARR], int NR,
                                         int N, int hd, int tid) {
        load(base, ld, N, hd, tid);
        store(lds, NR, tid, N, hd);
    }
};

// acc + a . b over the 8 bf16 of two 16-byte fragments, in element order (per dword: low half, high half).  The 16-row ring and
// stream backward keep the same sum written out: through this function hipcc swaps the operands of their multiplies and adds (same
// values, another instruction sequence), and those kernels are not to change
__device__ __forceinline__ float bf16x8_dot_acc(float acc, u32x4 a, u32x4 b) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        acc += __uint_as_float(a[e] << 16) * __uint_as_float(b[e] << 16) +
               __uint_as_float(a[e] & 0xffff0000u) * __uint_as_float(b[e] & 0xffff0000u);
    return acc;
}

// {Q, dO} fragments of one row straight from HBM and delta = dO . O of that row (returned, summed over the two half-waves).
// Padded queries (row_ok false, the pointers at a clamped row) get zero fragments: P = 0 through lse = +inf as well
template <int HD>
__device__ __forceinline__ float rows32_load_q_do_delta(const bf16_t* qrow, const bf16_t* dorow, const bf16_t* orow, bool row_ok, int hd,
                                                        int h, bf16x8 (&qf)[Cfg<bf16_t, HD>::NKK], bf16x8 (&dof)[Cfg<bf16_t, HD>::NKK]) {
    float del = 0.f;
#pragma unroll
    for (int kk = 0; kk < Cfg<bf16_t, HD>::NKK; ++kk) {
        const int d = (2 * kk + h) * 8;
        const bool ok = d < hd;
        const int dc = ok ? d : 0;
        u32x4 rq = *reinterpret_cast<const u32x4*>(qrow + dc);
        u32x4 rd = *reinterpret_cast<const u32x4*>(dorow + dc);
        u32x4 ro = *reinterpret_cast<const u32x4*>(orow + dc);
        const bool keep = ok && row_ok;
        rq = keep ? rq : zero4(); rd = keep ? rd : zero4(); ro = keep ? ro : zero4();
        qf[kk] = *reinterpret_cast<bf16x8*>(&rq);
        dof[kk] = *reinterpret_cast<bf16x8*>(&rd);
        del = bf16x8_dot_acc(del, ro, rd);
    }
    return del + __shfl_xor(del, 32, 64);
}

// End of a forward row: l summed over the two half-waves, lse (natural log) written where `write` holds; returns 1 / l
__device__ __forceinline__ float rows32_softmax_finish(float m_run, float l_run, float* __restrict__ lse, int64_t idx, bool write) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (lse && write) lse[idx] = (m_run + __builtin_amdgcn_logf(l_tot)) * LN2;
    return 1.0f / l_tot;
}

// Write one wave's 32 x HD result (accumulators in the transposed layout: lane = row l31, registers = d) as bf16 rows.
// Straight from registers this is a row-per-lane scatter of 8-byte pieces (64 rows touched per store instruction), which
// is store-issue bound; instead the wave transposes through a private [32][HD] LDS scratch and stores whole 128-byte
// rows: 16 bytes per lane, 64/CPR rows per instruction.
template <int HD>
__device__ __forceinline__ void store_rows_via_lds(char* scr, const f32x16 (&acc)[Cfg<bf16_t, HD>::NDB], float mul,
                                                   bf16_t* __restrict__ grow0, int64_t ldg, int rows_valid, int hd,
                                                   int lane) {
    typedef Cfg<bf16_t, HD> C;
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (bf16_t)(acc[db][4 * g + e] * mul);
            *reinterpret_cast<bf16x4*>(scr + l31 * C::RROW + (32 * db + 8 * g + 4 * h) * 2) = o;
        }
    __builtin_amdgcn_wave_barrier();
    constexpr int RPI = 64 / C::CPR;      // rows per instruction
    const int chunk = lane % C::CPR, r0 = lane / C::CPR;
#pragma unroll
    for (int k = 0; k < 32 / RPI; ++k) {
        const int r = r0 + RPI * k;
        const u32x4 v = *reinterpret_cast<const u32x4*>(scr + r * C::RROW + chunk * 16);
        if (r < rows_valid && chunk * 8 < hd) *reinterpret_cast<u32x4*>(grow0 + (int64_t)r * ldg + chunk * 8) = v;
    }
    __builtin_amdgcn_wave_barrier();
}

// one step of the forward over NU 32-key sub-tiles starting at key kv0 (Kt / Vt point at that row of the resident tiles)
template <int HD, int NU, bool MASK>
__device__ __forceinline__ void rows32_fwd_step(const char* Kt, const char* Vt, int kv0, int N,
                                               const bf16x8 (&qf)[Cfg<bf16_t, HD>::NKK], float sl, float& m_run,
                                               float& l_run, f32x16 (&o)[Cfg<bf16_t, HD>::NDB], int lane) {
    typedef Cfg<bf16_t, HD> C;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 s[2];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[u][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk)
            s[u] = mma_chunk(rtile_chunk<bf16_t, HD>(Kt, 32 * u + l31, 2 * kk + h), qf[kk], s[u]);
    }
    float mt = -INFINITY;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (MASK) s[u][r] = (kv0 + 32 * u + acc_row(r, h) < N) ? s[u][r] : -INFINITY;
            mt = fmaxf(mt, s[u][r]);
        }
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64)) * sl;          // log2 domain; every step holds at least one valid key
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(s[u][r] * sl - m_new);
            s[u][r] = p;
            ps += p;
        }
    l_run = l_run * alpha + ps;
    m_run = m_new;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db) o[db] *= alpha;
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) {
        const bf16x8 pb = pack_chunk((const bf16_t*)nullptr, s, c);
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) o[db] = mma_chunk(tr_chunk<HD>(Vt, 32 * db, c, lane), pb, o[db]);
    }
}

// phase A step (wave owns 32 queries): NU 32-key sub-tiles starting at kv0
template <int HD, int NU, bool MASK>
__device__ __forceinline__ void rows32_dq_step(const char* Kt, const char* Vt, int kv0, int N,
                                                 const bf16x8 (&qf)[Cfg<bf16_t, HD>::NKK],
                                                 const bf16x8 (&dof)[Cfg<bf16_t, HD>::NKK], float sl, float lse2,
                                                 float del, f32x16 (&dq)[Cfg<bf16_t, HD>::NDB], int lane) {
    typedef Cfg<bf16_t, HD> C;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 s[2], dp[2];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[u][r] = 0.f; dp[u][r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            s[u] = mma_chunk(rtile_chunk<bf16_t, HD>(Kt, 32 * u + l31, 2 * kk + h), qf[kk], s[u]);      // S^T[kv][q]
            dp[u] = mma_chunk(rtile_chunk<bf16_t, HD>(Vt, 32 * u + l31, 2 * kk + h), dof[kk], dp[u]);   // dP^T[kv][q]
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float p = __builtin_amdgcn_exp2f(s[u][r] * sl - lse2);
            if (MASK) p = (kv0 + 32 * u + acc_row(r, h) < N) ? p : 0.f;
            dp[u][r] = p * (dp[u][r] - del);                                   // dS^T / scale (scale applied to dQ once)
        }
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) {
        const bf16x8 dsb = pack_chunk((const bf16_t*)nullptr, dp, c);
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) dq[db] = mma_chunk(tr_chunk<HD>(Kt, 32 * db, c, lane), dsb, dq[db]);   // dQ^T[d][q]
    }
}

// phase B step (wave owns 32 keys): NU 32-query sub-tiles starting at q0; lse_t / del_t point at q0 (log2-scaled lse,
// +inf on padded queries so that P = 0 there).  Padded KEYS need no mask: a key is a lane here, and whatever a padded
// lane accumulates stays in its own dK/dV columns, which are never stored.
template <int HD, int NU>
__device__ __forceinline__ void rows32_dkdv_step(const char* Qt, const char* dOt, const float* lse_t, const float* del_t,
                                                  const bf16x8 (&kf)[Cfg<bf16_t, HD>::NKK],
                                                  const bf16x8 (&vf)[Cfg<bf16_t, HD>::NKK], float sl,
                                                  f32x16 (&dk)[Cfg<bf16_t, HD>::NDB], f32x16 (&dv)[Cfg<bf16_t, HD>::NDB],
                                                  int lane) {
    typedef Cfg<bf16_t, HD> C;
    const int l31 = lane & 31, h = lane >> 5;
    f32x16 s[2], dp[2];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[u][r] = 0.f; dp[u][r] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            s[u] = mma_chunk(rtile_chunk<bf16_t, HD>(Qt, 32 * u + l31, 2 * kk + h), kf[kk], s[u]);      // S[q][kv]
            dp[u] = mma_chunk(rtile_chunk<bf16_t, HD>(dOt, 32 * u + l31, 2 * kk + h), vf[kk], dp[u]);   // dP[q][kv]
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 L = *reinterpret_cast<const f32x4*>(lse_t + 32 * u + 8 * g + 4 * h);
            const f32x4 D = *reinterpret_cast<const f32x4*>(del_t + 32 * u + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                const float p = __builtin_amdgcn_exp2f(s[u][r] * sl - L[e]);
                s[u][r] = p;                                   // P
                dp[u][r] = p * (dp[u][r] - D[e]);              // dS / scale (scale applied to dK once)
            }
        }
#pragma unroll
    for (int c = 0; c < 2 * NU; ++c) {
        const bf16x8 pb = pack_chunk((const bf16_t*)nullptr, s, c);
        const bf16x8 dsb = pack_chunk((const bf16_t*)nullptr, dp, c);
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) {
            dv[db] = mma_chunk(tr_chunk<HD>(dOt, 32 * db, c, lane), pb, dv[db]);    // dV^T[d][kv]
            dk[db] = mma_chunk(tr_chunk<HD>(Qt, 32 * db, c, lane), dsb, dk[db]);    // dK^T[d][kv]
        }
    }
}

// The walks: a wave takes its step over every 32-row sub-tile of the tiles in LDS, 64 rows at a time.  Forward and dQ walk `rows`
// keys that start at key kv0 of N (resident tiles: 0, N, N): full 64-key steps, then the masked tail -- two sub-tiles when the last
// one is partial, one when 32 or fewer keys are left.  dK/dV walks NS query sub-tiles (padded queries carry P = 0: no mask).
template <int HD>
__device__ __forceinline__ void rows32_fwd_walk(const char* Kt, const char* Vt, int kv0, int rows, int N,
                                                const bf16x8 (&qf)[Cfg<bf16_t, HD>::NKK], float sl, float& m_run, float& l_run,
                                                f32x16 (&o)[Cfg<bf16_t, HD>::NDB], int lane) {
    constexpr int SUB = 32 * Cfg<bf16_t, HD>::RROW;
    const int NS = (rows + 31) >> 5;
    int t = 0;
    for (; 32 * (t + 2) <= rows; t += 2) rows32_fwd_step<HD, 2, false>(Kt + t * SUB, Vt + t * SUB, kv0 + 32 * t, N, qf, sl, m_run, l_run, o, lane);
    if (t + 2 <= NS)
        rows32_fwd_step<HD, 2, true>(Kt + t * SUB, Vt + t * SUB, kv0 + 32 * t, N, qf, sl, m_run, l_run, o, lane);
    else if (t < NS)
        rows32_fwd_step<HD, 1, true>(Kt + t * SUB, Vt + t * SUB, kv0 + 32 * t, N, qf, sl, m_run, l_run, o, lane);
}
template <int HD>
__device__ __forceinline__ void rows32_dq_walk(const char* Kt, const char* Vt, int kv0, int rows, int N,
                                               const bf16x8 (&qf)[Cfg<bf16_t, HD>::NKK], const bf16x8 (&dof)[Cfg<bf16_t, HD>::NKK], float sl,
                                               float lse2, float del, f32x16 (&dq)[Cfg<bf16_t, HD>::NDB], int lane) {
    constexpr int SUB = 32 * Cfg<bf16_t, HD>::RROW;
    const int NS = (rows + 31) >> 5;
    int t = 0;
    for (; 32 * (t + 2) <= rows; t += 2) rows32_dq_step<HD, 2, false>(Kt + t * SUB, Vt + t * SUB, kv0 + 32 * t, N, qf, dof, sl, lse2, del, dq, lane);
    if (t + 2 <= NS)
        rows32_dq_step<HD, 2, true>(Kt + t * SUB, Vt + t * SUB, kv0 + 32 * t, N, qf, dof, sl, lse2, del, dq, lane);
    else if (t < NS)
        rows32_dq_step<HD, 1, true>(Kt + t * SUB, Vt + t * SUB, kv0 + 32 * t, N, qf, dof, sl, lse2, del, dq, lane);
}
template <int HD>
__device__ __forceinline__ void rows32_dkdv_walk(const char* Qt, const char* dOt, const float* lse_t, const float* del_t, int NS,
                                                 const bf16x8 (&kf)[Cfg<bf16_t, HD>::NKK], const bf16x8 (&vf)[Cfg<bf16_t, HD>::NKK], float sl,
                                                 f32x16 (&dk)[Cfg<bf16_t, HD>::NDB], f32x16 (&dv)[Cfg<bf16_t, HD>::NDB], int lane) {
    constexpr int SUB = 32 * Cfg<bf16_t, HD>::RROW;
    int t = 0;
    for (; t + 2 <= NS; t += 2) rows32_dkdv_step<HD, 2>(Qt + t * SUB, dOt + t * SUB, lse_t + 32 * t, del_t + 32 * t, kf, vf, sl, dk, dv, lane);
    if (t < NS) rows32_dkdv_step<HD, 1>(Qt + t * SUB, dOt + t * SUB, lse_t + 32 * t, del_t + 32 * t, kf, vf, sl, dk, dv, lane);
}

// Persistent: a workgroup walks (batch, head) items with stride gridDim.x.  While item i is computed, the K/V rows and
// Q fragments of item i+1 are already in flight into registers; they are parked in LDS once every wave is done with
// item i -- HBM latency and the bursty all-CUs-load-at-once phase hide behind the math.
template <int HD>
__global__ __launch_bounds__(SM_THREADS) void attn_fwd_small_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                    bf16_t* __restrict__ out, int64_t ldo,
                                                                    float* __restrict__ lse, int N, int H, int hd,
                                                                    float scale, int items) {
    typedef Cfg<bf16_t, HD> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NS = (N + 31) >> 5, NR = NS * 32;
    const int tile_bytes = NR * C::RROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    char* Ks = smem;
    char* Vs = smem + tile_bytes;
    char* scr = smem + 2 * tile_bytes + wave * 32 * C::RROW;      // per-wave output transposition scratch
    const int Cdim = H * hd;
    const int q = 32 * wave + l31;
    const int qrow = (q < N) ? q : N - 1;
    const bool active = 32 * wave < N;      // wave-uniform
    const float sl = scale * LOG2E;
    const int64_t ldv[2] = {ld, ld};

    Rows32Stage<HD, 2> st;
    bf16x8 qf[C::NKK], qn[C::NKK];
    auto fresh_tid = [&]() { int t = tid; asm volatile("" : "+v"(t)); return t; };
    auto issue = [&](int it, bf16x8 (&qdst)[C::NKK]) {
        const bf16_t* qptr = qkv + (int64_t)(it / H) * N * ld + (it % H) * hd;
        const bf16_t* const bases[2] = {qptr + Cdim, qptr + 2 * Cdim};
        st.load(bases, ldv, N, hd, fresh_tid());
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            const int d = (2 * kk + h) * 8;
            const bool ok = d < hd;
            const u32x4 raw = *reinterpret_cast<const u32x4*>(qptr + (int64_t)qrow * ld + (ok ? d : 0));
            qdst[kk] = *reinterpret_cast<const bf16x8*>(&raw);      // (chunks past hd are zeroed by q_take, when the value is first needed)
        }
    };
    auto q_take = [&](const bf16x8 (&src)[C::NKK]) {
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            const bool ok = (2 * kk + h) * 8 < hd;
            u32x4 raw = *reinterpret_cast<const u32x4*>(&src[kk]);
            raw = ok ? raw : zero4();
            qf[kk] = *reinterpret_cast<bf16x8*>(&raw);
        }
    };
    auto park = [&]() {
        char* const tiles[2] = {Ks, Vs};
        st.store(tiles, NR, fresh_tid(), N, hd);
    };
    int it = blockIdx.x;
    issue(it, qn);
    park();
    q_take(qn);
    __syncthreads();
    for (; it < items; it += gridDim.x) {
        const int nxt = (it + (int)gridDim.x < items) ? it + (int)gridDim.x : it;
        TRACE_STAMP(it, 0);
        issue(nxt, qn);
        if (active) {
            f32x16 o[C::NDB];
            acc_zero(o);
            float m_run = -INFINITY, l_run = 0.f;
            rows32_fwd_walk<HD>(Ks, Vs, 0, N, N, qf, sl, m_run, l_run, o, lane);
            TRACE_STAMP(it, 1);
            const int b = it / H, head = it % H;
            const float inv = rows32_softmax_finish(m_run, l_run, lse, ((int64_t)b * H + head) * N + q, h == 0 && q < N);
            store_rows_via_lds<HD>(scr, o, inv, out + ((int64_t)b * N + 32 * wave) * ldo + head * hd, ldo, N - 32 * wave, hd, lane);
        }
        TRACE_STAMP(it, 2);
        __syncthreads();      // every wave is done with the K/V tiles of this item
        TRACE_STAMP(it, 3);
        park();
        TRACE_STAMP(it, 4);
        q_take(qn);
        __syncthreads();
        TRACE_STAMP(it, 5);
    }
}

// -----------------------------------------------------------------------------------------------------
// Resident-sequence kernels, ring form (SM_MINN < N <= RS_MAXN = 224: every Base / Large image, window and point-cloud shape).
// What per-wave time stamps of the kernels above showed (tools/attn_trace, N = 197, forward 15.3 k clocks per item):
// ~4 k clocks in which every wave sits in the ISSUE of its prefetch loads (the CU's vector-memory path takes ~32 B/clk: a
// whole item's 100 KB asked for at once backs the queue up and an in-order wave cannot get past a load it cannot issue),
// ~1 k parking the prefetched rows in LDS between two barriers, a step loop hipcc schedules as read -> wait -> MFMA one
// fragment at a time, and two 250-register waves per SIMD that cannot keep the VALU fed (tools/probe_valu).  The ring form:
//   * the NEXT item's arrays go global -> LDS by DMA (buffer_load ... lds) from dedicated LOADER waves, paced, into the half
//     of LDS the current phase does not read: nothing queues in front of the compute waves, no staging registers, no park
//     phase, one barrier per phase.  Rows are unpadded; the 16-byte chunks are XOR-swizzled on the SOURCE side (a DMA lane
//     chooses which global chunk lands in its fixed LDS slot) so that both the 16-byte row reads and the transposing
//     ds_read_b64_tr_b16 reads stay bank-conflict free.  Rows >= N and chunks >= hd arrive as zeros through the buffer
//     descriptor's bounds check.
//   * 16 waves of 16 rows (16 x 16 x 32 MFMA), <= 128 registers, four waves per SIMD.
//   * forward: two-pass softmax -- N <= 224 keeps the whole S^T row block in registers, so there is no running maximum, no
//     rescale of O and no per-step shuffle; MFMA passes software-pipelined by hand (sched_barrier).
typedef __attribute__((address_space(3))) void lds_dma_t;
constexpr int RS_MAXN = 224;
template <int HD> struct RCfg {
    static constexpr int RB = HD * 2;                          // bytes per (unpadded) row
    static constexpr int CPR = HD / 8;                         // 16-byte chunks per row
    static constexpr int RPI = 1024 / RB;                      // rows one DMA instruction fills (64 lanes x 16 B)
    static constexpr int SCR = 32 * Cfg<bf16_t, HD>::RROW;     // per-wave output transposition scratch (padded rows)
};
// -----------------------------------------------------------------------------------------------------
// Ring form with 16-query waves.  tools/probe_valu: ONE wave issues a VALU instruction every ~5 clocks whatever it is, but a SIMD
// retires one per ~1.9 (add / fma), ~2.8 (max3, cvt_pk, packed) or ~5.3 (exp) clocks once three or four waves feed it -- the
// softmax arithmetic of this kernel is bound by how many waves issue it, not by the VALU itself, and two 250-register waves per
// SIMD leave more than half of it idle.  So: 16 waves per workgroup (four per SIMD, <= 128 registers each), a wave owns 16
// queries and uses the 16 x 16 x 32 MFMA:
//   S^T tile (16 keys x 16 queries) = K rows (A: lane = key l & 15, d = 8 (l >> 4) ..) x Q^T (B: lane = query l & 15, same d)
//       -> lane (query l & 15, g = l >> 4) holds keys 16 t + 4 g + j, j = 0..3;
//   O^T tile (16 d x 16 queries) += V^T (A, transposing read) x P^T (B): a lane's 8 reduction slots of a 32-key step are
//       exactly the 2 x 4 accumulator registers it already holds (keys 32 kk + 4 g + j and 32 kk + 16 + 4 g + j), and the
//       transposing read fetches V^T in the same order -- no cross-lane movement between the two products.
// Waves 14 and 15 are the loaders (paced LDS-DMA of the next item's K and V into the other ring half), other waves >= ceil(N / 16)
// only keep the barrier.
constexpr int R16_THREADS = 1024;
constexpr int R16_SLEEP = 1;        // loader pacing: s_sleep units (64 clocks) behind every DMA piece
// slot of chunk c in row r: c ^ r16_swz(r).  HD = 64: the b128 operand read has lanes {0-3, 12-15} on rows r, chunk c and lanes
// {20-27} on rows 4-11, chunk c + 1 in one LDS cycle, the transposing read 8 consecutive rows x one aligned chunk pair: row bits
// 1..2 -> slot bits 1..2 separates both.  HD = 32 (four rows per 256-byte bank row): per 4-row block the values 0, 2, 3, 1.
template <int CPR> __device__ __forceinline__ int r16_swz(int r) {
    return CPR == 8 ? (((r >> 1) & 3) << 1) : ((0x78 >> (2 * ((r >> 2) & 3))) & 3);
}
__device__ __forceinline__ f32x4 mma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// -----------------------------------------------------------------------------------------------------
// The per-wave pieces below (r16_* / st16_* and R16Frags: a wave owns 16 rows) are shared by the six kernels on 16-row waves:
// attn_fwd_ring16 / attn_bwd_ring16 here and attn_fwd_stream16 / attn_bwd_dq_stream16 / attn_bwd_dkdv_stream16 /
// attn_bwd_dkdv_stream32 (N > SM_MAXN) further down.  Those differ in what sits in LDS and when, in their loaders and in how a
// workgroup comes by its items.
constexpr int ST_KC = 128;                            // streaming kernels: keys (rows) per chunk
constexpr int ST_RING = 3;                            // ... and LDS ring slots of one {array 0, array 1} chunk each

// a lane's byte offsets into an unpadded, swizzled array for the two fragment reads
template <int HD> struct R16Frags {
    typedef RCfg<HD> R;
    static constexpr int NKS = HD / 32;               // 32-wide d steps of a row-operand product (QK^T)
    static constexpr int NDT = HD / 16;               // 16-wide d tiles of a transposed-operand product (O^T)
    int koff[NKS];                                    // row-operand read: row 16 t + l15, chunk 4 ks + g
    int troff[NDT];                                   // transposing read: rows 32 kk + 16 r + 4 g + (l15 >> 2), 8 bytes at d = 16 dt + 4 (l15 & 3)
    __device__ __forceinline__ R16Frags(int l15, int g) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) koff[ks] = l15 * R::RB + 16 * ((4 * ks + g) ^ r16_swz<R::CPR>(l15));
        const int rr = 4 * g + (l15 >> 2);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
            troff[dt] = rr * R::RB + 16 * ((2 * dt + ((l15 & 3) >> 1)) ^ r16_swz<R::CPR>(rr)) + 8 * (l15 & 1);
    }
    __device__ __forceinline__ void rowread(const char* arr, int t, bf16x8 (&dst)[NKS]) const {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) dst[ks] = *reinterpret_cast<const bf16x8*>(arr + 16 * t * R::RB + koff[ks]);
    }
    // The same address summed in two ways, which hipcc compiles differently.  As an integer (default) it re-adds per read and keeps no
    // base live: the backward steps, which sit at the 128-register edge (the pointer form there: 26 spilled registers in
    // attn_bwd_ring16_kernel<64, 7>).  As a pointer (BASE) it keeps arr + troff[dt] in a register across the steps and folds the rest
    // into the instruction's offset: the forward's PV pass, which has the room (the integer form there: two more VALU adds per half-step)
    template <bool BASE = false> __device__ __forceinline__ bf16x8 trread(const char* arr, int kk, int dt) const {
        union { bf16x4 q4[2]; bf16x8 v; } a;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int off = (32 * kk + 16 * r) * R::RB;
            const uint32_t p = BASE ? (uint32_t)(uintptr_t)(arr + off + troff[dt]) : (uint32_t)(uintptr_t)arr + off + troff[dt];
            a.q4[r] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)p);
        }
        return a.v;
    }
};

// a wave's own rows, fetched raw from global ahead of their use (the chunk address clamped to 0 past hd): chunks of d past hd are zeros
template <int HD>
__device__ __forceinline__ void r16_take(const u32x4 (&raw)[HD / 32], int g, int hd, bf16x8 (&dst)[HD / 32]) {
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
        const u32x4 v = 32 * ks + 8 * g < hd ? raw[ks] : zero4();
        dst[ks] = *reinterpret_cast<const bf16x8*>(&v);
    }
}

// Forward, pass 1: S^T of NT 16-key tiles, two at a time; the operand chunks of the next pair are in flight while this pair's
// MFMAs run (software-pipelined by hand: left alone hipcc emits read -> wait -> MFMA one fragment at a time).  `stamp`: the item
// whose trace stamp 1 is taken behind the first pair (< 0: none)
template <int HD, int NT>
__device__ __forceinline__ void r16_st_pass(const R16Frags<HD>& fr, const char* Kb, const bf16x8 (&qf)[HD / 32], f32x4 (&s)[NT], int stamp) {
    constexpr int NKS = HD / 32;
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    bf16x8 ka[2][NKS], kb[2][NKS];
    auto kread = [&](int t, bf16x8 (&dst)[2][NKS]) {
        fr.rowread(Kb, t, dst[0]);
        fr.rowread(Kb, t + 1, dst[1]);
    };
    auto kmma = [&](int t, const bf16x8 (&src)[2][NKS]) {
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) s[t + tt] = mma16(src[tt][0], qf[0], zero4f);
#pragma unroll
        for (int ks = 1; ks < NKS; ++ks)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) s[t + tt] = mma16(src[tt][ks], qf[ks], s[t + tt]);
    };
    (void)stamp;
    kread(0, ka);
#pragma unroll
    for (int t = 0; t < NT; t += 4) {
        if (t + 2 < NT) kread(t + 2, kb);
        __builtin_amdgcn_sched_barrier(0);
        kmma(t, ka);
        __builtin_amdgcn_sched_barrier(0);
        if (t == 0 && stamp >= 0) { TRACE_STAMP(stamp, 1); }
        if (t + 2 < NT) {
            if (t + 4 < NT) kread(t + 4, ka);
            __builtin_amdgcn_sched_barrier(0);
            kmma(t + 2, kb);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
// Forward, pass 2: O^T += V^T P^T over NKK 32-key steps (`fresh`: O^T starts at zero), the d tiles in two halves: the V^T operand of
// the next half is in flight while this half's MFMAs run (half-steps keep the operand buffers at 2 x NDT / 2 fragments: the ring
// kernel has to fit 128 registers)
template <int HD, int NKK>
__device__ __forceinline__ void r16_pv_pass(const R16Frags<HD>& fr, const char* Vb, const f32x4 (&s)[2 * NKK], f32x4 (&o)[HD / 16], bool fresh) {
    constexpr int NH = HD / 32;
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    bf16x8 va[NH], vb[NH];
    auto vread = [&](int kk, int half, bf16x8 (&dst)[NH]) {
#pragma unroll
        for (int i = 0; i < NH; ++i) dst[i] = fr.template trread<true>(Vb, kk, NH * half + i);
    };
    vread(0, 0, va);
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
        vread(kk, 1, vb);
        bf16x8 pb;
#pragma unroll
        for (int e = 0; e < 4; ++e) { pb[e] = (bf16_t)s[2 * kk][e]; pb[4 + e] = (bf16_t)s[2 * kk + 1][e]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NH; ++i) o[i] = mma16(va[i], pb, fresh && kk == 0 ? zero4f : o[i]);
        __builtin_amdgcn_sched_barrier(0);
        if (kk + 1 < NKK) vread(kk + 1, 0, va);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NH; ++i) o[NH + i] = mma16(vb[i], pb, fresh && kk == 0 ? zero4f : o[NH + i]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// a softmax probability from its log2-domain argument: v_exp_f32 with the clamp output modifier (hipcc folds the med3 into it)
__device__ __forceinline__ float r16_p(float arg) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(arg), 0.f, 1.f); }

// four probabilities and their dS / scale (the 32-key dK / dV kernel):  pe = exp2(s * sl - l2),  ds = pe * (dp - d).  The same on
// PAIRS (measured and removed) -- v_pk_fma_f32 for the argument, v_pk_mul_f32 + v_pk_fma_f32 for dS, 3.5 instead of 5 VALU instructions per score (and, tried with
// it, the same form in every other backward kernel and v_pk_fma_f32 / v_pk_add_f32 in the forward kernels' exp2 + row sum) -- measured SLOWER everywhere (same box,
// profiles/r06_attn_bwd_stream32.txt: N = 197 forward 68.7 -> 74.7 us, backward 212.9 -> 222.7; N = 1568 forward 477 -> 504, backward
// 1 218 -> 1 247): the packed fp32 operations do not issue at the rate of two scalar ones here, and assembling the pairs costs moves.
__device__ __forceinline__ void r16_pds4(const f32x4& s, const f32x4& dp, float sl, const f32x4& l2, const f32x4& d, f32x4& pe, f32x4& ds) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pe[e] = r16_p(s[e] * sl - l2[e]);
        ds[e] = pe[e] * (dp[e] - d[e]);
    }
}

// Backward, a wave of 16 queries against 32 keys (tiles 2 kk, 2 kk + 1 of Kb / Vb): S^T and dP^T, dS^T = P^T o (dP^T - delta),
// dQ^T (+)= K^T dS^T (`first`: dQ^T starts at zero).  lse2 = lse * log2(e), +inf on padded queries -> P = 0.  Valid rows keep their
// exact lse; a padded key (zero K row, s = 0) evaluates to exp2(-lse2), which overflows for a row whose scores are all very negative
// -- and it only ever multiplies zeros.  Every P is therefore taken through r16_p(): exp2 with the result clamped to [0, 1] (the output
// modifier of v_exp_f32, no extra instruction), exact for real entries (P <= 1 by construction of lse) and finite for padded ones
template <int HD>
__device__ __forceinline__ void r16_dq_step(const R16Frags<HD>& fr, const char* Kb, const char* Vb, int kk, const bf16x8 (&qf)[HD / 32],
                                            const bf16x8 (&dof)[HD / 32], float sl, float lse2, float del, f32x4 (&dq)[HD / 16], bool first) {
    constexpr int NKS = HD / 32, NDT = HD / 16;
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    bf16x8 ka[2][NKS], va[2][NKS];
    fr.rowread(Kb, 2 * kk, ka[0]); fr.rowread(Kb, 2 * kk + 1, ka[1]);
    fr.rowread(Vb, 2 * kk, va[0]); fr.rowread(Vb, 2 * kk + 1, va[1]);
    f32x4 s[2], dp[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) { s[tt] = mma16(ka[tt][0], qf[0], zero4f); dp[tt] = mma16(va[tt][0], dof[0], zero4f); }
#pragma unroll
    for (int ks = 1; ks < NKS; ++ks)
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) { s[tt] = mma16(ka[tt][ks], qf[ks], s[tt]); dp[tt] = mma16(va[tt][ks], dof[ks], dp[tt]); }
    bf16x8 kt[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) kt[dt] = fr.trread(Kb, kk, dt);
    // keys >= N: their K rows are zeros, so whatever dS holds there adds nothing to dQ -- no mask
    bf16x8 dsb;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pe = r16_p(s[tt][e] * sl - lse2);
            dsb[4 * tt + e] = (bf16_t)(pe * (dp[tt][e] - del));      // dS^T / scale (scale applied to dQ once)
        }
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dq[dt] = mma16(kt[dt], dsb, first ? zero4f : dq[dt]);
}
// Backward, a wave of 16 keys (rows kf / vf) against 32 queries (tiles 2 qq, 2 qq + 1 of Qb / Db, their statistics at lsb / deb):
// S and dP, dV^T (+)= dO^T P, dK^T (+)= Q^T dS.  L2E: lsb holds lse as stored and is multiplied by log2(e) here; otherwise it holds
// the product already
template <int HD, bool L2E>
__device__ __forceinline__ void r16_dkdv_step(const R16Frags<HD>& fr, const char* Qb, const char* Db, const float* lsb, const float* deb,
                                              int qq, int g, const bf16x8 (&kf)[HD / 32], const bf16x8 (&vf)[HD / 32], float sl,
                                              f32x4 (&dk)[HD / 16], f32x4 (&dv)[HD / 16], bool first) {
    constexpr int NKS = HD / 32, NDT = HD / 16;
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    f32x4 s[2], dp[2];
    {
        bf16x8 qa[2][NKS];
        fr.rowread(Qb, 2 * qq, qa[0]); fr.rowread(Qb, 2 * qq + 1, qa[1]);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) s[tt] = mma16(qa[tt][0], kf[0], zero4f);
#pragma unroll
        for (int ks = 1; ks < NKS; ++ks)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) s[tt] = mma16(qa[tt][ks], kf[ks], s[tt]);
    }
    {
        bf16x8 da[2][NKS];
        fr.rowread(Db, 2 * qq, da[0]); fr.rowread(Db, 2 * qq + 1, da[1]);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) dp[tt] = mma16(da[tt][0], vf[0], zero4f);
#pragma unroll
        for (int ks = 1; ks < NKS; ++ks)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) dp[tt] = mma16(da[tt][ks], vf[ks], dp[tt]);
    }
    bf16x8 pb, dsb;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const f32x4 L = *reinterpret_cast<const f32x4*>(lsb + 16 * (2 * qq + tt) + 4 * g);
        const f32x4 D = *reinterpret_cast<const f32x4*>(deb + 16 * (2 * qq + tt) + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float pe = r16_p(s[tt][e] * sl - (L2E ? L[e] * LOG2E : L[e]));
            pb[4 * tt + e] = (bf16_t)pe;
            dsb[4 * tt + e] = (bf16_t)(pe * (dp[tt][e] - D[e]));      // dS / scale (scale applied to dK once)
        }
    }
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dv[dt] = mma16(fr.trread(Db, qq, dt), pb, first ? zero4f : dv[dt]);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) dk[dt] = mma16(fr.trread(Qb, qq, dt), dsb, first ? zero4f : dk[dt]);
}

// 16 accumulator rows (lane (row l & 15, g = l >> 4) holds d = 16 dt + 4 g + j), times `mul` -> bf16 rows of `grow0`, transposed through the
// wave's LDS scratch into whole 128-byte row stores.  The stores are BUFFER stores behind a descriptor that ends with the last
// valid row (rows past it and chunks past hd are dropped by the bounds check, never branched over): the number of memory
// operations is fixed, so a later wait for loads issued BEFORE these stores can be a counted vmcnt instead of vmcnt(0).
template <int HD>
__device__ __forceinline__ void r16_store_rows(char* scr, const f32x4 (&acc)[HD / 16], float mul, bf16_t* __restrict__ grow0,
                                               int64_t ldg, int rows_valid, int hd, int lane) {
    typedef Cfg<bf16_t, HD> C;
    const int l15 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt) {
        bf16x4 v4;
#pragma unroll
        for (int e = 0; e < 4; ++e) v4[e] = (bf16_t)(acc[dt][e] * mul);
        *reinterpret_cast<bf16x4*>(scr + l15 * C::RROW + (16 * dt + 4 * g) * 2) = v4;
    }
    __builtin_amdgcn_wave_barrier();
    constexpr int RPI = 64 / C::CPR;              // rows per store instruction
    const int chunk = lane % C::CPR, r0 = lane / C::CPR;
    const int nrec = rows_valid > 0 ? (int)(((int64_t)(rows_valid - 1) * ldg + hd) * 2) : 0;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(grow0, 0, nrec, 0x00020000);
#pragma unroll
    for (int k = 0; k < 16 / RPI; ++k) {
        const int r = r0 + RPI * k;
        const u32x4 v = *reinterpret_cast<const u32x4*>(scr + r * C::RROW + chunk * 16);
        const int off = chunk * 8 < hd ? (int)(r * ldg * 2) + chunk * 16 : 0x7f000000;
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, ME_POL_ATTN_ST);
    }
    __builtin_amdgcn_wave_barrier();
}

// A loader lane's source addressing for the LDS-DMA of an array with row stride ld: lane l fills LDS bytes [16 l, 16 l + 16) of an
// instruction's 1 KiB = slot `pos` of row `rg` of the row group, with the chunk that belongs there (the swizzle is applied on the
// SOURCE side).  voff: the lane's byte offset in piece 0, gstep: bytes from one piece to the next, rec: the descriptor's size --
// rows >= N and chunks >= hd (voff out of any range) are outside it and arrive as zeros
template <int HD>
__device__ __forceinline__ void r16_dma_lane(int lane, int64_t ld, int N, int hd, int& voff, int& gstep, int& rec) {
    typedef RCfg<HD> R;
    const int rg = (lane * 16) / R::RB, pos = ((lane * 16) % R::RB) / 16;
    const int csrc = pos ^ r16_swz<R::CPR>(rg);
    voff = (csrc * 8 < hd) ? rg * (int)ld * 2 + csrc * 16 : 0x7f000000;
    gstep = R::RPI * (int)ld * 2;
    rec = (int)(((int64_t)(N - 1) * ld + hd) * 2);
}

// The items of a workgroup of the streaming kernels: vid, vid + G, ... with an XCD-major virtual id -- the workgroups of one XCD
// (blockIdx & 7) take consecutive items = neighbouring row blocks of a head, so a head's streamed side comes out of HBM once
__device__ __forceinline__ int st16_vid(int G) {
    return (G & 7) == 0 ? ((int)blockIdx.x & 7) * (G >> 3) + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
}
__device__ __forceinline__ int st16_my_items(int vid, int items, int G) { return vid < items ? (items - vid + G - 1) / G : 0; }

// Loader waves of the streaming kernels: array 0 / 1 of a chunk from (a0, ld0) / (a1, ld1); FL: 128 floats of f0 / f1 per chunk.
// They keep a three-slot LDS ring of chunks two chunks ahead of the compute waves; chunk j of the workgroup's stream = chunk j % NCH
// of its (j / NCH)-th item.  NW waves per workgroup, the last NL of them load (the others past the compute waves keep the barrier
// count): NL = 4 (two waves per array -- an LDS-DMA piece costs its issuer 60-180 clocks, and 16 of them per 128-row chunk is about
// what the compute waves of a short row block need for the chunk), 2 (one per array) or 1 (one wave fills both arrays -- the 8-wave
// kernel with seven compute waves).
template <int HD, bool FL, int NW>
__device__ __forceinline__ void st16_loader(char* smem, char* fring, int wave, int lane, int NL, int total, int NCH, int vid, int G,
                                            int nblk, int H, int N, int hd, const bf16_t* a0, int64_t ld0, int64_t hoff0,
                                            const bf16_t* a1, int64_t ld1, int64_t hoff1, const float* f0, const float* f1) {
    typedef RCfg<HD> R;
    constexpr int arr_bytes = ST_KC * R::RB;
    constexpr int slot_bytes = 2 * arr_bytes;
    constexpr int NPC = ST_KC / R::RPI;
    static_assert(2 * NPC + 4 <= 63, "vmcnt range");
    if (wave < NW - NL) {                             // spare waves: the barrier count only
        for (int k = 0; k < total; ++k) __builtin_amdgcn_s_barrier();
        return;
    }
    const int lw = wave - (NW - NL);
    const int which0 = NL == 1 ? 0 : (lw & 1), nwhich = NL == 1 ? 2 : 1;
    const int part = lw >> 1, nparts = NL == 4 ? 2 : 1;
    auto fill = [&](int j) {
        if (j >= total) return;
        const int it = vid + (j / NCH) * G, c = j % NCH;
        const int bh = it / nblk;
        for (int w = 0; w < nwhich; ++w) {
            const int which = which0 + w;
            const bf16_t* const arr = which ? a1 : a0;
            const int64_t ldw = which ? ld1 : ld0, hoff = which ? hoff1 : hoff0;
            int dma_voff, dma_gstep, rec_bytes;
            r16_dma_lane<HD>(lane, ldw, N, hd, dma_voff, dma_gstep, rec_bytes);
            const bf16_t* base = arr + (int64_t)(bh / H) * N * ldw + (bh % H) * hd + hoff;
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(base), 0, rec_bytes, 0x00020000);
            char* dst = smem + (j % ST_RING) * slot_bytes + which * arr_bytes;
            const int voff = dma_voff + c * NPC * dma_gstep;
            if (nparts == 1) {
#pragma unroll
                for (int i = 0; i < NPC; ++i)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_dma_t*)(dst + i * 1024), 16, voff + i * dma_gstep, 0, 0, 0);
            } else {
#pragma unroll
                for (int i = 0; i < NPC / 2; ++i) {
                    const int p = 2 * i + part;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_dma_t*)(dst + p * 1024), 16, voff + p * dma_gstep, 0, 0, 0);
                }
            }
            if (FL) {
                // 128 floats of this array's statistics: two dword pieces of 64 (one each when two loaders share the array)
                const float* const farr = which ? f1 : f0;
                const __amdgpu_buffer_rsrc_t rf =
                    __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(farr + (int64_t)bh * N), 0, N * 4, 0x00020000);
                char* fdst = fring + ((j % ST_RING) * 2 + which) * (ST_KC * 4);
                const int fvoff = (c * ST_KC + lane) * 4;
                if (nparts == 1) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rf, (lds_dma_t*)fdst, 4, fvoff, 0, 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rf, (lds_dma_t*)(fdst + 256), 4, fvoff + 256, 0, 0, 0);
                } else {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rf, (lds_dma_t*)(fdst + 256 * part), 4, fvoff + 256 * part, 0, 0, 0);
                }
            }
        }
    };
    fill(0);
    fill(1);
    for (int k = 0; k < total; ++k) {
        // chunk k has landed once at most chunk k + 1's pieces (of this loader) are outstanding (in-order retirement)
        if (k + 1 >= total) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (NL == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPC + (FL ? 4 : 0)) : "memory");
        else if (NL == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPC + (FL ? 2 : 0)) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPC / 2 + (FL ? 1 : 0)) : "memory");
        __builtin_amdgcn_s_barrier();                 // chunk k ready; everybody is done with chunk k - 1
        fill(k + 2);                                  // ... whose slot takes chunk k + 2
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int HD, int NS>
__global__ __launch_bounds__(R16_THREADS) void attn_fwd_ring16_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                      bf16_t* __restrict__ out, int64_t ldo,
                                                                      float* __restrict__ lse, int N, int H, int hd,
                                                                      float scale, int items) {
    typedef Cfg<bf16_t, HD> C;
    typedef RCfg<HD> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NR = NS * 32;
    constexpr int arr_bytes = NR * R::RB;             // one array (K or V) of one item
    constexpr int NRI = NR / R::RPI;                  // DMA instructions per array
    constexpr int NT = 2 * NS;                        // 16-key tiles
    constexpr int NKS = HD / 32;                      // 32-wide d steps of QK^T
    constexpr int NDT = HD / 16;                      // 16-wide d tiles of O^T
    constexpr int SCR = 16 * C::RROW;                 // per-wave output transposition scratch
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int Cdim = H * hd;
    const int G = (int)gridDim.x;
    const bool active = 16 * wave < N;                // wave-uniform

    if (!active) {
        if (wave < 14) {                              // spare waves: the barrier count only
            __syncthreads();
            for (int it = blockIdx.x; it < items; it += G) __syncthreads();
            return;
        }
        // ---- the two loader waves (14: K, 15: V)
        int dma_voff, dma_gstep, rec_bytes;
        r16_dma_lane<HD>(lane, ld, N, hd, dma_voff, dma_gstep, rec_bytes);
        // PACED in the steady state (one piece per ~150 clocks and loader): asked for all at once, an item's 56 KiB backs up the
        // CU's vector-memory path and the compute waves' own loads and stores queue behind it
        const int which = wave - 14;                  // 0: K, 1: V
        auto fill = [&](int it, char* half, bool paced) {
            const bf16_t* base = qkv + (int64_t)(it / H) * N * ld + (it % H) * hd + (1 + which) * Cdim;
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(base), 0, rec_bytes, 0x00020000);
#pragma unroll
            for (int i = 0; i < NRI; ++i) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_dma_t*)(half + which * arr_bytes + i * 1024), 16, dma_voff + i * dma_gstep, 0, 0, 0);
                if (paced && R16_SLEEP) __builtin_amdgcn_s_sleep(R16_SLEEP);
            }
        };
        int it = blockIdx.x, cur = 0;
        fill(it, smem, false);
        __syncthreads();
        for (; it < items; it += G) {
            if (it + G < items) fill(it + G, smem + (cur ^ 1) * 2 * arr_bytes, true);
            __syncthreads();                          // (vmcnt(0) first: the fill has landed)
            cur ^= 1;
        }
        return;
    }

    // ---- compute waves
    char* scr = smem + 4 * arr_bytes + wave * SCR;
    const int q = 16 * wave + l15;
    const int qrow = (q < N) ? q : N - 1;
    const float sl = scale * LOG2E;
    const R16Frags<HD> fr(l15, g);

    bf16x8 qf[NKS];
    u32x4 qn[NKS];
    auto q_issue = [&](int it) {
        const bf16_t* qptr = qkv + (int64_t)(it / H) * N * ld + (it % H) * hd;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int d = 32 * ks + 8 * g;
            qn[ks] = *reinterpret_cast<const u32x4*>(qptr + (int64_t)qrow * ld + (d < hd ? d : 0));
        }
    };

    f32x4 o[NDT];
    float m2 = 0.f, l_tot = 1.f;
    int it_out = -1;
    auto flush = [&]() {
        const float inv = __builtin_amdgcn_rcpf(l_tot);      // (1 ulp; the result is rounded to bf16)
        const int b = it_out / H, head = it_out % H;
        r16_store_rows<HD>(scr, o, inv, out + ((int64_t)b * N + 16 * wave) * ldo + head * hd, ldo, N - 16 * wave, hd, lane);
        if (lse && g == 0 && q < N) lse[((int64_t)b * H + head) * N + q] = (m2 + __builtin_amdgcn_logf(l_tot)) * LN2;
    };

    int it = blockIdx.x;
    q_issue(it);
    int cur = 0;
    __syncthreads();
    for (; it < items; it += G) {
        const int nxt = (it + G < items) ? it + G : it;
        TRACE_STAMP(it, 0);
        r16_take<HD>(qn, g, hd, qf);
        const char* Kb = smem + cur * 2 * arr_bytes;
        const char* Vb = Kb + arr_bytes;
        // ---- pass 1: S^T of the whole row block
        f32x4 s[NT];
        r16_st_pass<HD, NT>(fr, Kb, qf, s, it);
        TRACE_STAMP(it, 3);
        q_issue(nxt);                                 // (here, not at the head of the item: the memory path is quiet now)
        // ---- softmax over the whole row (registers only); keys >= N sit in the last two tiles
        if (N & 31) {
            int nkeys = N - 4 * g;                    // (opaque per item: hipcc would hoist the lane masks into SGPRs)
            asm volatile("" : "+v"(nkeys));
#pragma unroll
            for (int t = NT - 2; t < NT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[t][e] = (16 * t + e < nkeys) ? s[t][e] : -INFINITY;
        }
        float mt = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) mt = fmaxf(mt, s[t][e]);
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        m2 = mt * sl;
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pe = __builtin_amdgcn_exp2f(s[t][e] * sl - m2);
                s[t][e] = pe;
                ps += pe;
            }
        ps += __shfl_xor(ps, 16, 64);
        l_tot = ps + __shfl_xor(ps, 32, 64);
        TRACE_STAMP(it, 4);
        // ---- pass 2: O^T = V^T P^T
        r16_pv_pass<HD, NS>(fr, Vb, s, o, true);
        it_out = it;
        TRACE_STAMP(it, 5);
        flush();
        TRACE_STAMP(it, 2);
        __syncthreads();      // the loader's fill of the other half has landed and every wave is done with `cur`
        TRACE_STAMP(it, 6);
        cur ^= 1;
    }
}

// One workgroup per (batch, head); LDS holds {Q, K, V, dO} (4 x 32 KB at N = 197).  Once every wave has lifted its K/V row
// fragments for phase B the K/V tiles are dead, and wave w reuses rows [32w, 32w+32) of them as its private scratch for
// the coalesced row stores of dQ, dK and dV.
template <int HD>
__global__ __launch_bounds__(SM_THREADS) void attn_bwd_small_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                    const bf16_t* __restrict__ out, int64_t ldo,
                                                                    const bf16_t* __restrict__ dout, int64_t lddo,
                                                                    const float* __restrict__ lse,
                                                                    float* __restrict__ delta,
                                                                    bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H,
                                                                    int hd, float scale) {
    typedef Cfg<bf16_t, HD> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NS = (N + 31) >> 5, NR = NS * 32;
    char* Qs = smem;
    char* Ks = Qs + NR * C::RROW;
    char* Vs = Ks + NR * C::RROW;
    char* dOs = Vs + NR * C::RROW;
    float* lse_s = reinterpret_cast<float*>(dOs + NR * C::RROW);   // [SM_MAXN]  lse * log2(e), +inf on padded rows
    float* del_s = lse_s + SM_MAXN;                                // [SM_MAXN]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Cdim = H * hd;
    const bf16_t* qptr = qkv + (int64_t)b * N * ld + head * hd;
    const bf16_t* doptr = dout + (int64_t)b * N * lddo + head * hd;
    const int64_t bh = ((int64_t)b * H + head) * N;
    const int row = 32 * wave + l31;        // the query (phase A) / key (phase B) this lane owns
    const bool row_ok = row < N;
    const int rowc = row_ok ? row : N - 1;
    const bool active = 32 * wave < N;      // wave-uniform
    const float sl = scale * LOG2E;

    const int trace_slot = blockIdx.y * gridDim.x + blockIdx.x;
    (void)trace_slot;
    TRACE_STAMP(trace_slot, 0);
    Rows32Stage<HD, 4> st;
    {
        const bf16_t* const bases[4] = {qptr, qptr + Cdim, qptr + 2 * Cdim, doptr};
        const int64_t ldv[4] = {ld, ld, ld, lddo};
        st.load(bases, ldv, N, hd, tid);
    }
    u32x4 of[C::NKK];      // O row fragments for delta: the same d-slices as the dO operand fragments
    {
        const bf16_t* optr = out + ((int64_t)b * N + rowc) * ldo + head * hd;
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            const int d = (2 * kk + h) * 8;
            const bool ok = d < hd;
            of[kk] = *reinterpret_cast<const u32x4*>(optr + (ok ? d : 0));
            of[kk] = ok ? of[kk] : zero4();
        }
    }
    const float lse_mine = (tid < N && tid < SM_MAXN) ? lse[bh + tid] * LOG2E : INFINITY;
    {
        char* const tiles[4] = {Qs, Ks, Vs, dOs};
        st.store(tiles, NR, tid, N, hd);
    }
    if (tid < SM_MAXN) lse_s[tid] = lse_mine;
    __syncthreads();
    TRACE_STAMP(trace_slot, 1);

    // ---- phase A: delta and dQ for the 32 queries of this wave
    f32x16 dq[C::NDB];
    if (active) {
        bf16x8 qf[C::NKK], dof[C::NKK];
        float del = 0.f;
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            qf[kk] = rtile_chunk<bf16_t, HD>(Qs, row, 2 * kk + h);
            dof[kk] = rtile_chunk<bf16_t, HD>(dOs, row, 2 * kk + h);
            del = bf16x8_dot_acc(del, of[kk], *reinterpret_cast<const u32x4*>(&dof[kk]));
        }
        del += __shfl_xor(del, 32, 64);
        if (h == 0) {
            del_s[row] = del;
            if (row_ok && delta) delta[bh + row] = del;
        }
        const float lse2 = lse_s[row];      // +inf on padded queries -> P = 0
        acc_zero(dq);
        rows32_dq_walk<HD>(Ks, Vs, 0, N, N, qf, dof, sl, lse2, del, dq, lane);
    }
    TRACE_STAMP(trace_slot, 2);
    __syncthreads();      // del_s complete; every phase-A loop over the K/V tiles is finished
    if (!active) {
        __syncthreads();
        return;
    }
    bf16x8 kf[C::NKK], vf[C::NKK];
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk) {
        kf[kk] = rtile_chunk<bf16_t, HD>(Ks, row, 2 * kk + h);
        vf[kk] = rtile_chunk<bf16_t, HD>(Vs, row, 2 * kk + h);
    }
    __syncthreads();      // K/V tiles are dead: rows [32 wave, +32) of each are this wave's scratch from here on
    TRACE_STAMP(trace_slot, 3);
    char* scr0 = Ks + 32 * wave * C::RROW;
    char* scr1 = Vs + 32 * wave * C::RROW;
    bf16_t* grow0 = dqkv + ((int64_t)b * N + 32 * wave) * lddq + head * hd;
    store_rows_via_lds<HD>(scr0, dq, scale, grow0, lddq, N - 32 * wave, hd, lane);

    TRACE_STAMP(trace_slot, 4);
    // ---- phase B: dK and dV for the 32 keys of this wave
    f32x16 dk[C::NDB], dv[C::NDB];
    acc_zero(dk);
    acc_zero(dv);
    rows32_dkdv_walk<HD>(Qs, dOs, lse_s, del_s, NS, kf, vf, sl, dk, dv, lane);
    TRACE_STAMP(trace_slot, 5);
    store_rows_via_lds<HD>(scr0, dk, scale, grow0 + Cdim, lddq, N - 32 * wave, hd, lane);
    store_rows_via_lds<HD>(scr1, dv, 1.0f, grow0 + 2 * Cdim, lddq, N - 32 * wave, hd, lane);
    TRACE_STAMP(trace_slot, 6);
}

// -----------------------------------------------------------------------------------------------------
// Long sequences (N > SM_MAXN), forward: the ring form with K / V STREAMED.  A workgroup (16 waves: up to 14 compute waves of 16
// queries + the two loader waves) owns a block of queries of one (batch, head) and walks the keys in chunks of 128; the loaders
// keep a three-slot LDS ring of {K, V} chunks two chunks ahead of the compute waves (one barrier per chunk: "chunk k has landed
// and everybody is done with chunk k - 1", whose slot the loaders then refill with chunk k + 2).  Online softmax per chunk (the
// row block no longer fits in registers); the same 16 x 16 x 32 products, operand swizzle and hand pipelining as the ring form.
// Replaces the one-workgroup-per-(batch, head) "mid" kernel and the 256-row "chunk" kernel in the forward: those ran 8 waves of
// 32 rows (two per SIMD) with register-staged loads.  Workgroups of one XCD take neighbouring query blocks of the same heads,
// so a head's K / V comes out of HBM once and is re-read from that XCD's L2.
// (Measured and dropped: 64-key chunks with the NEXT chunk's QK^T MFMAs issued ahead of this chunk's softmax arithmetic in every
// wave -- 511 us against 444 at N = 1568: twice the barriers, and the chunk barrier keeps all waves of a SIMD in the same phase;
// skipping the 64-key groups of the last chunk that lie past N with wave-uniform branches -- slower, 502 against 472 us: the joins
// cost the straight-line schedule more than the skipped MFMAs save.)
template <int HD>
__global__ __launch_bounds__(R16_THREADS) void attn_fwd_stream16_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                        bf16_t* __restrict__ out, int64_t ldo,
                                                                        float* __restrict__ lse, int N, int H, int hd, float scale,
                                                                        int QB, int nqb, int items) {
    typedef Cfg<bf16_t, HD> C;
    typedef RCfg<HD> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int arr_bytes = ST_KC * R::RB;          // one array (K or V) of one chunk
    constexpr int slot_bytes = 2 * arr_bytes;
    constexpr int NTC = ST_KC / 16;                   // 16-key tiles per chunk
    constexpr int NKS = HD / 32, NDT = HD / 16;
    constexpr int SCR = 16 * C::RROW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int Cdim = H * hd;
    const int G = (int)gridDim.x;
    const int NCH = (N + ST_KC - 1) / ST_KC;
    const int vid = st16_vid(G);
    const int my_items = st16_my_items(vid, items, G);
    if (16 * wave >= QB) {
        // ---- loader waves: the last two (QB = 224) or four (fewer compute waves) waves
        st16_loader<HD, false, 16>(smem, nullptr, wave, lane, QB <= 12 * 16 ? 4 : 2, my_items * NCH, NCH, vid, G, nqb, H, N, hd, qkv, ld, Cdim, qkv, ld,
                                   2 * Cdim, nullptr, nullptr);
        return;
    }

    // ---- compute waves
    char* scr = smem + ST_RING * slot_bytes + wave * SCR;
    const float sl = scale * LOG2E;
    const R16Frags<HD> fr(l15, g);
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    // the wave's own query rows: item ii + 1's are fetched under item ii's last chunk
    u32x4 qn[NKS];
    auto q_issue = [&](int it) {
        const int bh = it / nqb, qb = it % nqb;
        const int q = qb * QB + 16 * wave + l15;
        const bf16_t* qptr = qkv + ((int64_t)(bh / H) * N + (q < N ? q : N - 1)) * ld + (bh % H) * hd;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int d = 32 * ks + 8 * g;
            qn[ks] = *reinterpret_cast<const u32x4*>(qptr + (d < hd ? d : 0));
        }
    };
    if (my_items > 0) q_issue(vid);
    int j = 0;                                        // chunk index in the workgroup's stream
    for (int ii = 0; ii < my_items; ++ii) {
        const int it = vid + ii * G;
        const int bh = it / nqb, qb = it % nqb;
        const int b = bh / H, head = bh % H;
        const int q0 = qb * QB + 16 * wave;           // first query of this wave
        const int q = q0 + l15;
        bf16x8 qf[NKS];
        r16_take<HD>(qn, g, hd, qf);
        f32x4 o[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[dt] = zero4f;
        float m_run = -INFINITY, l_run = 0.f;         // l_run: this lane's own keys only (summed over the four key groups at the end)
        for (int c = 0; c < NCH; ++c, ++j) {
            __syncthreads();                          // chunk j has landed (the loaders waited for it); see the loader loop
            if (c == NCH - 1) q_issue(ii + 1 < my_items ? it + G : it);
            const char* Kb = smem + (j % ST_RING) * slot_bytes;
            const char* Vb = Kb + arr_bytes;
            const int nkeys = N - c * ST_KC;          // valid keys of this chunk (>= 1); wave-uniform
            // ---- S^T for the chunk's 16-key tiles
            f32x4 s[NTC];
            r16_st_pass<HD, NTC>(fr, Kb, qf, s, -1);
            // ---- online softmax
            if (nkeys < ST_KC) {
                int nk = nkeys - 4 * g;               // (opaque: hipcc would hoist the lane masks out of the loops into SGPRs)
                asm volatile("" : "+v"(nk));
#pragma unroll
                for (int t = 0; t < NTC; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[t][e] = (16 * t + e < nk) ? s[t][e] : -INFINITY;
            }
            float mt = -INFINITY;
#pragma unroll
            for (int t = 0; t < NTC; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) mt = fmaxf(mt, s[t][e]);
            mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float m_new = fmaxf(m_run, mt * sl);     // every chunk holds a valid key: finite from the first chunk on
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            float ps = 0.f;
#pragma unroll
            for (int t = 0; t < NTC; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pe = __builtin_amdgcn_exp2f(s[t][e] * sl - m_new);
                    s[t][e] = pe;
                    ps += pe;
                }
            l_run = l_run * alpha + ps;
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;
            // ---- O^T += V^T P^T
            r16_pv_pass<HD, ST_KC / 32>(fr, Vb, s, o, false);
        }
        // ---- finish the item: row sums over the four key groups, normalise, store
        l_run += __shfl_xor(l_run, 16, 64);
        l_run += __shfl_xor(l_run, 32, 64);
        const float inv = __builtin_amdgcn_rcpf(l_run);
        r16_store_rows<HD>(scr, o, inv, out + ((int64_t)b * N + q0) * ldo + head * hd, ldo, N - q0, hd, lane);
        if (lse && g == 0 && q < N) lse[((int64_t)b * H + head) * N + q] = (m_run + __builtin_amdgcn_logf(l_run)) * LN2;
    }
}

// -----------------------------------------------------------------------------------------------------
// Backward in the ring form (SM_MINN < N <= RS_MAXN), 16 waves, 16 rows per wave (see attn_fwd_ring16_kernel for why).
// LDS holds two 2-array regions, KV = {K, V} and QD = {Q, dO}, unpadded and swizzled (r16_swz).  Per item:
//   phase A (wave = 16 queries):  S^T, dP^T from the KV region + the wave's own Q / dO rows (registers, prefetched from global),
//                                 dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T;  delta = rowsum(dO o O) on the way in;
//                                 at the end the wave lifts its own 16 K / V rows (phase B's register operands)       -- barrier 1
//   phase B (wave = 16 keys):     S, dP from the QD region + those rows, dV^T += dO^T P, dK^T += Q^T dS                  -- barrier 2
// The KV region is dead during phase B and the QD region during phase A: the two loader waves (14: K then Q, 15: V then dO)
// refill each region by LDS-DMA while the OTHER phase computes -- the whole item's 100 KB arrives under compute, which the
// one-workgroup-per-item kernel above exposes completely (13 k of 40 k clocks per item).  S and dP are computed twice (7 MFMA
// products instead of 5) so that no gradient needs a cross-wave reduction; results are deterministic.
template <int HD, int NS>
__global__ __launch_bounds__(R16_THREADS) void attn_bwd_ring16_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                      const bf16_t* __restrict__ out, int64_t ldo,
                                                                      const bf16_t* __restrict__ dout, int64_t lddo,
                                                                      const float* __restrict__ lse, float* __restrict__ delta,
                                                                      bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H, int hd,
                                                                      float scale, int items, unsigned* __restrict__ ctr) {
    typedef Cfg<bf16_t, HD> C;
    typedef RCfg<HD> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NR = NS * 32;
    constexpr int arr_bytes = NR * R::RB;
    constexpr int NRI = NR / R::RPI;
    constexpr int NKS = HD / 32;
    constexpr int NDT = HD / 16;
    constexpr int SCR = 16 * C::RROW;
    char* const KVr = smem;                           // {K, V}
    char* const QDr = smem + 2 * arr_bytes;           // {Q, dO}
    float* const lse_s = reinterpret_cast<float*>(smem + 4 * arr_bytes);      // [NR] lse * log2(e), +inf on padded queries
    float* const del_s = lse_s + NR;                                          // [NR]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int Cdim = H * hd;
    const int G = (int)gridDim.x;
    const bool active = 16 * wave < N;                // wave-uniform
    // ---- items are CLAIMED (ctr != null; null under hipGraph capture = the static schedule it, it + G, ...): a workgroup's first item
    // is its block index, every further one a draw from a counter -- a workgroup that starts late, because its CU was held by a
    // communication kernel when this one was launched, then simply gets fewer items instead of making the whole launch wait for its
    // full static share (the resident GEMM does the same: gemm3.hip).  Wave 0 draws the next item's id during phase A and leaves it in
    // an LDS word ahead of barrier 1; everybody reads it behind that barrier.  Draws of one launch: (items - G) hits + one miss per
    // workgroup = items; whoever draws the last one zeroes the counter for the next launch on this stream.
    volatile int* const nextw = reinterpret_cast<volatile int*>(smem + 4 * arr_bytes + 2 * NR * (int)sizeof(float) + 16 * SCR);
    // The draw is issued at the head of phase A and its result picked up at the end of it (a returning atomic takes a couple of
    // microseconds; consumed where it is issued, wave 0 would sit on it and hold barrier 1 back -- measured +5 %): the atomic goes out
    // through inline asm with only lane 0 enabled, so that the compiler sees no pending result to wait for; the explicit vmcnt(0)
    // in draw_take() is the wait.
    auto draw_issue = [&]() -> unsigned {            // (wave 0 only)
        unsigned old = 0, one = 1;
        if (ctr) {
            unsigned long long saved;
            asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
                         : "=&v"(old), "=&s"(saved) : "v"(0u), "v"(one), "s"(ctr) : "memory");
        }
        return old;                                  // valid in lane 0 once the operation has retired
    };
    auto draw_take = [&](unsigned drawn, int it) {   // (wave 0 only)
        int nx = it + G;
        if (ctr) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(drawn) : : "memory");
            const unsigned t = __builtin_amdgcn_readfirstlane(drawn);
            if (t == (unsigned)(items > G ? items : G) - 1u && lane == 0) atomicExch(ctr, 0u);
            nx = G + (int)t;
        }
        if (lane == 0) *nextw = nx;
    };
    if (!active) {
        if (wave < 14) {                              // spare waves: the barrier count only
            __syncthreads();
            for (int it = blockIdx.x; it < items;) {
                __syncthreads();
                it = __builtin_amdgcn_readfirstlane(*nextw);
                __syncthreads();
            }
            return;
        }
        // ---- loader waves: 14 fills the first array of a region (K, Q), 15 the second (V, dO)
        const int which = wave - 14;
        int voff_a, gstep_a, rec_a, voff_d, gstep_d, rec_d;
        r16_dma_lane<HD>(lane, ld, N, hd, voff_a, gstep_a, rec_a);                        // rows of qkv
        r16_dma_lane<HD>(lane, which ? lddo : ld, N, hd, voff_d, gstep_d, rec_d);         // rows of the QD array of this loader
        auto fill = [&](const bf16_t* base, int rec, int voff, int gstep, char* dst, int paced) {
            const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(base), 0, rec, 0x00020000);
#pragma unroll
            for (int i = 0; i < NRI; ++i) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_dma_t*)(dst + i * 1024), 16, voff + i * gstep, 0, 0, 0);
                if (paced == 1) __builtin_amdgcn_s_sleep(1);
                if (paced == 2) __builtin_amdgcn_s_sleep(3);
            }
        };
        auto kv_base = [&](int it) { return qkv + (int64_t)(it / H) * N * ld + (it % H) * hd + (1 + which) * Cdim; };
        auto qd_base = [&](int it) {
            return which ? dout + (int64_t)(it / H) * N * lddo + (it % H) * hd : qkv + (int64_t)(it / H) * N * ld + (it % H) * hd;
        };
        int it = blockIdx.x;
        fill(kv_base(it), rec_a, voff_a, gstep_a, KVr + which * arr_bytes, 0);
        __syncthreads();
        while (it < items) {
            fill(qd_base(it), rec_d, voff_d, gstep_d, QDr + which * arr_bytes, 1);
            __syncthreads();                          // barrier 1 (vmcnt(0) first: the fill has landed)
            it = __builtin_amdgcn_readfirstlane(*nextw);      // the next item of this workgroup (>= items: none)
            if (it < items) fill(kv_base(it), rec_a, voff_a, gstep_a, KVr + which * arr_bytes, 2);
            __syncthreads();                          // barrier 2
        }
        return;
    }

    // ---- compute waves
    char* scr = smem + 4 * arr_bytes + 2 * NR * (int)sizeof(float) + wave * SCR;
    const int row = 16 * wave + l15;                  // the query (phase A) / key (phase B) of this lane
    const bool row_ok = row < N;
    const int rowc = row_ok ? row : N - 1;
    const float sl = scale * LOG2E;
    const R16Frags<HD> fr(l15, g);
    for (int i = tid; i < NR; i += 64 * ((N + 15) / 16)) { lse_s[i] = INFINITY; del_s[i] = 0.f; }      // rows no wave owns stay this way

    // own-row operands of the NEXT item's phase A, in flight across this item's phase B
    u32x4 qn[NKS], don[NKS], on[NKS];
    float lse_n = 0.f;
    // piece i of 3 NKS + 1: issued one per phase-B step -- asked for at once (13 waves x 7 loads on top of the loaders' DMA and the
    // dQ stores) the CU's vector-memory path backs up and every wave sits in the issue of its loads for thousands of clocks
    constexpr int NPF = 3 * NKS + 1;
    auto prefetch = [&](int it, int i) {
        const int b = it / H, head = it % H;
        const int ks = i % NKS, arr = i / NKS;
        const int d = 32 * ks + 8 * g, dc = d < hd ? d : 0;
        if (arr == 0) qn[ks] = *reinterpret_cast<const u32x4*>(qkv + ((int64_t)b * N + rowc) * ld + head * hd + dc);
        else if (arr == 1) don[ks] = *reinterpret_cast<const u32x4*>(dout + ((int64_t)b * N + rowc) * lddo + head * hd + dc);
        else if (arr == 2) on[ks] = *reinterpret_cast<const u32x4*>(out + ((int64_t)b * N + rowc) * ldo + head * hd + dc);
        else lse_n = lse[((int64_t)b * H + head) * N + rowc];
    };

    int it = blockIdx.x;
#pragma unroll
    for (int i = 0; i < NPF; ++i) prefetch(it, i);
    __syncthreads();
    while (it < items) {
        const int b = it / H, head = it % H;
        const int64_t bh = ((int64_t)b * H + head) * N;
        TRACE_STAMP(it, 0);
        unsigned drawn = 0;
        if (wave == 0) drawn = draw_issue();
        // ---- phase A: this wave's 16 queries.  Own rows: chunks past hd are zeros; delta from the O / dO fragments
        bf16x8 qf[NKS], dof[NKS];
        float del = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const bool ok = 32 * ks + 8 * g < hd;
            const u32x4 qv = ok ? qn[ks] : zero4(), dv4 = ok ? don[ks] : zero4(), ov = ok ? on[ks] : zero4();
            qf[ks] = *reinterpret_cast<const bf16x8*>(&qv);
            dof[ks] = *reinterpret_cast<const bf16x8*>(&dv4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                del += __uint_as_float(ov[e] << 16) * __uint_as_float(dv4[e] << 16) +
                       __uint_as_float(ov[e] & 0xffff0000u) * __uint_as_float(dv4[e] & 0xffff0000u);
        }
        del += __shfl_xor(del, 16, 64);
        del += __shfl_xor(del, 32, 64);
        const float lse2 = row_ok ? lse_n * LOG2E : INFINITY;      // +inf on padded queries -> P = 0 (see r16_dq_step)
        if (g == 0) {
            lse_s[row] = lse2;
            del_s[row] = del;
            if (row_ok && delta) delta[bh + row] = del;
        }
        TRACE_STAMP(it, 1);
        f32x4 dq[NDT];
#pragma unroll
        for (int kk = 0; kk < NS; ++kk) r16_dq_step<HD>(fr, KVr, KVr + arr_bytes, kk, qf, dof, sl, lse2, del, dq, kk == 0);
        // this wave's own K / V rows = phase B's register operands (the loaders overwrite the region behind barrier 1)
        bf16x8 kf[NKS], vf[NKS];
        fr.rowread(KVr, wave, kf);
        fr.rowread(KVr + arr_bytes, wave, vf);
        TRACE_STAMP(it, 2);
        if (wave == 0) draw_take(drawn, it);
        __syncthreads();      // barrier 1: KV region dead; {Q, dO} of this item landed; lse_s / del_s complete; next item's id published
        TRACE_STAMP(it, 3);
        const int nid = __builtin_amdgcn_readfirstlane(*nextw);      // (wave-uniform: keep the address arithmetic that follows scalar)
        const int nxt = nid < items ? nid : it;      // (own rows of the next item, or a harmless re-read of this one's)
        bf16_t* grow0 = dqkv + ((int64_t)b * N + 16 * wave) * lddq + head * hd;
        r16_store_rows<HD>(scr, dq, scale, grow0, lddq, N - 16 * wave, hd, lane);
        TRACE_STAMP(it, 4);
        // ---- phase B: this wave's 16 keys.  Padded keys need no mask: a key is a lane (column) here, whatever it accumulates
        // stays in its own dK / dV rows, which are never stored; padded queries have lse_s = +inf -> P = 0
        f32x4 dk[NDT], dv[NDT];
#pragma unroll
        for (int qq = 0; qq < NS; ++qq) {
#pragma unroll
            for (int i = qq * NPF / NS; i < (qq + 1) * NPF / NS; ++i) prefetch(nxt, i);
            r16_dkdv_step<HD, false>(fr, QDr, QDr + arr_bytes, lse_s, del_s, qq, g, kf, vf, sl, dk, dv, qq == 0);
        }
        TRACE_STAMP(it, 5);
        r16_store_rows<HD>(scr, dk, scale, grow0 + Cdim, lddq, N - 16 * wave, hd, lane);
        r16_store_rows<HD>(scr, dv, 1.0f, grow0 + 2 * Cdim, lddq, N - 16 * wave, hd, lane);
        TRACE_STAMP(it, 6);
        __syncthreads();      // barrier 2: QD region dead; {K, V} of the next item landed
        TRACE_STAMP(it, 7);
        it = nid;
    }
}

// -----------------------------------------------------------------------------------------------------
// Long sequences (N >= ST_BWD_MINN), backward: the two phases of the ring backward as two STREAMING kernels in the form of
// attn_fwd_stream16_kernel (16-row waves, three-slot LDS ring of 128-row chunks kept two chunks ahead by loader waves, one barrier
// per chunk, XCD-major items so that a head's streamed side comes out of HBM once):
//   attn_bwd_dq_stream16_kernel:    a workgroup owns <= 224 queries of a (batch, head) -- own Q / dO / O rows in registers, delta on the
//                                   way in (written out for the second kernel) -- and streams {K, V};       phase A of the ring form
//   attn_bwd_dkdv_stream16_kernel:  a workgroup owns <= 224 keys -- own K / V rows in registers -- and streams {Q, dO} together with the
//                                   chunk's lse / delta (dword LDS-DMA into a small float ring);               phase B of the ring form
// No masks: rows past N arrive as zeros from the bounds-checked DMA (K = V = 0 -> dS meets a zero K row; Q = dO = 0, lse = delta =
// 0 -> P = 1 meets a zero dO row and dS = 0), every P goes through r16_p() and stays finite, and rows a wave owns past N are
// never stored.  Replaces the 8-wave / 32-row chunk kernels (same box, profiles/r04_attn_bwd_stream16_vs_chunk.txt: N = 1568 1 442 vs
// 1 520 us, 1000: 657 vs 711, 592: 409 vs 477, 520: 634 vs 797; 3136: 2 672 vs 2 640).
// Round 6: where a key block fills seven 32-key waves the second phase runs as attn_bwd_dkdv_stream32_kernel (further down; -15 % on that phase).
constexpr int ST_BWD_MINN = 513;

template <int HD>
__global__ __launch_bounds__(R16_THREADS) void attn_bwd_dq_stream16_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                           const bf16_t* __restrict__ out, int64_t ldo,
                                                                           const bf16_t* __restrict__ dout, int64_t lddo,
                                                                           const float* __restrict__ lse, float* __restrict__ delta,
                                                                           bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H, int hd,
                                                                           float scale, int QB, int nqb, int items) {
    typedef Cfg<bf16_t, HD> C;
    typedef RCfg<HD> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int arr_bytes = ST_KC * R::RB;
    constexpr int slot_bytes = 2 * arr_bytes;
    constexpr int NKS = HD / 32, NDT = HD / 16;
    constexpr int SCR = 16 * C::RROW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int Cdim = H * hd;
    const int G = (int)gridDim.x;
    const int NCH = (N + ST_KC - 1) / ST_KC;
    const int vid = st16_vid(G);
    const int my_items = st16_my_items(vid, items, G);
    if (16 * wave >= QB) {
        st16_loader<HD, false, 16>(smem, nullptr, wave, lane, QB <= 12 * 16 ? 4 : 2, my_items * NCH, NCH, vid, G, nqb, H, N, hd, qkv, ld, Cdim, qkv, ld,
                                   2 * Cdim, nullptr, nullptr);
        return;
    }
    char* scr = smem + ST_RING * slot_bytes + wave * SCR;
    const float sl = scale * LOG2E;
    const R16Frags<HD> fr(l15, g);
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    // the wave's own rows (Q, dO, O, lse): the next item's are fetched under this item's last chunk
    u32x4 qn[NKS], don[NKS], on[NKS];
    float lse_n = 0.f;
    auto own_issue = [&](int it) {
        const int bh = it / nqb, qb = it % nqb;
        const int q = qb * QB + 16 * wave + l15;
        const int qc = q < N ? q : N - 1;
        const int b = bh / H, head = bh % H;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int d = 32 * ks + 8 * g, dc = d < hd ? d : 0;
            qn[ks] = *reinterpret_cast<const u32x4*>(qkv + ((int64_t)b * N + qc) * ld + head * hd + dc);
            don[ks] = *reinterpret_cast<const u32x4*>(dout + ((int64_t)b * N + qc) * lddo + head * hd + dc);
            on[ks] = *reinterpret_cast<const u32x4*>(out + ((int64_t)b * N + qc) * ldo + head * hd + dc);
        }
        lse_n = lse[(int64_t)bh * N + qc];
    };
    if (my_items > 0) own_issue(vid);
    int j = 0;
    for (int ii = 0; ii < my_items; ++ii) {
        const int it = vid + ii * G;
        const int bh = it / nqb, qb = it % nqb;
        const int b = bh / H, head = bh % H;
        const int q0 = qb * QB + 16 * wave;
        const int q = q0 + l15;
        const bool row_ok = q < N;
        bf16x8 qf[NKS], dof[NKS];
        float del = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const bool ok = 32 * ks + 8 * g < hd;
            const u32x4 qv = ok ? qn[ks] : zero4(), dv4 = ok ? don[ks] : zero4(), ov = ok ? on[ks] : zero4();
            qf[ks] = *reinterpret_cast<const bf16x8*>(&qv);
            dof[ks] = *reinterpret_cast<const bf16x8*>(&dv4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                del += __uint_as_float(ov[e] << 16) * __uint_as_float(dv4[e] << 16) +
                       __uint_as_float(ov[e] & 0xffff0000u) * __uint_as_float(dv4[e] & 0xffff0000u);
        }
        del += __shfl_xor(del, 16, 64);
        del += __shfl_xor(del, 32, 64);
        const float lse2 = row_ok ? lse_n * LOG2E : INFINITY;      // +inf on padded queries -> P = 0
        if (g == 0 && row_ok) delta[(int64_t)bh * N + q] = del;
        f32x4 dq[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) dq[dt] = zero4f;
        auto chunk = [&](int c) {
            const char* Kb = smem + (j % ST_RING) * slot_bytes;
            const char* Vb = Kb + arr_bytes;
#pragma unroll
            for (int kk = 0; kk < ST_KC / 32; ++kk) r16_dq_step<HD>(fr, Kb, Vb, kk, qf, dof, sl, lse2, del, dq, false);
        };
        for (int c = 0; c + 1 < NCH; ++c, ++j) {
            __syncthreads();                          // chunk j has landed (the loaders waited for it)
            chunk(c);
        }
        __syncthreads();
        own_issue(ii + 1 < my_items ? it + G : it);   // (the last chunk is peeled: the next item's rows are live only under it)
        chunk(NCH - 1);
        ++j;
        r16_store_rows<HD>(scr, dq, scale, dqkv + ((int64_t)b * N + q0) * lddq + head * hd, lddq, N - q0, hd, lane);
    }
}

template <int HD>
__global__ __launch_bounds__(R16_THREADS) void attn_bwd_dkdv_stream16_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                             const bf16_t* __restrict__ dout, int64_t lddo,
                                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                                             bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H, int hd,
                                                                             float scale, int KB, int nkb, int items) {
    typedef Cfg<bf16_t, HD> C;
    typedef RCfg<HD> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int arr_bytes = ST_KC * R::RB;
    constexpr int slot_bytes = 2 * arr_bytes;
    constexpr int NKS = HD / 32, NDT = HD / 16;
    constexpr int SCR = 16 * C::RROW;
    constexpr int FRING = ST_RING * 2 * ST_KC * 4;    // {lse, delta} of a chunk, per ring slot
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int Cdim = H * hd;
    const int G = (int)gridDim.x;
    const int NCH = (N + ST_KC - 1) / ST_KC;
    const int vid = st16_vid(G);
    const int my_items = st16_my_items(vid, items, G);
    char* const fring = smem + ST_RING * slot_bytes;
    if (16 * wave >= KB) {
        st16_loader<HD, true, 16>(smem, fring, wave, lane, KB <= 12 * 16 ? 4 : 2, my_items * NCH, NCH, vid, G, nkb, H, N, hd, qkv, ld, 0, dout, lddo, 0, lse,
                                  delta);
        return;
    }
    char* scr = fring + FRING + wave * SCR;
    const float sl = scale * LOG2E;
    const R16Frags<HD> fr(l15, g);
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    // the wave's own K / V rows: the next item's are fetched under this item's last chunk
    u32x4 kn[NKS], vn[NKS];
    auto own_issue = [&](int it) {
        const int bh = it / nkb, kb = it % nkb;
        const int k = kb * KB + 16 * wave + l15;
        const bf16_t* kptr = qkv + ((int64_t)(bh / H) * N + (k < N ? k : N - 1)) * ld + (bh % H) * hd + Cdim;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int d = 32 * ks + 8 * g, dc = d < hd ? d : 0;
            kn[ks] = *reinterpret_cast<const u32x4*>(kptr + dc);
            vn[ks] = *reinterpret_cast<const u32x4*>(kptr + Cdim + dc);
        }
    };
    if (my_items > 0) own_issue(vid);
    int j = 0;
    for (int ii = 0; ii < my_items; ++ii) {
        const int it = vid + ii * G;
        const int bh = it / nkb, kb = it % nkb;
        const int b = bh / H, head = bh % H;
        const int k0 = kb * KB + 16 * wave;
        bf16x8 kf[NKS], vf[NKS];
        r16_take<HD>(kn, g, hd, kf);
        r16_take<HD>(vn, g, hd, vf);
        f32x4 dk[NDT], dv[NDT];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) { dk[dt] = zero4f; dv[dt] = zero4f; }
        auto chunk = [&](int c) {
            const char* Qb = smem + (j % ST_RING) * slot_bytes;
            const char* Db = Qb + arr_bytes;
            const float* lsb = reinterpret_cast<const float*>(fring + (j % ST_RING) * 2 * (ST_KC * 4));
            const float* deb = lsb + ST_KC;
#pragma unroll
            for (int qq = 0; qq < ST_KC / 32; ++qq) r16_dkdv_step<HD, true>(fr, Qb, Db, lsb, deb, qq, g, kf, vf, sl, dk, dv, false);
        };
        for (int c = 0; c + 1 < NCH; ++c, ++j) {
            __syncthreads();
            chunk(c);
        }
        __syncthreads();
        own_issue(ii + 1 < my_items ? it + G : it);
        chunk(NCH - 1);
        ++j;
        bf16_t* grow0 = dqkv + ((int64_t)b * N + k0) * lddq + head * hd;
        r16_store_rows<HD>(scr, dk, scale, grow0 + Cdim, lddq, N - k0, hd, lane);
        r16_store_rows<HD>(scr, dv, 1.0f, grow0 + 2 * Cdim, lddq, N - k0, hd, lane);
    }
}

// -----------------------------------------------------------------------------------------------------
// The dK / dV kernel with 32 KEYS PER WAVE (round 6): 8 waves of up to 256 registers instead of 16 of 128 -- seven compute waves own 2 x 16
// keys each (224 keys per workgroup, as before), the eighth loads both arrays.  Every fragment a wave reads from the streamed {Q, dO} chunk
// (row form for S / dP, transposed form for the two gradient products) now feeds TWO 16-key tiles: half the LDS bytes per MFMA -- the
// 16-row kernel reads 16 KB per 20 MFMAs and keeps the LDS array busy 45 % of the time with the matrix pipe at 35 %
// (profiles/r04_attn_pmc_stream.txt) -- and twice the independent MFMA chains per wave, against half the waves issuing softmax arithmetic.
// Same box, profiles/r06_attn_bwd_stream32.txt: N = 1568 (config 5) 852 -> 763 us, 592 (config 4) 443 -> 411 us.  Taken when the key
// blocks fill seven waves (192 < keys per block <= 224); six compute waves on four SIMDs run as slowly as eight (N = 520: +12 %).
// The dQ kernel in the same form (8 waves: 575 vs 562 us at N = 1568; 12 waves of 137 registers, 320-query blocks: 547 vs 538 us; 12 waves with
// the steps staged like here: 573 vs 567 us) does
// not gain -- 12 MFMAs per 12 KB there, and it is not the LDS that paces it -- and stays on 16-row waves.
constexpr int ST32_THREADS = 512;

template <int HD>
__global__ __launch_bounds__(ST32_THREADS) void attn_bwd_dkdv_stream32_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                              const bf16_t* __restrict__ dout, int64_t lddo,
                                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                                              bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H, int hd,
                                                                              float scale, int KB, int nkb, int items) {
    typedef Cfg<bf16_t, HD> C;
    typedef RCfg<HD> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int arr_bytes = ST_KC * R::RB;
    constexpr int slot_bytes = 2 * arr_bytes;
    constexpr int NKS = HD / 32, NDT = HD / 16;
    constexpr int SCR = 16 * C::RROW;
    constexpr int FRING = ST_RING * 2 * ST_KC * 4;    // {lse, delta} of a chunk, per ring slot
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int Cdim = H * hd;
    const int G = (int)gridDim.x;
    const int NCH = (N + ST_KC - 1) / ST_KC;
    const int vid = st16_vid(G);
    const int my_items = st16_my_items(vid, items, G);
    char* const fring = smem + ST_RING * slot_bytes;
    const int ncw = KB >> 5;
    if (wave >= ncw) {
        st16_loader<HD, true, 8>(smem, fring, wave, lane, 8 - ncw >= 4 ? 4 : 8 - ncw >= 2 ? 2 : 1, my_items * NCH, NCH, vid, G, nkb, H, N, hd, qkv,
                                 ld, 0, dout, lddo, 0, lse, delta);
        return;
    }
    char* scr = fring + FRING + wave * SCR;
    const float sl = scale * LOG2E;
    const R16Frags<HD> fr(l15, g);
    const f32x4 zero4f = {0.f, 0.f, 0.f, 0.f};
    // the wave's own K / V rows (two 16-key tiles): the next item's are fetched under this item's last chunk
    u32x4 kn[2][NKS], vn[2][NKS];
    auto own_issue = [&](int it) {
        const int bh = it / nkb, kb = it % nkb;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int k = kb * KB + 32 * wave + 16 * r + l15;
            const bf16_t* kptr = qkv + ((int64_t)(bh / H) * N + (k < N ? k : N - 1)) * ld + (bh % H) * hd + Cdim;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int d = 32 * ks + 8 * g, dc = d < hd ? d : 0;
                kn[r][ks] = *reinterpret_cast<const u32x4*>(kptr + dc);
                vn[r][ks] = *reinterpret_cast<const u32x4*>(kptr + Cdim + dc);
            }
        }
    };
    if (my_items > 0) own_issue(vid);
    int j = 0;
    for (int ii = 0; ii < my_items; ++ii) {
        const int it = vid + ii * G;
        const int bh = it / nkb, kb = it % nkb;
        const int b = bh / H, head = bh % H;
        const int k0 = kb * KB + 32 * wave;
        bf16x8 kf[2][NKS], vf[2][NKS];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            r16_take<HD>(kn[r], g, hd, kf[r]);
            r16_take<HD>(vn[r], g, hd, vf[r]);
        }
        f32x4 dk[2][NDT], dv[2][NDT];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) { dk[r][dt] = zero4f; dv[r][dt] = zero4f; }
        // one chunk = four 32-query steps, software-pipelined in program order: the S / dP products of step qq + 1 are issued BEFORE the
        // softmax arithmetic of step qq (which then runs under them), the gradient products of step qq behind it
        auto chunk = [&](int c) {
            const char* Qb = smem + (j % ST_RING) * slot_bytes;
            const char* Db = Qb + arr_bytes;
            const float* lsb = reinterpret_cast<const float*>(fring + (j % ST_RING) * 2 * (ST_KC * 4));
            const float* deb = lsb + ST_KC;
            auto sdp = [&](int qq, f32x4 (&s)[2][2], f32x4 (&dp)[2][2]) {      // [query tile of the pair][key tile]
                {
                    bf16x8 qa[2][NKS];
                    fr.rowread(Qb, 2 * qq, qa[0]); fr.rowread(Qb, 2 * qq + 1, qa[1]);
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                        for (int r = 0; r < 2; ++r) s[tt][r] = mma16(qa[tt][0], kf[r][0], zero4f);
#pragma unroll
                    for (int ks = 1; ks < NKS; ++ks)
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                            for (int r = 0; r < 2; ++r) s[tt][r] = mma16(qa[tt][ks], kf[r][ks], s[tt][r]);
                }
                {
                    bf16x8 da[2][NKS];
                    fr.rowread(Db, 2 * qq, da[0]); fr.rowread(Db, 2 * qq + 1, da[1]);
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                        for (int r = 0; r < 2; ++r) dp[tt][r] = mma16(da[tt][0], vf[r][0], zero4f);
#pragma unroll
                    for (int ks = 1; ks < NKS; ++ks)
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                            for (int r = 0; r < 2; ++r) dp[tt][r] = mma16(da[tt][ks], vf[r][ks], dp[tt][r]);
                }
            };
            f32x4 s[2][2], dp[2][2];
            sdp(0, s, dp);
#pragma unroll
            for (int qq = 0; qq < ST_KC / 32; ++qq) {
                // stage order held by scheduling barriers (the compiler otherwise sinks the next step's products behind this step's and
                // waits on every transposed read pair in turn): next S / dP -> this step's transposed dO fragments + statistics ->
                // softmax arithmetic (under both) -> transposed Q fragments -> dV products (under which those land) -> dK products
                f32x4 s2[2][2], dp2[2][2];
                if (qq + 1 < ST_KC / 32) sdp(qq + 1, s2, dp2);
                __builtin_amdgcn_sched_barrier(0);
                bf16x8 td[NDT], tq[NDT];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) td[dt] = fr.trread(Db, qq, dt);
                f32x4 L[2], D[2];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    L[tt] = *reinterpret_cast<const f32x4*>(lsb + 16 * (2 * qq + tt) + 4 * g);
                    D[tt] = *reinterpret_cast<const f32x4*>(deb + 16 * (2 * qq + tt) + 4 * g);
                }
                __builtin_amdgcn_sched_barrier(0);
                bf16x8 pb[2], dsb[2];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const f32x4 L2 = L[tt] * LOG2E;
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        f32x4 pe, ds;
                        r16_pds4(s[tt][r], dp[tt][r], sl, L2, D[tt], pe, ds);      // dS / scale (scale applied to dK once)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { pb[r][4 * tt + e] = (bf16_t)pe[e]; dsb[r][4 * tt + e] = (bf16_t)ds[e]; }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) tq[dt] = fr.trread(Qb, qq, dt);      // (lands under the dV products)
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 2; ++r) dv[r][dt] = mma16(td[dt], pb[r], dv[r][dt]);
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                    for (int r = 0; r < 2; ++r) dk[r][dt] = mma16(tq[dt], dsb[r], dk[r][dt]);
                __builtin_amdgcn_sched_barrier(0);
                if (qq + 1 < ST_KC / 32) {
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                        for (int r = 0; r < 2; ++r) { s[tt][r] = s2[tt][r]; dp[tt][r] = dp2[tt][r]; }
                }
            }
        };
        for (int c = 0; c + 1 < NCH; ++c, ++j) {
            __syncthreads();
            chunk(c);
        }
        __syncthreads();
        own_issue(ii + 1 < my_items ? it + G : it);
        chunk(NCH - 1);
        ++j;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            bf16_t* grow0 = dqkv + ((int64_t)b * N + k0 + 16 * r) * lddq + head * hd;
            r16_store_rows<HD>(scr, dk[r], scale, grow0 + Cdim, lddq, N - k0 - 16 * r, hd, lane);
            r16_store_rows<HD>(scr, dv[r], 1.0f, grow0 + 2 * Cdim, lddq, N - k0 - 16 * r, hd, lane);
        }
    }
}

// =====================================================================================================
// mid-size sequences (256 < N <= 512: audio spectrogram tokens, 512 x 512 segmentation crops at /32, BASELINE config 3).
// The tiled kernels re-stream Q/dO (or K/V) once per 128-row block of the other side -- four times at N = 512 -- and pay
// two barriers per 64-row tile.  Here one 8-wave workgroup still owns a (batch, head), but LDS holds only TWO arrays at a
// time (2 x 512 rows x 144 B = 147 KB): K/V while a wave walks its (up to two) 32-query groups, then -- backward only --
// the same space is refilled with Q/dO for the pass in which a wave owns its 32-key groups.  Every array is fetched once
// into LDS plus once as row fragments; no barrier inside the key / query loops.  (The same scheme with 4-wave workgroups,
// two per CU, was measured for N <= 256 against the all-four-arrays-resident kernels above: 15-40 % slower there.)
// =====================================================================================================
constexpr int MD_MAXN = 512;

template <int HD, int NTHR, int MAXN>
__global__ __launch_bounds__(NTHR) void attn_fwd_mid_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                  bf16_t* __restrict__ out, int64_t ldo,
                                                                  float* __restrict__ lse, int N, int H, int hd, float scale) {
    typedef Cfg<bf16_t, HD> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NS = (N + 31) >> 5, NR = NS * 32;
    char* Ks = smem;
    char* Vs = smem + NR * C::RROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Cdim = H * hd;
    const bf16_t* qptr = qkv + (int64_t)b * N * ld + head * hd;
    Rows32Stage<HD, 2, MAXN, NTHR>().fill({qptr + Cdim, qptr + 2 * Cdim}, {ld, ld}, {Ks, Vs}, NR, N, hd, tid);
    __syncthreads();
    const float sl = scale * LOG2E;
    for (int sub = wave; sub < NS; sub += NTHR / 64) {      // wave-uniform
        const int q = 32 * sub + l31;
        const int qrow = (q < N) ? q : N - 1;
        bf16x8 qf[C::NKK];
        row_frags_load<HD>(qptr + (int64_t)qrow * ld, hd, h, qf);
        f32x16 o[C::NDB];
        acc_zero(o);
        float m_run = -INFINITY, l_run = 0.f;
        rows32_fwd_walk<HD>(Ks, Vs, 0, N, N, qf, sl, m_run, l_run, o, lane);
        const float inv = rows32_softmax_finish(m_run, l_run, lse, ((int64_t)b * H + head) * N + q, h == 0 && q < N);
        if (q < N) acc_store_row(out + ((int64_t)b * N + q) * ldo + head * hd, o, inv, hd, h);
    }
}

template <int HD, int NTHR, int MAXN>
__global__ __launch_bounds__(NTHR) void attn_bwd_mid_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                  const bf16_t* __restrict__ out, int64_t ldo,
                                                                  const bf16_t* __restrict__ dout, int64_t lddo,
                                                                  const float* __restrict__ lse, float* __restrict__ delta,
                                                                  bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H,
                                                                  int hd, float scale) {
    typedef Cfg<bf16_t, HD> C;
    constexpr int NWAVE = NTHR / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int NS = (N + 31) >> 5, NR = NS * 32;
    char* T0 = smem;                        // K, later Q
    char* T1 = smem + NR * C::RROW;         // V, later dO
    float* lse_s = reinterpret_cast<float*>(T1 + NR * C::RROW);   // [MD_MAXN]  lse * log2(e), +inf on padded rows
    float* del_s = lse_s + MAXN;                                  // [MAXN]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int head = blockIdx.x, b = blockIdx.y;
    const int Cdim = H * hd;
    const bf16_t* qptr = qkv + (int64_t)b * N * ld + head * hd;
    const bf16_t* doptr = dout + (int64_t)b * N * lddo + head * hd;
    const bf16_t* optr = out + (int64_t)b * N * ldo + head * hd;
    const int64_t bh = ((int64_t)b * H + head) * N;
    const float sl = scale * LOG2E;
    Rows32Stage<HD, 2, MAXN, NTHR>().fill({qptr + Cdim, qptr + 2 * Cdim}, {ld, ld}, {T0, T1}, NR, N, hd, tid);
    for (int i = tid; i < MAXN; i += NTHR) lse_s[i] = i < N ? lse[bh + i] * LOG2E : INFINITY;
    __syncthreads();

    // ---- pass A (K / V resident): delta and dQ, a wave walks its 32-query groups; row fragments come straight from HBM
    for (int sub = wave; sub < NS; sub += NWAVE) {
        const int row = 32 * sub + l31;
        const bool row_ok = row < N;
        const int rowc = row_ok ? row : N - 1;
        bf16x8 qf[C::NKK], dof[C::NKK];
        const float del = rows32_load_q_do_delta<HD>(qptr + (int64_t)rowc * ld, doptr + (int64_t)rowc * lddo, optr + (int64_t)rowc * ldo,
                                                     row_ok, hd, h, qf, dof);
        if (h == 0) {
            del_s[row] = del;
            if (row_ok && delta) delta[bh + row] = del;
        }
        const float lse2 = lse_s[row];
        f32x16 dq[C::NDB];
        acc_zero(dq);
        rows32_dq_walk<HD>(T0, T1, 0, N, N, qf, dof, sl, lse2, del, dq, lane);
        if (row_ok) acc_store_row(dqkv + ((int64_t)b * N + row) * lddq + head * hd, dq, scale, hd, h);
    }
    // ---- hand-over: lift the K / V row fragments of my key groups, then refill the two tiles with Q / dO
    constexpr int MAXG = MAXN / 32 / NWAVE;      // 2
    bf16x8 kf[MAXG][C::NKK], vf[MAXG][C::NKK];
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        int row = 32 * (wave + NWAVE * g) + l31;
        row = row < NR ? row : NR - 1;
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            kf[g][kk] = rtile_chunk<bf16_t, HD>(T0, row, 2 * kk + h);
            vf[g][kk] = rtile_chunk<bf16_t, HD>(T1, row, 2 * kk + h);
        }
    }
    __syncthreads();      // everyone is done with K / V (pass A loops and the lifts above); del_s is complete
    Rows32Stage<HD, 2, MAXN, NTHR>().fill({qptr, doptr}, {ld, lddo}, {T0, T1}, NR, N, hd, tid);
    __syncthreads();
    // ---- pass B (Q / dO resident): dK, dV, a wave walks its 32-key groups
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
        const int sub = wave + NWAVE * g;
        if (sub >= NS) break;      // wave-uniform
        const int row = 32 * sub + l31;
        f32x16 dk[C::NDB], dv[C::NDB];
        acc_zero(dk);
        acc_zero(dv);
        rows32_dkdv_walk<HD>(T0, T1, lse_s, del_s, NS, kf[g], vf[g], sl, dk, dv, lane);
        if (row < N) {
            bf16_t* dkrow = dqkv + ((int64_t)b * N + row) * lddq + Cdim + head * hd;
            acc_store_row_pair(dkrow, dk, scale, dkrow + Cdim, dv, 1.0f, hd, h);
        }
    }
}

// =====================================================================================================
// long sequences (N > 512: video tubelets N = 1568, dense-prediction grids), bf16, head_dim <= 64: the same 8-wave
// building blocks, but the other side of the attention matrix streams through LDS in CHUNKS of 256 rows (74 KB) instead
// of 64-row tiles: two barriers per 256 rows instead of per 64, a workgroup owns 256 rows (so the streamed side is
// re-read N/256 times, not N/128), and inside a chunk the per-wave loops run barrier-free on the step functions above.
//   forward : workgroup = 256 queries, K/V chunks stream (online softmax across chunks)
//   backward: (1) dQ + delta: workgroup = 256 queries, K/V chunks stream; (2) dK/dV: workgroup = 256 keys, Q/dO chunks
//             (+ their lse / delta) stream.  Deterministic, no atomics.
// =====================================================================================================
constexpr int CH_ROWS = 256;

template <int HD>
__global__ __launch_bounds__(SM_THREADS) void attn_fwd_chunk_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                    bf16_t* __restrict__ out, int64_t ldo,
                                                                    float* __restrict__ lse, int N, int H, int hd, float scale) {
    typedef Cfg<bf16_t, HD> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;
    char* Vs = smem + CH_ROWS * C::RROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int Cdim = H * hd;
    const bf16_t* qptr = qkv + (int64_t)b * N * ld + head * hd;
    const int q = blockIdx.x * CH_ROWS + 32 * wave + l31;
    const bool active = blockIdx.x * CH_ROWS + 32 * wave < N;      // wave-uniform
    const int qrow = (q < N) ? q : N - 1;
    bf16x8 qf[C::NKK];
    row_frags_load<HD>(qptr + (int64_t)qrow * ld, hd, h, qf);
    f32x16 o[C::NDB];
    acc_zero(o);
    float m_run = -INFINITY, l_run = 0.f;
    const float sl = scale * LOG2E;
    for (int kv0 = 0; kv0 < N; kv0 += CH_ROWS) {
        const int rows = N - kv0 < CH_ROWS ? N - kv0 : CH_ROWS;
        __syncthreads();      // the previous chunk is consumed
        Rows32Stage<HD, 2>().fill({qptr + Cdim + (int64_t)kv0 * ld, qptr + 2 * Cdim + (int64_t)kv0 * ld}, {ld, ld}, {Ks, Vs},
                                  (rows + 31) / 32 * 32, rows, hd, tid);
        __syncthreads();
        if (active) rows32_fwd_walk<HD>(Ks, Vs, kv0, rows, N, qf, sl, m_run, l_run, o, lane);
    }
    if (!active) return;
    const float inv = rows32_softmax_finish(m_run, l_run, lse, ((int64_t)b * H + head) * N + q, h == 0 && q < N);
    if (q < N) acc_store_row(out + ((int64_t)b * N + q) * ldo + head * hd, o, inv, hd, h);
}

// backward pass 1: delta and dQ for 256 queries; K/V stream in chunks
template <int HD>
__global__ __launch_bounds__(SM_THREADS) void attn_bwd_dq_chunk_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                       const bf16_t* __restrict__ out, int64_t ldo,
                                                                       const bf16_t* __restrict__ dout, int64_t lddo,
                                                                       const float* __restrict__ lse, float* __restrict__ delta,
                                                                       bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H,
                                                                       int hd, float scale) {
    typedef Cfg<bf16_t, HD> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;
    char* Vs = smem + CH_ROWS * C::RROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int Cdim = H * hd;
    const bf16_t* qptr = qkv + (int64_t)b * N * ld + head * hd;
    const bf16_t* doptr = dout + (int64_t)b * N * lddo + head * hd;
    const bf16_t* optr = out + (int64_t)b * N * ldo + head * hd;
    const int64_t bh = ((int64_t)b * H + head) * N;
    const int row = blockIdx.x * CH_ROWS + 32 * wave + l31;
    const bool active = blockIdx.x * CH_ROWS + 32 * wave < N;      // wave-uniform
    const bool row_ok = row < N;
    const int rowc = row_ok ? row : N - 1;
    bf16x8 qf[C::NKK], dof[C::NKK];
    const float del = rows32_load_q_do_delta<HD>(qptr + (int64_t)rowc * ld, doptr + (int64_t)rowc * lddo, optr + (int64_t)rowc * ldo, row_ok,
                                                 hd, h, qf, dof);
    if (h == 0 && row_ok) delta[bh + row] = del;
    const float lse2 = row_ok ? lse[bh + row] * LOG2E : INFINITY;      // padded queries: P = 0
    const float sl = scale * LOG2E;
    f32x16 dq[C::NDB];
    acc_zero(dq);
    for (int kv0 = 0; kv0 < N; kv0 += CH_ROWS) {
        const int rows = N - kv0 < CH_ROWS ? N - kv0 : CH_ROWS;
        __syncthreads();
        Rows32Stage<HD, 2>().fill({qptr + Cdim + (int64_t)kv0 * ld, qptr + 2 * Cdim + (int64_t)kv0 * ld}, {ld, ld}, {Ks, Vs},
                                  (rows + 31) / 32 * 32, rows, hd, tid);
        __syncthreads();
        if (active) rows32_dq_walk<HD>(Ks, Vs, kv0, rows, N, qf, dof, sl, lse2, del, dq, lane);
    }
    if (active && row_ok) acc_store_row(dqkv + ((int64_t)b * N + row) * lddq + head * hd, dq, scale, hd, h);
}

// backward pass 2: dK and dV for 256 keys; Q / dO (and their lse / delta) stream in chunks
template <int HD>
__global__ __launch_bounds__(SM_THREADS) void attn_bwd_dkdv_chunk_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                                         const bf16_t* __restrict__ dout, int64_t lddo,
                                                                         const float* __restrict__ lse,
                                                                         const float* __restrict__ delta,
                                                                         bf16_t* __restrict__ dqkv, int64_t lddq, int N, int H,
                                                                         int hd, float scale) {
    typedef Cfg<bf16_t, HD> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* dOs = smem + CH_ROWS * C::RROW;
    float* lse_s = reinterpret_cast<float*>(dOs + CH_ROWS * C::RROW);   // [CH_ROWS]
    float* del_s = lse_s + CH_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int Cdim = H * hd;
    const bf16_t* qptr = qkv + (int64_t)b * N * ld + head * hd;
    const bf16_t* doptr = dout + (int64_t)b * N * lddo + head * hd;
    const int64_t bh = ((int64_t)b * H + head) * N;
    const int row = blockIdx.x * CH_ROWS + 32 * wave + l31;
    const bool active = blockIdx.x * CH_ROWS + 32 * wave < N;      // wave-uniform
    const bool row_ok = row < N;
    const int rowc = row_ok ? row : N - 1;
    bf16x8 kf[C::NKK], vf[C::NKK];
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk) {
        const int d = (2 * kk + h) * 8;
        const bool ok = d < hd;
        const int dc = ok ? d : 0;
        u32x4 rk = *reinterpret_cast<const u32x4*>(qptr + Cdim + (int64_t)rowc * ld + dc);
        u32x4 rv = *reinterpret_cast<const u32x4*>(qptr + 2 * Cdim + (int64_t)rowc * ld + dc);
        rk = ok ? rk : zero4(); rv = ok ? rv : zero4();
        kf[kk] = *reinterpret_cast<bf16x8*>(&rk);
        vf[kk] = *reinterpret_cast<bf16x8*>(&rv);
    }
    const float sl = scale * LOG2E;
    f32x16 dk[C::NDB], dv[C::NDB];
    acc_zero(dk);
    acc_zero(dv);
    for (int q0 = 0; q0 < N; q0 += CH_ROWS) {
        const int rows = N - q0 < CH_ROWS ? N - q0 : CH_ROWS;
        const int NSc = (rows + 31) >> 5;
        __syncthreads();
        Rows32Stage<HD, 2>().fill({qptr + (int64_t)q0 * ld, doptr + (int64_t)q0 * lddo}, {ld, lddo}, {Qs, dOs}, NSc * 32, rows, hd, tid);
        if (tid < CH_ROWS) {
            const bool ok = tid < rows;
            lse_s[tid] = ok ? lse[bh + q0 + tid] * LOG2E : INFINITY;      // padded queries: P = 0
            del_s[tid] = ok ? delta[bh + q0 + tid] : 0.f;
        }
        __syncthreads();
        if (active) rows32_dkdv_walk<HD>(Qs, dOs, lse_s, del_s, NSc, kf, vf, sl, dk, dv, lane);
    }
    if (!active || !row_ok) return;
    bf16_t* dkrow = dqkv + ((int64_t)b * N + row) * lddq + Cdim + head * hd;
    acc_store_row_pair(dkrow, dk, scale, dkrow + Cdim, dv, 1.0f, hd, h);
}

constexpr size_t LDS_PER_CU = 160 * 1024;

// ---- the route: which kernel family takes a call, and the launch geometry that depends on more than (B, H).  The one place that
// decides by SM_MINN / SM_MAXN / RS_MAXN / MD_MAXN / ST_BWD_MINN, the 31-bit offset guard, the stride alignments and the row-block
// split; DESIGN 4.4 has the same conditions as a table.  No HIP calls.  Where the two directions differ the term says `backward`.
AttnRoute attn_route(const AttnCall& c, bool backward) {
    AttnRoute r = {};
    const int N = c.N, E = c.dtype == ME_BF16 ? 8 : 4;
    r.hd = c.hd <= 32 ? 32 : c.hd <= 64 ? 64 : 128;
    const bool no_drop = c.p_drop == 0.f;
    // very short sequences (the Tabular / Graph recipes): one wave per 16 tokens, attention_tiny.hip, bf16 and fp32.
    // SM_MINN: at or below one 64-key tile the tiled kernels (more workgroups per CU) win over the resident ones.
    // backward: dout and dqkv rows 16-byte aligned as well (the entry point only asks 4 elements of ld_dqkv)
    if (no_drop && N <= SM_MINN && attn_tiny_ok(c) && (!backward || (c.lddo % E == 0 && c.lddq % E == 0))) {
        r.form = ME_ATTN_TINY;
        return r;
    }
    // every other special form: bf16, no dropout, head_dim <= 64.
    // backward: all of them want ld_out % 8 (forward asks that of stream16 only, below; the entry point guarantees % 4)
    const bool bf16_form = no_drop && c.dtype == ME_BF16 && c.hd <= 64 && (!backward || c.ldo % 8 == 0);
    // ring16 / stream16 address rows with 31-bit byte offsets: of qkv, and of dout in backward
    auto off31 = [N](int64_t ld) { return (int64_t)N * ld * 2 < (int64_t)0x7e000000; };
    const bool offs_ok = off31(c.ld) && (!backward || off31(c.lddo));
    if (bf16_form && N > SM_MINN && N <= SM_MAXN) {
        if (N <= RS_MAXN && offs_ok) {
            r.form = ME_ATTN_RING16;
            r.ns = (N + 31) / 32;                 // 3 .. 7 (SM_MINN < N <= RS_MAXN)
        } else {
            r.form = ME_ATTN_RESIDENT;
        }
        return r;
    }
    // streaming form: row blocks of (at most) 14 x 16 rows, evened out over the sequence (queries; in the backward's second kernel, keys).
    // (head_dim <= 32: half the MFMA work per key for the same softmax arithmetic -- the 32-row kernels below measured faster there.)
    // Forward takes it from SM_MAXN + 1, backward from ST_BWD_MINN: up to MD_MAXN the mid backward kernel measured faster.
    // backward: ld_dqkv % 8 as well
    const int nblk = (N + 223) / 224;
    if (bf16_form && c.hd > 32 && N >= (backward ? ST_BWD_MINN : SM_MAXN + 1) && offs_ok && (int64_t)c.B * c.H * nblk < (int64_t)0x7fffffff &&
        c.ldo % 8 == 0 && (!backward || c.lddq % 8 == 0)) {
        r.form = ME_ATTN_STREAM16;
        r.nblk = nblk;
        r.rows = ((N + nblk - 1) / nblk + 15) / 16 * 16;
        // dK / dV: 32-key waves when the key blocks fill seven of them (see attn_bwd_dkdv_stream32_kernel)
        const int rows32 = (r.rows + 31) / 32 * 32;
        r.dkdv32 = backward && rows32 == 7 * 32;
        r.krows = r.dkdv32 ? rows32 : r.rows;
        return r;
    }
    // (the forward chunk arm used to test B <= 65535 as well: check_attn_args has rejected a larger B before any route is asked for)
    if (bf16_form && N > SM_MAXN) {
        r.form = N <= MD_MAXN ? ME_ATTN_MID : ME_ATTN_CHUNK;
        return r;
    }
    r.form = ME_ATTN_GENERIC;
    return r;
}

// ---- launches: one per form and direction
// grid of a persistent kernel: one workgroup per item up to per_cu workgroups on every CU
unsigned persistent_grid(int64_t items, int per_cu = 1) {
    const int64_t slots = (int64_t)device_cus() * per_cu;
    return (unsigned)(items < slots ? items : slots);
}
// f(Int<HD>) for the route's head width (the special forms: head_dim <= 64), f(Int<NS>) for the ring's sub-tile count
template <typename F> int by_hd(const AttnRoute& r, F f) { return r.hd <= 32 ? f(Int<32>()) : f(Int<64>()); }
template <typename F> int by_ns(const AttnRoute& r, F f) {
    switch (r.ns) {
        case 3: return f(Int<3>());
        case 4: return f(Int<4>());
        case 5: return f(Int<5>());
        case 6: return f(Int<6>());
        default: return f(Int<7>());
    }
}

template <int HD> int launch_fwd_small(const AttnCall& c) {
    typedef Cfg<bf16_t, HD> C;
    const auto p = c.as<bf16_t>();
    auto lds = [](int n) { return (size_t)(2 * ((n + 31) / 32 * 32) + SM_THREADS / 2) * C::RROW; };      // {K, V} + per-wave [32][HD] scratch
    const size_t smem = lds(c.N);
    const int64_t items = (int64_t)c.B * c.H;
    int per_cu = (int)(LDS_PER_CU / smem);
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    return launch_kernel<attn_fwd_small_kernel<HD>>("me_attention_fwd(small)", dim3(persistent_grid(items, per_cu)), SM_THREADS, smem, lds(SM_MAXN),
                                                  c.stream, p.qkv, c.ld, p.out, c.ldo, c.lse, c.N, c.H, c.hd, c.scale, (int)items);
}
template <int HD> int launch_bwd_small(const AttnCall& c) {
    typedef Cfg<bf16_t, HD> C;
    const auto p = c.as<bf16_t>();
    auto lds = [](int n) { return (size_t)4 * ((n + 31) / 32 * 32) * C::RROW + 2 * SM_MAXN * sizeof(float); };      // {Q, K, V, dO} + lse, delta
    return launch_kernel<attn_bwd_small_kernel<HD>>("me_attention_bwd(small)", dim3(c.H, c.B), SM_THREADS, lds(c.N), lds(SM_MAXN), c.stream, p.qkv, c.ld,
                                                  p.out, c.ldo, p.dout, c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale);
}
template <int HD, int NS> int launch_fwd_ring16(const AttnCall& c) {
    constexpr size_t smem = (size_t)4 * NS * 32 * RCfg<HD>::RB + (R16_THREADS / 64) * 16 * Cfg<bf16_t, HD>::RROW;
    const auto p = c.as<bf16_t>();
    const int64_t items = (int64_t)c.B * c.H;
    return launch_kernel<attn_fwd_ring16_kernel<HD, NS>>("me_attention_fwd(ring16)", dim3(persistent_grid(items)), R16_THREADS, smem, smem, c.stream, p.qkv,
                                                       c.ld, p.out, c.ldo, c.lse, c.N, c.H, c.hd, c.scale, (int)items);
}
template <int HD, int NS> int launch_bwd_ring16(const AttnCall& c) {
    constexpr size_t smem = (size_t)4 * NS * 32 * RCfg<HD>::RB + 2 * NS * 32 * sizeof(float) + (R16_THREADS / 64) * 16 * Cfg<bf16_t, HD>::RROW + 16;
    const auto p = c.as<bf16_t>();
    unsigned* ctr = me_work_counters(c.stream);      // (null while capturing: static schedule)
    if (ctr) ctr += 1;                                // word 1 of the stream's set (word 0: the resident GEMM, XCD 0)
    const int64_t items = (int64_t)c.B * c.H;
    return launch_kernel<attn_bwd_ring16_kernel<HD, NS>>("me_attention_bwd(ring16)", dim3(persistent_grid(items)), R16_THREADS, smem, smem, c.stream, p.qkv,
                                                       c.ld, p.out, c.ldo, p.dout, c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale, (int)items,
                                                       ctr);
}
template <int HD> int launch_fwd_stream16(const AttnCall& c, const AttnRoute& r) {
    constexpr size_t smem = (size_t)ST_RING * 2 * ST_KC * RCfg<HD>::RB + (R16_THREADS / 64) * 16 * Cfg<bf16_t, HD>::RROW;
    const auto p = c.as<bf16_t>();
    const int64_t items = (int64_t)c.B * c.H * r.nblk;
    return launch_kernel<attn_fwd_stream16_kernel<HD>>("me_attention_fwd(stream16)", dim3(persistent_grid(items)), R16_THREADS, smem, smem, c.stream, p.qkv, c.ld,
                                                     p.out, c.ldo, c.lse, c.N, c.H, c.hd, c.scale, r.rows, r.nblk, (int)items);
}
template <int HD> int launch_bwd_stream16(const AttnCall& c, const AttnRoute& r) {
    constexpr size_t ring = (size_t)ST_RING * 2 * ST_KC * RCfg<HD>::RB, fl = (size_t)ST_RING * 2 * ST_KC * sizeof(float);
    constexpr size_t smem1 = ring + (R16_THREADS / 64) * 16 * Cfg<bf16_t, HD>::RROW;
    constexpr size_t smem2 = smem1 + fl;
    constexpr size_t smem3 = ring + (ST32_THREADS / 64) * 16 * Cfg<bf16_t, HD>::RROW + fl;
    const auto p = c.as<bf16_t>();
    const int64_t items = (int64_t)c.B * c.H * r.nblk;
    const dim3 grid(persistent_grid(items));
    if (int rc = launch_kernel<attn_bwd_dq_stream16_kernel<HD>>("me_attention_bwd(dq stream16)", grid, R16_THREADS, smem1, smem1, c.stream, p.qkv, c.ld, p.out,
                                                              c.ldo, p.dout, c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale, r.rows, r.nblk,
                                                              (int)items))
        return rc;
    if (!r.dkdv32)
        return launch_kernel<attn_bwd_dkdv_stream16_kernel<HD>>("me_attention_bwd(dkdv stream16)", grid, R16_THREADS, smem2, smem2, c.stream, p.qkv, c.ld, p.dout,
                                                              c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale, r.krows, r.nblk, (int)items);
    return launch_kernel<attn_bwd_dkdv_stream32_kernel<HD>>("me_attention_bwd(dkdv stream32)", grid, ST32_THREADS, smem3, smem3, c.stream, p.qkv, c.ld, p.dout,
                                                          c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale, r.krows, r.nblk, (int)items);
}
template <int HD> int launch_fwd_mid(const AttnCall& c) {
    typedef Cfg<bf16_t, HD> C;
    const auto p = c.as<bf16_t>();
    auto lds = [](int n) { return (size_t)2 * ((n + 31) / 32 * 32) * C::RROW; };      // {K, V}
    return launch_kernel<attn_fwd_mid_kernel<HD, 512, MD_MAXN>>("me_attention_fwd(mid)", dim3(c.H, c.B), 512, lds(c.N), lds(MD_MAXN), c.stream, p.qkv, c.ld,
                                                              p.out, c.ldo, c.lse, c.N, c.H, c.hd, c.scale);
}
template <int HD> int launch_bwd_mid(const AttnCall& c) {
    typedef Cfg<bf16_t, HD> C;
    const auto p = c.as<bf16_t>();
    auto lds = [](int n) { return (size_t)2 * ((n + 31) / 32 * 32) * C::RROW + 2 * MD_MAXN * sizeof(float); };      // {K, V} then {Q, dO} + lse, delta
    return launch_kernel<attn_bwd_mid_kernel<HD, 512, MD_MAXN>>("me_attention_bwd(mid)", dim3(c.H, c.B), 512, lds(c.N), lds(MD_MAXN), c.stream, p.qkv, c.ld,
                                                              p.out, c.ldo, p.dout, c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale);
}
template <int HD> int launch_fwd_chunk(const AttnCall& c) {
    const size_t smem = (size_t)2 * CH_ROWS * Cfg<bf16_t, HD>::RROW;
    const auto p = c.as<bf16_t>();
    return launch_kernel<attn_fwd_chunk_kernel<HD>>("me_attention_fwd(chunk)", dim3((c.N + CH_ROWS - 1) / CH_ROWS, c.H, c.B), SM_THREADS, smem, smem, c.stream,
                                                  p.qkv, c.ld, p.out, c.ldo, c.lse, c.N, c.H, c.hd, c.scale);
}
template <int HD> int launch_bwd_chunk(const AttnCall& c) {
    const size_t smem1 = (size_t)2 * CH_ROWS * Cfg<bf16_t, HD>::RROW, smem2 = smem1 + 2 * CH_ROWS * sizeof(float);
    const auto p = c.as<bf16_t>();
    const dim3 grid((c.N + CH_ROWS - 1) / CH_ROWS, c.H, c.B);
    if (int rc = launch_kernel<attn_bwd_dq_chunk_kernel<HD>>("me_attention_bwd(dq chunk)", grid, SM_THREADS, smem1, smem1, c.stream, p.qkv, c.ld, p.out, c.ldo,
                                                           p.dout, c.lddo, c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale))
        return rc;
    return launch_kernel<attn_bwd_dkdv_chunk_kernel<HD>>("me_attention_bwd(dkdv chunk)", grid, SM_THREADS, smem2, smem2, c.stream, p.qkv, c.ld, p.dout, c.lddo,
                                                       c.lse, c.delta, p.dqkv, c.lddq, c.N, c.H, c.hd, c.scale);
}

// ME_ATTN_GENERIC: the packed call as the descriptor of the tiled kernels (attention_qkv.hip) -- q | k | v = qkv + {0, C, 2C} on one row
// stride, dq | dk | dv = dqkv + {0, C, 2C} likewise, Nq = Nk = N, not causal
me_attn_qkv_desc tiled_desc(const AttnCall& c) {
    const size_t Cb = (size_t)c.H * c.hd * me_dtype_size(c.dtype);      // one third of a row, bytes
    const char* q = static_cast<const char*>(c.qkv);
    char* dq = static_cast<char*>(c.dqkv);                              // (null in a forward call)
    me_attn_qkv_desc d = {};
    d.q = q; d.k = q + Cb; d.v = q + 2 * Cb;
    d.ld_q = d.ld_k = d.ld_v = c.ld;
    d.out = c.out; d.ld_out = c.ldo;
    d.lse = c.lse;
    d.dout = c.dout; d.ld_dout = c.lddo;
    d.delta = c.delta;
    if (dq) { d.dq = dq; d.dk = dq + Cb; d.dv = dq + 2 * Cb; }
    d.ld_dq = d.ld_dk = d.ld_dv = c.lddq;
    d.seed = c.seed;
    d.B = c.B; d.Nq = d.Nk = c.N; d.H = c.H; d.head_dim = c.hd;
    d.dtype = c.dtype; d.causal = 0;
    d.scale = c.scale; d.p_drop = c.p_drop;
    return d;
}

int check_attn_args(const char* fn, int64_t ld, int B, int N, int H, int hd, int dtype) {
    ME_CHECK_ARG(me_dtype_ok(dtype), "%s: bad dtype", fn);
    ME_CHECK_ARG(B > 0 && N > 0 && H > 0 && hd > 0, "%s: bad shape B=%d N=%d H=%d hd=%d", fn, B, N, H, hd);
    const int E = dtype == ME_BF16 ? 8 : 4;
    ME_CHECK_ARG(hd % E == 0, "%s: head_dim=%d must be a multiple of %d", fn, hd, E);
    ME_CHECK_ARG(hd <= 128, "%s: head_dim=%d > 128 unsupported", fn, hd);
    ME_CHECK_ARG(ld % E == 0, "%s: row stride must be a multiple of %d elements", fn, E);
    ME_CHECK_ARG(B <= 65535 && H <= 65535, "%s: B and H must be <= 65535", fn);
    return ME_OK;
}

}  // namespace

extern "C" int me_attention_fwd(const void* qkv, int64_t ld_qkv, void* out, int64_t ld_out, float* lse, int B, int N,
                                int H, int head_dim, float scale, int dtype, float p_drop, uint64_t seed, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ProfScope prof(ME_PROF_ATTN_FWD, dtype, (int64_t)B * H, N, head_dim, stream);
    ME_CHECK_ARG(qkv && out, "me_attention_fwd: null pointer");
    int rc = check_attn_args("me_attention_fwd", ld_qkv, B, N, H, head_dim, dtype);
    if (rc) return rc;
    ME_CHECK_ARG(ld_out % 4 == 0, "me_attention_fwd: ld_out must be a multiple of 4");
    ME_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "me_attention_fwd: p_drop must be in [0, 1)");
    const AttnCall c = {qkv, ld_qkv, out, ld_out, nullptr, 0, lse, nullptr, nullptr, 0, B, N, H, head_dim, scale, dtype, p_drop, seed, stream};
    const AttnRoute r = attn_route(c, false);
    prof.plan = r.plan();
    switch (r.form) {
        case ME_ATTN_TINY: return launch_attn_tiny(c, false);
        case ME_ATTN_RING16: return by_hd(r, [&](auto HD) { return by_ns(r, [&](auto NS) { return launch_fwd_ring16<HD(), NS()>(c); }); });
        case ME_ATTN_RESIDENT: return by_hd(r, [&](auto HD) { return launch_fwd_small<HD()>(c); });
        case ME_ATTN_STREAM16: return launch_fwd_stream16<64>(c, r);
        case ME_ATTN_MID: return by_hd(r, [&](auto HD) { return launch_fwd_mid<HD()>(c); });
        case ME_ATTN_CHUNK: return by_hd(r, [&](auto HD) { return launch_fwd_chunk<HD()>(c); });
    }
    return launch_attn_tiled_fwd(tiled_desc(c), stream);
}

extern "C" int me_attention_bwd(const void* qkv, int64_t ld_qkv, const void* out, int64_t ld_out, const void* dout,
                                int64_t ld_dout, const float* lse, float* delta, void* dqkv, int64_t ld_dqkv, int B,
                                int N, int H, int head_dim, float scale, int dtype, float p_drop, uint64_t seed,
                                void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ProfScope prof(ME_PROF_ATTN_BWD, dtype, (int64_t)B * H, N, head_dim, stream);
    ME_CHECK_ARG(qkv && out && dout && lse && delta && dqkv, "me_attention_bwd: null pointer");
    int rc = check_attn_args("me_attention_bwd", ld_qkv, B, N, H, head_dim, dtype);
    if (rc) return rc;
    const int E = dtype == ME_BF16 ? 8 : 4;
    ME_CHECK_ARG(ld_dout % E == 0 && ld_dqkv % 4 == 0, "me_attention_bwd: bad strides");
    ME_CHECK_ARG(p_drop >= 0.f && p_drop < 1.f, "me_attention_bwd: p_drop must be in [0, 1)");
    const AttnCall c = {qkv, ld_qkv, const_cast<void*>(out), ld_out, dout, ld_dout, const_cast<float*>(lse), delta, dqkv, ld_dqkv,
                        B, N, H, head_dim, scale, dtype, p_drop, seed, stream};
    const AttnRoute r = attn_route(c, true);
    prof.plan = r.plan();
    switch (r.form) {
        case ME_ATTN_TINY: return launch_attn_tiny(c, true);
        case ME_ATTN_RING16: return by_hd(r, [&](auto HD) { return by_ns(r, [&](auto NS) { return launch_bwd_ring16<HD(), NS()>(c); }); });
        case ME_ATTN_RESIDENT: return by_hd(r, [&](auto HD) { return launch_bwd_small<HD()>(c); });
        case ME_ATTN_STREAM16: return launch_bwd_stream16<64>(c, r);
        case ME_ATTN_MID: return by_hd(r, [&](auto HD) { return launch_bwd_mid<HD()>(c); });
        case ME_ATTN_CHUNK: return by_hd(r, [&](auto HD) { return launch_bwd_chunk<HD()>(c); });
    }
    if ((rc = launch_attn_delta(out, ld_out, dout, ld_dout, dtype, delta, B, N, H, head_dim, stream))) return rc;      // delta = dO . O
    return launch_attn_tiled_bwd(tiled_desc(c), stream);
}
