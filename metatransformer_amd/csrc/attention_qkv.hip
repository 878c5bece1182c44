// attention_qkv.hip -- the tiled attention kernels: multi-head attention over SEPARATE Q, K and V operands, two sequence lengths and a causal
// flag, flash-style.  Two callers:
//   * me_attention_qkv_fwd / _bwd (here): the decoder side of the Time-Series forecaster.  Replaces FullAttention.forward
//     (Time-Series/layers/SelfAttention_Family.py:56-75) together with the head reshapes of AttentionLayer (:195-211): scores = Q K^T,
//     TriangularCausalMask (utils/masking.py:4-8) when mask_flag, softmax(scale * scores), dropout, A V.
//   * the ME_ATTN_GENERIC arm of me_attention_fwd / _bwd (attention.hip): the packed [B*N, 3C] call is q = qkv, k = qkv + C, v = qkv + 2C
//     on one row stride, Nq = Nk, not causal -- exact-fp32, head_dim > 64, dropout, and what no special form of attn_route takes.
// Both reach the kernels through launch_attn_tiled_fwd / _bwd (attention_host.h).
//
// Q, K and V are addressed in place, each by its own pointer and row stride, so one call reads Q from a [B*Nq, C] projection and K / V
// from one packed [B*Nk, 2C] GEMM output (cross-attention) or all three from a packed [B*N, 3C] (self-attention).  The [B,H,Nq,Nk]
// score matrix is never written: K / V tiles of 64 keys are staged in LDS (attention_tile.h), a block takes 128 queries (32 per wave),
// the softmax runs online in registers, and O is written head-major straight into [tokens, C].  Instantiated for HD 32 / 64 / 128.
//
// MFMA formulation (32x32 shapes, see common.h): every product is issued "transposed" so that the softmax
// row (one query) lives in ONE lane (plus its partner lane^32):
//   S^T[kv][q] = K Q^T           A = K rows (from LDS), B = Q rows (registers)      -> lane q, regs kv
//   O^T[d][q] += V^T P^T         A = V^T rows d (LDS, transposed while staging), B = P (registers, in place)
// The row max / row sum are 16-register reductions plus one xor-32 shuffle; the running rescale of O^T is a
// per-lane scalar.  The reduction-index permutation the accumulator layout imposes on P is absorbed by reading
// V^T with the same permutation (common.h: any assignment works if A and B agree).
// fp32 runs the same code on the exact-fp32 MFMA (parity mode); bf16 is the performance mode.
//
//   * causal: tiles entirely on the masked side of the diagonal are skipped (the loop bounds are block-uniform, a wave skips the
//     compute of a tile none of its rows sees), the tiles the diagonal crosses are masked element-wise,
//   * the dropout stream is indexed ((b*H + h)*Nq + q)*Nk + k.
// Backward: a delta pass chosen by the entry point (dO . O, or from the tiles: attn_qkv_delta_kernel says when), dK / dV (a wave owns
// 32 keys, walks query tiles), dQ (a wave owns 32 queries, walks key tiles).  No atomics, every output element is written exactly
// once, two runs are bit-identical.
#include "attention_host.h"
#include "attention_tile.h"
#include <stdint.h>

namespace {

// key kv is visible to query q
__device__ __forceinline__ bool qkv_visible(int kv, int q, int Nk, int causal) { return kv < Nk && (!causal || kv <= q); }

// fp32: the transposed [HD][64] copy of a tile written from the registers of its row-major stage.  RowStage<float> and TransStage<float> fetch
// the same 16 bytes per item, so the backward kernels stage Q / dO / K once and store them twice instead of loading them twice
// (a second register set for the transposed copy is what no longer fits beside the accumulators at HD 128).
template <int HD> __device__ __forceinline__ void store_transposed(const RowStage<float, HD>& st, char* lds, int tid) {
    typedef Cfg<float, HD> C;
#pragma unroll
    for (int i = 0; i < C::R_ITEMS; ++i) {
        const int it = tid + AT_THREADS * i;
        const int chunk = it % C::CPR, row = it / C::CPR;
        if (row < KVT) {
#pragma unroll
            for (int e = 0; e < 4; ++e) *reinterpret_cast<uint32_t*>(lds + (chunk * 4 + e) * C::TROW + row * 4) = st.v[i][e];
        }
    }
}
template <int HD> __device__ __forceinline__ void store_transposed(const RowStage<bf16_t, HD>&, char*, int) {}      // bf16 reads row tiles with tr

// =====================================================================================================
// forward
// =====================================================================================================
template <typename T, int HD>
__global__ __launch_bounds__(AT_THREADS) void attn_qkv_fwd_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                                  const T* __restrict__ v, int64_t ldv, T* __restrict__ out, int64_t ldo,
                                                                  float* __restrict__ lse, int Nq, int Nk, int H, int hd, float scale,
                                                                  int causal, float p_drop, uint64_t seed) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool TT = TRead<T, HD>::kNeedsTransposedTile;
    char* Ks = smem;
    char* Vs = smem + C::R_BYTES;              // fp32: transposed [HD][64]; bf16: row-major [64][HD] (read with tr)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qbase = blockIdx.x * QPB + wave * 32;
    const T* qptr = q + (int64_t)b * Nq * ldq + head * hd;
    const T* kptr = k + (int64_t)b * Nk * ldk + head * hd;
    const T* vptr = v + (int64_t)b * Nk * ldv + head * hd;

    chunk_t qf[C::NKK];
    {
        const int qrow = (qbase + l31 < Nq) ? qbase + l31 : Nq - 1;      // out-of-range rows read the last row and are never stored
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            const int d = (2 * kk + h) * C::E;
            u32x4 raw = (d < hd) ? *reinterpret_cast<const u32x4*>(qptr + (int64_t)qrow * ldq + d) : zero4();
            qf[kk] = *reinterpret_cast<chunk_t*>(&raw);
        }
    }
    f32x16 o[C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const bool active = qbase < Nq;      // wave-uniform
    const int qi = qbase + l31;          // this lane's query (unclamped: a row past Nq only sees more keys)
    int ntiles = (Nk + KVT - 1) / KVT;
    if (causal) {                        // block-uniform: key tiles that start beyond the block's last query are all masked
        const int qlast = min(blockIdx.x * QPB + QPB - 1, Nq - 1);
        ntiles = min(ntiles, qlast / KVT + 1);
    }

    RowStage<T, HD> ks, vrs;
    TransStage<T, HD> vts;
    ks.load(kptr, ldk, 0, Nk, hd, tid);
    if (TT) vts.load(vptr, ldv, 0, Nk, hd, tid); else vrs.load(vptr, ldv, 0, Nk, hd, tid);
    for (int j = 0; j < ntiles; ++j) {
        __syncthreads();
        ks.store(Ks, tid);
        if (TT) vts.store(Vs, tid); else vrs.store(Vs, tid);
        __syncthreads();
        if (j + 1 < ntiles) {
            ks.load(kptr, ldk, (j + 1) * KVT, Nk, hd, tid);
            if (TT) vts.load(vptr, ldv, (j + 1) * KVT, Nk, hd, tid); else vrs.load(vptr, ldv, (j + 1) * KVT, Nk, hd, tid);
        }
        const int kv0 = j * KVT;
        if (!active || (causal && kv0 > qbase + 31)) continue;      // wave-uniform: no row of this wave sees the tile
        f32x16 s[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[u][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < C::NKK; ++kk)
                s[u] = mma_chunk(rtile_chunk<T, HD>(Ks, 32 * u + l31, 2 * kk + h), qf[kk], s[u]);
        }
        float mt = -INFINITY;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kv = kv0 + 32 * u + acc_row(r, h);
                const float sv = qkv_visible(kv, qi, Nk, causal) ? s[u][r] * scale : -INFINITY;
                s[u][r] = sv;
                mt = fmaxf(mt, sv);
            }
        // One lane holds half of the tile's keys, and on a tile the diagonal crosses all of them may be masked: mt = -inf here.  After
        // the fold with the partner lane it is finite on EVERY tile that gets this far: kv0 < Nk always, and under `causal` kv0 and qbase
        // are multiples of 32 with kv0 <= qbase + 31, hence kv0 <= qbase <= qi -- key kv0 is visible to every row of the wave.  So m_new is
        // finite, exp(-inf - m_new) = 0 for the masked entries, and m_run - m_new is -inf - finite (alpha = 0) on the first processed tile
        // (tile 0: it is never skipped) and finite - finite afterwards: -inf - (-inf) cannot occur.
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __expf(m_run - m_new);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(s[u][r] - m_new);
                s[u][r] = p;
                ps += p;
            }
        l_run = l_run * alpha + ps;
        m_run = m_new;
        if (p_drop > 0.f) {      // FullAttention's dropout acts on the NORMALISED probabilities -- the row sum stays unmasked
            const float keep = 1.0f / (1.0f - p_drop);
            const uint64_t rowbase = (((uint64_t)b * H + head) * Nq + (uint64_t)qi) * (uint64_t)Nk;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s[u][r] = u01_hash(seed, rowbase + (uint64_t)(kv0 + 32 * u + acc_row(r, h))) >= p_drop ? s[u][r] * keep : 0.f;
        }
#pragma unroll
        for (int db = 0; db < C::NDB; ++db) o[db] *= alpha;
#pragma unroll
        for (int c = 0; c < C::NPC; ++c) {
            const chunk_t pb = pack_chunk((const T*)nullptr, s, c);
#pragma unroll
            for (int db = 0; db < C::NDB; ++db)
                o[db] = mma_chunk(TRead<T, HD>::chunk(Vs, Vs, db, c, lane), pb, o[db]);
        }
    }
    if (!active) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (qi < Nq) {
        T* orow = out + ((int64_t)b * Nq + qi) * ldo + head * hd;
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * db + 8 * g + 4 * h;
                if (d < hd)
                    store_quad<T>(orow + d, f32x4{o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv,
                                                  o[db][4 * g + 3] * inv});
            }
        if (lse && h == 0) lse[((int64_t)b * H + head) * Nq + qi] = m_run + __logf(l_tot);
    }
}

// =====================================================================================================
// backward
//   delta[q]   = sum_d dO[q,d] O[q,d]
//   P          = exp(S*scale - lse[q]) on the visible entries, 0 elsewhere ; dP = dO V^T ; dS = P * (dP - delta[q]) * scale
//   dV = P^T dO ; dK = dS^T Q ; dQ = dS K
// Two kernels, no atomics: (1) dK/dV: a wave owns 32 keys, walks query tiles; (2) dQ: a wave owns 32 queries,
// walks key tiles (recomputing S and dP).
// =====================================================================================================

// ---- dK / dV: a wave owns 32 keys and walks the 64-query tiles that can see them.  The launch accumulates the NDBO 32-wide d blocks from
// DB0 on: all of them in one launch, except fp32 at HD 128 -- there the K and V rows (128 registers) and a full dK / dV accumulator pair (128)
// leave no room for S, dP and the staged tile without spilling, so two launches take two d blocks each (S and dP are formed in both).
template <typename T, int HD, int DB0, int NDBO>
__global__ __launch_bounds__(AT_THREADS) void attn_qkv_bwd_dkdv_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                                       const T* __restrict__ v, int64_t ldv, const T* __restrict__ dout,
                                                                       int64_t lddo, const float* __restrict__ lse,
                                                                       const float* __restrict__ delta, T* __restrict__ dk_out, int64_t lddk,
                                                                       T* __restrict__ dv_out, int64_t lddv, int Nq, int Nk, int H, int hd,
                                                                       float scale, int causal, float p_drop, uint64_t seed) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TB = TRead<T, HD>::kNeedsTransposedTile ? C::T_BYTES : 0;   // bf16 reads the row tiles transposed (tr)
    char* Qs = smem;                           // [64 q][HD]
    char* dOs = Qs + C::R_BYTES;               // [64 q][HD]
    char* QTs = dOs + C::R_BYTES;              // [HD][64 q]   (fp32 only)
    char* dOTs = QTs + TB;                     // [HD][64 q]   (fp32 only)
    float* lse_s = reinterpret_cast<float*>(dOTs + TB);           // [64]
    float* del_s = lse_s + KVT;                                   // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int kblock = blockIdx.x;
    const int kvbase = kblock * QPB + wave * 32;
    const T* qptr = q + (int64_t)b * Nq * ldq + head * hd;
    const T* kptr = k + (int64_t)b * Nk * ldk + head * hd;
    const T* vptr = v + (int64_t)b * Nk * ldv + head * hd;
    const T* doptr = dout + (int64_t)b * Nq * lddo + head * hd;
    const float* lse_bh = lse + ((int64_t)b * H + head) * Nq;
    const float* del_bh = delta + ((int64_t)b * H + head) * Nq;

    chunk_t kf[C::NKK], vf[C::NKK];
    {
        const int kvrow = (kvbase + l31 < Nk) ? kvbase + l31 : Nk - 1;
#pragma unroll
        for (int kk = 0; kk < C::NKK; ++kk) {
            const int d = (2 * kk + h) * C::E;
            u32x4 rk = (d < hd) ? *reinterpret_cast<const u32x4*>(kptr + (int64_t)kvrow * ldk + d) : zero4();
            u32x4 rv = (d < hd) ? *reinterpret_cast<const u32x4*>(vptr + (int64_t)kvrow * ldv + d) : zero4();
            kf[kk] = *reinterpret_cast<chunk_t*>(&rk);
            vf[kk] = *reinterpret_cast<chunk_t*>(&rv);
        }
    }
    f32x16 dk[NDBO], dv[NDBO];
#pragma unroll
    for (int db = 0; db < NDBO; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[db][r] = 0.f; dv[db][r] = 0.f; }
    const bool active = kvbase < Nk;
    const int kvi = kvbase + l31;
    const bool kv_ok = kvi < Nk;
    const int ntiles = (Nq + KVT - 1) / KVT;
    // causal (Nq == Nk): query tiles that end before the block's first key see none of its keys.  Block-uniform; kblock * QPB < Nk = Nq,
    // so j0 < ntiles and the first staged tile exists.
    const int j0 = causal ? (kblock * QPB) / KVT : 0;

    constexpr bool TT = TRead<T, HD>::kNeedsTransposedTile;
    RowStage<T, HD> qs, dos;
    float lse_r = INFINITY, del_r = 0.f;
    auto gload = [&](int q0) {
        qs.load(qptr, ldq, q0, Nq, hd, tid);
        dos.load(doptr, lddo, q0, Nq, hd, tid);
        if (tid < KVT) {
            const int qq = q0 + tid;
            lse_r = (qq < Nq) ? lse_bh[qq] : INFINITY;          // exp(s - inf) = 0 masks padded queries
            del_r = (qq < Nq) ? del_bh[qq] : 0.f;
        }
    };
    gload(j0 * KVT);
    for (int j = j0; j < ntiles; ++j) {
        __syncthreads();
        qs.store(Qs, tid);
        dos.store(dOs, tid);
        if (TT) {
            store_transposed<HD>(qs, QTs, tid);
            store_transposed<HD>(dos, dOTs, tid);
        }
        if (tid < KVT) {
            lse_s[tid] = lse_r;
            del_s[tid] = del_r;
        }
        __syncthreads();
        if (j + 1 < ntiles) gload((j + 1) * KVT);            // next tile's global loads fly during this tile's MFMAs
        if (!active || (causal && j * KVT + KVT - 1 < kvbase)) continue;      // wave-uniform: the tile's last query precedes the wave's first key
        f32x16 s[2], dp[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[u][r] = 0.f; dp[u][r] = 0.f; }
#pragma unroll
            for (int kk = 0; kk < C::NKK; ++kk) {
                s[u] = mma_chunk(rtile_chunk<T, HD>(Qs, 32 * u + l31, 2 * kk + h), kf[kk], s[u]);      // S[q][kv]
                dp[u] = mma_chunk(rtile_chunk<T, HD>(dOs, 32 * u + l31, 2 * kk + h), vf[kk], dp[u]);   // dP[q][kv]
            }
            // lane: kv = l31 (fixed), regs: q = 32u + acc_row(r,h)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 L = *reinterpret_cast<const f32x4*>(lse_s + 32 * u + 8 * g + 4 * h);
                const f32x4 D = *reinterpret_cast<const f32x4*>(del_s + 32 * u + 8 * g + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    const int qq = j * KVT + 32 * u + acc_row(r, h);
                    const float p = (kv_ok && (!causal || kvi <= qq)) ? __expf(s[u][r] * scale - L[e]) : 0.f;
                    float pm = p, dpm = dp[u][r];
                    if (p_drop > 0.f) {      // same mask as forward: dV sees the dropped P, dS the dropped dP
                        const uint64_t idx = (((uint64_t)b * H + head) * Nq + (uint64_t)qq) * (uint64_t)Nk + (uint64_t)kvi;
                        const float keep = u01_hash(seed, idx) >= p_drop ? 1.0f / (1.0f - p_drop) : 0.f;
                        pm *= keep; dpm *= keep;
                    }
                    s[u][r] = pm;                                  // (dropped) P
                    dp[u][r] = p * (dpm - D[e]) * scale;           // dS
                }
            }
            // this 32-query half goes into dV / dK before the other half's S and dP are formed (chunks still in ascending order, with half
            // the S / dP registers live)
#pragma unroll
            for (int c = u * (C::NPC / 2); c < (u + 1) * (C::NPC / 2); ++c) {
                const chunk_t pb = pack_chunk((const T*)nullptr, s, c);
                const chunk_t dsb = pack_chunk((const T*)nullptr, dp, c);
#pragma unroll
                for (int db = 0; db < NDBO; ++db) {
                    dv[db] = mma_chunk(TRead<T, HD>::chunk(dOTs, dOs, DB0 + db, c, lane), pb, dv[db]);   // dV^T[d][kv]
                    dk[db] = mma_chunk(TRead<T, HD>::chunk(QTs, Qs, DB0 + db, c, lane), dsb, dk[db]);  // dK^T[d][kv]
                }
            }
        }
    }
    if (!active || !kv_ok) return;
    T* dkrow = dk_out + ((int64_t)b * Nk + kvi) * lddk + head * hd;
    T* dvrow = dv_out + ((int64_t)b * Nk + kvi) * lddv + head * hd;
#pragma unroll
    for (int db = 0; db < NDBO; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * (DB0 + db) + 8 * g + 4 * h;
            if (d < hd) {
                store_quad<T>(dkrow + d, f32x4{dk[db][4 * g], dk[db][4 * g + 1], dk[db][4 * g + 2], dk[db][4 * g + 3]});
                store_quad<T>(dvrow + d, f32x4{dv[db][4 * g], dv[db][4 * g + 1], dv[db][4 * g + 2], dv[db][4 * g + 3]});
            }
        }
}

// ---- delta for bf16: delta[q] = sum_k P~[q,k] dP[q,k] (P~: the dropped probabilities) from the tiles, in fp32.  In exact arithmetic this is
// dO . O, which is how the fp32 path (and me_attention_bwd) forms it; in bf16 that O is the rounded output of a forward that rounded P
// too, and in the first rows of a causal call, where a few keys carry large probabilities, the error reaches dS undamped (measured: dQ
// off by 0.5 % of max|dQ| at N = 129, head_dim 96).  Formed here, dS sums to zero over the keys as it should.  Same walk as the dQ kernel.
template <typename T, int HD>
__global__ __launch_bounds__(AT_THREADS) void attn_qkv_delta_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                                    const T* __restrict__ v, int64_t ldv, const T* __restrict__ dout,
                                                                    int64_t lddo, const float* __restrict__ lse, float* __restrict__ delta,
                                                                    int Nq, int Nk, int H, int hd, float scale, int causal, float p_drop,
                                                                    uint64_t seed) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                    // [64 kv][HD]
    char* Vs = Ks + C::R_BYTES;         // [64 kv][HD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qbase = blockIdx.x * QPB + wave * 32;
    const T* qptr = q + (int64_t)b * Nq * ldq + head * hd;
    const T* kptr = k + (int64_t)b * Nk * ldk + head * hd;
    const T* vptr = v + (int64_t)b * Nk * ldv + head * hd;
    const T* doptr = dout + (int64_t)b * Nq * lddo + head * hd;

    const int qi = qbase + l31;
    const bool q_ok = qi < Nq;
    const int qrow = q_ok ? qi : Nq - 1;
    chunk_t qf[C::NKK], dof[C::NKK];
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk) {
        const int d = (2 * kk + h) * C::E;
        u32x4 rq = (d < hd) ? *reinterpret_cast<const u32x4*>(qptr + (int64_t)qrow * ldq + d) : zero4();
        u32x4 rd = (d < hd) ? *reinterpret_cast<const u32x4*>(doptr + (int64_t)qrow * lddo + d) : zero4();
        qf[kk] = *reinterpret_cast<chunk_t*>(&rq);
        dof[kk] = *reinterpret_cast<chunk_t*>(&rd);
    }
    const float lse_q = lse[((int64_t)b * H + head) * Nq + qrow];
    const bool active = qbase < Nq;
    int ntiles = (Nk + KVT - 1) / KVT;
    if (causal) {                        // block-uniform, as in the forward
        const int qlast = min(blockIdx.x * QPB + QPB - 1, Nq - 1);
        ntiles = min(ntiles, qlast / KVT + 1);
    }
    float acc = 0.f;
    RowStage<T, HD> ks, vs;
    auto gload = [&](int kv0) {
        ks.load(kptr, ldk, kv0, Nk, hd, tid);
        vs.load(vptr, ldv, kv0, Nk, hd, tid);
    };
    gload(0);
    for (int j = 0; j < ntiles; ++j) {
        const int kv0 = j * KVT;
        __syncthreads();
        ks.store(Ks, tid);
        vs.store(Vs, tid);
        __syncthreads();
        if (j + 1 < ntiles) gload((j + 1) * KVT);
        if (!active || (causal && kv0 > qbase + 31)) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int kk = 0; kk < C::NKK; ++kk) {
                s = mma_chunk(rtile_chunk<T, HD>(Ks, 32 * u + l31, 2 * kk + h), qf[kk], s);       // S^T[kv][q]
                dp = mma_chunk(rtile_chunk<T, HD>(Vs, 32 * u + l31, 2 * kk + h), dof[kk], dp);    // dP^T[kv][q]
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kv = kv0 + 32 * u + acc_row(r, h);
                const float p = qkv_visible(kv, qi, Nk, causal) ? __expf(s[r] * scale - lse_q) : 0.f;
                float dpm = dp[r];
                if (p_drop > 0.f) {
                    const uint64_t idx = (((uint64_t)b * H + head) * Nq + (uint64_t)qi) * (uint64_t)Nk + (uint64_t)kv;
                    dpm = u01_hash(seed, idx) >= p_drop ? dpm * (1.0f / (1.0f - p_drop)) : 0.f;
                }
                acc += p * dpm;
            }
        }
    }
    if (!active) return;
    acc += __shfl_xor(acc, 32, 64);
    if (q_ok && h == 0) delta[((int64_t)b * H + head) * Nq + qi] = acc;
}

// ---- dQ: a wave owns 32 queries and walks the 64-key tiles they see
template <typename T, int HD>
__global__ __launch_bounds__(AT_THREADS) void attn_qkv_bwd_dq_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                                     const T* __restrict__ v, int64_t ldv, const T* __restrict__ dout,
                                                                     int64_t lddo, const float* __restrict__ lse,
                                                                     const float* __restrict__ delta, T* __restrict__ dq_out, int64_t lddq,
                                                                     int Nq, int Nk, int H, int hd, float scale, int causal, float p_drop,
                                                                     uint64_t seed) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                    // [64 kv][HD]
    char* Vs = Ks + C::R_BYTES;         // [64 kv][HD]
    char* KTs = Vs + C::R_BYTES;        // [HD][64 kv]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qbase = blockIdx.x * QPB + wave * 32;
    const T* qptr = q + (int64_t)b * Nq * ldq + head * hd;
    const T* kptr = k + (int64_t)b * Nk * ldk + head * hd;
    const T* vptr = v + (int64_t)b * Nk * ldv + head * hd;
    const T* doptr = dout + (int64_t)b * Nq * lddo + head * hd;

    const int qi = qbase + l31;
    const bool q_ok = qi < Nq;
    const int qrow = q_ok ? qi : Nq - 1;
    chunk_t qf[C::NKK], dof[C::NKK];
#pragma unroll
    for (int kk = 0; kk < C::NKK; ++kk) {
        const int d = (2 * kk + h) * C::E;
        u32x4 rq = (d < hd) ? *reinterpret_cast<const u32x4*>(qptr + (int64_t)qrow * ldq + d) : zero4();
        u32x4 rd = (d < hd) ? *reinterpret_cast<const u32x4*>(doptr + (int64_t)qrow * lddo + d) : zero4();
        qf[kk] = *reinterpret_cast<chunk_t*>(&rq);
        dof[kk] = *reinterpret_cast<chunk_t*>(&rd);
    }
    const float lse_q = lse[((int64_t)b * H + head) * Nq + qrow];
    const float del_q = delta[((int64_t)b * H + head) * Nq + qrow];
    f32x16 dq[C::NDB];
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[db][r] = 0.f;
    const bool active = qbase < Nq;
    int ntiles = (Nk + KVT - 1) / KVT;
    if (causal) {                        // block-uniform, as in the forward
        const int qlast = min(blockIdx.x * QPB + QPB - 1, Nq - 1);
        ntiles = min(ntiles, qlast / KVT + 1);
    }

    constexpr bool TT = TRead<T, HD>::kNeedsTransposedTile;
    RowStage<T, HD> ks, vs;
    auto gload = [&](int kv0) {
        ks.load(kptr, ldk, kv0, Nk, hd, tid);
        vs.load(vptr, ldv, kv0, Nk, hd, tid);
    };
    gload(0);
    for (int j = 0; j < ntiles; ++j) {
        const int kv0 = j * KVT;
        __syncthreads();
        ks.store(Ks, tid);
        vs.store(Vs, tid);
        if (TT) store_transposed<HD>(ks, KTs, tid);
        __syncthreads();
        if (j + 1 < ntiles) gload((j + 1) * KVT);
        if (!active || (causal && kv0 > qbase + 31)) continue;
        f32x16 s[2], dp[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[u][r] = 0.f; dp[u][r] = 0.f; }
#pragma unroll
            for (int kk = 0; kk < C::NKK; ++kk) {
                s[u] = mma_chunk(rtile_chunk<T, HD>(Ks, 32 * u + l31, 2 * kk + h), qf[kk], s[u]);      // S^T[kv][q]
                dp[u] = mma_chunk(rtile_chunk<T, HD>(Vs, 32 * u + l31, 2 * kk + h), dof[kk], dp[u]);   // dP^T[kv][q]
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kv = kv0 + 32 * u + acc_row(r, h);
                const float p = qkv_visible(kv, qi, Nk, causal) ? __expf(s[u][r] * scale - lse_q) : 0.f;
                float dpm = dp[u][r];
                if (p_drop > 0.f) {
                    const uint64_t idx = (((uint64_t)b * H + head) * Nq + (uint64_t)qi) * (uint64_t)Nk + (uint64_t)kv;
                    dpm = u01_hash(seed, idx) >= p_drop ? dpm * (1.0f / (1.0f - p_drop)) : 0.f;
                }
                dp[u][r] = p * (dpm - del_q) * scale;          // dS^T
            }
#pragma unroll
        for (int c = 0; c < C::NPC; ++c) {
            const chunk_t dsb = pack_chunk((const T*)nullptr, dp, c);
#pragma unroll
            for (int db = 0; db < C::NDB; ++db)
                dq[db] = mma_chunk(TRead<T, HD>::chunk(KTs, Ks, db, c, lane), dsb, dq[db]);   // dQ^T[d][q]
        }
    }
    if (!active || !q_ok) return;
    T* dqrow = dq_out + ((int64_t)b * Nq + qi) * lddq + head * hd;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * db + 8 * g + 4 * h;
            if (d < hd)
                store_quad<T>(dqrow + d, f32x4{dq[db][4 * g], dq[db][4 * g + 1], dq[db][4 * g + 2], dq[db][4 * g + 3]});
        }
}

// ---- delta = dO . O
// delta[q] = sum_d dO[q,d] O[q,d]: the first pass of the tiled backward (N = query rows per batch item)
__global__ __launch_bounds__(256) void attn_delta_kernel(const void* __restrict__ o, int64_t ldo,
                                                         const void* __restrict__ dout, int64_t lddo, int dt,
                                                         float* __restrict__ delta, int N, int H, int hd, int64_t rows) {
    // one wave per (token row, head)
    const int lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= rows * H) return;
    const int64_t row = gw / H;
    const int head = (int)(gw % H);
    float s = 0.f;
    for (int d = lane; d < hd; d += 64)
        s += load1_as_f32(o, dt, row * ldo + head * hd + d) * load1_as_f32(dout, dt, row * lddo + head * hd + d);
    s = wave_sum(s);
    if (lane == 0) {
        const int64_t b = row / N, n = row % N;
        delta[(b * H + head) * N + n] = s;
    }
}

// vector path for bf16 with head_dim a power-of-two multiple of 8 (<= 512): one wave per token row, a lane owns 8
// consecutive channels (16-byte loads of O and dO), the head_dim/8 lanes of a head fold with xor-shuffles.
__global__ __launch_bounds__(256) void attn_delta_vec_kernel(const bf16_t* __restrict__ o, int64_t ldo,
                                                             const bf16_t* __restrict__ dout, int64_t lddo,
                                                             float* __restrict__ delta, int N, int H, int hd, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int C8 = (H * hd) / 8, lph = hd / 8;      // chunks per row, lanes per head
    const int64_t b = row / N, n = row % N;
    for (int c = lane; c < ((C8 + 63) / 64) * 64; c += 64) {
        float s = 0.f;
        if (c < C8) {
            const u32x4 ro = *reinterpret_cast<const u32x4*>(o + row * ldo + c * 8);
            const u32x4 rd = *reinterpret_cast<const u32x4*>(dout + row * lddo + c * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                s += __uint_as_float(ro[e] << 16) * __uint_as_float(rd[e] << 16) +
                     __uint_as_float(ro[e] & 0xffff0000u) * __uint_as_float(rd[e] & 0xffff0000u);
        }
        for (int off = 1; off < lph; off <<= 1) s += __shfl_xor(s, off, 64);
        if (c < C8 && (c % lph) == 0) delta[(b * H + c / lph) * N + n] = s;
    }
}

// ---- host
template <typename T, int HD> int launch_fwd(const me_attn_qkv_desc& d, hipStream_t stream) {
    typedef Cfg<T, HD> C;
    const size_t smem = C::R_BYTES + (C::T_BYTES > C::R_BYTES ? C::T_BYTES : C::R_BYTES);   // V tile: transposed (fp32) or row-major (bf16)
    return attn_launch<attn_qkv_fwd_kernel<T, HD>>("attention tiled fwd", dim3((d.Nq + QPB - 1) / QPB, d.H, d.B), AT_THREADS, smem, smem, stream,
                                                   (const T*)d.q, d.ld_q, (const T*)d.k, d.ld_k, (const T*)d.v, d.ld_v, (T*)d.out, d.ld_out, d.lse,
                                                   d.Nq, d.Nk, d.H, d.head_dim, d.scale, d.causal, d.p_drop, d.seed);
}
template <typename T, int HD> int launch_bwd(const me_attn_qkv_desc& d, hipStream_t stream) {
    typedef Cfg<T, HD> C;
    constexpr size_t TB = TRead<T, HD>::kNeedsTransposedTile ? C::T_BYTES : 0;
    const size_t smem1 = 2 * C::R_BYTES + 2 * TB + 2 * KVT * sizeof(float);
    const size_t smem2 = 2 * C::R_BYTES + TB;
    const dim3 gridk((d.Nk + QPB - 1) / QPB, d.H, d.B);
    auto dkdv = [&](auto DB0, auto NDBO) {
        return attn_launch<attn_qkv_bwd_dkdv_kernel<T, HD, DB0(), NDBO()>>("attention tiled bwd (dkdv)", gridk, AT_THREADS, smem1, smem1, stream,
                                                                           (const T*)d.q, d.ld_q, (const T*)d.k, d.ld_k, (const T*)d.v, d.ld_v,
                                                                           (const T*)d.dout, d.ld_dout, d.lse, d.delta, (T*)d.dk, d.ld_dk, (T*)d.dv,
                                                                           d.ld_dv, d.Nq, d.Nk, d.H, d.head_dim, d.scale, d.causal, d.p_drop, d.seed);
    };
    // fp32 at head_dim > 64: two launches of two d blocks each, no scratch, S and dP formed in both -- against ONE launch of
    // attn_qkv_bwd_dkdv_kernel<float, 128, 0, 4> (440 bytes of scratch per lane), same bits.  NOT TIMED against each other: the rule
    // assumes that the launch without scratch traffic is no slower.  Both entry points take it.
    if constexpr (sizeof(T) == 4 && HD == 128) {
        if (int rc = dkdv(Int<0>(), Int<2>())) return rc;
        if (d.head_dim > 64)
            if (int rc = dkdv(Int<2>(), Int<2>())) return rc;
    } else {
        if (int rc = dkdv(Int<0>(), Int<C::NDB>())) return rc;
    }
    return attn_launch<attn_qkv_bwd_dq_kernel<T, HD>>("attention tiled bwd (dq)", dim3((d.Nq + QPB - 1) / QPB, d.H, d.B), AT_THREADS, smem2, smem2, stream,
                                                      (const T*)d.q, d.ld_q, (const T*)d.k, d.ld_k, (const T*)d.v, d.ld_v, (const T*)d.dout, d.ld_dout,
                                                      d.lse, d.delta, (T*)d.dq, d.ld_dq, d.Nq, d.Nk, d.H, d.head_dim, d.scale, d.causal, d.p_drop, d.seed);
}
// bf16 delta of me_attention_qkv_bwd: from the tiles (attn_qkv_delta_kernel, which says why)
template <int HD> int launch_qkv_delta_bf16(const me_attn_qkv_desc& d, hipStream_t stream) {
    typedef bf16_t T;
    constexpr size_t smem = 2 * Cfg<T, HD>::R_BYTES;
    return attn_launch<attn_qkv_delta_kernel<T, HD>>("me_attention_qkv_bwd(delta)", dim3((d.Nq + QPB - 1) / QPB, d.H, d.B), AT_THREADS, smem, smem, stream,
                                                     (const T*)d.q, d.ld_q, (const T*)d.k, d.ld_k, (const T*)d.v, d.ld_v, (const T*)d.dout, d.ld_dout,
                                                     d.lse, d.delta, d.Nq, d.Nk, d.H, d.head_dim, d.scale, d.causal, d.p_drop, d.seed);
}

// f(Int<HD>) for the instantiated head width
template <typename F> int qkv_by_hd(int hd, F f) {
    if (hd <= 32) return f(Int<32>());
    return hd <= 64 ? f(Int<64>()) : f(Int<128>());
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_qkv_desc(const char* fn, const me_attn_qkv_desc* d, bool backward) {
    ME_CHECK_ARG(d, "%s: null descriptor", fn);
    ME_CHECK_ARG(d->q && d->k && d->v && d->out, "%s: null pointer", fn);
    if (backward) ME_CHECK_ARG(d->dout && d->lse && d->delta && d->dq && d->dk && d->dv, "%s: null pointer", fn);
    ME_CHECK_ARG(me_dtype_ok(d->dtype), "%s: bad dtype", fn);
    ME_CHECK_ARG(d->B > 0 && d->Nq > 0 && d->Nk > 0 && d->H > 0 && d->head_dim > 0, "%s: bad shape B=%d Nq=%d Nk=%d H=%d hd=%d", fn, d->B, d->Nq,
                 d->Nk, d->H, d->head_dim);
    ME_CHECK_ARG(!d->causal || d->Nq == d->Nk, "%s: causal needs Nq == Nk (got %d, %d)", fn, d->Nq, d->Nk);
    const int E = d->dtype == ME_BF16 ? 8 : 4;
    ME_CHECK_ARG(d->head_dim % E == 0, "%s: head_dim=%d must be a multiple of %d", fn, d->head_dim, E);
    ME_CHECK_ARG(d->head_dim <= 128, "%s: head_dim=%d > 128 unsupported", fn, d->head_dim);
    ME_CHECK_ARG(d->B <= 65535 && d->H <= 65535, "%s: B and H must be <= 65535", fn);
    const int64_t C = (int64_t)d->H * d->head_dim;
    ME_CHECK_ARG(d->ld_q % E == 0 && d->ld_k % E == 0 && d->ld_v % E == 0, "%s: ld_q, ld_k, ld_v must be multiples of %d elements", fn, E);
    ME_CHECK_ARG(d->ld_out % 4 == 0, "%s: ld_out must be a multiple of 4", fn);
    ME_CHECK_ARG(d->ld_q >= C && d->ld_k >= C && d->ld_v >= C && d->ld_out >= C, "%s: a row stride is smaller than H * head_dim", fn);
    ME_CHECK_ARG(aligned16(d->q) && aligned16(d->k) && aligned16(d->v) && aligned16(d->out), "%s: operands must be 16-byte aligned", fn);
    ME_CHECK_ARG(d->p_drop >= 0.f && d->p_drop < 1.f, "%s: p_drop must be in [0, 1)", fn);
    if (backward) {
        ME_CHECK_ARG(d->ld_dout % E == 0 && d->ld_dq % 4 == 0 && d->ld_dk % 4 == 0 && d->ld_dv % 4 == 0, "%s: bad gradient strides", fn);
        ME_CHECK_ARG(d->ld_dout >= C && d->ld_dq >= C && d->ld_dk >= C && d->ld_dv >= C, "%s: a gradient row stride is smaller than H * head_dim", fn);
        ME_CHECK_ARG(aligned16(d->dout) && aligned16(d->dq) && aligned16(d->dk) && aligned16(d->dv), "%s: gradients must be 16-byte aligned", fn);
    }
    return ME_OK;
}

}  // namespace

int launch_attn_tiled_fwd(const me_attn_qkv_desc& d, hipStream_t stream) {
    if (d.dtype == ME_BF16) return qkv_by_hd(d.head_dim, [&](auto HD) { return launch_fwd<bf16_t, HD()>(d, stream); });
    return qkv_by_hd(d.head_dim, [&](auto HD) { return launch_fwd<float, HD()>(d, stream); });
}

int launch_attn_tiled_bwd(const me_attn_qkv_desc& d, hipStream_t stream) {
    if (d.dtype == ME_BF16) return qkv_by_hd(d.head_dim, [&](auto HD) { return launch_bwd<bf16_t, HD()>(d, stream); });
    return qkv_by_hd(d.head_dim, [&](auto HD) { return launch_bwd<float, HD()>(d, stream); });
}

int launch_attn_delta(const void* out, int64_t ldo, const void* dout, int64_t lddo, int dtype, float* delta, int B, int N, int H, int hd,
                      hipStream_t stream) {
    const int64_t rows = (int64_t)B * N;
    const int64_t nw = rows * H;
    const int lph = hd / 8;
    if (dtype == ME_BF16 && hd % 8 == 0 && (lph & (lph - 1)) == 0 && lph <= 64 && ldo % 8 == 0 && lddo % 8 == 0) {
        hipLaunchKernelGGL(attn_delta_vec_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)out, ldo, (const bf16_t*)dout,
                           lddo, delta, N, H, hd, rows);
    } else {
        hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, stream, out, ldo, dout, lddo, dtype, delta, N, H, hd, rows);
    }
    ME_CHECK_LAUNCH("attention delta");
    return ME_OK;
}

extern "C" int me_attention_qkv_fwd(const me_attn_qkv_desc* d, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (int rc = check_qkv_desc("me_attention_qkv_fwd", d, false)) return rc;
    ProfScope prof(ME_PROF_ATTN_FWD, d->dtype, (int64_t)d->B * d->H, d->Nq, d->head_dim, stream);
    prof.plan = ME_ATTN_QKV;
    return launch_attn_tiled_fwd(*d, stream);
}

extern "C" int me_attention_qkv_bwd(const me_attn_qkv_desc* d, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (int rc = check_qkv_desc("me_attention_qkv_bwd", d, true)) return rc;
    ProfScope prof(ME_PROF_ATTN_BWD, d->dtype, (int64_t)d->B * d->H, d->Nq, d->head_dim, stream);
    prof.plan = ME_ATTN_QKV;
    // delta pass: fp32 -> dO . O; bf16 -> from the tiles
    if (int rc = d->dtype == ME_BF16 ? qkv_by_hd(d->head_dim, [&](auto HD) { return launch_qkv_delta_bf16<HD()>(*d, stream); })
                                     : launch_attn_delta(d->out, d->ld_out, d->dout, d->ld_dout, d->dtype, d->delta, d->B, d->Nq, d->H, d->head_dim, stream))
        return rc;
    return launch_attn_tiled_bwd(*d, stream);
}
