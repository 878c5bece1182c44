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
// Backward: a delta pass chosen by the entry point (dO . O, or from the tiles: qrows_bwd says when), dK / dV (a wave owns
// 32 keys, walks query tiles), dQ (a wave owns 32 queries, walks key tiles).  No atomics, every output element is written exactly
// once, two runs are bit-identical.
#include "attention_host.h"
#include "attention_tile.h"
#include <stdint.h>

namespace {

// fp32: the transposed [HD][64] copy of a tile written from the registers of its row-major stage (TRead<float> reads its operand from
// it; bf16 reads the row tile with tr).  So a tile that is needed both ways is staged once and stored twice instead of loaded twice (a
// second register set for the transposed copy is what no longer fits beside the accumulators at HD 128).
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

// =====================================================================================================
// The per-wave pieces of the four kernels.  A block is (128-row block x, head y, batch z), wave w owns rows [128 x + 32 w, + 32) of one
// side (queries: forward, delta, dQ; keys: dK / dV), lane l31 one of them, and the other side walks by in 64-row LDS tiles.  With
// acc_zero, row_frags_load and acc_store_row(_pair) of attention_tile.h each of these is written once.
// =====================================================================================================

// row `row` of batch item b, head `head` in a [B*N, ld] operand
template <typename P> __device__ __forceinline__ P head_rows(P p, int64_t ld, int b, int N, int head, int hd, int row = 0) {
    return p + ((int64_t)b * N + row) * ld + head * hd;
}

// The score matrix of one (batch, head): which entries exist, what the backward recomputes of them, and their dropout stream
struct Scores {
    int Nq, Nk, causal;
    float scale, p_drop, keep;      // keep = 1 / (1 - p_drop)
    uint64_t seed, bh;              // bh = b * H + head
    // key kv is visible to query q
    __device__ __forceinline__ bool visible(int kv, int q) const { return kv < Nk && (!causal || kv <= q); }
    // P[q][kv] from the raw score and the row's lse; 0 where the key is masked
    __device__ __forceinline__ float prob(float s, float lse, int kv, int q) const { return visible(kv, q) ? __expf(s * scale - lse) : 0.f; }
    // x at probability (q, kv) after dropout: the stream is indexed ((b*H + h)*Nq + q)*Nk + kv = drop_row(q) + kv, what is kept is
    // scaled by `keep`
    __device__ __forceinline__ uint64_t drop_row(int q) const { return (bh * (uint64_t)Nq + (uint64_t)q) * (uint64_t)Nk; }
    __device__ __forceinline__ float dropped(float x, uint64_t row, int kv) const {
        return u01_hash(seed, row + (uint64_t)kv) >= p_drop ? x * keep : 0.f;
    }
    // P and dS of register r of a sub-tile from lse / delta under the mask and the dropout stream: s[r] (raw score) becomes the dropped
    // P, which dV consumes, and dp[r] (dP) becomes dS = P (dropped dP - delta) scale -- the forward's mask on both
    __device__ __forceinline__ void p_ds(f32x16& s, f32x16& dp, int r, float lse, float delta, int kv, int q) const {
        const float p = prob(s[r], lse, kv, q);
        float pm = p, dpm = dp[r];
        if (p_drop > 0.f) { pm = dropped(p, drop_row(q), kv); dpm = dropped(dpm, drop_row(q), kv); }
        s[r] = pm;
        dp[r] = p * (dpm - delta) * scale;
    }
};
__device__ __forceinline__ Scores scores_of(const me_attn_qkv_desc& d, int b, int head) {
    return Scores{d.Nq, d.Nk, d.causal, d.scale, d.p_drop, 1.0f / (1.0f - d.p_drop), d.seed, (uint64_t)b * d.H + head};
}

// 64-key tiles a block of queries walks.  causal: tiles that start beyond the block's last query are all masked (block-uniform)
__device__ __forceinline__ int key_tiles(int Nq, int Nk, int causal) {
    int ntiles = (Nk + KVT - 1) / KVT;
    if (causal) {
        const int qlast = min(blockIdx.x * QPB + QPB - 1, Nq - 1);
        ntiles = min(ntiles, qlast / KVT + 1);
    }
    return ntiles;
}

// The walk over tiles j0 .. ntiles - 1 of the other side.  load(r0) fetches the tile that starts at row r0 into registers, park() writes
// the fetched tile to LDS, use(j) is the wave's work on tile j; it returns at once where no row of the wave sees the tile (a
// wave-uniform test, after the barriers and the prefetch).  The next tile's global loads fly during this tile's MFMAs.
// The three are lambdas of the kernel marked INLINED: they become part of the kernel before anything is optimised, as if written in
// the loop (left to the inliner they are optimised on their own first, with every captured value unknown).
#define INLINED __attribute__((always_inline))
template <typename Load, typename Park, typename Use>
__device__ __forceinline__ void walk_tiles(int j0, int ntiles, Load load, Park park, Use use) {
    load(j0 * KVT);
    for (int j = j0; j < ntiles; ++j) {
        __syncthreads();
        park();
        __syncthreads();
        if (j + 1 < ntiles) load((j + 1) * KVT);
        use(j);
    }
}

// Rows [32 u, 32 u + 32) of a row-major LDS tile times the lane's row fragments.  For a wave that owns queries that is S^T = K Q^T or
// dP^T = V dO^T of the sub-tile, for one that owns keys S = Q K^T or dP = dO V^T.  -> lane: the wave's row, register r: tile row
// 32 u + acc_row(r, h)
template <typename T, int HD>
__device__ __forceinline__ f32x16 subtile_product(const char* tile, int u, int lane, const typename Chunk<T>::type (&f)[Cfg<T, HD>::NKK]) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < Cfg<T, HD>::NKK; ++kk)
        acc = mma_chunk(rtile_chunk<T, HD>(tile, 32 * u + (lane & 31), 2 * kk + (lane >> 5)), f[kk], acc);
    return acc;
}

// =====================================================================================================
// forward
// =====================================================================================================
template <typename T, int HD> __global__ __launch_bounds__(AT_THREADS) void attn_qkv_fwd_kernel(const me_attn_qkv_desc d) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool TT = TRead<T, HD>::kNeedsTransposedTile;
    char* Ks = smem;
    char* Vs = smem + C::R_BYTES;              // fp32: transposed [HD][64]; bf16: row-major [64][HD] (read with tr)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int Nq = d.Nq, Nk = d.Nk, hd = d.head_dim;
    const int qbase = blockIdx.x * QPB + wave * 32;
    const Scores sc = scores_of(d, b, head);
    const T* kptr = head_rows((const T*)d.k, d.ld_k, b, Nk, head, hd);
    const T* vptr = head_rows((const T*)d.v, d.ld_v, b, Nk, head, hd);

    chunk_t qf[C::NKK];      // out-of-range rows read the last row and are never stored
    row_frags_load<HD>(head_rows((const T*)d.q, d.ld_q, b, Nq, head, hd) + (int64_t)min(qbase + l31, Nq - 1) * d.ld_q, hd, h, qf);
    f32x16 o[C::NDB];
    acc_zero(o);
    float m_run = -INFINITY, l_run = 0.f;
    const bool active = qbase < Nq;      // wave-uniform
    const int qi = qbase + l31;          // this lane's query (unclamped: a row past Nq only sees more keys)

    RowStage<T, HD> ks, vs;
    walk_tiles(
        0, key_tiles(Nq, Nk, d.causal),
        [&](int kv0) INLINED {
            ks.load(kptr, d.ld_k, kv0, Nk, hd, tid);
            vs.load(vptr, d.ld_v, kv0, Nk, hd, tid);
        },
        [&]() INLINED {
            ks.store(Ks, tid);
            if constexpr (TT) store_transposed<HD>(vs, Vs, tid); else vs.store(Vs, tid);
        },
        [&](int j) INLINED {
            const int kv0 = j * KVT;
            if (!active || (d.causal && kv0 > qbase + 31)) return;      // wave-uniform: no row of this wave sees the tile
            f32x16 s[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) s[u] = subtile_product<T, HD>(Ks, u, lane, qf);
            float mt = -INFINITY;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = sc.visible(kv0 + 32 * u + acc_row(r, h), qi) ? s[u][r] * sc.scale : -INFINITY;
                    s[u][r] = sv;
                    mt = fmaxf(mt, sv);
                }
            // One lane holds half of the tile's keys, and on a tile the diagonal crosses all of them may be masked: mt = -inf here.  After
            // the fold with the partner lane it is finite on EVERY tile that gets this far: kv0 < Nk always, and under `causal` kv0 and
            // qbase are multiples of 32 with kv0 <= qbase + 31, hence kv0 <= qbase <= qi -- key kv0 is visible to every row of the wave.
            // So m_new is finite, exp(-inf - m_new) = 0 for the masked entries, and m_run - m_new is -inf - finite (alpha = 0) on the first
            // processed tile (tile 0: it is never skipped) and finite - finite afterwards: -inf - (-inf) cannot occur.
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
            if (sc.p_drop > 0.f) {      // FullAttention's dropout acts on the NORMALISED probabilities -- the row sum stays unmasked
                const uint64_t row = sc.drop_row(qi);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[u][r] = sc.dropped(s[u][r], row, kv0 + 32 * u + acc_row(r, h));
            }
#pragma unroll
            for (int db = 0; db < C::NDB; ++db) o[db] *= alpha;
#pragma unroll
            for (int c = 0; c < C::NPC; ++c) {
                const chunk_t pb = pack_chunk((const T*)nullptr, s, c);
#pragma unroll
                for (int db = 0; db < C::NDB; ++db) o[db] = mma_chunk(TRead<T, HD>::chunk(Vs, Vs, db, c, lane), pb, o[db]);
            }
        });
    if (!active) return;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (qi < Nq) {
        acc_store_row(head_rows((T*)d.out, d.ld_out, b, Nq, head, hd, qi), o, 1.0f / l_tot, hd, h);
        if (d.lse && h == 0) d.lse[(int64_t)sc.bh * Nq + qi] = m_run + __logf(l_tot);
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
__global__ __launch_bounds__(AT_THREADS) void attn_qkv_bwd_dkdv_kernel(const me_attn_qkv_desc d) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool TT = TRead<T, HD>::kNeedsTransposedTile;
    constexpr int TB = TT ? C::T_BYTES : 0;      // bf16 reads the row tiles transposed (tr)
    char* Qs = smem;                           // [64 q][HD]
    char* dOs = Qs + C::R_BYTES;               // [64 q][HD]
    char* QTs = dOs + C::R_BYTES;              // [HD][64 q]   (fp32 only)
    char* dOTs = QTs + TB;                     // [HD][64 q]   (fp32 only)
    float* lse_s = reinterpret_cast<float*>(dOTs + TB);           // [64]
    float* del_s = lse_s + KVT;                                   // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int Nq = d.Nq, Nk = d.Nk, hd = d.head_dim;
    const int kblock = blockIdx.x;
    const int kvbase = kblock * QPB + wave * 32;
    const Scores sc = scores_of(d, b, head);
    const T* qptr = head_rows((const T*)d.q, d.ld_q, b, Nq, head, hd);
    const T* doptr = head_rows((const T*)d.dout, d.ld_dout, b, Nq, head, hd);
    const float* lse_bh = d.lse + (int64_t)sc.bh * Nq;
    const float* del_bh = d.delta + (int64_t)sc.bh * Nq;

    chunk_t kf[C::NKK], vf[C::NKK];
    const int kvrow = min(kvbase + l31, Nk - 1);
    row_frags_load<HD>(head_rows((const T*)d.k, d.ld_k, b, Nk, head, hd) + (int64_t)kvrow * d.ld_k, hd, h, kf);
    row_frags_load<HD>(head_rows((const T*)d.v, d.ld_v, b, Nk, head, hd) + (int64_t)kvrow * d.ld_v, hd, h, vf);
    f32x16 dk[NDBO], dv[NDBO];
    acc_zero(dk);
    acc_zero(dv);
    const bool active = kvbase < Nk;
    const int kvi = kvbase + l31;
    // causal (Nq == Nk): query tiles that end before the block's first key see none of its keys.  Block-uniform; kblock * QPB < Nk = Nq,
    // so j0 < ntiles and the first staged tile exists.
    const int j0 = d.causal ? (kblock * QPB) / KVT : 0;

    RowStage<T, HD> qs, dos;
    float lse_r = INFINITY, del_r = 0.f;
    walk_tiles(
        j0, (Nq + KVT - 1) / KVT,
        [&](int q0) INLINED {
            qs.load(qptr, d.ld_q, q0, Nq, hd, tid);
            dos.load(doptr, d.ld_dout, q0, Nq, hd, tid);
            if (tid < KVT) {
                const int qq = q0 + tid;
                lse_r = (qq < Nq) ? lse_bh[qq] : INFINITY;          // exp(s - inf) = 0 masks padded queries
                del_r = (qq < Nq) ? del_bh[qq] : 0.f;
            }
        },
        [&]() INLINED {
            qs.store(Qs, tid);
            dos.store(dOs, tid);
            if constexpr (TT) {
                store_transposed<HD>(qs, QTs, tid);
                store_transposed<HD>(dos, dOTs, tid);
            }
            if (tid < KVT) {
                lse_s[tid] = lse_r;
                del_s[tid] = del_r;
            }
        },
        [&](int j) INLINED {
            if (!active || (d.causal && j * KVT + KVT - 1 < kvbase)) return;      // wave-uniform: the tile's last query precedes the wave's first key
            f32x16 s[2], dp[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                s[u] = subtile_product<T, HD>(Qs, u, lane, kf);         // S[q][kv]
                dp[u] = subtile_product<T, HD>(dOs, u, lane, vf);       // dP[q][kv]
                // lane: kv = l31 (fixed), regs: q = 32u + acc_row(r,h)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 L = *reinterpret_cast<const f32x4*>(lse_s + 32 * u + 8 * g + 4 * h);
                    const f32x4 D = *reinterpret_cast<const f32x4*>(del_s + 32 * u + 8 * g + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        sc.p_ds(s[u], dp[u], 4 * g + e, L[e], D[e], kvi, j * KVT + 32 * u + acc_row(4 * g + e, h));
                }
                // this 32-query half goes into dV / dK before the other half's S and dP are formed (chunks still in ascending order, with
                // half the S / dP registers live)
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
        });
    if (!active || kvi >= Nk) return;
    acc_store_row_pair<DB0>(head_rows((T*)d.dk, d.ld_dk, b, Nk, head, hd, kvi), dk, 1.0f,
                            head_rows((T*)d.dv, d.ld_dv, b, Nk, head, hd, kvi), dv, 1.0f, hd, h);
}

// ---- dQ, and delta for bf16: a wave owns 32 queries and walks the 64-key tiles they see, recomputing S^T and dP^T.  Two consumers:
//   dQ (DELTA false): dS^T from lse / delta, dQ^T += K^T dS^T.
//   delta (DELTA true): delta[q] = sum_k P~[q,k] dP[q,k] (P~: the dropped probabilities) from the tiles, in fp32.  In exact arithmetic this is
//   dO . O, which is how the fp32 path (and me_attention_bwd) forms it; in bf16 that O is the rounded output of a forward that rounded P
//   too, and in the first rows of a causal call, where a few keys carry large probabilities, the error reaches dS undamped (measured: dQ
//   off by 0.5 % of max|dQ| at N = 129, head_dim 96).  Formed here, dS sums to zero over the keys as it should.
template <typename T, int HD, bool DELTA> __device__ __forceinline__ void qrows_bwd(const me_attn_qkv_desc& d) {
    typedef Cfg<T, HD> C;
    typedef typename Chunk<T>::type chunk_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool TT = !DELTA && TRead<T, HD>::kNeedsTransposedTile;
    char* Ks = smem;                    // [64 kv][HD]
    char* Vs = Ks + C::R_BYTES;         // [64 kv][HD]
    char* KTs = Vs + C::R_BYTES;        // [HD][64 kv]   (dQ, fp32 only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int Nq = d.Nq, Nk = d.Nk, hd = d.head_dim;
    const int qbase = blockIdx.x * QPB + wave * 32;
    const Scores sc = scores_of(d, b, head);
    const T* kptr = head_rows((const T*)d.k, d.ld_k, b, Nk, head, hd);
    const T* vptr = head_rows((const T*)d.v, d.ld_v, b, Nk, head, hd);

    const int qi = qbase + l31;
    const bool q_ok = qi < Nq;
    const int qrow = q_ok ? qi : Nq - 1;
    chunk_t qf[C::NKK], dof[C::NKK];
    row_frags_load<HD>(head_rows((const T*)d.q, d.ld_q, b, Nq, head, hd) + (int64_t)qrow * d.ld_q, hd, h, qf);
    row_frags_load<HD>(head_rows((const T*)d.dout, d.ld_dout, b, Nq, head, hd) + (int64_t)qrow * d.ld_dout, hd, h, dof);
    const float lse_q = d.lse[(int64_t)sc.bh * Nq + qrow];
    const float del_q = DELTA ? 0.f : d.delta[(int64_t)sc.bh * Nq + qrow];
    f32x16 dq[DELTA ? 1 : C::NDB];
    acc_zero(dq);
    float acc = 0.f;
    const bool active = qbase < Nq;

    RowStage<T, HD> ks, vs;
    walk_tiles(
        0, key_tiles(Nq, Nk, d.causal),
        [&](int kv0) INLINED {
            ks.load(kptr, d.ld_k, kv0, Nk, hd, tid);
            vs.load(vptr, d.ld_v, kv0, Nk, hd, tid);
        },
        [&]() INLINED {
            ks.store(Ks, tid);
            vs.store(Vs, tid);
            if constexpr (TT) store_transposed<HD>(ks, KTs, tid);
        },
        [&](int j) INLINED {
            const int kv0 = j * KVT;
            if (!active || (d.causal && kv0 > qbase + 31)) return;      // wave-uniform: no row of this wave sees the tile
            f32x16 s[2], dp[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                s[u] = subtile_product<T, HD>(Ks, u, lane, qf);         // S^T[kv][q]
                dp[u] = subtile_product<T, HD>(Vs, u, lane, dof);       // dP^T[kv][q]
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = kv0 + 32 * u + acc_row(r, h);
                    if constexpr (DELTA) {
                        const float p = sc.prob(s[u][r], lse_q, kv, qi);
                        acc += p * (sc.p_drop > 0.f ? sc.dropped(dp[u][r], sc.drop_row(qi), kv) : dp[u][r]);
                    } else {
                        sc.p_ds(s[u], dp[u], r, lse_q, del_q, kv, qi);      // dp: dS^T
                    }
                }
            }
            if constexpr (!DELTA) {
#pragma unroll
                for (int c = 0; c < C::NPC; ++c) {
                    const chunk_t dsb = pack_chunk((const T*)nullptr, dp, c);
#pragma unroll
                    for (int db = 0; db < C::NDB; ++db) dq[db] = mma_chunk(TRead<T, HD>::chunk(KTs, Ks, db, c, lane), dsb, dq[db]);   // dQ^T[d][q]
                }
            }
        });
    if (!active) return;
    if constexpr (DELTA) {
        acc += __shfl_xor(acc, 32, 64);
        if (q_ok && h == 0) d.delta[(int64_t)sc.bh * Nq + qi] = acc;
    } else {
        if (q_ok) acc_store_row(head_rows((T*)d.dq, d.ld_dq, b, Nq, head, hd, qi), dq, 1.0f, hd, h);
    }
}
template <typename T, int HD> __global__ __launch_bounds__(AT_THREADS) void attn_qkv_delta_kernel(const me_attn_qkv_desc d) {
    qrows_bwd<T, HD, true>(d);
}
template <typename T, int HD> __global__ __launch_bounds__(AT_THREADS) void attn_qkv_bwd_dq_kernel(const me_attn_qkv_desc d) {
    qrows_bwd<T, HD, false>(d);
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

// ---- host: every kernel takes the checked descriptor by value
// blocks of 128 rows x heads x batch items
dim3 row_blocks(int N, const me_attn_qkv_desc& d) { return dim3((N + QPB - 1) / QPB, d.H, d.B); }

template <typename T, int HD> int launch_fwd(const me_attn_qkv_desc& d, hipStream_t stream) {
    typedef Cfg<T, HD> C;
    const size_t smem = C::R_BYTES + (C::T_BYTES > C::R_BYTES ? C::T_BYTES : C::R_BYTES);   // V tile: transposed (fp32) or row-major (bf16)
    return launch_kernel<attn_qkv_fwd_kernel<T, HD>>("attention tiled fwd", row_blocks(d.Nq, d), AT_THREADS, smem, smem, stream, d);
}
template <typename T, int HD> int launch_bwd(const me_attn_qkv_desc& d, hipStream_t stream) {
    typedef Cfg<T, HD> C;
    constexpr size_t TB = TRead<T, HD>::kNeedsTransposedTile ? C::T_BYTES : 0;
    const size_t smem1 = 2 * C::R_BYTES + 2 * TB + 2 * KVT * sizeof(float);
    const size_t smem2 = 2 * C::R_BYTES + TB;
    auto dkdv = [&](auto DB0, auto NDBO) {
        return launch_kernel<attn_qkv_bwd_dkdv_kernel<T, HD, DB0(), NDBO()>>("attention tiled bwd (dkdv)", row_blocks(d.Nk, d), AT_THREADS, smem1, smem1,
                                                                           stream, d);
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
    return launch_kernel<attn_qkv_bwd_dq_kernel<T, HD>>("attention tiled bwd (dq)", row_blocks(d.Nq, d), AT_THREADS, smem2, smem2, stream, d);
}
// bf16 delta of me_attention_qkv_bwd: from the tiles (qrows_bwd, which says why)
template <int HD> int launch_qkv_delta_bf16(const me_attn_qkv_desc& d, hipStream_t stream) {
    constexpr size_t smem = 2 * Cfg<bf16_t, HD>::R_BYTES;
    return launch_kernel<attn_qkv_delta_kernel<bf16_t, HD>>("me_attention_qkv_bwd(delta)", row_blocks(d.Nq, d), AT_THREADS, smem, smem, stream, d);
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
