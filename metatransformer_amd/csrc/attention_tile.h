// attention_tile.h -- device pieces shared by the tiled attention kernels of attention_qkv.hip and the sequence-resident kernels of
// attention.hip: tile geometry, global -> LDS staging, MFMA operand reads.  Device code only.  Included inside no namespace;
// everything here has internal linkage.
// Both families (the four tiled kernels and the 32-row kernels, rows32_* of attention.hip) use Cfg, zero4, rtile_chunk, tr_chunk,
// pack_chunk and the per-lane pieces at the end: acc_zero, row_frags_load, acc_store_row / acc_store_row_pair (on store_quad).  RowStage,
// TRead and the fp32 ttile_chunk serve the tiled kernels alone (the 32-row kernels are bf16 and stage through Rows32Stage).
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int AT_THREADS = 256;
constexpr int KVT = 64;      // keys per LDS tile
constexpr int QPB = 128;     // queries per block (32 per wave)

template <typename T, int HD> struct Cfg {
    static constexpr int E = 16 / sizeof(T);
    static constexpr int CPR = HD / E;                       // 16-byte chunks per row along d
    static constexpr int NKK = HD / (2 * E);                 // chunk pairs along d
    static constexpr int NDB = HD / 32;                      // 32-wide d blocks
    static constexpr int RROW = HD * sizeof(T) + 16;         // row-major tile row stride (bytes), conflict-free pad
    static constexpr int TROW = KVT * sizeof(T) + (sizeof(T) == 2 ? 8 : 16);   // transposed tile row stride
    static constexpr int R_BYTES = KVT * RROW;               // [64][HD] row-major tile
    static constexpr int T_BYTES = HD * TROW;                // [HD][64] transposed tile
    static constexpr int NPC = KVT / (2 * E);                // P chunks per 64-key tile (4 bf16 / 8 fp32)
    static constexpr int R_ITEMS = (KVT * CPR + AT_THREADS - 1) / AT_THREADS;
};

__device__ __forceinline__ u32x4 zero4() { return u32x4{0u, 0u, 0u, 0u}; }

// ---- row-major [64][HD] tile: global -> regs -> LDS
template <typename T, int HD> struct RowStage {
    typedef Cfg<T, HD> C;
    u32x4 v[C::R_ITEMS];
    __device__ __forceinline__ void load(const T* __restrict__ base, int64_t ld, int r0, int nrows, int hd, int tid) {
#pragma unroll
        for (int i = 0; i < C::R_ITEMS; ++i) {
            const int it = tid + AT_THREADS * i;
            const int chunk = it % C::CPR, row = it / C::CPR;
            const bool ok = (row < KVT) && (r0 + row < nrows) && (chunk * C::E < hd);
            v[i] = ok ? *reinterpret_cast<const u32x4*>(base + (int64_t)(r0 + row) * ld + chunk * C::E) : zero4();
        }
    }
    __device__ __forceinline__ void store(char* lds, int tid) const {
#pragma unroll
        for (int i = 0; i < C::R_ITEMS; ++i) {
            const int it = tid + AT_THREADS * i;
            const int chunk = it % C::CPR, row = it / C::CPR;
            if (row < KVT) *reinterpret_cast<u32x4*>(lds + row * C::RROW + chunk * 16) = v[i];
        }
    }
};

// A-operand chunk from a row-major tile: row, d-chunk index (2*kk + h)
template <typename T, int HD>
__device__ __forceinline__ typename Chunk<T>::type rtile_chunk(const char* lds, int row, int chunk) {
    return *reinterpret_cast<const typename Chunk<T>::type*>(lds + row * Cfg<T, HD>::RROW + chunk * 16);
}
// fp32 A-operand chunk from a transposed [HD][64] tile: row d, P-chunk c (0..NPC-1) of the 64-wide tile, half h.
// Element e of the chunk is reduction index 8c + 4h + e within the 64-tile, which is exactly the index that accumulator register
// (4*(c % 4) + e) of 32-subtile u = c / 4 holds in half h (acc_row), so S/P registers feed the next MFMA without any cross-lane
// movement.  (bf16, tr_chunk below: 16c + 4h + (e&3) + 8(e>>2), registers 8*(c % 2) + e of u = c / 2.)
template <int HD>
__device__ __forceinline__ f32x4 ttile_chunk(const float*, const char* lds, int d, int c, int h) {
    return *reinterpret_cast<const f32x4*>(lds + d * Cfg<float, HD>::TROW + (8 * c + 4 * h) * 4);
}
// bf16: the same operand straight from a ROW-MAJOR [64][HD] tile with the LDS transpose read (ds_read_b64_tr_b16),
// no transposed staging at all.  A 16-lane group reads four reduction rows x 16 columns; lane p of the group supplies
// the address of row +(p>>2), columns +4*(p&3) and receives column +p of the four rows (tools/probe_isa.hip).  Rows are
// picked so that element e = 4r + j of half h is reduction index 16c + 8r + 4h + j == the accumulator-register mapping
// above, so P / dS registers still feed the MFMA unchanged.
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;
template <int HD>
__device__ __forceinline__ bf16x8 tr_chunk(const char* tile, int dbase, int c, int lane) {
    const int g = lane >> 4, p = lane & 15, h = g >> 1;
    const int col = dbase + 16 * (g & 1) + 4 * (p & 3);
    const uint32_t base = (uint32_t)(uintptr_t)tile + col * 2;
    union { bf16x4 q[2]; bf16x8 v; } u;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 16 * c + 8 * r + 4 * h + (p >> 2);
        u.q[r] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(base + row * Cfg<bf16_t, HD>::RROW));
    }
    return u.v;
}
// "operand with the reduction index along the tile rows": fp32 -> transposed tile + 16-byte reads, bf16 -> row tile + tr reads
template <typename T, int HD> struct TRead;
template <int HD> struct TRead<float, HD> {
    static constexpr bool kNeedsTransposedTile = true;
    static __device__ __forceinline__ f32x4 chunk(const char* ttile, const char*, int db, int c, int lane) {
        return ttile_chunk<HD>((const float*)nullptr, ttile, 32 * db + (lane & 31), c, lane >> 5);
    }
};
template <int HD> struct TRead<bf16_t, HD> {
    static constexpr bool kNeedsTransposedTile = false;
    static __device__ __forceinline__ bf16x8 chunk(const char*, const char* rtile, int db, int c, int lane) {
        return tr_chunk<HD>(rtile, 32 * db, c, lane);
    }
};

// B-operand chunk c from the two 32x32 accumulators of a 64-wide tile
__device__ __forceinline__ bf16x8 pack_chunk(const bf16_t*, const f32x16 (&s)[2], int c) {
    const int u = c >> 1, o = (c & 1) * 8;
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (bf16_t)s[u][o + e];
    return r;
}
__device__ __forceinline__ f32x4 pack_chunk(const float*, const f32x16 (&s)[2], int c) {
    const int u = c >> 2, o = (c & 3) * 4;
    return f32x4{s[u][o], s[u][o + 1], s[u][o + 2], s[u][o + 3]};
}

template <typename T> __device__ __forceinline__ void store_quad(T* p, f32x4 v);
template <> __device__ __forceinline__ void store_quad<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> __device__ __forceinline__ void store_quad<bf16_t>(bf16_t* p, f32x4 v) {
    bf16x4 o;
    o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3];
    *reinterpret_cast<bf16x4*>(p) = o;
}

// ---- per-lane pieces of a wave that owns 32 rows: lane = row l31 = lane & 31, half h = lane >> 5 (common.h)
template <int NDB> __device__ __forceinline__ void acc_zero(f32x16 (&acc)[NDB]) {
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;
}

// The B-operand fragments of one row straight from HBM (row: that row's head slice); chunks past hd are zeros.  Branch-free: a chunk
// past hd reads a clamped (valid) address and is zeroed after the load
template <int HD, typename T>
__device__ __forceinline__ void row_frags_load(const T* row, int hd, int h, typename Chunk<T>::type (&f)[Cfg<T, HD>::NKK]) {
#pragma unroll
    for (int kk = 0; kk < Cfg<T, HD>::NKK; ++kk) {
        const int d = (2 * kk + h) * Cfg<T, HD>::E;
        const bool ok = d < hd;
        u32x4 raw = *reinterpret_cast<const u32x4*>(row + (ok ? d : 0));
        raw = ok ? raw : zero4();
        f[kk] = *reinterpret_cast<typename Chunk<T>::type*>(&raw);
    }
}

// A lane's row of accumulators (transposed layout: lane = row l31, registers = d) times mul, four elements per store.  grow: that row's
// head slice; the caller has checked that the row exists.  acc holds the NDBO 32-wide d blocks from DB0 on.  The pair form stores two
// rows (dK and dV) under one d < hd test per quad: as two single calls it measured +33 / +64 instructions in
// attn_bwd_dkdv_chunk_kernel<32 / 64> and +77 / +145 in attn_bwd_mid_kernel (pair: 0 / 0 and +15 / +25), all outside the loops
// (profiles/attention_rows32_refactor.txt)
template <typename T> __device__ __forceinline__ void acc_store_quad(T* p, const f32x16& acc, int g, float mul) {
    store_quad<T>(p, f32x4{acc[4 * g] * mul, acc[4 * g + 1] * mul, acc[4 * g + 2] * mul, acc[4 * g + 3] * mul});
}
template <int DB0 = 0, typename T, int NDBO>
__device__ __forceinline__ void acc_store_row(T* grow, const f32x16 (&acc)[NDBO], float mul, int hd, int h) {
#pragma unroll
    for (int db = 0; db < NDBO; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * (DB0 + db) + 8 * g + 4 * h;
            if (d < hd) acc_store_quad(grow + d, acc[db], g, mul);
        }
}
template <int DB0 = 0, typename T, int NDBO>
__device__ __forceinline__ void acc_store_row_pair(T* grow0, const f32x16 (&acc0)[NDBO], float mul0, T* grow1, const f32x16 (&acc1)[NDBO],
                                                   float mul1, int hd, int h) {
#pragma unroll
    for (int db = 0; db < NDBO; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 32 * (DB0 + db) + 8 * g + 4 * h;
            if (d < hd) {
                acc_store_quad(grow0 + d, acc0[db], g, mul0);
                acc_store_quad(grow1 + d, acc1[db], g, mul1);
            }
        }
}

}  // namespace
