// gemm3.hip -- GEMM family "g3": bf16 NT (both operands reduction-contiguous), 256 x 256 tile, K-tile 64, 8 waves,
// ping-pong K-loop in 4 phases per K-tile with the LDS-DMA stream running 7 half-tiles ahead.
//
// Why a third family: the PMC profile of "g2w" (gemm2b.hip, K-step 32, one barrier per step) shows the waves
// issue-stalled half the time with MFMA busy 0.28-0.43.  Three structural changes address that:
//   * K-tile 64: an operand row is one full 128-byte line per tile (K-step 32 fetched every line twice, as two 64-byte
//     halves in different steps), and the barrier / wait overhead per MFMA halves.
//   * four phases per K-tile, 16 MFMAs (v_mfma_f32_16x16x32_bf16) each = one 64 x 32 quadrant of the wave's 128 x 64
//     output x the whole K-tile.  The two wave rows (waves 0-3 / 4-7: one of each per SIMD) run ONE BARRIER out of
//     phase: while one row issues its 16 MFMAs under s_setprio 1, its SIMD partner reads the next phase's fragments
//     from LDS and issues its share of the DMA, then they swap.  The matrix pipe of every SIMD always has a wave in
//     an MFMA-only segment; LDS reads and DMA issue never sit in front of an MFMA of the same wave.
//   * the DMA stream is issued one half-tile (128 rows x 64 k = 16 KiB, two instructions per wave) per phase, seven
//     half-tiles ahead of the phase that reads it, and waited for with ONE counted vmcnt per K-tile (never 0 in the
//     loop): every half-tile has >= 5 phases to land.
//
// LDS: 2 buffers x 4 half-tiles x 16 KiB = 128 KiB.  Half-tiles are ordered by first use:
//   j = 0  B-X  weight rows  wc*64 +  0..31  (all four wave columns)       read in phase 0
//   j = 1  A-X  token rows   wr*128 +  0..63 (both wave rows)              read in phase 0
//   j = 2  B-Y  weight rows  wc*64 + 32..63                                read in phase 1
//   j = 3  A-Y  token rows   wr*128 + 64..127                              read in phase 2
//   phase 0: X x X quadrant   phase 1: A-X x B-Y   phase 2: A-Y x B-Y   phase 3: A-Y x B-X (no reads)
// A half-tile is 128 rows of 128 bytes (64 k); a DMA instruction (1 KiB, lane-linear destination) is 8 rows; chunk c
// (16 bytes = 8 k) of local row r sits in slot c ^ ((r >> 1) & 7) of its row -- two rows share a 256-byte bank row,
// so the 16 lanes a ds_read_b128 services together (MI355X_MICROARCH.md, LDS) hit 16 different 16-byte slots.  The
// permutation is applied on the SOURCE address of the DMA and again on the fragment read.
//
// Hazards (phase index P = 4 t + p counts over the whole K-loop; wave row 1 runs one barrier behind wave row 0):
//   RAW  half-tile i is issued in phase i - 7 and read in phase >= 4 (i/4); every wave waits "all of K-tile t+1 has
//        landed" (vmcnt(6): three younger half-tiles may stay in flight) BEFORE the first barrier of phase 3 of
//        K-tile t, so both wave rows have passed that wait before either reads K-tile t+1.
//   WAR  slot reuse: half-tile i+8 is issued in phase i+1.  A-X, B-Y, A-Y were last read in phase i-1 (two phases and
//        >= 2 barriers earlier for both wave rows).  B-X is read in phase i itself: its four reads are issued first
//        and retired with lgkmcnt(8) before that phase's first barrier, which the issuing wave row passes later.
// The shared device code -- state, DMA issue, the 4-phase K-tile, the LDS-free epilogue -- lives in gemm3_core.h; this file holds the
// kernels the library ships (one tile per workgroup, resident, wgrad) and their launchers.
#include "gemm3_core.h"

namespace {
constexpr int G3_ROWOP_AHEAD = 4;              // row-operand slabs in flight ahead of their use in a whole tile's epilogue (6 until round 4: proj 84.6 -> 80.6 us,
                                               // fc2 205.7 -> 201.7 us sustained, profiles/r04_rowop_ahead.txt: fewer spills at the seam)
constexpr int G3_ROWOP_AHEAD_HALF = 4;         // ... in a 128-row item's epilogue (two: proj 80.5 -> 84.2 us, fc2 203 -> 206 us)
constexpr int G3_ROWOP_AHEAD_STATS = 4;        // ... in the statistics / gelu'(row operand) epilogues

// ---- one tile per workgroup
template <int EPI, bool WRAP = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_g3_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2;

    // Work ids: F = p.g3_full_tiles whole tiles, then the tiles of the last, mostly empty round as S = p.g3_split parts
    // each (tile quantisation: the encoder's N = 768 outputs are 591 tiles = 2.31 rounds on 256 CUs; as whole tiles that is
    // 3 rounds of time, as 510 tiles + 81 x 3 thirds it is 2.31).  Block b runs on XCD b % 8: every XCD gets a contiguous
    // range of the whole tiles (neighbours share operand panels through its L2) AND its share of the parts, so all XCDs
    // carry the same amount of work.
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int F = p.g3_full_tiles;
    const int nf = (F >> 3) + (xcd < (F & 7) ? 1 : 0);
    const int base_f = xcd * (F >> 3) + (xcd < (F & 7) ? xcd : (F & 7));
    int tile, part = -1;
    if (slot < nf) {
        tile = base_f + slot;
    } else {
        const int base_all = xcd * (nwg >> 3) + (xcd < (nwg & 7) ? xcd : (nwg & 7));
        const int tid_ = base_all - base_f + (slot - nf);                 // index among the parts
        const int tq = __builtin_amdgcn_readfirstlane(tid_ / p.g3_split);
        tile = F + tq;
        part = tid_ - tq * p.g3_split;
    }
    const int tm = __builtin_amdgcn_readfirstlane(tile / p.tiles_n), tn = tile - tm * p.tiles_n;
    const int64_t m0 = (int64_t)tm * G3_BM, n0 = (int64_t)tn * G3_BN;

    G3State s;
    g3_init_lane(s, p, smem, wave, lane);
    g3_zero(s);
    const G3Src src = g3_make_src(p, tm, tn);

    const int nkt = (int)(p.K / G3_BK);          // even, >= 2 (g3_supported)
    int kt0 = 0, kt1 = nkt;
    if (part >= 0) {
        kt0 = part * p.g3_ktp;
        kt1 = kt0 + p.g3_ktp < nkt ? kt0 + p.g3_ktp : nkt;
    }
    s.wrap_kt = WRAP ? p.a_wrap_kt : 0;
    g3_prime<WRAP>(s, src, kt0, wr);

    // past the end of the K-range the source is a null descriptor (see g3_phase)
    const G3Src null = g3_null_src(p);
    for (int kt = kt0; kt < kt1 - 2; kt += 2) {
        g3_ktile<0, false, 0, false, 0, WRAP>(s, src, kt + 1, src, kt + 2);
        g3_ktile<1, false, 0, false, 0, WRAP>(s, src, kt + 2, src, kt + 3);
    }
    g3_ktile<0, false, 0, false, 0, WRAP>(s, src, kt1 - 1, null, 0);
    g3_ktile<1, false, 0, false, 0, WRAP>(s, null, 0, null, 0);
    g3_drain(wr);
    if (part >= 0) {
        // a part of a split tile: raw partial sums; the fold that follows the launch applies the real epilogue
        const int64_t row0 = (int64_t)(F / p.tiles_n) * G3_BM;
        g3_epilogue<5>(p, s, m0, n0, lane, p.g3_slabs + (int64_t)part * (p.M - row0) * p.N, row0);
        return;
    }
    g3_epilogue<EPI>(p, s, m0, n0, lane);
}

// ---- resident form: one workgroup per CU walks its work items (same ids and XCD mapping as gemm_g3_kernel: item
// (xcd, slot) for slot = c, c + G/8, ...), and the operand stream never stops at a tile boundary:
//   * the last two K-tiles of an item already fetch the first two of the next one (the K-loop's sources are just
//     (descriptor, K-tile) pairs), the one half-tile the loop would issue right AFTER the boundary goes out right before
//     the epilogue, and the epilogue touches no LDS -- so the whole prologue latency of the next tile, and its workgroup
//     launch, hide under the epilogue of this one;
//   * vmcnt retires in order and counts stores, so a K-loop that waits for "everything but my last 6 DMAs" right after an
//     epilogue would first drain the epilogue's stores.  The epilogue therefore issues an EXACT number of memory
//     operations (buffer stores / loads whose edge handling is the descriptor's bounds check, never a branch), and the
//     first K-tile after it waits with that many more operations allowed in flight (g3_phase<.., SEAM>): the stores
//     drain under the next tile's first two K-tiles.
// bf16 outputs / row operands only (launch3r checks).  Parts of split tiles (EPI 5 slabs) are the last items of a
// workgroup; should another item follow one, the queue is drained and re-primed.
// The bias is not added here: the accumulators START at the bias of their columns (g3r_bias / s.binit; alpha = 1),
// loaded for the NEXT tile at the top of this epilogue, ahead of its stores -- a load issued behind the stores could only be
// waited for by draining them.
// this lane's index, recomputed from the hardware where it is needed (two VALU operations): a lane id kept in a register
// across the item loop of the resident kernel is the first thing hipcc spills
__device__ __forceinline__ int g3_lane_now() {
    unsigned z = 0;
    asm volatile("" : "+v"(z));          // (opaque: not common-subexpression'd with, or hoisted to, an earlier copy)
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
}
// One ticket from a work counter, drawn by lane 0 alone.  Inline asm with the exec mask narrowed by hand: written as
// `if (lane == 0) atomic` hipcc waits for the result with vmcnt(0) at the join of the branch -- a drain of every store and DMA
// in flight.  The instruction is invisible to the compiler's own wait counting (it is OLDER than everything the callers
// wait for afterwards, which only makes their waits stricter); the caller retires it with a counted s_waitcnt.
__device__ __forceinline__ unsigned g3r_draw(unsigned* ctr) {
    unsigned old, zero = 0, one = 1;
    unsigned long long saved;
    asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
                 : "=&v"(old), "=&s"(saved)
                 : "v"(zero), "v"(one), "s"(ctr)
                 : "memory");
    return old;      // valid in lane 0 once the operation has retired
}
// wave 0 hands the ticket to the other waves through the LDS word behind the operand buffers; whoever draws the last ticket
// of the launch (nx - 1) puts the counter back to zero
__device__ __forceinline__ void g3r_publish(unsigned drawn, unsigned* ctr, int nx, uint32_t lds_tick) {
    const unsigned t = __builtin_amdgcn_readfirstlane(drawn);
    if (t == (unsigned)(nx - 1)) {
        unsigned zero = 0;
        unsigned long long saved;
        asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tglobal_store_dword %1, %1, %2\n\ts_mov_b64 exec, %0"
                     : "=&s"(saved) : "v"(zero), "s"(ctr) : "memory");
    }
    asm volatile("ds_write_b32 %0, %1" ::"v"(lds_tick), "v"(t) : "memory");
}
struct G3Bias { f32x4 v[4]; };       // this lane's bias for n-tiles 0..3 of its wave column (accumulator layout)
__device__ __forceinline__ G3Bias g3r_bias(const __amdgpu_buffer_rsrc_t brs, int tn, int wave, int lane) {
    G3Bias b;
    (void)lane;
    lane = g3_lane_now();                // (derive the offset here: hoisted out of the item loop it would be spilled)
    const int col = tn * G3_BN + (wave & 3) * 64 + 4 * (lane >> 4);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)      // (no bias, or columns past N: zero records / out of range -> zeros)
        b.v[nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(brs, (col + nt * 16) * 4, 0, 0));
    return b;
}
__device__ __forceinline__ void g3r_set_binit(G3State& s, const G3Bias& b, bool zero) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) s.binit[j] = zero ? z : b.v[j];
    // (used HERE: the wait for the loads lands in the caller's straight-line code, with the number of younger stores known;
    // at the first real use, behind the item loop's joins, it would be a drain)
    asm volatile("" ::"v"(s.binit[0]), "v"(s.binit[1]), "v"(s.binit[2]), "v"(s.binit[3]));
}

// Store pattern: a store instruction that covers 16 rows x 64 bytes (what the permlane16 re-deal alone gives) costs a CU
// 4.6 us per 256 x 256 bf16 tile, one that covers 8 rows x 128 bytes -- whole cache lines -- 1.7 us (tools/store_probe).
// So the two 64-byte halves (q = 0 / 1) of the wave's 128-byte row segment are re-dealt once more, between the lanes of
// rows r and r + 8 (DPP row_ror:8 under a bank mask): afterwards half A holds rows 0..7 and half B rows 8..15 of the
// 16-row slab, lane (r = l & 15, g = l >> 4) owning the 16-byte chunk (r >> 3) * 4 + 2 (g & 1) + (g >> 1) of row r & 7.
__device__ __forceinline__ void g3r_rows8(f32x4& x0, f32x4& x1, f32x4& y0, f32x4& y1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned a0 = __float_as_uint(x0[e]), a1 = __float_as_uint(x1[e]), b0 = __float_as_uint(y0[e]), b1 = __float_as_uint(y1[e]);
        // lanes 8..15 of every row of 16 take the q = 1 value of the lane 8 below; lanes 0..7 the q = 0 value of the lane 8 above
        x0[e] = __uint_as_float(__builtin_amdgcn_update_dpp(a0, b0, 0x128, 0xf, 0xc, false));
        x1[e] = __uint_as_float(__builtin_amdgcn_update_dpp(a1, b1, 0x128, 0xf, 0xc, false));
        y0[e] = __uint_as_float(__builtin_amdgcn_update_dpp(b0, a0, 0x128, 0xf, 0x3, false));
        y1[e] = __uint_as_float(__builtin_amdgcn_update_dpp(b1, a1, 0x128, 0xf, 0x3, false));
    }
}

__device__ __forceinline__ void g3r_rows8_packed(u32x4& x, u32x4& y) {      // the same re-deal on packed bf16 pairs
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned a = x[e], b = y[e];
        x[e] = __builtin_amdgcn_update_dpp(a, b, 0x128, 0xf, 0xc, false);
        y[e] = __builtin_amdgcn_update_dpp(b, a, 0x128, 0xf, 0x3, false);
    }
}

// Which LANES hold a cache line matters as much as which lines an instruction covers: with the lanes of one 128-byte row
// segment scattered over the wave (r, r + 8, r + 16 ..: what the re-deals above leave) a store instruction costs the CU
// ~77 clocks, with eight CONSECUTIVE lanes per line ~31 (time stamps in the kernel, debug bit 8; tools/store_probe).  So the
// packed 16-byte chunks take one more trip through the lane crossbar (ds_bpermute_b32: no LDS memory involved, the operand
// buffers stay untouched) into the order lane t = row (t >> 3), chunk (t & 7); row operands are loaded in that order and
// taken the opposite way.
__device__ __forceinline__ u32x4 g3r_lanes(const u32x4& v, int addr) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)v[e]);
    return o;
}

// ---- PRE 5: the folded LayerNorm's row pairs from the 256-column partials of the launch in front (see g3_epilogue_r).  Thread
// t = 64 wave + lane of the workgroup owns rows 2 (t >> 2), + 1 of an item (m0 = its first row, rows = how many exist) and part
// t & 3 (< row_nparts <= 4): ONE 16-byte load per thread -- 8 wave-level memory instructions per tile (a first version with 64 of them,
// one 8-byte load per 64-column partial, cost the CU's memory path ~2 k clocks per tile in front of the stores).
struct G3Parts { f32x4 v; };
__device__ __forceinline__ G3Parts g3r_parts_load(const GemmParams& p, int64_t m0, int rows, int wave) {
    G3Parts o;
    const int lane = g3_lane_now();
    const int t = wave * 64 + lane, rp = t >> 2, j = t & 3;
    // [part][M] pairs seen from row m0: the last part ends `rows` rows in (rows past the item / the matrix: out of range -> zeros;
    // an odd last row: the second pair of its 16 bytes is out of range -> zeros, never read back)
    const __amdgpu_buffer_rsrc_t pars = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.row_affine) + (rows > 0 ? m0 * 2 : 0), 0,
                                                                           rows > 0 ? (int)((((int64_t)p.row_nparts - 1) * p.M + rows) * 8) : 0, 0x00020000);
    const uint32_t off = (j < p.row_nparts && 2 * rp < rows) ? (uint32_t)(((int64_t)j * p.M + 2 * rp) * 8) : 0x80000000u;
    o.v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(pars, (int)off, 0, 0));
    return o;
}
// ... folded into (rstd, -rstd * mean) of LayerNorm(256 row_nparts, row_eps) for both rows and written to LDS `lds_pairs`[row]: the
// arithmetic of row_stats_combine_kernel (mean of the part means, M2 = sum M2_j + 256 sum (mean_j - mean)^2) with the sums over a
// quad of lanes (two DPP swaps; the order (a + b) + (c + d) is the same in all four lanes: they hold the same bits)
__device__ __forceinline__ void g3r_parts_fold(const GemmParams& p, const G3Parts& q, int wave, uint32_t lds_pairs) {
    const int lane = g3_lane_now();
    const int t = wave * 64 + lane, rp = t >> 2, j = t & 3;
    auto quad = [](float x) {
        x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0xB1, 0xf, 0xf, true));      // quad_perm [1, 0, 3, 2]
        x += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x4E, 0xf, 0xf, true));      // quad_perm [2, 3, 0, 1]
        return x;
    };
    const float w = j < p.row_nparts ? 1.0f : 0.0f;
    const float inv_np = __builtin_amdgcn_rcpf((float)p.row_nparts);
    const float inv_c = inv_np * (1.0f / 256.0f);
    u32x4 out;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float mean = quad(q.v[2 * r]) * inv_np;                           // (parts past row_nparts / rows past the item are zeros)
        const float m2 = quad(q.v[2 * r + 1]);
        const float d = (q.v[2 * r] - mean) * w;
        const float dev = quad(d * d);
        const float rstd = __builtin_amdgcn_rsqf((m2 + 256.0f * dev) * inv_c + p.row_eps);
        out[2 * r] = __float_as_uint(rstd);
        out[2 * r + 1] = __float_as_uint(-rstd * mean);
    }
    // the four lanes of a row pair hold the same 16 bytes and write them to the same place: no exec-mask games
    asm volatile("ds_write_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" ::"v"(lds_pairs + (uint32_t)rp * 16), "v"(out) : "memory");
}

// EPI: 0 bias, 1 GELU (PRE: 0 nothing saved, 1 pre-activation saved, 2 gelu'(pre-activation) saved), 2 + residual row
// operand, 3 * gelu'(row operand), 6 * row operand.
// PRE 3 (EPI 0 / 1): a LayerNorm folded into this Linear (GemmParams::row_affine / col_shift): the accumulators start at zero
// and the epilogue applies v = rstd_m * acc + (-rstd_m mean_m) * s[n] + c[n] in the accumulator layout (one row per lane and
// 16-row slab, four consecutive columns per register quad), ahead of the activation; nothing is saved.
// PRE 5 (EPI 0 / 1): the same folded LayerNorm, its row pairs formed HERE from the 64-column partials (mean_i, M2_i) the residual
// launch in front of this one left behind (PRE 4; GemmParams::row_affine = [row_nparts][M] pairs over 256 columns each, row_nparts <= 4) -- no
// row_stats_combine launch between the two GEMMs (24 per Base forward).  Software-pipelined over the items of a workgroup so that
// neither the memory latency nor the arithmetic sits in front of an epilogue: the epilogue of item i (a) reads item i's 256 pairs
// from 2 KiB of LDS BESIDE the operand buffers (buffer i & 1), (b) issues the load of item i + 1's partials at its top -- thread t
// of the workgroup takes rows 2 (t >> 2), + 1 of that item and part t & 3: one 16-byte load -- and (c) folds them BEHIND its last store, where the
// CU's memory path is busy draining the stores and the first K-tile of item i + 1 would only wait for it (measured: K-tile 1 takes
// 4.3 .. 5.1 k clocks against 2.4 k in steady state): the arithmetic of row_stats_combine_kernel (mean of the part means, M2 = sum
// M2_j + 256 sum (mean_j - mean)^2; the parts of a row meet through two DPP swaps), pairs into buffer (i + 1) & 1.  A workgroup's
// first item is folded in the prologue.  A first version that loaded, folded and exchanged the pairs at the TOP of each epilogue
// (one workgroup barrier) cost 1 us per tile, and one 8-byte load per 64-column partial (64 wave-level loads per tile) 2 k clocks of
// the CU's memory path in front of the stores -- each as much as the launches it removed (profiles/r06_row_parts_ab.txt).
// All LDS traffic is inline asm: a compiler-visible LDS access would be guarded with vmcnt(0) while the next tile's DMA is in flight.
// PRE 4 (EPI 2): the per-row statistics of the OUTPUT rows on the side (GemmParams::row_stats) -- the LayerNorm that reads this
// residual stream next then needs no pass of its own over it (me_row_stats_combine folds the partials).  After the row re-deal
// eight lanes hold one row's 64 columns of this wave: per half slab every lane forms (S, Q) = sum (v - P), sum (v - P)^2 of its
// eight values against a pivot P = the row's first value in this wave column (shifted sums: no cancellation however far the row
// mean is from zero; P reaches the eight lanes through one DPP move and two lane-row swaps), and the sixteen (half slab) pairs of
// a wave are summed over the eight lanes as a REDUCE-SCATTER -- DPP row_ror:8, v_permlane16_swap, v_permlane32_swap, each step
// halving the number of live values -- so that every lane ends up with two finished rows: (mean, M2) over n = 64 columns
// (a 128-row item: four slabs, one row per lane).  Round 6: these per-wave-column pairs no longer go to memory -- the four wave columns
// of a row meet in 8 KiB of LDS behind the last store and ONE pair per row over the tile's 256 columns is stored, [N / 256][M] (see
// the block behind the slab loop).  The statistics are those of the values AS STORED (rounded to
// bf16 and converted back: eight more operations per half slab) -- for a row whose mean dwarfs its spread the rounding IS the
// spread, and the reference's LayerNorm sees the rounded stream too.
// HALF: a 128 x 256 item (g3_make_src_half): accumulator slabs 0..3 only, this wave row's rows are m0 + 64 wr + ..; the
// epilogue is padded with stores no descriptor admits up to the whole tile's operation count, so that the counted waits behind it
// (g3_phase<.., SEAM>, the ticket wait) are the same for both item kinds.
template <int EPI, int PRE, bool HALF = false>
__device__ __forceinline__ void g3_epilogue_r(const GemmParams& p, G3State& s, int64_t m0, int tn, int lane, const G3Src& nxt, int nk,
                                              const __amdgpu_buffer_rsrc_t brs, int ntn, bool next_zero, unsigned* ctr, int nx,
                                              uint32_t lds_tick, int64_t next_m0 = 0, int next_rows = 0, int par = 0) {
    // PRE 6 (EPI 1 / EPI 6): gelu'(h) travels as EIGHT BITS (ME_GG8: q = rint((g + 0.13) x 255 / 1.26), g in [-0.129, 1.129]) -- EPI 1 saves it,
    // EPI 6 multiplies by it.  Half the bytes of the bf16 factor (310 MB less written and 310 MB less read per layer at config 2: at ~120 pJ
    // per HBM byte the largest single item a train step can shed, profiles/r06_energy_probe.txt); the same number of memory operations,
    // each half as wide (8 bytes per lane, 8 consecutive lanes = the wave's 64-byte row segment), so every counted wait stays what it is.
    // Step 0.0049: |error| <= 0.0025 absolute, about what bf16 leaves at g ~ 1 and more than bf16 leaves near 0.
    constexpr bool G8 = PRE == 6, G8S = G8 && EPI == 1, G8L = G8 && EPI == 6;
    static_assert(!G8 || EPI == 1 || EPI == 6, "8-bit gelu': the fc1 forward that saves it, the fc2 dgrad that reads it");
    constexpr bool SAVE = PRE == 1 || PRE == 2 || G8S, LNF = PRE == 3 || PRE == 5, LNP = PRE == 5, STATS = PRE == 4;
    static_assert(!STATS || EPI == 2, "row statistics: the residual epilogue");
    constexpr int NMT = HALF ? 4 : 8, WROWS = HALF ? 64 : 128;      // 16-row slabs per wave, rows per wave row
    // (claimed schedule: wave 0 draws the ticket for the item after next FIRST, ahead of every store of this epilogue)
    unsigned drawn = 0;
    if (ctr && s.wave == 0) drawn = g3r_draw(ctr);
    (void)lane;
    lane = g3_lane_now();
    const int wr = s.wave >> 2, wc = s.wave & 3;
    const int r = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)tn * G3_BN;
    int64_t rows = p.M - m0, cols = p.N - n0;
    rows = rows < 2 * WROWS ? rows : 2 * WROWS;
    rows = rows < 1 ? 1 : rows;                 // (an item past the last row: every access below is then out of range)
    cols = cols < G3_BN ? cols : G3_BN;
    const bool item_ok = p.M > m0;
    auto tile_rsrc = [&](const void* base, int64_t ld, int esz = 2) {
        if (!item_ok) return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0, 0x00020000);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(base)) + (m0 * ld + n0) * esz, 0,
                                                 (int)(((rows - 1) * ld + cols) * esz), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t crs = tile_rsrc(p.C, p.ldc);
    const __amdgpu_buffer_rsrc_t prs = SAVE ? tile_rsrc(p.preact, p.ldpre, G8S ? 1 : 2) : crs;
    const __amdgpu_buffer_rsrc_t rrs = EPI == 2 ? tile_rsrc(p.residual, p.ldres) : (EPI == 3 || EPI == 6) ? tile_rsrc(p.aux, p.ldaux, G8L ? 1 : 2) : crs;
    const int rop_ld = (int)(EPI == 2 ? p.ldres : p.ldaux);
    // memory side: lane t = row t >> 3 of an 8-row half slab, 16-byte chunk t & 7 of the wave's 128-byte row segment.  A
    // chunk past the column edge gets an offset no descriptor admits; rows past the row edge fall behind the descriptor's end.
    const int colb = wc * 128 + (lane & 7) * 16;
    const bool ok = (colb >> 1) + 8 <= (int)cols;
    const int row = wr * WROWS + (lane >> 3);
    const uint32_t coff = ok ? (uint32_t)(row * (int)p.ldc * 2 + colb) : 0x80000000u;
    const uint32_t poff = ok && SAVE ? (G8S ? (uint32_t)(row * (int)p.ldpre + (colb >> 1)) : (uint32_t)(row * (int)p.ldpre * 2 + colb)) : 0x80000000u;
    const uint32_t roff = ok ? (G8L ? (uint32_t)(row * rop_ld + (colb >> 1)) : (uint32_t)(row * rop_ld * 2 + colb)) : 0x80000000u;
    const int cstep = (int)p.ldc * 16, pstep = (int)p.ldpre * (G8S ? 8 : 16), rstep = rop_ld * (G8L ? 8 : 16);       // 8 rows, bytes
    // register side (after g3r_rows8): lane (r, g) = row r & 7, chunk 4 (r >> 3) + 2 (g & 1) + (g >> 1).  to_mem: the lane
    // that holds memory lane t's chunk; to_reg: the memory lane that holds this lane's chunk (x 4: bpermute byte addresses)
    const int to_mem = 4 * ((lane >> 3) + 8 * ((lane >> 2) & 1) + 16 * (((lane >> 1) & 1) | ((lane & 1) << 1)));
    const int to_reg = 4 * (8 * (r & 7) + 4 * (r >> 3) + 2 * (g & 1) + (g >> 1));
    auto fetch = [&](const int mt, u32x4 (&raw)[2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (G8L) {
                const u32x2 t = __builtin_amdgcn_raw_buffer_load_b64(rrs, (int)(roff + (2 * mt + h) * rstep), 0, G3_POL_R);
                raw[h] = u32x4{t[0], t[1], 0u, 0u};
            } else {
                raw[h] = __builtin_amdgcn_raw_buffer_load_b128(rrs, (int)(roff + (2 * mt + h) * rstep), 0, G3_POL_R);
            }
        }
    };
    // 8-bit gelu' (ME_GG8): eight bytes <-> eight factors
    auto unpack8 = [](const u32x4& rw, f32x4& a, f32x4& b) {
        const f32x4 qa = {(float)(rw[0] & 0xffu), (float)((rw[0] >> 8) & 0xffu), (float)((rw[0] >> 16) & 0xffu), (float)(rw[0] >> 24)};
        const f32x4 qb = {(float)(rw[1] & 0xffu), (float)((rw[1] >> 8) & 0xffu), (float)((rw[1] >> 16) & 0xffu), (float)(rw[1] >> 24)};
        a = qa * ME_GG8_STEP + ME_GG8_LO;
        b = qb * ME_GG8_STEP + ME_GG8_LO;
    };
    auto pack8 = [](const f32x4& a, const f32x4& b) {
        // v_cvt_pk_u8_f32 rounds to nearest even and saturates to 0 .. 255 (NaN -> 0): tools/cvt_pk_u8_probe.hip -- one fma and one pack per factor
        unsigned w0 = 0u, w1 = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w0 = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(a[e], 1.0f / ME_GG8_STEP, -ME_GG8_LO / ME_GG8_STEP), e, w0);
            w1 = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_fmaf(b[e], 1.0f / ME_GG8_STEP, -ME_GG8_LO / ME_GG8_STEP), e, w1);
        }
        return u32x4{w0, w1, 0u, 0u};
    };
    auto lanes2 = [](const u32x4& v, int addr) {        // g3r_lanes on the two live words
        u32x4 o = {0u, 0u, 0u, 0u};
        o[0] = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)v[0]);
        o[1] = (unsigned)__builtin_amdgcn_ds_bpermute(addr, (int)v[1]);
        return o;
    };
    auto unpack = [](const u32x4& rw, f32x4& a, f32x4& b) {
        a[0] = __uint_as_float(rw[0] << 16); a[1] = __uint_as_float(rw[0] & 0xffff0000u);
        a[2] = __uint_as_float(rw[1] << 16); a[3] = __uint_as_float(rw[1] & 0xffff0000u);
        b[0] = __uint_as_float(rw[2] << 16); b[1] = __uint_as_float(rw[2] & 0xffff0000u);
        b[2] = __uint_as_float(rw[3] << 16); b[3] = __uint_as_float(rw[3] & 0xffff0000u);
    };
    auto pack = [](const f32x4& a, const f32x4& b) {
        bf16x8 o;
        o[0] = (bf16_t)a[0]; o[1] = (bf16_t)a[1]; o[2] = (bf16_t)a[2]; o[3] = (bf16_t)a[3];
        o[4] = (bf16_t)b[0]; o[5] = (bf16_t)b[1]; o[6] = (bf16_t)b[2]; o[7] = (bf16_t)b[3];
        return __builtin_bit_cast(u32x4, o);
    };
    // (STATS) destination of this TILE's partials: [part = tn][M] pairs over its 256 columns; a part past the last whole column tile, or an
    // item past the last row, gets a descriptor that admits nothing (the operation count stays what it is).  The four wave columns'
    // 64-column pairs meet in 8 KiB of LDS beside the operand buffers ([row][wave column] pairs, behind the ticket word)
    float st_a[2][3], st_b[2][3];
    __amdgpu_buffer_rsrc_t srs = crs;
    const uint32_t lds_stats = lds_tick + 64;
    if (STATS) {
        const bool part_ok = item_ok && ((int64_t)tn + 1) * 256 <= p.N;
        srs = __builtin_amdgcn_make_buffer_rsrc(p.row_stats + (part_ok ? ((int64_t)tn * p.M + m0) * 2 : 0), 0, part_ok ? (int)(rows * 8) : 0, 0x00020000);
    }
    constexpr int AHEAD = HALF ? G3_ROWOP_AHEAD_HALF : (EPI == 3 || STATS) ? G3_ROWOP_AHEAD_STATS : G3_ROWOP_AHEAD;      // row-operand slabs in flight ahead of their use (more spills: into the K-loop for gelu', onto the ticket register otherwise)
    u32x4 rowop[8][2];
    if (EPI == 2 || EPI == 3 || EPI == 6) {
#pragma unroll
        for (int mt = 0; mt < AHEAD; ++mt) fetch(mt, rowop[mt]);
    }
    // folded LayerNorm: this tile's per-row pairs (rows wr*128 + 16 mt + r) and per-column s / c, all ahead of the DMA below
    f32x2 lnf_row[8];
    G3Bias lnf_s, lnf_c;
    G3Parts lnp;                                // (LNP) this thread's share of the NEXT item's partials (folded behind the stores)
    u32x2 lnq[8];                               // (LNP) this item's pairs on their way in from LDS
    if (LNF) {
        const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.col_shift), 0, (int)(p.N * 4), 0x00020000);
        if (LNP) {
            const uint32_t pa = lds_tick + 64 + (uint32_t)par * 2048 + (uint32_t)(wr * WROWS + r) * 8;
#define G3R_PAIR(i) if ((i) < NMT) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(lnq[i]) : "v"(pa), "i"((i) * 128) : "memory");
            G3R_PAIR(0) G3R_PAIR(1) G3R_PAIR(2) G3R_PAIR(3) G3R_PAIR(4) G3R_PAIR(5) G3R_PAIR(6) G3R_PAIR(7)
#undef G3R_PAIR
            lnp = g3r_parts_load(p, next_m0, next_rows, s.wave);
        } else {
            const __amdgpu_buffer_rsrc_t rars = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.row_affine) + m0 * 2, 0, item_ok ? (int)(rows * 8) : 0, 0x00020000);
#pragma unroll
            for (int mt = 0; mt < NMT; ++mt)    // (rows past the edge: out of range -> zeros; their outputs are never stored)
                lnf_row[mt] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rars, (wr * WROWS + mt * 16 + r) * 8, 0, 0));
        }
        lnf_s = g3r_bias(srs, tn, s.wave, lane);
        lnf_c = g3r_bias(brs, tn, s.wave, lane);
    }
    // the half-tile phase 0 of the next K-tile would issue (see SEAM), behind the first row-operand loads so that their
    // wait does not include it; then the next tile's bias
    if (HALF) g3_issue<2>(s, nxt, 1, nk);       // (a 128-row item's stream: phase 0 of a K-tile issues the NEXT one's B-Y)
    else g3_issue<3>(s, nxt, 1, nk);
    const G3Bias nb = g3r_bias(brs, ntn, s.wave, lane);
    __builtin_amdgcn_sched_barrier(0);
    if (LNP) {
        if (NMT == 8) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lnq[0]), "+v"(lnq[1]), "+v"(lnq[2]), "+v"(lnq[3]), "+v"(lnq[4]), "+v"(lnq[5]), "+v"(lnq[6]), "+v"(lnq[7])::"memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lnq[0]), "+v"(lnq[1]), "+v"(lnq[2]), "+v"(lnq[3])::"memory");
#pragma unroll
        for (int mt = 0; mt < NMT; ++mt) lnf_row[mt] = __builtin_bit_cast(f32x2, lnq[mt]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < NMT; ++mt) {
        f32x4 ro[2][2];
        if (EPI == 2 || EPI == 3 || EPI == 6) {
            if (G8L) {
                unpack8(lanes2(rowop[mt][0], to_reg), ro[0][0], ro[0][1]);
                unpack8(lanes2(rowop[mt][1], to_reg), ro[1][0], ro[1][1]);
            } else {
                unpack(g3r_lanes(rowop[mt][0], to_reg), ro[0][0], ro[0][1]);
                unpack(g3r_lanes(rowop[mt][1], to_reg), ro[1][0], ro[1][1]);
            }
            if (mt + AHEAD < NMT) fetch(mt + AHEAD, rowop[mt + AHEAD]);
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 v[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            v[q][0] = s.acc[mt][2 * q]; v[q][1] = s.acc[mt][2 * q + 1];
            if (LNF) {
                v[q][0] = v[q][0] * lnf_row[mt][0] + (lnf_s.v[2 * q] * lnf_row[mt][1] + lnf_c.v[2 * q]);
                v[q][1] = v[q][1] * lnf_row[mt][0] + (lnf_s.v[2 * q + 1] * lnf_row[mt][1] + lnf_c.v[2 * q + 1]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[q][0][e]), __float_as_uint(v[q][1][e]), false, false);
                v[q][0][e] = __uint_as_float(sw[0]);
                v[q][1][e] = __uint_as_float(sw[1]);
            }
        }
        if ((EPI == 0 || EPI == 1) && !SAVE) {
            // no row operand, one output: the arithmetic runs in the old layout and the PACKED result is re-dealt (half the
            // DPP moves)
            if (EPI == 1) {
                v[0][0] = gelu_bf16_4(v[0][0]); v[0][1] = gelu_bf16_4(v[0][1]);
                v[1][0] = gelu_bf16_4(v[1][0]); v[1][1] = gelu_bf16_4(v[1][1]);
            }
            u32x4 o0 = pack(v[0][0], v[0][1]), o1 = pack(v[1][0], v[1][1]);
            g3r_rows8_packed(o0, o1);
            __builtin_amdgcn_raw_buffer_store_b128(g3r_lanes(o0, to_mem), crs, (int)(coff + (2 * mt) * cstep), 0, G3_POL_C);
            __builtin_amdgcn_raw_buffer_store_b128(g3r_lanes(o1, to_mem), crs, (int)(coff + (2 * mt + 1) * cstep), 0, G3_POL_C);
            continue;
        }
        g3r_rows8(v[0][0], v[0][1], v[1][0], v[1][1]);
        float st_s[2], st_q[2], st_p[2];        // (STATS) this slab's two half slabs
#pragma unroll
        for (int h = 0; h < 2; ++h) {           // half A: rows 0..7 of the slab, half B: rows 8..15
            f32x4 v0 = v[h][0], v1 = v[h][1];
            if (EPI == 1) {
                if (PRE == 2 || G8S) {
                    // gelu and gelu' from the same Phi / Gaussian parts: the backward GEMM multiplies by the saved factor.  (The
                    // erf form stays here: with BOTH outputs wanted it shares one exponential between them, and the two
                    // polynomial chains of the bf16-mode forms measured no faster -- 344 against 339 us per fc1 launch.)
                    f32x4 ph0, ga0, ph1, ga1;
                    phi_parts4(v0, ph0, ga0);
                    phi_parts4(v1, ph1, ga1);
                    const f32x4 d0 = ph0 + v0 * ga0 * 0.3989422804014327f, d1 = ph1 + v1 * ga1 * 0.3989422804014327f;
                    if (G8S) {
                        const u32x4 q8 = lanes2(pack8(d0, d1), to_mem);
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{q8[0], q8[1]}, prs, (int)(poff + (2 * mt + h) * pstep), 0, G3_POL_P);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b128(g3r_lanes(pack(d0, d1), to_mem), prs, (int)(poff + (2 * mt + h) * pstep), 0, G3_POL_P);
                    }
                    v0 *= ph0;
                    v1 *= ph1;
                } else {
                    if (SAVE) __builtin_amdgcn_raw_buffer_store_b128(g3r_lanes(pack(v0, v1), to_mem), prs, (int)(poff + (2 * mt + h) * pstep), 0, G3_POL_P);
                    v0 = gelu_bf16_4(v0);
                    v1 = gelu_bf16_4(v1);
                }
            }
            if (EPI == 6) { v0 *= ro[h][0]; v1 *= ro[h][1]; }
            if (EPI == 3) {
                v0 *= gelu_bf16_grad4(ro[h][0]);
                v1 *= gelu_bf16_grad4(ro[h][1]);
            }
            if (EPI == 2) { v0 += ro[h][0]; v1 += ro[h][1]; }
            const u32x4 pk = pack(v0, v1);
            if (STATS) {
                // the values AS STORED (rounded to bf16): what the LayerNorm behind this launch reads
                unpack(pk, v0, v1);
                // pivot: chunk 0 of the row lives in lane (r & 7) of lane row 0
                unsigned pu = __float_as_uint(v0[0]);
                pu = __builtin_amdgcn_update_dpp(pu, pu, 0x128, 0xf, 0xc, false);                    // lanes 8..15 <- lanes 0..7
                pu = __builtin_amdgcn_permlane16_swap(pu, pu, false, false)[0];                       // lane rows 1, 3 <- rows 0, 2
                pu = __builtin_amdgcn_permlane32_swap(pu, pu, false, false)[0];                       // lane rows 2, 3 <- rows 0, 1
                const float P = __uint_as_float(pu);
                const f32x4 d0 = v0 - P, d1 = v1 - P;
                const f32x4 sd = d0 + d1, qd = d0 * d0 + d1 * d1;
                st_s[h] = (sd[0] + sd[1]) + (sd[2] + sd[3]);
                st_q[h] = (qd[0] + qd[1]) + (qd[2] + qd[3]);
                st_p[h] = P;
            }
            __builtin_amdgcn_raw_buffer_store_b128(g3r_lanes(pk, to_mem), crs, (int)(coff + (2 * mt + h) * cstep), 0, EPI == 2 ? G3_POL_C_RES : G3_POL_C);
        }
        if (STATS) {
            // reduce-scatter over the eight lanes of a row: lane bit 3 (DPP) picks the half slab, bit 4 (permlane16) the slab of
            // a pair, bit 5 (permlane32) the pair of a quadruple; after slab 3 / 7 one finished value per lane and quantity
            auto ror8 = [](float x) { return x + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0x128, 0xf, 0xf, true)); };
            const bool b3 = (lane >> 3) & 1, b4 = (lane >> 4) & 1, b5 = (lane >> 5) & 1;
            const float a_s0 = ror8(st_s[0]), a_s1 = ror8(st_s[1]), a_q0 = ror8(st_q[0]), a_q1 = ror8(st_q[1]);
            st_a[mt & 1][0] = b3 ? a_s1 : a_s0;
            st_a[mt & 1][1] = b3 ? a_q1 : a_q0;
            st_a[mt & 1][2] = b3 ? st_p[1] : st_p[0];
            if (mt & 1) {
                auto fold16 = [](float x, float y) {
                    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
                };
                const int k = (mt >> 1) & 1;
                st_b[k][0] = fold16(st_a[0][0], st_a[1][0]);
                st_b[k][1] = fold16(st_a[0][1], st_a[1][1]);
                st_b[k][2] = b4 ? st_a[1][2] : st_a[0][2];
                if ((mt & 3) == 3) {
                    auto fold32 = [](float x, float y) {
                        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
                        return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
                    };
                    const float S = fold32(st_b[0][0], st_b[1][0]), Q = fold32(st_b[0][1], st_b[1][1]);
                    const float P = b5 ? st_b[1][2] : st_b[0][2];
                    // this lane's row of slabs mt - 3 .. mt: slab 4 (mt >> 2) + 2 b5 + b4, half b3, row r & 7
                    const float ds = S * (1.0f / 64.0f);
                    const u32x2 out = {__float_as_uint(P + ds), __float_as_uint(Q - S * ds)};
                    const int srow = wr * WROWS + 16 * (4 * (mt >> 2) + 2 * (int)b5 + (int)b4) + 8 * (int)b3 + (lane & 7);
                    asm volatile("ds_write_b64 %0, %1" ::"v"(lds_stats + (uint32_t)(srow * 32 + wc * 8)), "v"(out) : "memory");
                }
            }
        }
    }
    if (STATS) {
        // behind the last store: the four wave columns' (mean, M2) over 64 columns each -> ONE pair per row over the tile's 256 columns
        // (Chan's combination for equal counts, pairwise; thread t of the workgroup: row t >> 1 of the item, wave columns 2 (t & 1) + {0, 1},
        // the two halves of a row meet through one DPP swap), one 8-byte store per row -- a quarter of the partials, and of the
        // statistics stores, of the per-wave-column form; what the consumer (PRE 5) or me_row_stats_combine folds is 3 pairs per row at
        // C = 768 instead of 12.  Both wave rows stand side by side here (see gemm_g3r_kernel), so the barrier costs the skew of one epilogue.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int t = s.wave * 64 + lane, lr = t >> 1, h = t & 1;
        u32x4 raw;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(raw) : "v"(lds_stats + (uint32_t)(lr * 32 + h * 16)) : "memory");
        const float ma = __uint_as_float(raw[0]), qa = __uint_as_float(raw[1]), mb = __uint_as_float(raw[2]), qb = __uint_as_float(raw[3]);
        const float d1 = mb - ma;
        const float m1 = (ma + mb) * 0.5f, q1 = (qa + qb) + d1 * d1 * 32.0f;                 // n = 64 + 64
        auto swap1 = [](float x) { return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), 0xB1, 0xf, 0xf, true)); };      // quad_perm [1, 0, 3, 2]
        const float mo = swap1(m1), qo = swap1(q1);
        const float d2 = mo - m1;
        const u32x2 tot = {__float_as_uint((m1 + mo) * 0.5f), __float_as_uint((q1 + qo) + d2 * d2 * 64.0f)};      // n = 128 + 128
        __builtin_amdgcn_raw_buffer_store_b64(tot, srs, h == 0 ? lr * 8 : (int)0x80000000u, 0, 0);
    }
    if (LNP) {
        // the next item's pairs, behind this item's last store (the other pair buffer: slower waves may still be reading this item's)
        __builtin_amdgcn_sched_barrier(0);
        g3r_parts_fold(p, lnp, s.wave, lds_tick + 64 + (uint32_t)(par ^ 1) * 2048);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (HALF) {
        // as many memory operations as a whole tile's epilogue issues behind the A-Y half-tile (stores: half of them went out
        // above; late row-operand loads: a whole tile issues 2 (8 - AHEAD) of them, this one none)
        constexpr int PAD = (SAVE ? 16 : 8) + ((EPI == 2 || EPI == 6) ? 4 : EPI == 3 ? 8 : 0) ;      // (the statistics store: one per lane for either item kind)
        const u32x4 z = {0u, 0u, 0u, 0u};
        const __amdgpu_buffer_rsrc_t none = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < PAD; ++i) __builtin_amdgcn_raw_buffer_store_b128(z, none, 0, 0, 0);
    }
    // the next tile's accumulators start at its bias (s.binit)
    __builtin_amdgcn_sched_barrier(0);
    g3r_set_binit(s, nb, next_zero);
    if (ctr && s.wave == 0) {
        // everything this epilogue issued behind the draw may stay in flight: the A-Y half-tile (2), the bias (4), the
        // stores (16 / 32, padding included) and the row operands (16; a 128-row item 8 + 4 or 8 of the padding)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + 4 + 16 + (SAVE ? 16 : 0) + ((EPI == 2 || EPI == 3 || EPI == 6) ? (HALF ? 8 : 16) : 0)) : "memory");
        g3r_publish(drawn, ctr, nx, lds_tick);
    }
}

// memory operations one g3_epilogue_r issues per wave behind the next tile's A-Y half-tile: >= the stores (+ the later
// row-operand loads); an under-count only makes the wait stricter
template <int EPI, int PRE> constexpr int g3r_seam() { return (PRE == 1 || PRE == 2 || (PRE == 6 && EPI == 1)) ? 32 : EPI >= 2 ? 20 : 16; }

// HI: this instantiation also carries the 128-row item form (run_item<HALF>): a second K-loop and epilogue in the kernel.  Only the
// bias-only forms are built with it (launch3r): around the row-operand epilogues the extra scalar state pushed 16-27 VGPRs of
// per-item spills into the seams (fc2 dgrad 244 -> 280 us in the training step), for items that buy next to nothing there.
template <int EPI, int PRE, bool HI = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_g3r_kernel(const GemmParams p) {
    constexpr int SEAM = g3r_seam<EPI, PRE>();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2;

    const int bid = blockIdx.x, xcd = bid & 7, c = bid >> 3, G8 = gridDim.x >> 3;
    const int tiles = p.tiles_m * p.tiles_n, F = p.g3_full_tiles;
    const int nwork = F + (tiles - F) * 2;                             // (F == tiles unless p.g3_half)
    const int nf = (F >> 3) + (xcd < (F & 7) ? 1 : 0);                 // whole tiles / all items of this XCD
    const int nx = (nwork >> 3) + (xcd < (nwork & 7) ? 1 : 0);
    const int base_f = xcd * (F >> 3) + (xcd < (F & 7) ? xcd : (F & 7));
    const int base_all = xcd * (nwork >> 3) + (xcd < (nwork & 7) ? xcd : (nwork & 7));
    const int nkt = (int)(p.K / G3_BK);
    auto decode = [&](int slot, int& tile, int& part, int& kt0, int& kt1) {
        part = -1; kt0 = 0; kt1 = nkt;
        if (slot < nf) {
            tile = base_f + slot;
        } else {
            // a tile of the last, mostly empty round: two 128-row items (part = which half), the whole reduction each
            const int pi = base_all - base_f + (slot - nf);
            tile = F + (pi >> 1);
            part = pi & 1;
        }
    };
    auto src_of = [&](int tile, int part, int& tm, int& tn) {
        tm = __builtin_amdgcn_readfirstlane(tile / p.tiles_n);
        tn = tile - tm * p.tiles_n;
        return part >= 0 ? g3_make_src_half(p, tm, tn, part, wr) : g3_make_src(p, tm, tn);
    };
    const bool dyn = p.g3_tickets != nullptr;
    unsigned* const ctr = dyn ? p.g3_tickets + xcd * 16 : nullptr;
    const uint32_t lds_tick = (uint32_t)(uintptr_t)smem + G3_LDS;
    int slot = c;
    if (slot >= nx) return;

    G3State s;
    g3_init_lane(s, p, smem, wave, lane);
    const G3Src null = g3_null_src(p);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? (int)(p.N * 4) : 0, 0x00020000);
    // SEAM stores nothing admits: the in-order queue looks the same ahead of the first item as behind an epilogue
    auto prime = [&]() {
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < SEAM; ++i) __builtin_amdgcn_raw_buffer_store_b128(z, null.a, 0, 0, 0);
    };

    unsigned drawn0 = 0;
    if (dyn && wave == 0) drawn0 = g3r_draw(ctr);          // item 1 (item 0 is this workgroup's own slot)

    int tile, part, kt0, kt1, tm, tn;
    decode(slot, tile, part, kt0, kt1);
    G3Src cur = src_of(tile, part, tm, tn);
    g3_issue<0>(s, cur, 0, kt0); g3_issue<1>(s, cur, 0, kt0); g3_issue<2>(s, cur, 0, kt0); g3_issue<3>(s, cur, 0, kt0);
    g3_issue<0>(s, cur, 1, kt0 + 1); g3_issue<1>(s, cur, 1, kt0 + 1); g3_issue<2>(s, cur, 1, kt0 + 1); g3_issue<3>(s, cur, 1, kt0 + 1);
    {
        const G3Bias b0 = g3r_bias(brs, tn, wave, lane);
        g3r_set_binit(s, b0, PRE == 3 || PRE == 5);
    }
    if (PRE == 5) {      // the first item's LayerNorm pairs (every later item's are folded behind the epilogue in front of it)
        const int64_t m00 = (int64_t)tm * G3_BM + (part >= 0 ? part * 128 : 0);
        int64_t r0 = p.M - m00;
        r0 = r0 < (part >= 0 ? 128 : 256) ? r0 : (part >= 0 ? 128 : 256);
        const G3Parts q0 = g3r_parts_load(p, m00, r0 > 0 ? (int)r0 : 0, wave);
        g3r_parts_fold(p, q0, wave, lds_tick + 64);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (dyn && wave == 0) g3r_publish(drawn0, ctr, nx, lds_tick);
    prime();
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();

    int item_par = 0;                    // (PRE 5) which LDS pair buffer holds the current item's LayerNorm pairs
    // Which item comes next: static (slot + G8: every workgroup owns a fixed list) or, with p.g3_tickets, CLAIMED from the
    // XCD's counter -- a CU that is slow, or that could not take its workgroup for a while because a communication kernel
    // sat on it, then simply ends up with fewer tiles instead of holding the whole launch back (the first item stays static:
    // no round trip before the first DMA).  Wave 0 draws one item ahead: in the prologue for item 1, at the top of the
    // epilogue of item i (ahead of its stores, so that retiring the draw does not drain them) for item i + 2, and leaves the
    // ticket in one LDS word; every wave picks it up behind the first K-tile pair of the following item (>= 2 pairs per item
    // and whole tiles only in this mode: launch3r).  Tickets 0 .. nx - 1 are drawn per XCD and launch (nx - G8 hits, one miss
    // per workgroup): whoever draws the last one zeroes the counter for the next launch on this stream.
    while (true) {
        int nslot = 0, ntile = tile, npart = -1, nkt0 = 0, nkt1 = 2, ntm = 0, ntn = 0;
        bool has_next = false;
        G3Src nxt = null;
        auto resolve_next = [&](int ns) {
            nslot = ns;
            has_next = ns < nx;
            if (has_next) {
                decode(nslot, ntile, npart, nkt0, nkt1);
                nxt = src_of(ntile, npart, ntm, ntn);
            }
        };
        if (!dyn) resolve_next(slot + G8);
        const int np = (kt1 - kt0) >> 1;
        // One item: the K-loop and the epilogue, instantiated for whole tiles and for 128-row items (HALF).  The two forms meet
        // only behind their epilogues, where no accumulator is live.
        auto run_item = [&](auto half_tag) {
            constexpr bool HALF = decltype(half_tag)::value;
            {
                G3Src sb = cur;
                int kb = kt0 + 2, kc = kt0 + 3;
                if (np == 1) { sb = nxt; kb = nkt0; kc = nkt0 + 1; }
                g3_ktile<0, false, SEAM, HALF>(s, cur, 0, sb, kb);
                g3_ktile<1, false, 0, HALF, HALF ? SEAM : 0>(s, sb, kb, sb, kc);
            }
            if (dyn) {
                unsigned t;
                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(t) : "v"(lds_tick) : "memory");
                resolve_next(G8 + (int)__builtin_amdgcn_readfirstlane(t));
            }
            for (int i = 1; i < np; ++i) {
                const int k = kt0 + 2 * i;
                G3Src sb = cur;
                int kb = k + 2, kc = k + 3;
                if (i == np - 1) { sb = nxt; kb = nkt0; kc = nkt0 + 1; }
                g3_ktile<0, false, 0, HALF>(s, cur, k + 1, sb, kb);
                g3_ktile<1, false, 0, HALF>(s, sb, kb, sb, kc);
            }
            // the two wave rows run their epilogues SIDE BY SIDE: left one barrier apart, row 1 could not start its epilogue
            // before row 0 had finished its own and reached the next K-tile's first barrier, and row 0 would then wait out
            // row 1's (measured with per-item time stamps: 4.6 k of 40 k clocks per tile).  Row 0 gives up its one-barrier
            // lead here and row 1 re-opens it behind the epilogue.
            if (wr == 0) __builtin_amdgcn_s_barrier();
            int64_t nm0 = 0;
            int nrows = 0;
            if (PRE == 5 && has_next) {
                nm0 = (int64_t)ntm * G3_BM + (npart >= 0 ? npart * 128 : 0);
                const int64_t left = p.M - nm0, cap = npart >= 0 ? 128 : 256;
                nrows = (int)(left < cap ? (left > 0 ? left : 0) : cap);
            }
            g3_epilogue_r<EPI, PRE, HALF>(p, s, (int64_t)tm * G3_BM + (HALF ? part * 128 : 0), tn, 0, nxt, nkt0 + 1, brs, ntn, PRE == 3 || PRE == 5,
                                          has_next ? ctr : nullptr, nx, lds_tick, nm0, nrows, item_par);
        };
        if constexpr (HI) {
            if (part >= 0) run_item(std::true_type{});
            else run_item(std::false_type{});
        } else {
            run_item(std::false_type{});
        }
        if (!has_next) break;
        if (wr == 1) __builtin_amdgcn_s_barrier();
        item_par ^= 1;
        slot = nslot; tile = ntile; part = npart; kt0 = nkt0; kt1 = nkt1; tm = ntm; tn = ntn;
        cur = nxt;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the trailing null DMAs must land before the LDS is released
}

// ---- wgrad: one (output tile, K-range) per workgroup; raw fp32 partial sums into slab blockIdx.y ... the deterministic
// fold (splitk_reduce_kernel, gemm.hip) sums the slabs and applies the epilogue.  The plain form of the walk in gemm3_core.h
// (g3_tn_part, g3_tn_walk).
// The fold stays a separate launch: inside this kernel it measured 211 us per wgrad launch against 176 us for kernel + fold (round
// 4) -- there the slab write-through, the wait for the tile row and the read-back are exposed one after the other on every CU.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_g3tn_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2;
    const G3TnPart w = g3_tn_part(p, xcd_major_wgid(blockIdx.x, gridDim.x));

    G3State s;
    g3_init_lane_tn(s, p, smem, wave, lane);
    g3_zero(s);
    G3Turn turn = g3_tn_colsum_begin(s, p, w.tn);
    g3_tn_walk(s, p, g3_make_src_tn(p, w.tm, w.tn), w.kt0, w.kt1, wr, turn);
    g3_tn_store_colsum(p, s, (int64_t)w.split * p.tiles_n + w.tn, w.m0, lane);      // [split * tiles_n + tn][M]
    g3_epilogue<5>(p, s, w.m0, w.n0, lane, reinterpret_cast<float*>(p.C) + (int64_t)w.split * p.slab_stride, 0);
}


// ---- wgrad on a workgroup count that is NOT a multiple of the tile count (a communication kernel holds R CUs: me_gemm_reserve_cus).  The
// (tile, split) grid above gives every workgroup one whole item and wants all 256 CUs at once; with ANY CU held its last workgroups run as a
// SECOND ROUND (+100 % per launch, +3.5 % per train step for R = 8 .. 32: profiles/r05_contention.txt), and a uniform split for 256 - R slots
// quantises badly (36 tiles on 240 slots: 6 parts of 132 K-tiles instead of 7 of 114 = +16 %).  Here p.sk_wgs workgroups carry the same load:
//   * workgroups [0, S T): S = p.sk_levels whole split levels of L1 = p.sk_l1 K-tile pairs per tile, split-major exactly as above -- the
//     workgroups an XCD runs together read the SAME rows of dY and X (a first version that cut the whole tile-major unit list evenly lost
//     that sharing: every workgroup streamed private rows, ~5x the operand traffic, +22 % on the weight gradients: profiles/r06_contention.txt);
//   * the E = sk_wgs - S T workgroups left over share the LEFTOVER U - S L1 pairs of every tile as one tile-major list, evenly, across tile
//     boundaries: such a workgroup may end one tile and begin the next (a segment and a slab each).
// Parts stay static -- a part is a fixed K range and a fixed slab, the fold sums a tile's slabs in K order (levels, then leftover parts) -- so
// the result is bit-reproducible per (shape, workgroups).  Bias gradient: the N-tiles of a tile row share the column sums round-robin pair by
// pair ([level x tiles_n + tn][M] partial rows for the levels, [S tiles_n + leftover part x tiles_n + tn][M] for the leftover segments).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void gemm_g3tn_sk_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2;
    const int wgid = xcd_major_wgid(blockIdx.x, gridDim.x);
    const int T = p.tiles_m * p.tiles_n, S = p.sk_levels, L1 = p.sk_l1, E = p.sk_wgs - S * T, Ul = p.sk_upt - S * L1;
    const int64_t TUl = (int64_t)T * Ul;
    const bool regular = wgid < S * T;
    // leftover workgroups: units [u0, u1) of the tile-major leftover list; a regular workgroup is one segment (u0 = 0, u1 = 1: one pass)
    int64_t u0 = 0, u1 = 1;
    if (!regular) {
        const int e = wgid - S * T;
        u0 = __builtin_amdgcn_readfirstlane((int)((int64_t)e * TUl / E));
        u1 = __builtin_amdgcn_readfirstlane((int)((int64_t)(e + 1) * TUl / E));
    }
    G3State s;
    g3_init_lane_tn(s, p, smem, wave, lane);
    while (u0 < u1) {
        int tile, kt0, kt1, part, cs_row;
        int64_t ue;
        if (regular) {
            const int level = __builtin_amdgcn_readfirstlane(wgid / T);
            tile = wgid - level * T;
            kt0 = level * L1 * 2; kt1 = kt0 + L1 * 2;
            part = level;
            ue = u1;
        } else {
            tile = __builtin_amdgcn_readfirstlane((int)(u0 / Ul));
            const int64_t tu0 = (int64_t)tile * Ul;
            ue = u1 < tu0 + Ul ? u1 : tu0 + Ul;
            kt0 = (S * L1 + (int)(u0 - tu0)) * 2; kt1 = (S * L1 + (int)(ue - tu0)) * 2;
            part = S + (wgid - S * T) - sk_first(tile, E, Ul, TUl);
        }
        const int tm = __builtin_amdgcn_readfirstlane(tile / p.tiles_n), tn = tile - tm * p.tiles_n;
        cs_row = regular ? part * p.tiles_n + tn : S * p.tiles_n + (part - S) * p.tiles_n + tn;
        const int64_t m0 = (int64_t)tm * G3_BM, n0 = (int64_t)tn * G3_BN;
        g3_zero(s);
        // column sums: inside a level all N-tiles of a tile row walk the same K range; the leftover segments of different N-tiles are ragged
        // (G3Turn: the turn follows the absolute pair index)
        G3Turn turn = g3_tn_colsum_begin(s, p, regular ? tn : (tn + p.tiles_n - ((kt0 >> 1) % p.tiles_n)) % p.tiles_n);
        g3_tn_walk(s, p, g3_make_src_tn(p, tm, tn), kt0, kt1, wr, turn);      // (drained: the next segment may refill the LDS)
        g3_tn_store_colsum(p, s, cs_row, m0, lane);
        g3_epilogue<5>(p, s, m0, n0, g3_lane_now(), reinterpret_cast<float*>(p.C) + (int64_t)part * p.slab_stride, 0);
        u0 = ue;
    }
}


// The work counters of the resident kernel: every stream gets its own set (launches on a stream are serialised, and the
// kernel leaves its counters at zero), handed out on the host from a per-device pool (keyed by the STREAM's device) that is
// allocated and zeroed once, at the first resident launch on the device; a set is zeroed again, on its own stream, when it is
// first handed to a stream.  A launch that is being CAPTURED into a hipGraph always runs the static schedule: a kernel node
// keeps the counter set of its capture stream, but replays run on whatever stream launches the graph (torch.cuda.graph
// captures every graph on one shared stream), so replays on different streams -- or a replay next to eager work on the capture
// stream -- would draw from ONE set and break the "exactly nx draws, the last one resets" invariant.  On a free GPU the two
// schedules time the same; claiming matters next to a communication kernel, i.e. in eager training.
unsigned* g3r_tickets(hipStream_t stream) {
    constexpr int SETS = 64, SET_WORDS = 8 * 16;
    struct Pool {
        unsigned* base = nullptr;
        bool failed = false;
        int next = 0;
        std::map<hipStream_t, int> idx;
    };
    static std::mutex mu;
    static std::map<int, Pool> pools;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;      // static schedule
    int dev = 0;
    if (hipStreamGetDevice(stream, &dev) != hipSuccess) (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    Pool& P = pools[dev];
    if (!P.base) {
        if (P.failed) return nullptr;
        unsigned* buf = nullptr;
        if (hipMalloc(&buf, (size_t)SETS * SET_WORDS * sizeof(unsigned)) != hipSuccess ||
            hipMemset(buf, 0, (size_t)SETS * SET_WORDS * sizeof(unsigned)) != hipSuccess) {
            P.failed = true;
            return nullptr;
        }
        P.base = buf;
    }
    auto it = P.idx.find(stream);
    if (it == P.idx.end()) {
        if (P.next >= SETS) return nullptr;
        unsigned* set = P.base + (size_t)P.next * SET_WORDS;
        if (hipMemsetAsync(set, 0, SET_WORDS * sizeof(unsigned), stream) != hipSuccess) return nullptr;
        it = P.idx.emplace(stream, P.next++).first;
    }
    return P.base + (size_t)it->second * SET_WORDS;
}

template <int EPI, int PRE> int launch3r(const GemmParams& q0, int G, hipStream_t stream) {
    // which forms carry the 128-row items (see the kernel): the plain, residual and GELU kernels (fc1's 2 364 tiles leave a last round of
    // 60); not the x-row-operand kernel (fc2 dgrad, the same 2 364 tiles: 243 -> 251 us sustained with them, measured and removed)
    constexpr bool HI = EPI == 0 || EPI == 2 || EPI == 1;
    constexpr int LDS_BYTES = G3_LDS + 64 + (PRE == 5 ? 4096 : PRE == 4 ? 8192 : 0);      // operand buffers + the ticket word (+ PRE 5: two buffers of 256 LayerNorm row pairs; PRE 4: 256 rows x 4 wave columns of partial pairs)
    GemmParams q = q0;
    // Tile quantisation: T tiles on G resident workgroups take ceil(T / G) rounds, and the encoder's N = 768 outputs are 591 tiles =
    // 2.31 rounds (N = 3072: 9.23).  When at most half the CUs would work in the last round, its tiles run as two 128-row items
    // each -- same kernel, same epilogue, no slabs (g3_phase<.., HALF>): the last round then costs a little over half a round.
    const int tiles = q.tiles_m * q.tiles_n, rem = tiles % G;
    q.g3_full_tiles = tiles; q.g3_split = 1; q.g3_half = 0;
    if (HI && tiles >= G && rem > 0 && 2 * rem <= G && q.K >= 4 * G3_BK) {
        q.g3_full_tiles = tiles - rem;
        q.g3_half = 1;
    }
    // claimed items need >= 2 K-tile pairs per item (see the kernel)
    q.g3_tickets = q.K >= 4 * G3_BK ? g3r_tickets(stream) : nullptr;
    return launch_kernel<gemm_g3r_kernel<EPI, PRE, HI>>("me_gemm(g3 resident)", dim3((unsigned)G), 512, LDS_BYTES, LDS_BYTES, stream, q);
}

int launch3r_any(int epi, int pre, const GemmParams& q, int G, hipStream_t stream) {
    switch (epi) {
        case 0: return pre == G3_PRE_ROW_PARTS ? launch3r<0, G3_PRE_ROW_PARTS>(q, G, stream) : pre == G3_PRE_ROW_AFFINE ? launch3r<0, G3_PRE_ROW_AFFINE>(q, G, stream) : launch3r<0, G3_PRE_NONE>(q, G, stream);
        case 1: return pre == G3_PRE_GG8 ? launch3r<1, G3_PRE_GG8>(q, G, stream) : pre == G3_PRE_ROW_PARTS ? launch3r<1, G3_PRE_ROW_PARTS>(q, G, stream) :
                       pre == G3_PRE_ROW_AFFINE ? launch3r<1, G3_PRE_ROW_AFFINE>(q, G, stream) : pre == G3_PRE_SAVE_GELU_GRAD ? launch3r<1, G3_PRE_SAVE_GELU_GRAD>(q, G, stream) :
                       pre ? launch3r<1, G3_PRE_SAVE_PREACT>(q, G, stream) : launch3r<1, G3_PRE_NONE>(q, G, stream);
        case 2: return pre == G3_PRE_ROW_STATS ? launch3r<2, G3_PRE_ROW_STATS>(q, G, stream) : launch3r<2, G3_PRE_NONE>(q, G, stream);
        case 3: return launch3r<3, G3_PRE_NONE>(q, G, stream);
        default: return pre == G3_PRE_GG8 ? launch3r<6, G3_PRE_GG8>(q, G, stream) : launch3r<6, G3_PRE_NONE>(q, G, stream);
    }
}

// one tile (or one K-part of a split tail tile) per workgroup
template <int EPI, bool WRAP> int launch3t(const GemmParams& q, int nwg, hipStream_t stream) {
    return launch_kernel<gemm_g3_kernel<EPI, WRAP>>(WRAP ? "me_gemm(g3, wrapped A)" : "me_gemm(g3)", dim3((unsigned)nwg), 512, G3_LDS, G3_LDS, stream, q);
}

template <int EPI> int launch3e(const GemmParams& q, const G3Form& f, hipStream_t stream) {
    // (A held as two planes [hi | lo], three reduction segments: the plain / generic / fp32-residual epilogues only -- g3_form)
    if constexpr (EPI == 0 || EPI == 4 || EPI == 8)
        if (f.kernel == G3_ONE_TILE_WRAP) return launch3t<EPI, true>(q, f.nwg, stream);
    return launch3t<EPI, false>(q, f.nwg, stream);
}

}  // namespace

// the same per-stream counter sets for the other persistent kernels of the library (attention): words 1..15 of a set are free (the
// resident GEMM uses words 0, 16, 32, ...); null while the stream is capturing -> static schedule
unsigned* me_work_counters(hipStream_t stream) { return g3r_tickets(stream); }

// TN: p.split_k slabs of p.ksteps_per_split K-tiles (of 64) each into p.C = [split_k][M][N] fp32
int launch_g3_tn(const GemmParams& p, hipStream_t stream) {
    const int nwg = p.tiles_m * p.tiles_n * p.split_k;
    return launch_kernel<gemm_g3tn_kernel>("me_gemm(g3 tn)", dim3((unsigned)nwg), 512, G3_LDS, G3_LDS, stream, p);
}

int launch_g3_tn_sk(const GemmParams& p, hipStream_t stream) {
    return launch_kernel<gemm_g3tn_sk_kernel>("me_gemm(g3 tn, balanced partition)", dim3((unsigned)p.sk_wgs), 512, G3_LDS, G3_LDS, stream, p);
}

bool g3_tn_supported(const GemmParams& p) {
    // 16-byte chunks of 8 columns; lane offsets and per-K-tile steps are 32-bit; the bounds check spans the whole matrix
    return p.M % 8 == 0 && p.N % 8 == 0 && p.lda % 8 == 0 && p.ldb % 8 == 0 && p.K * p.lda * 2 < (1ll << 31) &&
           p.K * p.ldb * 2 < (1ll << 31);
}

bool g3_supported(const GemmParams& p, int op) {
    if (op != ME_GEMM_NT) return false;
    if (p.K % (2 * G3_BK) != 0 || p.N % 8 != 0) return false;
    // per-tile buffer descriptors and lane offsets are 32-bit
    if (256 * p.lda * 2 >= (1ll << 31) || 256 * p.ldb * 2 >= (1ll << 31)) return false;
    return true;
}

int g3_cu_count() { return device_cus(); }

// The one place that says which NT kernel a descriptor runs on.  The resident form (one workgroup per CU, operand stream running
// through the epilogues) whenever one of its (EPI, PRE) instantiations covers the epilogue, every CU gets work and the output / row
// operands are bf16 with tile-local 32-bit offsets; else the one-tile kernel -- which cannot emit row statistics, fold LayerNorm
// partials or read / write ME_GG8.
G3Form g3_form(const GemmParams& p, int cus) {
    G3Form f;
    const int e = pick_epi_ex(p);
    // (the residual forms carry the column scale -- layer-scale Blocks; the others do not: generic epilogue)
    f.epi = (p.colscale && e != 2 && e != 8) || !((e >= 0 && e <= 3) || (e >= 6 && e <= 10)) ? 4 : e;
    const int EPI = f.epi, tiles = p.tiles_m * p.tiles_n;
    const bool split = p.g3_split > 1 && p.g3_slabs != nullptr;      // tiles [g3_full_tiles, tiles) run as g3_split K-parts each
    f.nwg = split ? p.g3_full_tiles + (tiles - p.g3_full_tiles) * p.g3_split : tiles;
    f.G = cus & ~7;
    if (p.a_wrap_kt) {      // A as two planes [hi | lo], three reduction segments: plain / generic / fp32-residual epilogues (asked of e: before the column-scale rule)
        f.kernel = (e == 0 || e == 4 || e == 8) ? G3_ONE_TILE_WRAP : G3_UNSUPPORTED;
        return f;
    }
    f.repi = EPI <= 3 ? EPI : -1;
    f.pre = (EPI == 1 && p.preact) ? G3_PRE_SAVE_PREACT : G3_PRE_NONE;
    const bool plain = p.beta == 0.0f && p.out_group_rows == 0 && p.res_row_mod == 0 && !p.colscale && !p.residual;
    if (EPI == 4 && p.row_affine && !p.flags && plain && !p.preact && !p.aux) {       // folded LayerNorm (bias / GELU forms)
        f.repi = p.act == ME_ACT_GELU ? 1 : 0;
        f.pre = p.row_nparts ? G3_PRE_ROW_PARTS : G3_PRE_ROW_AFFINE;       // (parts: row_affine holds the 64-column partials of the launch in front, see g3_epilogue_r)
    }
    if (EPI == 4 && p.flags && !p.row_affine) {
        // the two halves of the "save gelu'" pair (pick_epi sends flagged descriptors to the generic epilogue)
        if (plain && p.flags == ME_GEMM_SAVE_GELU_GRAD && p.act == ME_ACT_GELU && p.preact && !p.aux) { f.repi = 1; f.pre = G3_PRE_SAVE_GELU_GRAD; }
        if (plain && p.flags == ME_GEMM_AUX_IS_FACTOR && p.act == ME_ACT_NONE && p.aux && (p.aux_dtype == ME_BF16 || p.aux_dtype == ME_GG8) && !p.preact) f.repi = 6;
    }
    if (EPI == 6) f.repi = 6;                                   // (pick_epi_ex has checked the same conditions)
    if (EPI == 7) { f.repi = 1; f.pre = G3_PRE_SAVE_GELU_GRAD; }
    if (f.repi == 1 && f.pre == G3_PRE_SAVE_GELU_GRAD && p.preact_dtype == ME_GG8) f.pre = G3_PRE_GG8;       // gelu' in eight bits, both halves of the pair
    if (f.repi == 6 && p.aux_dtype == ME_GG8) f.pre = G3_PRE_GG8;
    if (EPI == 2 && p.row_stats) f.pre = G3_PRE_ROW_STATS;
    const int64_t ldmax = std::max(std::max(p.ldc, p.preact ? p.ldpre : 0), std::max(p.residual ? p.ldres : 0, p.aux ? p.ldaux : 0));
    const bool bf16_preact = !(f.pre == G3_PRE_SAVE_PREACT || f.pre == G3_PRE_SAVE_GELU_GRAD) || p.preact_dtype == ME_BF16;
    const bool gg8_rows = f.pre != G3_PRE_GG8 || !p.preact || p.ldpre % 8 == 0;
    const bool resident_only = p.row_stats || p.row_nparts || (p.preact && p.preact_dtype == ME_GG8) || (p.aux && p.aux_dtype == ME_GG8);
    if (f.repi >= 0 && !p.colscale && f.G >= 8 && f.nwg >= f.G && !split && p.alpha == 1.0f && p.c_dtype == ME_BF16 && bf16_preact && gg8_rows &&
        256 * ldmax * 2 < (1ll << 31))
        f.kernel = G3_RESIDENT;
    else
        f.kernel = resident_only ? G3_UNSUPPORTED : G3_ONE_TILE;
    return f;
}

int launch_g3(const GemmParams& p, const G3Form& f, hipStream_t stream) {
    if (f.kernel == G3_UNSUPPORTED) {      // (me_gemm refuses these from the form, each with its own message, before it comes here)
        me_set_error("me_gemm(g3): no kernel serves this descriptor");
        return ME_ERR_UNSUPPORTED;
    }
    GemmParams q = p;
    if (q.g3_split <= 1 || q.g3_slabs == nullptr) { q.g3_full_tiles = q.tiles_m * q.tiles_n; q.g3_split = 1; q.g3_ktp = 0; q.g3_slabs = nullptr; }
    if (f.kernel == G3_RESIDENT) return launch3r_any(f.repi, f.pre, q, f.G, stream);
    switch (f.epi) {
        case 0: return launch3e<0>(q, f, stream);
        case 1: return launch3e<1>(q, f, stream);
        case 2: return launch3e<2>(q, f, stream);
        case 3: return launch3e<3>(q, f, stream);
        case 6: return launch3e<6>(q, f, stream);
        case 7: return launch3e<7>(q, f, stream);
        case 8: return launch3e<8>(q, f, stream);
        case 9: return launch3e<9>(q, f, stream);
        case 10: return launch3e<10>(q, f, stream);
        default: return launch3e<4>(q, f, stream);
    }
}
