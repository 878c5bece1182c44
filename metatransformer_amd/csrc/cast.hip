// cast.hip -- dtype casts and weight repacks: me_cast, the ME_BF16X3 plane split (me_split3) and the transposed / batched
// copies of the encoder weights (me_transpose_cast, me_transpose_cast_batched, me_split3_batched).
// Pure load, convert, store: coalesced 16-byte accesses, grid-stride loops, LDS only where a transpose needs it.
#include "common.h"

namespace {

// fp16 exists at the boundary only (ME_F16: storage dtype of me_cast / me_transpose_cast -- `.half()` checkpoints and
// fp16-autocast call sites are converted to bf16 / fp32 on the way in and back on the way out; no kernel computes in it)
__device__ __forceinline__ float ld1_any(const void* base, int dt, int64_t i) {
    if (dt == ME_F16) return (float)reinterpret_cast<const _Float16*>(base)[i];
    return load1_as_f32(base, dt, i);
}
__device__ __forceinline__ void st1_any(void* base, int dt, int64_t i, float v) {
    if (dt == ME_F16) reinterpret_cast<_Float16*>(base)[i] = (_Float16)v;
    else store1_from_f32(base, dt, i, v);
}
__global__ __launch_bounds__(EW_THREADS) void cast_any_kernel(const void* __restrict__ src, int sdt, void* __restrict__ dst,
                                                              int ddt, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * EW_THREADS)
        st1_any(dst, ddt, i, ld1_any(src, sdt, i));
}

__global__ __launch_bounds__(EW_THREADS) void cast_kernel(const void* __restrict__ src, int sdt, void* __restrict__ dst,
                                                          int ddt, int64_t n) {
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS)
        store4_from_f32(dst, ddt, i * 4, load4_as_f32(src, sdt, i * 4));
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = n4 * 4 + threadIdx.x;
        store1_from_f32(dst, ddt, i, load1_as_f32(src, sdt, i));
    }
}

}  // namespace

extern "C" int me_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(src && dst && n >= 0, "me_cast: bad args");
    ME_CHECK_ARG(me_storage_dtype_ok(src_dtype) && me_storage_dtype_ok(dst_dtype), "me_cast: bad dtype");
    if (n == 0) return ME_OK;
    if (src_dtype == ME_F16 || dst_dtype == ME_F16 || !aligned4(src, src_dtype) || !aligned4(dst, dst_dtype)) {      // (a slice that starts off a four-element boundary: element by element)
        hipLaunchKernelGGL(cast_any_kernel, dim3(grid_blocks(n)), dim3(EW_THREADS), 0, stream, src, src_dtype, dst, dst_dtype, n);
        ME_CHECK_LAUNCH("me_cast");
        return ME_OK;
    }
    hipLaunchKernelGGL(cast_kernel, dim3(grid_blocks(n / 4 + 1)), dim3(EW_THREADS), 0, stream, src, src_dtype, dst, dst_dtype, n);
    ME_CHECK_LAUNCH("me_cast");
    return ME_OK;
}

namespace {

// fp32 [rows, cols] -> ME_BF16X3 [rows, 3 * cols]: one read of the fp32 values, three bf16 plane stores (6 bytes per element)
__global__ __launch_bounds__(EW_THREADS) void split3_kernel(const float* __restrict__ src, int64_t ld_src, uint16_t* __restrict__ dst,
                                                            int64_t rows, int64_t cols, int right_operand) {
    const int64_t q = cols / 4, n4 = rows * q;
    for (int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * EW_THREADS) {
        const int64_t r = i / q, c = (i - r * q) * 4;
        store4_split3(dst + r * 3 * cols, cols, c, *reinterpret_cast<const f32x4*>(src + r * ld_src + c), right_operand != 0);
    }
}

// batched forms: the block finds its matrix by walking the (<= 48 entry) tile-count prefix.  On return item k holds the block's
// tile t, tx_tiles tiles to a tile row; false for a block past the last tile.
__device__ __forceinline__ bool tc_find_tile(const me_tc_batch& b, int& k, int64_t& t, int64_t& tx_tiles) {
    t = blockIdx.x;
    k = 0;
    tx_tiles = 0;
    for (; k < b.n; ++k) {
        tx_tiles = (b.item[k].cols + 63) / 64;
        const int64_t nt = tx_tiles * ((b.item[k].rows + 63) / 64);
        if (t < nt) break;
        t -= nt;
    }
    return k < b.n;
}

// fp32 weights -> ME_BF16X3 right-operand planes [hi | hi | lo], of W itself (transposed = 0: dst [rows, 3 cols]) or of W^T
// (transposed = 1: dst [cols, 3 rows], the dgrad GEMMs' B operand), for up to ME_TC_BATCH matrices in one launch.  Same 64 x 64 tiles as
// the batched transpose; rows and cols multiples of 4.
__global__ __launch_bounds__(256) void split3_batched_kernel(const me_tc_batch b, int transposed, int right_operand) {
    __shared__ float tile[64][65];
    int64_t t, tx_tiles;
    int k;
    if (!tc_find_tile(b, k, t, tx_tiles)) return;
    const float* src = reinterpret_cast<const float*>(b.item[k].src);
    uint16_t* dst = reinterpret_cast<uint16_t*>(b.item[k].dst);
    const int64_t rows = b.item[k].rows, cols = b.item[k].cols;
    const int64_t r0 = (t / tx_tiles) * 64, c0 = (t % tx_tiles) * 64;
    const int q = threadIdx.x & 15, p = threadIdx.x >> 4;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int i = p + 16 * pass;
        const int64_t r = r0 + i, c = c0 + 4 * q;
        if (r < rows && c < cols) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + r * cols + c);
            if (!transposed) {
                store4_split3(dst + r * 3 * cols, cols, c, v, right_operand != 0);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) tile[i][4 * q + e] = v[e];
            }
        }
    }
    if (!transposed) return;          // (block-uniform)
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int i = p + 16 * pass;
        const int64_t c = c0 + i, r = r0 + 4 * q;
        if (c < cols && r < rows)
            store4_split3(dst + c * 3 * rows, rows, r, f32x4{tile[4 * q][i], tile[4 * q + 1][i], tile[4 * q + 2][i], tile[4 * q + 3][i]}, right_operand != 0);
    }
}

// dst[c, r] = src[r, c]; 64x64 tiles through LDS (padded), coalesced on both sides
__global__ __launch_bounds__(256) void transpose_cast_batched_kernel(const me_tc_batch b) {
    __shared__ float tile[64][65];
    int64_t t, tx_tiles;
    int k;
    if (!tc_find_tile(b, k, t, tx_tiles)) return;
    const void* src = b.item[k].src;
    void* dst = b.item[k].dst;
    const int64_t rows = b.item[k].rows, cols = b.item[k].cols;
    const int64_t r0 = (t / tx_tiles) * 64, c0 = (t % tx_tiles) * 64;
    const int ssz = b.src_dtype == ME_F32 ? 4 : 2, dsz = b.dst_dtype == ME_F32 ? 4 : 2;
    if (b.src_dtype != ME_F16 && b.dst_dtype != ME_F16 && rows % 4 == 0 && cols % 4 == 0 && (uintptr_t)src % (4 * ssz) == 0 && (uintptr_t)dst % (4 * dsz) == 0) {      // (block-uniform)
        // four elements per lane on both sides: 16 lanes read 64 columns of a row (128 / 256 contiguous bytes), 16 lanes write 64 rows
        // of a destination row; the 65-word tile rows keep both LDS passes conflict-free (bank = row + column)
        const int q = threadIdx.x & 15, p = threadIdx.x >> 4;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int i = p + 16 * pass;
            const int64_t r = r0 + i, c = c0 + 4 * q;
            const f32x4 v = (r < rows && c < cols) ? load4_as_f32(src, b.src_dtype, r * cols + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[i][4 * q + e] = v[e];
        }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int i = p + 16 * pass;
            const int64_t c = c0 + i, r = r0 + 4 * q;
            if (c < cols && r < rows) store4_from_f32(dst, b.dst_dtype, c * rows + r, f32x4{tile[4 * q][i], tile[4 * q + 1][i], tile[4 * q + 2][i], tile[4 * q + 3][i]});
        }
        return;
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int64_t r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? ld1_any(src, b.src_dtype, r * cols + c) : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int64_t c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) st1_any(dst, b.dst_dtype, c * rows + r, tile[tx][i]);
    }
}

// what every item of a batch must be, and what me_split3_batched's four-wide kernel asks on top
bool tc_item_ok(const void* src, const void* dst, int64_t rows, int64_t cols) { return src && dst && rows > 0 && cols > 0; }
bool split3_item_ok(const void* src, const void* dst, int64_t rows, int64_t cols) {
    return tc_item_ok(src, dst, rows, cols) && rows % 4 == 0 && cols % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 8 == 0;
}
// validates the items of a batch and counts its 64 x 64 tiles (= the blocks of the launch; 0: nothing to do)
int tc_count_tiles(const me_tc_batch* b, bool (*item_ok)(const void*, const void*, int64_t, int64_t), const char* bad_item,
                   const char* who, int64_t* tiles) {
    *tiles = 0;
    for (int k = 0; k < b->n; ++k) {
        ME_CHECK_ARG(item_ok(b->item[k].src, b->item[k].dst, b->item[k].rows, b->item[k].cols), bad_item, k);
        *tiles += ((b->item[k].cols + 63) / 64) * ((b->item[k].rows + 63) / 64);
    }
    ME_CHECK_ARG(*tiles < (1ll << 31), "%s: too many tiles", who);
    return ME_OK;
}

}  // namespace

extern "C" int me_split3(const float* src, int64_t ld_src, void* dst, int64_t rows, int64_t cols, int right_operand, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(src && dst && rows >= 0 && cols > 0 && cols % 4 == 0 && ld_src >= cols && ld_src % 4 == 0, "me_split3: bad args");
    ME_CHECK_ARG(((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 8 == 0), "me_split3: src must be 16-byte, dst 8-byte aligned");
    if (rows == 0) return ME_OK;
    hipLaunchKernelGGL(split3_kernel, dim3(grid_blocks(rows * (cols / 4))), dim3(EW_THREADS), 0, stream, src, ld_src,
                       reinterpret_cast<uint16_t*>(dst), rows, cols, right_operand);
    ME_CHECK_LAUNCH("me_split3");
    return ME_OK;
}

extern "C" int me_transpose_cast_batched(const me_tc_batch* b, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(b && b->n >= 0 && b->n <= ME_TC_BATCH, "me_transpose_cast_batched: bad batch");
    ME_CHECK_ARG(me_storage_dtype_ok(b->src_dtype) && me_storage_dtype_ok(b->dst_dtype), "me_transpose_cast_batched: bad dtype");
    int64_t tiles;
    const int rc = tc_count_tiles(b, tc_item_ok, "me_transpose_cast_batched: bad item %d", "me_transpose_cast_batched", &tiles);
    if (rc != ME_OK || tiles == 0) return rc;
    hipLaunchKernelGGL(transpose_cast_batched_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, *b);
    ME_CHECK_LAUNCH("me_transpose_cast_batched");
    return ME_OK;
}

// a batch of one matrix
extern "C" int me_transpose_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t rows, int64_t cols,
                                 void* stream_) {
    ME_CHECK_ARG(src && dst && rows > 0 && cols > 0, "me_transpose_cast: bad args");
    ME_CHECK_ARG(me_storage_dtype_ok(src_dtype) && me_storage_dtype_ok(dst_dtype), "me_transpose_cast: bad dtype");
    const me_tc_batch b = {1, src_dtype, dst_dtype, 0, {{src, dst, rows, cols}}};
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(transpose_cast_batched_kernel, dim3((unsigned)(((cols + 63) / 64) * ((rows + 63) / 64))), dim3(256), 0, stream, b);
    ME_CHECK_LAUNCH("me_transpose_cast");
    return ME_OK;
}

extern "C" int me_split3_batched(const me_tc_batch* b, int transposed, int right_operand, void* stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    ME_CHECK_ARG(b && b->n >= 0 && b->n <= ME_TC_BATCH, "me_split3_batched: bad batch");
    ME_CHECK_ARG(b->src_dtype == ME_F32 && b->dst_dtype == ME_BF16X3, "me_split3_batched: fp32 sources, ME_BF16X3 destinations");
    int64_t tiles;
    const int rc = tc_count_tiles(b, split3_item_ok, "me_split3_batched: bad item %d (rows, cols multiples of 4; src 16-byte, dst 8-byte aligned)",
                                  "me_split3_batched", &tiles);
    if (rc != ME_OK || tiles == 0) return rc;
    hipLaunchKernelGGL(split3_batched_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, *b, transposed, right_operand);
    ME_CHECK_LAUNCH("me_split3_batched");
    return ME_OK;
}
