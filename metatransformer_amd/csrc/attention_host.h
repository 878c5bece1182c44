// attention_host.h -- host side of the attention entry points: what me_attention_fwd / _bwd (attention.hip) hand from validation to
// route to launch, shared with the N <= 64 kernels of attention_tiny.hip, the tiled kernels of attention_qkv.hip and with block.hip.
// No device code.
#pragma once
#include "common.h"
#include <type_traits>

template <int V> using Int = std::integral_constant<int, V>;      // a compile-time width handed to a generic lambda

// One call's arguments, filled once by the entry point after validation.  The backward-only fields stay null / 0 in a forward call.
struct AttnCall {
    const void* qkv; int64_t ld;
    void* out; int64_t ldo;            // (backward reads it)
    const void* dout; int64_t lddo;
    float* lse;                        // (backward reads it)
    float* delta;
    void* dqkv; int64_t lddq;
    int B, N, H, hd;
    float scale;
    int dtype;
    float p_drop;
    uint64_t seed;
    hipStream_t stream;
    // the typed pointers of a kernel instantiated for element type T
    template <typename T> struct Ptrs { const T* qkv; T* out; const T* dout; T* dqkv; };
    template <typename T> Ptrs<T> as() const {
        return {static_cast<const T*>(qkv), static_cast<T*>(out), static_cast<const T*>(dout), static_cast<T*>(dqkv)};
    }
};

// What attn_route (attention.hip) decides for a call.  form: ME_ATTN_* of include/metaenc.h.
struct AttnRoute {
    int form;
    int hd;                // instantiated head width: 32, 64 or 128
    int ns;                // ring16: 32-row sub-tiles of the sequence (3 .. 7)
    int nblk, rows;        // stream16: row blocks per (batch, head) and rows per block
    int krows;             // stream16 backward: keys per block of the dK / dV kernel
    bool dkdv32;           // stream16 backward: dK / dV on the 32-key kernel
    int plan() const { return form | (dkdv32 ? ME_ATTN_DKDV32 : 0); }       // me_gemm_profile_rec.plan
};

// attention_tiny.hip: N <= 64, one small workgroup per (batch, head)
bool attn_tiny_ok(const AttnCall& c);
int launch_attn_tiny(const AttnCall& c, bool backward);

// attention_qkv.hip: the tiled kernels (128 queries per block, 64-key LDS tiles; either dtype, head_dim up to 128, dropout), launched on
// a descriptor that its entry point has checked: me_attention_qkv_fwd / _bwd, and the ME_ATTN_GENERIC arm of me_attention_fwd / _bwd with
// the packed call written as one.  No argument checks, no ProfScope and no delta pass: the backward reads d.delta, which its caller filled.
int launch_attn_tiled_fwd(const me_attn_qkv_desc& d, hipStream_t stream);
int launch_attn_tiled_bwd(const me_attn_qkv_desc& d, hipStream_t stream);      // dK / dV, then dQ
// delta[b, h, n] = dO . O over the head's channels, out and dout [B*N, H*hd]: the delta pass of me_attention_bwd and of the fp32 me_attention_qkv_bwd
int launch_attn_delta(const void* out, int64_t ldo, const void* dout, int64_t lddo, int dtype, float* delta, int B, int N, int H, int hd,
                      hipStream_t stream);

// an ME_BF16X3 Block runs its attention as three bf16 products (attention_x3.hip) at this shape, on the exact-fp32 kernels otherwise
// (N <= 64: the exact-fp32 one-workgroup-per-head kernels, attention_tiny.hip, are faster and exact)
inline bool attn_x3_takes(int hd, int N) { return hd == 64 && N > 64; }
