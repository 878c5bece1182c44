// gemm_host.h -- what gemm.hip / gemm3_x3.hip offer the library's other translation units besides the public me_gemm entry points.
// Host declarations only (no device code): block.hip includes this file alone, the GEMM files get it through gemm_common.h.
#pragma once
#include "common.h"

struct GemmParams;

// validation + parameter block of a descriptor, as me_gemm does it (patch_embed.hip: the projection runs on its own kernel)
int gemm_fill_params(const me_gemm_desc* d, GemmParams& p);
// me_gemm for a g3 wgrad problem with the split-K kernel launch replaced (patch_embed.hip gathers its B operand from the image,
// gemm3_x3.hip walks three plane segments); planning, slabs, the deterministic fold with alpha / beta / column sums stay me_gemm's.
// A problem the planner does not give to the g3 wgrad family is refused (ME_ERR_UNSUPPORTED) instead of run.
typedef int (*GemmTnLaunch)(const GemmParams& p, hipStream_t stream, const void* ctx);
int gemm_tn_with_launcher(const me_gemm_desc* d, hipStream_t stream, GemmTnLaunch launch, const void* ctx);
int gemm_tn_is_g3(const me_gemm_desc* d);      // 1 / 0: would the planner take that route
// gemm3_x3.hip: the weight gradient of an ME_BF16X3 Linear (three plane products) as one launch of the split-K wgrad kernel
int gemm_tn_x3_planes(const me_gemm_desc* d, hipStream_t stream);
