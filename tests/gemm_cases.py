"""The case table of the me_gemm contract tests: the smallest shapes that reach each kernel form of plan_gemm (csrc/gemm.hip), with the
plan the library must report for each.  A plain module: test_gpu_gemm_contract.py (strides, guard bands, products) and
test_gpu_gemm_epilogue_values.py (the epilogue's own values on exact accumulators) read the same table, so neither can silently stop
covering a kernel the other still names."""
import ctypes

import torch

from metatransformer_amd import _capi

F32, BF16 = torch.float32, torch.bfloat16
NT, TN = _capi.ME_GEMM_NT, _capi.ME_GEMM_TN
G128, G2B, G2W, G3 = 0, 2, 3, 4
SAVE_GG, FACTOR = _capi.ME_GEMM_SAVE_GELU_GRAD, _capi.ME_GEMM_AUX_IS_FACTOR

# epilogues: what the descriptor carries besides A, B, C.  "c" overrides the case's output dtype.
EPI = {
    "plain": {},                                                                    # 0
    "bias": dict(bias=True),                                                        # 0
    "gelu_pre": dict(bias=True, gelu=True, preact="c"),                             # 1 (+ saved pre-activation)
    "alpha_beta": dict(alpha=0.5, beta=2.0),                                        # generic
    "res": dict(res=BF16),                                                          # 2
    "bias_res": dict(bias=True, res=BF16),                                          # 2
    "res_stats": dict(bias=True, res=BF16, row_stats=True),                         # 2 + the output's row statistics (resident g3 only)
    "aux": dict(aux=BF16),                                                          # 3: x gelu'(aux)
    "factor": dict(aux=BF16, flags=FACTOR),                                         # 6
    "save_gg": dict(bias=True, gelu=True, preact=BF16, flags=SAVE_GG),              # 7
    "bias_res32": dict(bias=True, res=F32, c=F32),                                  # 8
    "generic": dict(bias=True, colscale=True, res=F32, group=100),                  # 4: column scale, fp32 residual, res_row_mod, out_group
    "folded": dict(bias=True, row_affine=True),                                     # a LayerNorm folded in: row_affine [M][2] + col_shift [N]
    "beta1": dict(beta=1.0),
    "colsum": dict(colsum=True),
    "colsum_beta1": dict(colsum=True, beta=1.0),
}
ALL_SMALL = ["plain", "bias", "gelu_pre", "res", "aux", "factor", "save_gg", "generic", "folded"]


def plan_code(family, parts=1, split=False, balanced=False):
    return family | (16 if split else 0) | (32 if balanced else 0) | (parts << 8)


# (id, op, operand dtype, output dtype, M, N, K, expected plan, epilogues[, reserved CUs])
CASES = [
    ("nt_f32_g128", NT, F32, F32, 130, 132, 72, plan_code(G128), ["plain", "gelu_pre", "alpha_beta"]),
    ("nt_g128_n4", NT, BF16, BF16, 130, 132, 72, plan_code(G128), ["plain", "res"]),                    # N % 8 = 4
    ("nt_g128_m100", NT, BF16, BF16, 100, 256, 64, plan_code(G128), ["plain"]),                         # M < 128
    ("nt_g128_k72", NT, BF16, BF16, 300, 256, 72, plan_code(G128), ["plain"]),                          # K % 32 != 0
    ("nt_g2b_64x128", NT, BF16, BF16, 200, 384, 64, plan_code(G2B), ALL_SMALL),
    ("nt_g2b_split8", NT, BF16, BF16, 200, 384, 2048, plan_code(G2B, 8, split=True), ["gelu_pre", "res"]),      # the fold applies the epilogue
    ("nt_g2b_128x128", NT, BF16, BF16, 5966, 384, 64, plan_code(G2B), ["plain", "bias_res"]),
    ("nt_g2b_128x256", NT, BF16, BF16, 8957, 512, 64, plan_code(G2B), ["plain", "aux"]),
    ("nt_g2b_128x256_n264", NT, BF16, BF16, 300, 264, 96, plan_code(G2B), ["plain", "gelu_pre"]),       # an 8-column last tile
    ("nt_g2w", NT, BF16, BF16, 300, 776, 64, plan_code(G2W), ["plain", "res", "save_gg", "factor"]),
    ("nt_g2w_split2", NT, BF16, BF16, 300, 776, 512, plan_code(G2W, 2, split=True), ["bias_res"]),
    ("nt_g2w_tail2", NT, BF16, BF16, 17408, 1000, 544, plan_code(G2W, 2, split=True), ["gelu_pre"]),    # 1024 tail rows in 2 parts
    ("nt_g3_one_tile", NT, BF16, BF16, 1800, 4096, 128, plan_code(G3), ALL_SMALL + ["bias_res32"]),     # 128 tiles < CUs
    ("nt_g3_one_tile_n3848", NT, BF16, BF16, 1800, 3848, 128, plan_code(G3), ALL_SMALL + ["bias_res32"]),
    ("nt_g3_one_tile_f32", NT, BF16, F32, 3900, 4096, 128, plan_code(G3), ["bias_res32"]),              # fp32 output: never resident
    ("nt_g3_resident", NT, BF16, BF16, 3900, 4096, 128, plan_code(G3), ["plain", "gelu_pre", "save_gg", "res_stats", "aux", "factor", "folded"]),
    ("nt_g3_resident_n3848", NT, BF16, BF16, 3900, 3848, 256, plan_code(G3), ["plain", "gelu_pre", "save_gg", "res_stats", "aux", "factor", "folded"]),
    ("nt_g3_tail8", NT, BF16, F32, 17508, 1024, 2048, plan_code(G3, 8, split=True), ["bias_res32"]),    # 1124 tail rows in 8 parts
    ("tn_f32_g128", TN, F32, F32, 136, 72, 130, plan_code(G128), ["plain"]),
    ("tn_g128_tiny", TN, BF16, F32, 8, 8, 65, plan_code(G128), ["plain"]),
    ("tn_g2b_128", TN, BF16, F32, 136, 264, 640, plan_code(G2B), ["plain", "beta1"]),
    ("tn_g2b_split4_128", TN, BF16, F32, 136, 264, 2048, plan_code(G2B, 4, split=True), ["colsum", "colsum_beta1"]),
    ("tn_g2b_split4_256", TN, BF16, F32, 136, 512, 2048, plan_code(G2B, 4, split=True), ["colsum", "colsum_beta1"]),
    ("tn_g3_wgrad33", TN, BF16, F32, 264, 328, 4133, plan_code(G3, 33, split=True), ["colsum", "colsum_beta1"]),       # ragged reduction
    # 9 tiles on 240 workgroups: 26 whole levels of 2 K-tile pairs + 3 leftover pairs per tile on 6 workgroups, a tile's leftover in <= 2 parts
    ("tn_g3_wgrad_balanced", TN, BF16, F32, 520, 520, 6917, plan_code(G3, 28, split=True, balanced=True), ["colsum"], 16),
]
CASE_BY_ID = {c[0]: c for c in CASES}


def dtype_code(dt):
    return _capi.ME_F32 if dt == F32 else _capi.ME_BF16


def device_cus(lib):
    cus, lds, mhz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    name = ctypes.create_string_buffer(128)
    _capi.check(lib.me_device_info(torch.cuda.current_device(), ctypes.byref(cus), ctypes.byref(lds), ctypes.byref(mhz), name, 128), "me_device_info")
    return cus.value


def describe(plan):
    return f"family {plan & 15}, split {bool(plan & 16)}, balanced {bool(plan & 32)}, parts {plan >> 8} ({plan:#x})"


def assert_g3_form(lib, name, cdt, M, N):
    """the g3 NT form is not in the plan code: it follows from the tile count against the CUs (g3_form: resident when every one of the
    CUs, rounded down to whole rounds of 8, gets a tile and the output is bf16), so the names are checked against the device"""
    tiles, slots = -(-M // 256) * -(-N // 256), device_cus(lib) & ~7
    if name.startswith("nt_g3_resident"):
        assert tiles >= slots, f"{name}: {tiles} tiles do not reach the resident kernel on {slots} CUs"
    if name.startswith("nt_g3_one_tile") and cdt == BF16:
        assert tiles < slots, f"{name}: {tiles} tiles run resident on {slots} CUs"
