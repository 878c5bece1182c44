"""Run a few launches of selected GEMM shapes (for rocprofv3 --pmc passes).  python tools/gemm_one.py qkv_fwd fc2_fwd --iters 3"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from metatransformer_amd import ops, _capi

M = 256 * 197
SHAPES = [  # (name, op, M, N, K)   names ending in _gelu / _res / _aux use that fused epilogue
    ("fc1_fwd_gelu", "nt", M, 3072, 768), ("fc2_fwd_res", "nt", M, 768, 3072), ("proj_fwd_res", "nt", M, 768, 768),
    ("fc2_dgrad_aux", "nt", M, 3072, 768),
    ("qkv_fwd", "nt", M, 2304, 768), ("proj_fwd", "nt", M, 768, 768), ("fc1_fwd", "nt", M, 3072, 768),
    ("fc2_fwd", "nt", M, 768, 3072), ("fc1_dgrad", "nt", M, 768, 3072), ("fc2_dgrad", "nt", M, 3072, 768),
    ("qkv_dgrad", "nt", M, 768, 2304),
    ("qkv_wgrad", "tn", 2304, 768, M), ("proj_wgrad", "tn", 768, 768, M), ("fc1_wgrad", "tn", 3072, 768, M),
    ("fc2_wgrad", "tn", 768, 3072, M),
]

names = [a for a in sys.argv[1:] if not a.startswith("--")]
iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 3
dev = torch.device("cuda:0")
for name, op, m, n, k in SHAPES:
    if name not in names:
        continue
    g = torch.Generator().manual_seed(1)
    if op == "nt":
        a = torch.randn(m, k, generator=g).bfloat16().to(dev); b = (0.05 * torch.randn(n, k, generator=g)).bfloat16().to(dev)
        code, odt = _capi.ME_GEMM_NT, torch.bfloat16
    else:
        a = torch.randn(k, m, generator=g).bfloat16().to(dev); b = torch.randn(k, n, generator=g).bfloat16().to(dev)
        code, odt = _capi.ME_GEMM_TN, torch.float32
    for _ in range(iters):
        ops.gemm(a, b, op=code, out_dtype=odt)
    torch.cuda.synchronize()
print("done")
