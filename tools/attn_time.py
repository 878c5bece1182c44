"""Developer tool: time the attention forward / backward entry points through the product library (no stamps) on rotating
buffers.    python tools/attn_time.py [--lib path/to/libmetaenc.so] [--fp32] [B N H hd]
            python tools/attn_time.py [--lib ...] [--fp32] --qkv Nq Nk [--causal] [--p-drop P] [B H hd]     # me_attention_qkv_fwd / _bwd"""
import os
import sys
import torch
sys.path.insert(0, __file__.rsplit("/", 2)[0])
from metatransformer_amd import _capi, ops

if "--lib" in sys.argv:          # an older build of the library (build that commit in a git worktree)
    i = sys.argv.index("--lib")
    _capi.LIB_PATH = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
DT = torch.bfloat16
if "--fp32" in sys.argv:
    sys.argv.remove("--fp32")
    DT = torch.float32
QKV = None
if "--qkv" in sys.argv:          # the Q/K/V entry points: a dense Q and K | V as the halves of one [B*Nk, 2C], as the decoder calls them
    i = sys.argv.index("--qkv")
    QKV = (int(sys.argv[i + 1]), int(sys.argv[i + 2]))
    del sys.argv[i:i + 3]
CAUSAL = "--causal" in sys.argv
if CAUSAL:
    sys.argv.remove("--causal")
P_DROP = 0.0
if "--p-drop" in sys.argv:
    i = sys.argv.index("--p-drop")
    P_DROP = float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
dev = torch.device("cuda:0")


def timed(name, fn, flops, what):
    for i in range(3):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    iters = 30
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000 / iters
    print(f"{name:14s} {what}{' fp32' if DT == torch.float32 else ''}: {us:8.1f} us   {flops / us / 1e6:7.1f} TF/s")


if QKV:
    Nq, Nk = QKV
    B, H, hd = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (32, 8, 96)
    C = H * hd
    NB = 6
    qs = [torch.randn(B * Nq, C, device=dev).to(DT) for _ in range(NB)]
    kvs = [torch.randn(B * Nk, 2 * C, device=dev).to(DT) for _ in range(NB)]
    douts = [torch.randn(B * Nq, C, device=dev).to(DT) for _ in range(NB)]
    scale = hd ** -0.5
    kw = dict(causal=CAUSAL, p_drop=P_DROP, seed=7)
    out, lse = ops.attention_qkv_fwd(qs[0], kvs[0][:, :C], kvs[0][:, C:], B, Nq, Nk, H, hd, scale, need_lse=True, **kw)
    grads = (torch.empty_like(qs[0]), torch.empty(B * Nk, C, dtype=DT, device=dev), torch.empty(B * Nk, C, dtype=DT, device=dev))
    torch.cuda.synchronize()
    what = f"qkv B={B} Nq={Nq} Nk={Nk} H={H} hd={hd}{' causal' if CAUSAL else ''}{f' p_drop={P_DROP}' if P_DROP else ''}"
    flops = 4.0 * B * H * Nq * Nk * hd * (0.5 if CAUSAL else 1.0)
    timed("fwd", lambda i: ops.attention_qkv_fwd(qs[i % NB], kvs[i % NB][:, :C], kvs[i % NB][:, C:], B, Nq, Nk, H, hd, scale, need_lse=True, **kw),
          flops, what)
    timed("bwd", lambda i: ops.attention_qkv_bwd(qs[i % NB], kvs[i % NB][:, :C], kvs[i % NB][:, C:], out, douts[i % NB], lse, B, Nq, Nk, H, hd,
                                                 scale, grads=grads, **kw), 2.5 * flops, what)
    sys.exit(0)

B, N, H, hd = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (256, 197, 12, 64)
C = H * hd
NB = 6      # rotating buffers: B * N * 3C * 2 bytes = 232 MB each at the default shape (beyond the 256 MiB Infinity Cache together)
qkvs = [torch.randn(B * N, 3 * C, device=dev).to(DT) for _ in range(NB)]
douts = [torch.randn(B * N, C, device=dev).to(DT) for _ in range(NB)]
scale = hd ** -0.5
out, lse = ops.attention_fwd(qkvs[0], B, N, H, hd, scale, True)
ops.attention_bwd(qkvs[0], out, douts[0], lse, B, N, H, hd, scale)
torch.cuda.synchronize()
for name, fn in (("fwd", lambda i: ops.attention_fwd(qkvs[i % NB], B, N, H, hd, scale, True)),
                 ("fwd (no lse)", lambda i: ops.attention_fwd(qkvs[i % NB], B, N, H, hd, scale, False)),
                 ("bwd", lambda i: ops.attention_bwd(qkvs[i % NB], out, douts[i % NB], lse, B, N, H, hd, scale))):
    timed(name, fn, 4.0 * B * H * N * N * hd * (1 if name.startswith("fwd") else 2.5), f"B={B} N={N} H={H} hd={hd}")
