"""Trace of the attention entry points (me_attention_fwd / me_attention_bwd, then me_attention_qkv_fwd / _bwd) over every kernel form
their route has, for comparing two commits: run it at each, the two outputs must be byte-identical.

    python tools/attention_route_trace.py OUT                 # per case: sha256 of out, lse, dqkv (qkv entries: out, lse, dq, dk, dv)
    python tools/attention_route_trace.py --host-time [CALLS]  # wall time of CALLS (2000) back-to-back forward + backward calls

It uses only names that both sides of such a comparison have: ops.attention_fwd / ops.attention_bwd, ops.attention_qkv_fwd /
ops.attention_qkv_bwd (since 1005188), and the ctypes entries for the cases with a padded row stride.  Under `rocprofv3 --kernel-trace -- python tools/attention_route_trace.py OUT` the kernel
sequence (name, grid, workgroup, LDS bytes) is the record of which kernel each case took.  The first cases are those of
tests/test_gpu_ops.py::test_attention_route (profiles/attention_route_equivalence.txt holds the record made with them), the rest walk the
generic route, and the records of the qkv entry points come last."""
import hashlib
import sys
import time

import torch

from metatransformer_amd import _capi, ops
from metatransformer_amd._capi import check, dtype_code, ptr, stream_ptr

dev = torch.device("cuda", 0)
# (N, head_dim, dtype, p_drop, B, H)
CASES = [(64, 64, "bf16", 0.0, 2, 2), (64, 64, "fp32", 0.0, 2, 2), (65, 64, "bf16", 0.0, 2, 2), (224, 64, "bf16", 0.0, 2, 2),
         (128, 24, "bf16", 0.0, 2, 2), (129, 40, "bf16", 0.0, 2, 2), (225, 64, "bf16", 0.0, 2, 2), (256, 64, "bf16", 0.0, 2, 2),
         (257, 64, "bf16", 0.0, 2, 2), (512, 64, "bf16", 0.0, 2, 2), (257, 32, "bf16", 0.0, 2, 2), (300, 24, "bf16", 0.0, 2, 2),
         (513, 64, "bf16", 0.0, 2, 2), (700, 64, "bf16", 0.0, 2, 2), (592, 64, "bf16", 0.0, 2, 2), (1568, 64, "bf16", 0.0, 1, 1),
         (513, 32, "bf16", 0.0, 2, 2), (600, 24, "bf16", 0.0, 2, 2), (130, 128, "bf16", 0.0, 2, 2), (64, 128, "bf16", 0.0, 2, 2),
         (65, 64, "fp32", 0.0, 2, 2), (197, 64, "bf16", 0.1, 2, 2), (100, 24, "bf16", 0.1, 2, 2),
         # the generic route at every instantiation of the tiled kernels (HD 32 / 64 / 128, both dtypes) and every boundary of their tiling
         # (one key, 64-key tile + 1, 128-query block + 1 / + 2, two blocks + 1), with and without dropout; appended, so the lines above stay
         # comparable with older records
         (1, 8, "fp32", 0.1, 2, 2), (65, 8, "fp32", 0.0, 2, 2), (129, 64, "fp32", 0.1, 2, 2), (130, 96, "fp32", 0.0, 2, 2),
         (130, 128, "fp32", 0.0, 2, 2), (257, 128, "fp32", 0.1, 2, 2), (37, 12, "fp32", 0.1, 2, 2),
         (65, 24, "bf16", 0.1, 2, 2), (129, 48, "bf16", 0.1, 2, 2), (130, 64, "bf16", 0.5, 2, 2), (257, 72, "bf16", 0.0, 2, 2),
         (70, 96, "bf16", 0.0, 2, 2), (130, 128, "bf16", 0.1, 2, 2),
         # the 32-row kernels: resident at HD = 32, a last chunk of 33 rows (masked two-sub-tile tail), three full chunks (no tail step)
         (250, 24, "bf16", 0.0, 2, 2), (545, 32, "bf16", 0.0, 1, 2), (768, 24, "bf16", 0.0, 1, 1),
         # the 16-row kernels: six ring sub-tiles (N = 161); enough (batch, head) pairs that a workgroup walks more than one item, in the
         # ring form (N = 197, 100) and the streaming one (N = 300, 600); head_dim below the template width in the ring form (N = 100)
         # and in the streaming kernels (N = 577, 600); 176-row blocks, which take four loader waves (N = 700)
         (161, 64, "bf16", 0.0, 2, 2), (197, 64, "bf16", 0.0, 40, 12), (100, 48, "bf16", 0.0, 30, 12), (300, 64, "bf16", 0.0, 40, 12),
         (577, 40, "bf16", 0.0, 3, 2), (600, 48, "bf16", 0.0, 24, 12), (700, 64, "bf16", 0.0, 9, 4)]
DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
# me_attention_qkv_*: (Nq, Nk, causal) -- causal N and two-length pairs on every edge of the tiling (one row, a 64-key tile and + 1, a
# 128-query block + 1, two blocks).  qkv_cases() gives each shape two head_dims, both layouts and both dropout settings, per dtype
QKV_SHAPES = [(n, n, True) for n in (1, 64, 65, 129, 200)] + [(a, b, False) for a, b in ((1, 65), (33, 1), (129, 65), (144, 96), (70, 17))]
QKV_HDS = [8, 24, 64, 96, 128]


def qkv_cases():
    """[(Nq, Nk, causal, head_dim, dtype, p_drop, layout)], B = H = 2"""
    out = []
    for dt in ("fp32", "bf16"):
        for rot in (0, 2):
            for i, (a, b, c) in enumerate(QKV_SHAPES):
                out.append((a, b, c, QKV_HDS[(i + rot) % 5], dt, 0.1 if (i + rot // 2) % 3 == 0 else 0.0, ("q_kv2", "padded")[(i + rot // 2) % 2]))
    return out


def sha(t):
    t = t.detach().contiguous()
    return f"{str(t.dtype)[6:]}{list(t.shape)} " + hashlib.sha256(t.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def inputs(B, N, H, hd, dt, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * H * hd, generator=g).to(dev, DT[dt])
    dout = torch.randn(B * N, H * hd, generator=g).to(dev, DT[dt])
    return qkv, dout


def trace(path):
    out_f = open(path, "w")
    for i, (N, hd, dt, p, B, H) in enumerate(CASES):
        qkv, dout = inputs(B, N, H, hd, dt, 100 + i)
        scale = hd ** -0.5
        out, lse = ops.attention_fwd(qkv, B, N, H, hd, scale, True, p_drop=p, seed=7)
        dqkv = ops.attention_bwd(qkv, out, dout, lse, B, N, H, hd, scale, p_drop=p, seed=7)
        torch.cuda.synchronize()
        out_f.write(f"== N={N} hd={hd} {dt} p_drop={p} B={B} H={H}\n  out: {sha(out)}\n  lse: {sha(lse)}\n  dqkv: {sha(dqkv)}\n")
    # padded row strides (the Python wrappers always pass dense ones): the ctypes entries
    lib = _capi.load()
    bf = dtype_code(torch.bfloat16)
    # forward with ld_out = C + 4: the mid kernel at N = 300, the chunk kernel at N = 545 (the only forward that takes it at head_dim 64)
    for N, seed in ((300, 200), (545, 201)):
        B, H, hd = 2, 2, 64
        C = H * hd
        qkv, dout = inputs(B, N, H, hd, "bf16", seed)
        out = torch.zeros(B * N, C + 4, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, H, N, dtype=torch.float32, device=dev)
        check(lib.me_attention_fwd(ptr(qkv), 3 * C, ptr(out), C + 4, ptr(lse), B, N, H, hd, hd ** -0.5, bf, 0.0, 0, stream_ptr()), "me_attention_fwd")
        torch.cuda.synchronize()
        out_f.write(f"== N={N} hd={hd} bf16 ld_out=C+4 B={B} H={H} (forward only)\n  out: {sha(out)}\n  lse: {sha(lse)}\n")
    # backward at N = 545 with a dense out and ld_dqkv = 3C + 4: the two chunk kernels at head_dim 64
    out, lse = ops.attention_fwd(qkv, B, N, H, hd, hd ** -0.5, True)
    delta = torch.empty(B, H, N, dtype=torch.float32, device=dev)
    dqkv = torch.zeros(B * N, 3 * C + 4, dtype=torch.bfloat16, device=dev)
    check(lib.me_attention_bwd(ptr(qkv), 3 * C, ptr(out), C, ptr(dout), C, ptr(lse), ptr(delta), ptr(dqkv), 3 * C + 4, B, N, H, hd, hd ** -0.5, bf,
                               0.0, 0, stream_ptr()), "me_attention_bwd")
    torch.cuda.synchronize()
    out_f.write(f"== N={N} hd={hd} bf16 ld_dqkv=3C+4 B={B} H={H} (backward only)\n  delta: {sha(delta)}\n  dqkv: {sha(dqkv)}\n")
    trace_qkv(out_f)
    out_f.close()


def trace_qkv(out_f):
    """layouts: q_kv2 = a dense Q and K | V as the halves of one [B*Nk, 2C]; padded = three tensors with a row stride of C + 8.  The
    gradients are written into views of the same layout"""
    B, H = 2, 2
    for i, (Nq, Nk, causal, hd, dt, p, layout) in enumerate(qkv_cases()):
        C = H * hd
        g = torch.Generator().manual_seed(300 + i)
        q, k, v, dout = (torch.randn(B * n, C, generator=g).to(dev, DT[dt]) for n in (Nq, Nk, Nk, Nq))

        def place(vals):
            if layout == "q_kv2":
                kv = torch.zeros(B * Nk, 2 * C, dtype=DT[dt], device=dev)
                views = (torch.zeros(B * Nq, C, dtype=DT[dt], device=dev), kv[:, :C], kv[:, C:])
            else:
                views = tuple(torch.zeros(x.shape[0], C + 8, dtype=DT[dt], device=dev)[:, :C] for x in vals)
            for dst, src in zip(views, vals):
                dst.copy_(src)
            return views

        qd, kd, vd = place((q, k, v))
        scale = hd ** -0.5
        out, lse = ops.attention_qkv_fwd(qd, kd, vd, B, Nq, Nk, H, hd, scale, causal=causal, need_lse=True, p_drop=p, seed=7)
        dq, dk, dv = ops.attention_qkv_bwd(qd, kd, vd, out, dout, lse, B, Nq, Nk, H, hd, scale, causal=causal, p_drop=p, seed=7,
                                           grads=place((torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v))))
        torch.cuda.synchronize()
        out_f.write(f"== qkv Nq={Nq} Nk={Nk} causal={int(causal)} hd={hd} {dt} p_drop={p} {layout} B={B} H={H}\n  out: {sha(out)}\n  lse: {sha(lse)}\n"
                    f"  dq: {sha(dq)}\n  dk: {sha(dk)}\n  dv: {sha(dv)}\n")


def host_time(calls):
    B, N, H, hd = 1, 16, 4, 64
    qkv, dout = inputs(B, N, H, hd, "bf16", 1)
    scale = hd ** -0.5
    for n in (200, calls):                    # warm-up, then the timed run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out, lse = ops.attention_fwd(qkv, B, N, H, hd, scale, True)
            ops.attention_bwd(qkv, out, dout, lse, B, N, H, hd, scale)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    print(f"host-time: {calls} x (attention_fwd + attention_bwd) at B=1 N=16 H=4 hd=64 bf16: {dt * 1e3:.2f} ms ({dt / calls * 1e6:.2f} us per pair)")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--host-time":
        host_time(int(sys.argv[2]) if len(sys.argv) > 2 else 2000)
    else:
        trace(sys.argv[1])
