"""Trace of what the Python host of a Block (encoder.py, weight_cache.py, heads.pack_encoder, parallel.FusedAdamW) asks of the library,
for comparing two commits: run it at each, the two outputs must be byte-identical.

    python tools/block_host_trace.py OUT

It uses only names that both sides of such a comparison have (Block, build_encoder, encoder_forward_inference, heads.pack_encoder,
parallel.FlatParams / FusedAdamW, ops.*).  ops.cast, ops.transpose_cast, ops.transpose_cast_many, ops.split3 and ops.split3_many are
wrapped to log each call with the number of matrices in it, and the library's GEMM profile is on.  One encoder of depth 2, dim 256,
4 heads, B = 2, N = 70, fixed seeds, goes through every route the host code has; per case the output holds sha256 of every result
(output, x.grad, parameter gradients or the flat gradient buffer, the parameters after each optimizer step), the logged op
sequence and the gemm_profile_read(with_plan=True) sequence without its `ms` field (not for the captured forward).  profiles/block_host_equivalence.txt holds the
record made with it."""
import copy
import gc
import hashlib
import os
import sys

import torch

import metatransformer_amd as M
from metatransformer_amd import heads, ops, parallel

DEPTH, DIM, HEADS, B, N = 2, 256, 4, 2, 70
dev = torch.device("cuda", 0)
out = open(sys.argv[1], "w")
oplog = []


def wrap(name, count):
    inner = getattr(ops, name)

    def logged(*a, **k):
        oplog.append(f"{name} {count(a[0])}")
        return inner(*a, **k)
    setattr(ops, name, logged)


for _n in ("cast", "transpose_cast", "split3"):
    wrap(_n, lambda first: 1)
for _n in ("transpose_cast_many", "split3_many"):
    wrap(_n, len)


def sha(t):
    if t is None:
        return "None"
    t = t.detach().contiguous()
    return f"{str(t.dtype)[6:]}{list(t.shape)} " + hashlib.sha256(t.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def case(title, body, profile=True):
    """one case: its results (written by `body` through put), or the library's refusal, then what it made the library do.
    profile=False: no GEMM profile (its events cannot be recorded into a graph capture)"""
    gc.collect()                    # (encoders of earlier cases: the weight cache refreshes the copies of every LIVE block)
    out.write(f"== {title}\n")
    oplog.clear()
    ops.gemm_profile(profile)
    try:
        body()
    except M.MetaEncError as e:
        out.write(f"  refused: {e}\n")
    torch.cuda.synchronize()
    recs = ops.gemm_profile_read(with_plan=True) if profile else []
    ops.gemm_profile(False)
    out.write(f"  ops ({len(oplog)}): " + ", ".join(oplog) + "\n")
    out.write(f"  gemms ({len(recs)}):\n" if profile else "  gemms: not profiled\n")
    for op, ab, m, n, k, _ms, plan in recs:
        out.write(f"    {op} {ab} {m} {n} {k} {plan}\n")
    out.flush()


def put(label, t):
    out.write(f"  {label}: {sha(t)}\n")


def encoder(dtype=None, **kw):
    torch.manual_seed(1)
    enc = M.build_encoder(DEPTH, DIM, HEADS, **kw).to(dev)
    return enc if dtype is None else enc.to(dtype)


_g = torch.Generator().manual_seed(5)
X, GO = torch.randn(B, N, DIM, generator=_g).to(dev), torch.randn(B, N, DIM, generator=_g).to(dev)
bf16 = lambda on=True: torch.autocast("cuda", dtype=torch.bfloat16, enabled=on)      # noqa: E731


def train_flat(title, steps, autocast, fp32_mode=None, **opt_kw):
    enc = encoder().train()
    if fp32_mode is not None:
        M.set_fp32_mode(enc, fp32_mode)

    def body():
        flat = parallel.FlatParams(enc.named_parameters(), no_decay=parallel.no_decay_rule)
        opt = parallel.FusedAdamW(flat, lr=1e-3, **opt_kw)
        for s in range(steps):
            flat.zero_grad()
            xr = X.clone().requires_grad_(True)
            with bf16(autocast):
                y = enc(xr)
            (y.float() * GO).sum().backward()
            put(f"step {s} y", y)
            put(f"step {s} x.grad", xr.grad)
            if not opt_kw.get("overlap"):           # (the overlapped optimizer has consumed and zeroed the gradients by now)
                put(f"step {s} flat_grad", flat.flat_grad)
            opt.step()
            put(f"step {s} flat_param", flat.flat_param)
    case(title, body)
    return enc


def train_plain(title, enc, autocast=True, grid=None, x=None):
    def body():
        torch.manual_seed(0)
        for p in enc.parameters():
            p.grad = None
        xr = (X if x is None else x).clone().requires_grad_(True)
        with bf16(autocast):
            if grid is None:
                y = enc(xr)
            else:
                y = xr
                for blk in enc:
                    y = blk(y, *grid)
        (y.float() * GO).sum().backward()
        put("y", y)
        put("x.grad", xr.grad)
        for k, p in enc.named_parameters():
            put(f"grad {k}", p.grad)
    case(title, body)


def infer(title, fn, profile=True):
    def body():
        with torch.no_grad():
            put("y", fn())
    case(title, body, profile)


for mirror in (True, False):
    for overlap in (False, True):
        trained = train_flat(f"bf16 autocast training, FusedAdamW(bf16_mirror={mirror}, overlap={overlap})", 3, True,
                             bf16_mirror=mirror, overlap=overlap)
train_flat("fp32 training, fp32_mode = 3xbf16", 2, False, fp32_mode="3xbf16")
train_flat("fp32 training, fp32_mode = exact", 2, False, fp32_mode="exact")

train_plain("op-by-op: drop_path = drop = attn_drop = 0.1", encoder(drop_path=0.1, drop=0.1, attn_drop=0.1).train())
train_plain("op-by-op: layer_scale", encoder(layer_scale=True).train())
train_plain("op-by-op: windowed, window_size 4 on a 10 x 7 grid", encoder(windowed=True, window_size=4).train(), grid=(10, 7))
enc = encoder().train()
for blk in enc:
    blk.c_side = False
train_plain("op-by-op: c_side = False", enc)
train_plain("op-by-op: c_side = False, fp32 exact", enc, autocast=False)
train_plain("fp16 parameters and tokens", encoder(torch.float16).train(), autocast=False, x=X.half())

enc = encoder(torch.bfloat16).eval()
xb = X.bfloat16()
for fold in ("always", False):
    for blk in enc:
        blk.fold_norm = fold
    infer(f"bf16 eval, fold_norm = {fold!r}", lambda: enc(xb))
enc = encoder(torch.bfloat16).eval()
for blk in enc:
    blk.attn_fp8 = True
infer("bf16 eval, attn_fp8", lambda: enc(xb))
enc = encoder(torch.float16).eval()
infer("fp16 eval", lambda: enc(X.half()))
enc = encoder(torch.bfloat16).eval()
for graph in (False, True):
    infer(f"encoder_forward_inference(graph={graph}) bf16", lambda: M.encoder_forward_inference(enc, xb, graph=graph), profile=not graph)
enc32 = encoder().eval()
for graph in (False, True):
    infer(f"encoder_forward_inference(graph={graph}) fp32", lambda: M.encoder_forward_inference(enc32, X, graph=graph), profile=not graph)


def packed(cd):
    enc = encoder()
    for blk in enc:
        blk.compute_dtype = cd
    flat = heads.pack_encoder(enc, warm=True)
    put("flat_param", flat.flat_param)
    xr = X.clone().requires_grad_(True)
    y = enc(xr)
    (y.float() * GO).sum().backward()
    put("y", y)
    put("x.grad", xr.grad)
    put("flat_grad", flat.flat_grad)


for cd in (torch.bfloat16, "fp32_3xbf16"):
    case(f"pack_encoder(warm=True), compute_dtype = {cd!r}", lambda: packed(cd))

twin = copy.deepcopy(trained).eval()
with bf16():
    infer("deepcopy of the trained encoder, eval, bf16 autocast", lambda: twin(X))
out.close()
print("block_host_trace: done, package", os.path.dirname(M.__file__))
