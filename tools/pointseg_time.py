"""Point segmentation decoder + head timing at the recipe shapes: forward and forward + backward, split per kernel family, the
three_nn kernel against me_knn(k = 3), and the split first conv against the concatenation route.

    python tools/pointseg_time.py [--iters 5] [--json PATH]

Shapes (width 768, training mode, the head's Dropout included): S3DIS [8, 24000] (PointViTDecoder 'cls,max' + SegHead(13,
[256], ln1d)) and ShapeNetPart [8, 2048] (PointViTPartDecoder 'cls,max,avg' + SegHead(50, [256], bn)); p1 / p2 are FPS
subsets (N / 4, N / 16) and the encoder tokens are random.  Whole-call times are device events around the call after warm-up,
using forward_split + SegHead.forward_split.  The family split of the forward brackets every library call with events in a
separate (instrumented) pass: three_nn / interp (me_three_interpolate) / gemm (heads.linear) / norm+relu (BatchNorm glue or
LayerNorm1d, ReLU) / pool / glue (the rest).  interp bwd is me_three_interpolate_bwd on its own per stage.  interp GB/s
counts the bytes a kernel must move: the three gathered rows, the output row (read too when accumulating), indices and
weights.
"""
import argparse
import json
import os
import sys
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metatransformer_amd as M  # noqa: E402
from metatransformer_amd import _capi, heads  # noqa: E402
from metatransformer_amd._capi import ptr, stream_ptr  # noqa: E402

C = 768
CASES = {"s3dis": (False, 8, 24000), "shapenetpart": (True, 8, 2048)}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


class Split:
    """event brackets around the library calls of one forward: ms per family"""

    def __init__(self):
        self.ev = []

    def wrap(self, fam, fn):
        def run(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.ev.append((fam, e0, e1))
            return out
        return run

    def install(self, mp):
        for name, fam in (("three_nn_weights", "three_nn"), ("_interpolate_rows", "interp"), ("linear", "gemm"),
                          ("_post", "norm+relu"), ("pool_tokens", "pool")):
            mp.append((heads, name, getattr(heads, name)))
            setattr(heads, name, self.wrap(fam, getattr(heads, name)))

    def result(self, total):
        torch.cuda.synchronize()
        out = defaultdict(float)
        for fam, e0, e1 in self.ev:
            out[fam] += e0.elapsed_time(e1)
        res = {k: round(v, 3) for k, v in out.items()}
        res["glue"] = round(total - sum(out.values()), 3)
        return res


def build(part, dev):
    if part:
        dec = M.PointViTPartDecoder([7, 384, C], global_feat="cls,max,avg", progressive_input=True, act_args={"act": "gelu"})
        head = M.SegHead(50, dec.out_channels, mlps=[256], norm_args={"norm": "bn"})
    else:
        dec = M.PointViTDecoder([7, 384, C], global_feat="cls,max", progressive_input=True)
        head = M.SegHead(13, dec.out_channels, mlps=[256], norm_args={"norm": "ln1d"})
    return dec.to(dev).train(), head.to(dev).train()


def interp_bytes(B, n, m, Cc, acc):
    return B * n * (3 * Cc * 4 + Cc * 4 * (2 if acc else 1) + 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pointseg_time needs a GPU"
    dev = torch.device("cuda:0")
    lib = _capi.load()
    report = {}
    for name, (part, B, N) in CASES.items():
        torch.manual_seed(0)
        dec, head = build(part, dev)
        p0 = (torch.rand(B, N, 3) * 2 - 1).to(dev)
        p1 = torch.gather(p0, 1, heads.furthest_point_sample(p0, N // 4).long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        p2 = torch.gather(p1, 1, heads.furthest_point_sample(p1, N // 16).long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        fs = [torch.randn(B, 7, N, device=dev), torch.randn(B, 384, N // 4, device=dev), torch.randn(B, C, N // 16 + 1, device=dev)]
        fr = [t.clone().requires_grad_(True) for t in fs]
        extra = [torch.randint(0, 16, (B, 1), device=dev)] if part else []

        def fwd():
            with torch.no_grad():
                head.forward_split(*dec.forward_split([p0, p1, p2], list(fs), *extra))

        def fwd_bwd():
            head.forward_split(*dec.forward_split([p0, p1, p2], list(fr), *extra)).sum().backward()
        r = {"shape": [B, N], "fwd_ms": round(timed(fwd, a.iters), 3), "fwd_bwd_ms": round(timed(fwd_bwd, a.iters), 3)}
        mp, split = [], Split()
        split.install(mp)
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd()
            e1.record()
            torch.cuda.synchronize()
            r["fwd_family_ms"] = split.result(e0.elapsed_time(e1))
        finally:
            for obj, nm, orig in reversed(mp):
                setattr(obj, nm, orig)
        stages = {}
        for s, (dense, sparse, Cs) in enumerate(((p1, p2, 384), (p0, p1, 7)), start=1):
            n, m = dense.shape[1], sparse.shape[1]
            st = {"n": n, "m": m}
            st["three_nn_ms"] = round(timed(lambda: heads.three_nn_weights(dense, sparse), a.iters), 3)
            st["knn3_ms"] = round(timed(lambda: heads.knn_indices(sparse, dense, 3), a.iters), 3)
            idx, w = heads.three_nn_weights(dense, sparse)
            fsp = torch.randn(B * m, C, device=dev)
            out = torch.empty(B * n, C, device=dev)
            t_w = timed(lambda: lib.me_three_interpolate(ptr(fsp), C, ptr(idx), ptr(w), ptr(out), C, 0, B, n, m, C, 0, stream_ptr()), a.iters)
            t_a = timed(lambda: lib.me_three_interpolate(ptr(fsp), C, ptr(idx), ptr(w), ptr(out), C, 0, B, n, m, C, 1, stream_ptr()), a.iters)
            st["interp_ms"], st["interp_GBps"] = round(t_w, 3), round(interp_bytes(B, n, m, C, False) / t_w / 1e6, 1)
            st["interp_acc_ms"], st["interp_acc_GBps"] = round(t_a, 3), round(interp_bytes(B, n, m, C, True) / t_a / 1e6, 1)
            ws = torch.empty(int(lib.me_three_interpolate_bwd_workspace(B, n, m)), dtype=torch.uint8, device=dev)
            dfs = torch.empty(B * m, C, device=dev)
            st["interp_bwd_ms"] = round(timed(lambda: lib.me_three_interpolate_bwd(ptr(out), C, 0, ptr(idx), ptr(w), ptr(dfs), C, B, n, m, C,
                                                                                     ptr(ws), ws.numel(), stream_ptr()), a.iters), 3)
            # the first conv of the stage: split (skip GEMM + sparse GEMM + accumulate) against interpolate-into-concat + one GEMM
            W = torch.randn(C, Cs + C, device=dev) * 0.02
            skip = torch.randn(B * n, Cs, device=dev)
            Kp = (Cs + C + 7) // 8 * 8
            Wp = torch.nn.functional.pad(W, (0, Kp - Cs - C))

            def split_route():
                with torch.no_grad():
                    heads._interpolate_rows(heads._lin(fsp, W[:, Cs:]).view(B, m, C), idx, w, heads._lin(skip, W[:, :Cs]))

            def concat_route():
                with torch.no_grad():
                    cat = torch.zeros(B * n, Kp, device=dev)
                    cat[:, :Cs] = skip
                    lib.me_three_interpolate(ptr(fsp), C, ptr(idx), ptr(w), ptr(cat), Kp, Cs, B, n, m, C, 0, stream_ptr())
                    heads.linear(cat, Wp, None)
            st["first_conv_split_ms"] = round(timed(split_route, a.iters), 3)
            st["first_conv_concat_ms"] = round(timed(concat_route, a.iters), 3)
            stages[f"stage{s}"] = st
        r["stages"] = stages
        r["peak_mem_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 1)
        report[name] = r
        print(json.dumps({name: r}), flush=True)
        del dec, head
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
