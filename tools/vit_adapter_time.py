"""Time the ViT-Adapter backbone's image-side parts on the GPU, per recipe shape (segmentation 2 x 512 x 512, detection
1 x 800 x 1344): the spatial prior module, the tail (up, resizes, norms) and the whole backbone, forward and forward + backward,
against the same modules composed from nn.Conv2d / F.max_pool2d / F.interpolate / nn.ConvTranspose2d in channel-first layout
(sharing the parameters) on the same GPU.

    python tools/vit_adapter_time.py [--out profiles/vit_adapter_time.txt] [--windows 5] [--iters 5]

Per figure: two warm-up calls, then `windows` windows of `iters` calls each between two events; the median window and the
spread (max - min) / median over the windows are reported.  "slower by more than the spread" is the condition DESIGN.md 7d
discusses; no ratio is fixed in advance.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import metatransformer_amd as M  # noqa: E402
from metatransformer_amd import adapter  # noqa: E402
import vit_adapter_cases as vc  # noqa: E402

SHAPES = {"segmentation 2x512x512": (2, 512, 512), "detection 1x800x1344": (1, 800, 1344)}


def spm_torch(spm, x):
    """SpatialPriorModule.forward from PyTorch's channel-first ops, on spm's own parameters"""
    def seq(s, t):
        for m in s:
            t = F.conv2d(t, m.weight, None, m.stride, m.padding) if isinstance(m, torch.nn.Conv2d) else \
                (m(t) if not isinstance(m, torch.nn.ReLU) else F.relu(t))
        return t
    c1 = seq(spm.stem, x)
    c2 = seq(spm.conv2, c1)
    c3 = seq(spm.conv3, c2)
    c4 = seq(spm.conv4, c3)
    fc = lambda m, t: F.conv2d(t, m.weight, m.bias)      # noqa: E731
    c1, c2, c3, c4 = fc(spm.fc1, c1), fc(spm.fc2, c2), fc(spm.fc3, c3), fc(spm.fc4, c4)
    return c1, c2.flatten(2).transpose(1, 2), c3.flatten(2).transpose(1, 2), c4.flatten(2).transpose(1, 2)


def tail_rows(m, c1, c, x, B, H, W):
    D = x.shape[-1]
    n2, n3 = 4 * H * W, H * W
    c2, c3, c4 = c[:, :n2].reshape(-1, D), c[:, n2:n2 + n3].reshape(-1, D), c[:, n2 + n3:].reshape(-1, D)
    c1 = M.conv_transpose2x2_rows(c2, m.up.weight, m.up.bias, B, 2 * H, 2 * W, add=c1)
    x3 = x.reshape(-1, D)
    c1 = c1 + M.resize_rows_batched(x3, B, H, W, scale_factor=4)
    c2 = c2 + M.resize_rows_batched(x3, B, H, W, scale_factor=2)
    c3 = c3 + x3
    c4 = c4 + M.resize_rows_batched(x3, B, H, W, scale_factor=0.5)
    return [adapter._rows_to_image(n(t), B, h, w) for n, t, h, w in ((m.norm1, c1, 4 * H, 4 * W), (m.norm2, c2, 2 * H, 2 * W),
                                                                      (m.norm3, c3, H, W), (m.norm4, c4, H // 2, W // 2))]


def tail_torch(m, c1, c, x, B, H, W):
    """vit_adapter.py:110-132 as written there (c1 channel-first)"""
    D = x.shape[-1]
    n2, n3 = 4 * H * W, H * W
    c2 = c[:, :n2].transpose(1, 2).view(B, D, 2 * H, 2 * W).contiguous()
    c3 = c[:, n2:n2 + n3].transpose(1, 2).view(B, D, H, W).contiguous()
    c4 = c[:, n2 + n3:].transpose(1, 2).view(B, D, H // 2, W // 2).contiguous()
    c1 = m.up(c2) + c1
    x3 = x.transpose(1, 2).view(B, D, H, W).contiguous()
    x1 = F.interpolate(x3, scale_factor=4, mode="bilinear", align_corners=False)
    x2 = F.interpolate(x3, scale_factor=2, mode="bilinear", align_corners=False)
    x4 = F.interpolate(x3, scale_factor=0.5, mode="bilinear", align_corners=False)
    return [m.norm1(c1 + x1), m.norm2(c2 + x2), m.norm3(c3 + x3), m.norm4(c4 + x4)]


def measure(fn, windows, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    ms.sort()
    med = ms[len(ms) // 2]
    return med, (ms[-1] - ms[0]) / med


def with_backward(fn, leaves):
    def run():
        for t in leaves:
            t.grad = None
        outs = fn()
        torch.autograd.backward([o for o in outs], [torch.ones_like(o) for o in outs])
    return run


def kernel_bandwidth(dev, windows, iters):
    """each kernel alone at a segmentation-recipe size: ms and bytes moved (compulsory reads + writes) per second"""
    B = 2
    out = ["# kernels alone, fp32, segmentation sizes (B = 2): GB/s = compulsory bytes read + written / time"]

    def one(name, fn, nbytes):
        ms, sp = measure(fn, windows, iters)
        out.append(f"{name:34s} {ms:8.3f} ms (spread {sp:5.1%})  {nbytes / ms / 1e6:8.1f} GB/s")
        print(out[-1], flush=True)
    H = W = 256
    x = torch.randn(B * H * W, 64, device=dev, requires_grad=True)
    cols = adapter._Conv3x3UnfoldFn.apply(x, B, H, W, 1)
    g = torch.randn_like(cols)
    one("me_conv3x3_gather 256x256x64 s1", lambda: adapter._Conv3x3UnfoldFn.apply(x.detach(), B, H, W, 1), 4 * (x.numel() + cols.numel()))
    one("me_conv3x3_scatter 256x256x64 s1", lambda: torch.autograd.grad(cols, x, g, retain_graph=True), 4 * (x.numel() + cols.numel()))
    y = M.max_pool3x3s2_rows(x, B, H, W)
    gy = torch.randn_like(y)
    one("me_maxpool3x3s2_rows 256x256x64", lambda: M.max_pool3x3s2_rows(x.detach(), B, H, W), 4 * x.numel() + 5 * y.numel())
    one("me_maxpool3x3s2_rows_bwd", lambda: torch.autograd.grad(y, x, gy, retain_graph=True), 4 * x.numel() + 5 * y.numel())
    h = w = 32
    t = torch.randn(B * h * w, 768, device=dev, requires_grad=True)
    for f in (4, 2, 0.5):
        r = M.resize_rows_batched(t, B, h, w, scale_factor=f)
        gr = torch.randn_like(r)
        one(f"me_resize_rows_batched 32x32x768 x{f}", lambda f=f: M.resize_rows_batched(t.detach(), B, h, w, scale_factor=f), 4 * (t.numel() + r.numel()))
        one(f"me_resize_rows_batched_bwd x{f}", lambda r=r, gr=gr: torch.autograd.grad(r, t, gr, retain_graph=True), 4 * (t.numel() + r.numel()))
    c2 = torch.randn(B * 64 * 64, 4 * 768, device=dev, requires_grad=True)
    bias = torch.randn(768, device=dev)
    add = torch.randn(B * 128 * 128, 768, device=dev)
    up = adapter._Upsample2xFn.apply(c2, bias, add, B, 64, 64)
    gu = torch.randn_like(up)
    one("me_upsample2x_rows 64x64x768 +add", lambda: adapter._Upsample2xFn.apply(c2.detach(), bias, add, B, 64, 64), 4 * (c2.numel() + 2 * up.numel()))
    one("me_upsample2x_rows_bwd", lambda: torch.autograd.grad(up, c2, gu, retain_graph=True), 4 * (c2.numel() + up.numel()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_adapter_time.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-backbone", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/vit_adapter_time.py on {torch.cuda.get_device_name(0)}: ms per call, median of {args.windows} windows x {args.iters} calls "
             "(spread = (max - min) / median over the windows); fp32, training mode", "# rows = this package (token rows, HIP); torch = the same "
             "parameters through nn.Conv2d / F.max_pool2d / F.interpolate / nn.ConvTranspose2d, channel-first"]
    model = M.ViTAdapter(**vc.DET_BASE).to(dev).train()
    for label, (B, Hi, Wi) in SHAPES.items():
        H, W, D = Hi // 16, Wi // 16, 768
        img = torch.randn(B, 3, Hi, Wi, device=dev)
        c1r = torch.randn(B * 16 * H * W, D, device=dev, requires_grad=True)
        c1i = torch.randn(B, D, 4 * H, 4 * W, device=dev, requires_grad=True)
        c = torch.randn(B, 4 * H * W + H * W + (H // 2) * (W // 2), D, device=dev, requires_grad=True)
        x = torch.randn(B, H * W, D, device=dev, requires_grad=True)
        parts = {
            "spm": (lambda: model.spm(img), lambda: spm_torch(model.spm, img), []),
            "tail": (lambda: tail_rows(model, c1r, c, x, B, H, W), lambda: tail_torch(model, c1i, c, x, B, H, W), [c1r, c1i, c, x]),
        }
        for part, (rows_fn, torch_fn, leaves) in parts.items():
            for mode in ("fwd", "fwd+bwd"):
                res = []
                for fn in (rows_fn, torch_fn):
                    if mode == "fwd":
                        def call(fn=fn):
                            with torch.no_grad():
                                fn()
                    else:
                        call = with_backward(fn, leaves + list(model.parameters()))
                    res.append(measure(call, args.windows, args.iters))
                (r, rs), (t, ts) = res
                lines.append(f"{label:24s} {part:5s} {mode:8s} rows {r:9.3f} ms (spread {rs:5.1%})   torch {t:9.3f} ms (spread {ts:5.1%})   "
                             f"rows / torch {r / t:5.2f}")
                print(lines[-1], flush=True)
        # the fp32 convolutions as ONE me_gemm call each (what heads.linear would do), against the 128-column chunks of conv3x3_rows
        keep = adapter.CONV_K_CHUNK
        adapter.CONV_K_CHUNK = 1 << 30
        try:
            for mode in ("fwd", "fwd+bwd"):
                if mode == "fwd":
                    def call():
                        with torch.no_grad():
                            model.spm(img)
                else:
                    call = with_backward(lambda: model.spm(img), list(model.parameters()))
                r, rs = measure(call, args.windows, args.iters)
                lines.append(f"{label:24s} spm   {mode:8s} rows, one GEMM call per convolution {r:9.3f} ms (spread {rs:5.1%})")
                print(lines[-1], flush=True)
        finally:
            adapter.CONV_K_CHUNK = keep
        if not args.skip_backbone:
            for mode in ("fwd", "fwd+bwd"):
                if mode == "fwd":
                    def call():
                        with torch.no_grad():
                            model(img)
                else:
                    call = with_backward(lambda: model(img), list(model.parameters()))
                r, rs = measure(call, args.windows, max(1, args.iters // 2))
                lines.append(f"{label:24s} whole {mode:8s} rows {r:9.3f} ms (spread {rs:5.1%})")
                print(lines[-1], flush=True)
    lines += kernel_bandwidth(dev, args.windows, args.iters)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
