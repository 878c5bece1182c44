"""Multi-scale deformable attention timing at the ViT-Adapter recipe sizes: me_ms_deform_attn_fwd / _bwd next to the same
operation composed from F.grid_sample in PyTorch on the same GPU (what there was before the kernel).

    python tools/msda_time.py [--iters 20] [--out PATH] [--rev LABEL]

Geometries (12 heads x 32 channels, 4 points): the injector (ViT tokens on the stride-16 grid attend to the three pyramid levels)
and the extractor (the pyramid tokens attend to the ViT tokens), at the detection recipe's 1333 x 800 input (50 x 84 tokens,
pyramid 100 x 168 / 50 x 84 / 25 x 42) and the segmentation recipe's 512 x 512 crop (32 x 32; 64 x 64 / 32 x 32 / 16 x 16), N in
{1, 2}.  Reference points on the pixel centres, offsets uniform in +-4 pixels, attention weights uniform.  Times are device
events around windows of back-to-back calls, each window at least 20 ms and at least `iters` calls long, after 5 warm-up calls;
the HIP and the PyTorch windows alternate and the table gives the median and the spread of 7 windows.  The forwards of 20 us and
less are launch and host-side overhead figures, not kernel times.  Backward = all three gradients
(autograd's backward for the PyTorch form, me_ms_deform_attn_bwd with its workspace allocation for the kernel).  Gathered
bytes = 4 corners x 4 D bytes per (query, head, level, point) sample, the forward's mandatory reads.
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metatransformer_amd as M  # noqa: E402
from metatransformer_amd import adapter  # noqa: E402

HEADS, D, P = 12, 32, 4
SIZES = {"det 50x84": (50, 84), "seg 32x32": (32, 32)}


def grid_sample_form(value, shapes, starts, loc, attn):
    N, S, M_, Dh = value.shape
    Lq, L, Pn = loc.shape[1], loc.shape[3], loc.shape[4]
    taps = []
    for l, ((H, W), st) in enumerate(zip(shapes, starts)):
        img = value[:, st:st + H * W].permute(0, 2, 3, 1).reshape(N * M_, Dh, H, W)
        grid = (2 * loc[:, :, :, l] - 1).permute(0, 2, 1, 3, 4).reshape(N * M_, Lq, Pn, 2)
        taps.append(F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False))
    w = attn.permute(0, 2, 1, 3, 4).reshape(N * M_, 1, Lq, L * Pn)
    return (torch.cat(taps, -1) * w).sum(-1).view(N, M_ * Dh, Lq).transpose(1, 2).contiguous()


WINDOW_MS = 20.0      # a timed window lasts at least this long, so that it measures the kernels and not one scheduling hiccup


def calls_per_window(fn, floor):
    """warm up (5 calls), then size the window from a 10-call estimate"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    per_call = max(e0.elapsed_time(e1) / 10, 1e-3)
    return max(floor, int(WINDOW_MS / per_call) + 1)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def timed_pair(hip, pt, floor, windows=7):
    """the two sides in alternating windows -> ((median, min, max) HIP, (median, min, max) PyTorch), us per call"""
    n_hip, n_pt = calls_per_window(hip, floor), calls_per_window(pt, floor)
    a, b = [], []
    for _ in range(windows):
        a.append(window(hip, n_hip))
        b.append(window(pt, n_pt))
    return tuple((statistics.median(x), min(x), max(x)) for x in (a, b))


def case(hw, geometry, N, dev):
    h, w = hw
    pyramid, vit = [(2 * h, 2 * w), (h, w), (h // 2, w // 2)], [(h, w)]
    q_shapes, shapes = (vit, pyramid) if geometry == "injector" else (pyramid, vit)
    starts, S = [], 0
    for a, b in shapes:
        starts.append(S)
        S += a * b
    ref = M.get_reference_points(q_shapes, dev)                                  # [1, Lq, 1, 2]
    Lq, L = ref.shape[1], len(shapes)
    g = torch.Generator(device=dev).manual_seed(1)
    norm = torch.tensor([[b, a] for a, b in shapes], dtype=torch.float32, device=dev)
    off = (torch.rand(N, Lq, HEADS, L, P, 2, device=dev, generator=g) * 8 - 4) / norm[None, None, None, :, None, :]
    loc = (ref[:, :, None, :, None, :] + off).contiguous()
    attn = torch.rand(N, Lq, HEADS, L, P, device=dev, generator=g) / (L * P)
    value = torch.randn(N, S, HEADS, D, device=dev, generator=g)
    dout = torch.randn(N, Lq, HEADS * D, device=dev, generator=g)
    return value, shapes, starts, loc, attn, dout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rev", default=None, help="label of the measured tree for the header (default: git rev-parse --short HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rev = args.rev
    if not rev:
        try:
            rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                 cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
        except OSError:
            rev = ""
    lines = [f"# tools/msda_time.py --iters {args.iters} --rev {rev or 'unknown'!r}   ({torch.cuda.get_device_name(0)}; --rev names the tree)",
             f"# us per call: median (min-max) of 7 windows of >= {WINDOW_MS:.0f} ms, HIP and PyTorch windows alternating, 5 warm-up calls;",
             "# GB/s = gathered bytes of the forward / median forward time; x = PyTorch median / HIP median",
             f"{'size':<10} {'geometry':<10} {'N':>2} {'Lq':>6} {'S':>6} | {'fwd HIP':>22} {'GB/s':>6} {'fwd torch':>24} {'x':>6} | "
             f"{'bwd HIP':>24} {'bwd torch':>24} {'x':>5}"]

    def cell(t):
        return f"{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})"
    for size, hw in SIZES.items():
        for geometry in ("injector", "extractor"):
            for N in (1, 2):
                value, shapes, starts, loc, attn, dout = case(hw, geometry, N, dev)
                Lq, L, S = loc.shape[1], len(shapes), value.shape[1]
                gathered = N * Lq * HEADS * L * P * 4 * D * 4
                v, lo, aw = (t.clone().requires_grad_() for t in (value, loc, attn))
                out = grid_sample_form(v, shapes, starts, lo, aw)
                f_hip, f_pt = timed_pair(lambda: M.ms_deform_attn(value, shapes, starts, loc, attn),
                                         lambda: grid_sample_form(value, shapes, starts, loc, attn), args.iters)
                b_hip, b_pt = timed_pair(lambda: adapter._msda_backward(value, shapes, starts, loc, attn, dout, True, True),
                                         lambda: torch.autograd.grad(out, (v, lo, aw), dout, retain_graph=True), args.iters)
                lines.append(f"{size:<10} {geometry:<10} {N:>2} {Lq:>6} {S:>6} | {cell(f_hip):>22} {gathered / f_hip[0] / 1e3:>6.0f} "
                             f"{cell(f_pt):>24} {f_pt[0] / f_hip[0]:>6.2f} | {cell(b_hip):>24} {cell(b_pt):>24} {b_pt[0] / b_hip[0]:>5.2f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
