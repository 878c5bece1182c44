"""Hyperspectral tokenizer timing: forward and forward + parameter gradients of HyperSpectralEmbed through four paths on the same GPU

  auto       the default route: fused under bf16; with fp32 arithmetic me_hsi_gather + me_gemm forward (bias, position rows and the cls-row
             offset in the GEMM's epilogue) and the fused backward
  fused      me_hsi_embed_fwd / me_hsi_embed_wgrad (the gathered tensor is never written)
  gathered   this library's unfused route: me_hsi_gather into a K-padded buffer, me_gemm, the cls / position rows added afterwards
  torch      plain PyTorch on the device: reflect / roll indexing of the cube, F.linear, cat, add

    python tools/hyperspectral_time.py [--iters 20] [--out PATH] [--rev LABEL] [--suite "N passed"]

Shapes: Indian Pines (145 x 145 x 200, patch 7, band_patch 3) at B = 64 and B = 1024, Pavia (610 x 340 x 103, same windows) at B = 1024;
C = 768; fp32 parameters, and the same under torch.autocast(bfloat16).  Method of tools/graph_tokenizer_time.py: device events around
windows of back-to-back calls, each at least 20 ms and `iters` calls long, 5 warm-up calls, the paths in alternating windows,
median (min-max) of 7 windows.  Below the table: the distance of each path's output and gradients to a float64 evaluation on the CPU
(Indian Pines, B = 64), max |x - ref| / max |ref|.
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

WINDOW_MS = 20.0
SHAPES = (("Indian Pines", 145, 145, 200, 64), ("Indian Pines", 145, 145, 200, 1024), ("Pavia", 610, 340, 103, 1024))
PATCH, BAND_PATCH, C = 7, 3, 768


def calls_per_window(fn, floor):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return max(floor, int(WINDOW_MS / max(e0.elapsed_time(e1) / 10, 1e-3)) + 1)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def timed(fns, floor, windows=7):
    n = [calls_per_window(f, floor) for f in fns]
    t = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            t[i].append(window(f, n[i]))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def torch_tokens(cube, points, patch, band_patch):
    """the gathered tensor by PyTorch indexing on the cube's device (include/metaenc.h states the formula)"""
    H, W, bands = cube.shape
    p, nn = patch, band_patch // 2
    dev = cube.device
    off = torch.arange(p, device=dev) - p // 2

    def refl(i, n):
        return torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))
    rows, cols = refl(points[:, 0:1] + off[None, :], H), refl(points[:, 1:2] + off[None, :], W)
    win = cube[rows[:, :, None], cols[:, None, :], :].reshape(points.shape[0], p * p, bands)
    shifts = [(g - nn) if (p == 1 or g >= nn) else -(g + 1) for g in range(band_patch)]
    return torch.cat([torch.roll(win, -s, dims=2) for s in shifts], dim=1).transpose(1, 2)


def torch_embed(emb, cube, points):
    x = torch_tokens(cube, points, emb.patch, emb.near_band)
    y = F.linear(x, emb.patch_to_embedding.weight, emb.patch_to_embedding.bias)
    y = torch.cat([emb.cls_token.expand(y.shape[0], -1, -1).to(y.dtype), y], dim=1)
    return y + emb.pos_embedding[:, :y.shape[1]].to(y.dtype)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def distances(emb, cube, points, dout):
    """name -> {path: (forward, worst gradient)} against float64 on the CPU"""
    e64 = M.HyperSpectralEmbed(emb.bands, emb.patch, emb.near_band, C).double()
    e64.load_state_dict({k: v.double().cpu() for k, v in emb.state_dict().items()})
    y64 = torch_embed(e64, cube.double().cpu(), points.cpu())
    g64 = torch.autograd.grad(y64, list(e64.parameters()), dout.double().cpu())
    res = {}
    params = list(emb.parameters())
    for mode in ("fp32", "bf16"):
        for path in ("auto", "fused", "gathered", "torch"):
            emb.route = path if path != "torch" else "fused"
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
                y = torch_embed(emb, cube, points) if path == "torch" else emb(cube, points)
            g = torch.autograd.grad(y, params, dout.to(y.dtype))
            res[(mode, path)] = (rel(y, y64), max(rel(a, b) for a, b in zip(g, g64)))
    emb.route = "auto"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rev", default=None, help="label of the measured tree for the header (default: git rev-parse --short HEAD)")
    ap.add_argument("--suite", default=None, help="the test suite's pass count on the measured tree, recorded in the header")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rev = args.rev
    if not rev:
        try:
            rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                 cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
        except OSError:
            rev = ""
    lines = [f"# tools/hyperspectral_time.py --iters {args.iters} --rev {rev or 'unknown'!r}   ({torch.cuda.get_device_name(0)}; --rev names the tree)",
             f"# test suite on this tree: {args.suite or 'not recorded'}",
             f"# us per call: median (min-max) of 7 windows of >= {WINDOW_MS:.0f} ms, the paths alternating, 5 warm-up calls; patch {PATCH}, "
             f"band_patch {BAND_PATCH} (K = {PATCH * PATCH * BAND_PATCH}), C = {C}",
             f"{'scene':<13} {'B':>5} {'dtype':<5} {'pass':<8} | {'auto':>26} {'fused':>26} {'gathered':>26} {'torch':>26}"]

    def cell(t):
        return f"{t[0]:.1f} ({t[1]:.1f}-{t[2]:.1f})"
    dist = None
    for scene, H, W, bands, B in SHAPES:
        g = torch.Generator().manual_seed(B + bands)
        cube = torch.rand(H, W, bands, generator=g).to(dev)
        points = torch.stack([torch.randint(0, H, (B,), generator=g), torch.randint(0, W, (B,), generator=g)], 1).to(dev)
        torch.manual_seed(0)
        emb = M.HyperSpectralEmbed(bands, PATCH, BAND_PATCH, C).to(dev)
        dout = torch.randn(B, bands + 1, C, generator=g).to(dev)
        params = list(emb.parameters())
        if dist is None:
            dist = distances(emb, cube, points, dout)
        for mode in ("fp32", "bf16"):
            ac = mode == "bf16"
            dy = dout.bfloat16() if ac else dout

            def fwd(path):
                def run():
                    emb.route = path if path != "torch" else "fused"
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                        return torch_embed(emb, cube, points) if path == "torch" else emb(cube, points)
                return run

            def both(path):
                def run():
                    emb.route = path if path != "torch" else "fused"
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                        y = torch_embed(emb, cube, points) if path == "torch" else emb(cube, points)
                    torch.autograd.grad(y, params, dy.to(y.dtype))
                return run
            for label, make in (("fwd", fwd), ("fwd+grad", both)):
                t = timed([make(p) for p in ("auto", "fused", "gathered", "torch")], args.iters)
                lines.append(f"{scene:<13} {B:>5} {mode:<5} {label:<8} | " + " ".join(f"{cell(x):>26}" for x in t))
                print(lines[-1], flush=True)
        emb.route = "auto"
    lines.append("# distance to float64 (Indian Pines, B = 64): forward / worst parameter gradient, max |x - ref| / max |ref|")
    for (mode, path), (f, gr) in dist.items():
        lines.append(f"#   {mode:<5} {path:<9} {f:.2e} / {gr:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
