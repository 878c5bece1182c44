"""VideoMAE pre-training step timing: one step (forward, loss, backward) of PretrainVisionTransformer through two routes on the same GPU

  visible    this package's route: me_tubelet_gather of the visible tubelets + me_gemm, me_mae_assemble_fwd, me_mae_loss
  composed   what a user of this package composed before: VideoPatchEmbed of all tubelets + the position table, boolean indexing
             (x[~mask]), torch.cat of the decoder input, the per-patch normalised target of the WHOLE clip from full-size torch
             temporaries (Video/engine_for_pretraining.py:75-98) and the loss in torch -- on the same Blocks, norms and Linears

    python tools/video_mae_time.py [--iters 3] [--batch 32] [--out PATH] [--rev LABEL]

Shape: VideoMAE Base (encoder 768 / 12 heads / 12 blocks, decoder 384 / 6 heads / 4 blocks, 16 frames of 224 x 224, tubelets 2 x 16 x 16:
1568 tokens), mask ratio 0.9 (1411 masked, 157 visible), fp32 parameters under torch.autocast(bfloat16).  Also timed alone: the token embed of the
visible tokens (forward), and the target + loss (forward and gradient to the prediction).  Method of tools/hyperspectral_time.py: device
events around windows of back-to-back calls, each at least 20 ms and `iters` calls long, warm-up calls first, the routes in
alternating windows, median (min-max) of 7 windows.  Below the table: how far the two routes' loss and gradients are apart.
"""
import argparse
import os
import statistics
import subprocess
import sys
from functools import partial

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metatransformer_amd as M  # noqa: E402
from metatransformer_amd import video_mae as vm  # noqa: E402
from metatransformer_amd.heads import linear  # noqa: E402

WINDOW_MS = 20.0
MASK_RATIO = 0.9


def calls_per_window(fn, floor):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return max(floor, int(WINDOW_MS / max(e0.elapsed_time(e1) / 3, 1e-3)) + 1)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def timed(fns, floor, windows=7):
    n = [calls_per_window(f, floor) for f in fns]
    t = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            t[i].append(window(f, n[i]))
    return [(statistics.median(x), min(x), max(x)) for x in t]


def torch_target(clip, decoded, kt, kh, kw):
    """engine_for_pretraining.py:75-98 in plain torch (the rearranges written as reshape / permute): labels of the decoded tokens"""
    B, C, T, H, W = clip.shape
    mean = torch.as_tensor(vm.IMAGENET_DEFAULT_MEAN, device=clip.device)[None, :, None, None, None]
    std = torch.as_tensor(vm.IMAGENET_DEFAULT_STD, device=clip.device)[None, :, None, None, None]
    unnorm = clip * std + mean
    sq = unnorm.reshape(B, C, T // kt, kt, H // kh, kh, W // kw, kw).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, -1, kt * kh * kw, C)
    norm = (sq - sq.mean(dim=-2, keepdim=True)) / (sq.var(dim=-2, unbiased=True, keepdim=True).sqrt() + 1e-6)
    patches = norm.reshape(B, sq.shape[1], -1)
    return patches[decoded].reshape(B, -1, patches.shape[-1])


def torch_loss(pred, labels, cal):
    loss = ((pred - labels) ** 2).mean(dim=-1)
    return (loss * cal).sum() / cal.sum()


def composed_tokens(model, clip, mask):
    enc = model.encoder
    x = enc.patch_embed(clip) + enc.pos_embed
    return x[~mask].reshape(x.shape[0], -1, x.shape[-1])


def composed_forward(model, clip, mask):
    enc = model.encoder
    B = clip.shape[0]
    x = composed_tokens(model, clip, mask).float()
    for blk in enc.blocks:
        x = blk(x)
    x = linear(vm._norm(x, enc.norm, vm._stream_dtype(enc.norm.weight, torch.bfloat16)), model.encoder_to_decoder.weight, None)      # as the model does
    pos = model.pos_embed.expand(B, -1, -1)
    Cd = pos.shape[-1]
    x_full = torch.cat([x + pos[~mask].reshape(B, -1, Cd), model.mask_token + pos[mask].reshape(B, -1, Cd)], dim=1)
    return model.decoder(x_full, int(mask[0].sum()))


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
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
    B = args.batch
    torch.manual_seed(0)
    model = M.PretrainVisionTransformer(encoder_embed_dim=768, encoder_depth=12, encoder_num_heads=12, decoder_num_classes=1536, decoder_embed_dim=384,
                                        decoder_depth=4, decoder_num_heads=6, mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6)).to(dev)
    N = model.encoder.patch_embed.num_patches
    g = torch.Generator().manual_seed(1)
    clip = torch.randn(B, 3, 16, 224, 224, generator=g).to(dev)
    nmask = int(round(N * MASK_RATIO))
    mask = torch.zeros(B, N, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(N, generator=g)[:nmask]] = True
    mask = mask.to(dev)
    geom = (2, 16, 16)
    params = [p for p in model.parameters() if p.requires_grad]
    ac = partial(torch.autocast, "cuda", dtype=torch.bfloat16)

    def step_visible():
        with ac():
            y = model(clip, mask)
        loss = M.mae_reconstruction_loss(y, clip, mask)
        return loss, torch.autograd.grad(loss, params, allow_unused=True)

    def step_composed():
        with ac():
            y = composed_forward(model, clip, mask)
        loss = torch_loss(y, torch_target(clip, mask, *geom), torch.ones(B, nmask, device=dev))
        return loss, torch.autograd.grad(loss, params, allow_unused=True)

    def embed_visible():
        with torch.no_grad(), ac():
            (vis_idx,) = vm.token_indices("time", ~mask)
            pe = model.encoder.patch_embed
            return vm._VisibleEmbedFn.apply(clip, vis_idx, pe.proj.weight, pe.proj.bias, model.encoder.pos_embed, geom, torch.bfloat16, torch.float32)

    def embed_composed():
        with torch.no_grad(), ac():
            return composed_tokens(model, clip, mask)

    pred = torch.randn(B, nmask, 1536, device=dev)

    def loss_visible():
        p = pred.detach().requires_grad_(True)
        return torch.autograd.grad(M.mae_reconstruction_loss(p, clip, mask), p)

    def loss_composed():
        p = pred.detach().requires_grad_(True)
        return torch.autograd.grad(torch_loss(p, torch_target(clip, mask, *geom), torch.ones(B, nmask, device=dev)), p)

    lines = [f"# tools/video_mae_time.py --iters {args.iters} --batch {B} --rev {rev or 'unknown'!r}   ({torch.cuda.get_device_name(0)}; --rev names the tree)",
             f"# ms per call: median (min-max) of 7 windows of >= {WINDOW_MS:.0f} ms, the routes alternating; VideoMAE Base, B = {B}, {N} tokens, "
             f"{N - nmask} visible, fp32 parameters under bf16 autocast",
             f"{'what':<34} | {'visible':>26} {'composed':>26}"]

    def cell(t):
        return f"{t[0]:.2f} ({t[1]:.2f}-{t[2]:.2f})"
    for label, fns in (("pre-training step (fwd+loss+bwd)", (step_visible, step_composed)), ("token embed, forward", (embed_visible, embed_composed)),
                       ("target + loss, fwd + dpred", (loss_visible, loss_composed))):
        t = timed(list(fns), args.iters)
        lines.append(f"{label:<34} | " + " ".join(f"{cell(x):>26}" for x in t))
        print(lines[-1], flush=True)
    la, ga = step_visible()
    lb, gb = step_composed()
    lines.append(f"# visible against composed: loss {float(la.detach()):.6f} / {float(lb.detach()):.6f}; worst parameter gradient distance "
                 f"{max(rel(a, b) for a, b in zip(ga, gb) if a is not None and b is not None):.2e} (max |a - b| / max |b|)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
