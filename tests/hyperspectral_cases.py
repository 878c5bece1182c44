"""Cases of the hyperspectral tokenizer tests and the plain-torch restatement of the reference's input pipeline
(Hyper-spectrum/train.py:80-125 as stated in include/metaenc.h).  A plain module: tools/make_hyperspectral_golden.py imports it to
build tests/golden/hyperspectral.npz from the reference's own functions, the CPU and GPU tests import it to compare against that.

Small cases: inputs, parameters and the reference's results are IN the fixture.  Wide cases (the reference's K = 147 setting, the odd
Pavia band count) are synthesised here from a seed and checked against the restatement, which the CPU test ties to the reference."""
from __future__ import annotations

import numpy as np
import torch

# name -> (H, W, bands, patch, band_patch)
SMALL = {
    "p1b1": (9, 11, 13, 1, 1), "p1b3": (9, 11, 13, 1, 3), "p1b5": (9, 11, 13, 1, 5), "p3b3": (9, 11, 13, 3, 3),
    "p7b3": (9, 11, 13, 7, 3), "p7b5": (9, 11, 13, 7, 5), "p5b7": (5, 6, 7, 5, 7),
}
SMALL_C = 24                         # a multiple of 8 that is no multiple of a 16- or 32-channel tile
# name -> (H, W, bands, patch, band_patch, B)
WIDE = {"indian": (12, 10, 200, 7, 3, 5), "pavia": (12, 10, 103, 3, 3, 3)}
WIDE_C = (768, 64)
# the 2-block classifier case: geometry of a small case + the reference constructor's arguments
CLASSIFIER = dict(case="p3b3", num_classes=5, dim=64, depth=2, heads=4, mlp_dim=128)


def _seed(name: str) -> int:
    return 1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def geometry(name: str):
    g = SMALL.get(name) or WIDE[name]
    return g[:5]


def small_points(H: int, W: int) -> np.ndarray:
    """the four corners, the centre and one duplicate (of a corner: two rows of a batch that read the same window)"""
    return np.array([[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1], [H // 2, W // 2], [H - 1, 0]], dtype=np.int64)


def make_cube(name: str) -> np.ndarray:
    H, W, bands = geometry(name)[:3]
    return np.random.default_rng(_seed(name)).random((H, W, bands), dtype=np.float32)       # band-normalised data lies in [0, 1]


def make_points(name: str) -> np.ndarray:
    if name in SMALL:
        H, W = SMALL[name][:2]
        return small_points(H, W)
    H, W, _, _, _, B = WIDE[name]
    rng = np.random.default_rng(_seed(name) + 1)
    pts = np.stack([rng.integers(0, H, B), rng.integers(0, W, B)], axis=1).astype(np.int64)
    pts[0] = (0, 0)
    pts[-1] = (H - 1, W - 1)
    return pts


def make_params(name: str, C: int) -> dict:
    """the tokenizer's parameters under the reference's names (float32 numpy)"""
    _, _, bands, p, bp = geometry(name)
    K = p * p * bp
    rng = np.random.default_rng(_seed(name) + 7 * C)
    return {"patch_to_embedding.weight": (rng.standard_normal((C, K)) / np.sqrt(K)).astype(np.float32),
            "patch_to_embedding.bias": (0.1 * rng.standard_normal(C)).astype(np.float32),
            "cls_token": rng.standard_normal((1, 1, C)).astype(np.float32),
            "pos_embedding": rng.standard_normal((1, bands + 1, C)).astype(np.float32)}


def make_dy(name: str, C: int, B: int) -> torch.Tensor:
    bands = geometry(name)[2]
    g = torch.Generator().manual_seed(_seed(name) + 13 * C)
    return torch.randn(B, bands + 1, C, generator=g)


def _refl(i: torch.Tensor, n: int) -> torch.Tensor:
    return torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))


def band_shift(g: int, nn: int, p: int) -> int:
    if p == 1 or g >= nn:
        return g - nn
    return -(g + 1)


def restate(cube: torch.Tensor, points: torch.Tensor, patch: int, band_patch: int) -> torch.Tensor:
    """[B, bands, patch^2 band_patch]: token (b, j), feature k = g p^2 + dy p + dx = cube[refl(r + dy - p // 2), refl(c + dx - p // 2),
    (j + s(g)) mod bands] -- pure indexing, so it is exact in any dtype and differentiable in nothing"""
    H, W, bands = cube.shape
    p, nn = patch, band_patch // 2
    points = points.long()
    off = torch.arange(p) - p // 2
    rows = _refl(points[:, 0:1] + off[None, :], H)                           # [B, p]
    cols = _refl(points[:, 1:2] + off[None, :], W)                           # [B, p]
    win = cube[rows[:, :, None], cols[:, None, :], :]                        # [B, p, p, bands]
    win = win.reshape(points.shape[0], p * p, bands)
    j = torch.arange(bands)
    groups = [win[:, :, (j + band_shift(g, nn, p)) % bands] for g in range(band_patch)]      # each [B, p^2, bands]
    return torch.cat(groups, dim=1).transpose(1, 2).contiguous()


def embed_reference(x: torch.Tensor, params: dict) -> torch.Tensor:
    """the reference's tokenizer forward (Hyper-spectrum/metatransformer.py:152-158) in plain torch, in x's dtype; x [B, n, K]"""
    P = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v).to(x.dtype) for k, v in params.items()}
    y = torch.nn.functional.linear(x, P["patch_to_embedding.weight"], P["patch_to_embedding.bias"])
    B, n, _ = y.shape
    y = torch.cat([P["cls_token"].expand(B, -1, -1), y], dim=1)
    return y + P["pos_embedding"][:, :n + 1]
