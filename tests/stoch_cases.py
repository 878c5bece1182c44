"""Host restatement of the masks of the stochastic ops (dropout, drop-path, attn_drop), so that every one of them has a deterministic
float64 reference: no statistics, no exempted elements.

The stream is a pure function (csrc/common.h, u01_hash): SplitMix64's output function on the state seed + (idx + 1) * GOLDEN, top 24
bits -> u in [0, 1); an element is KEPT iff u >= p (both fp32) and a kept value is scaled by 1 / (1 - p).  What differs between the
ops is the index (include/metaenc.h):
    attention probabilities   idx = ((b * H + h) * N + q) * N + k          over the batch the kernel is launched on
    me_dropout_add, dropout   idx = r * cols + c
    me_dropout_add, drop-path idx = r // rows_per_sample, on the stream of seed ^ PATH_XOR
A training-mode Block draws ONE int64 seed per call from torch's CPU generator and gives each op seed + offset
(metatransformer_amd/encoder.py: SEED_BRANCH1 / SEED_MLP_HIDDEN / SEED_BRANCH2 / SEED_ATTN_DROP).

numpy arrays carry the element index (uint64 arithmetic wraps); everything that involves the seed alone is done in Python integers
mod 2^64.  tests/test_stoch_cases_cpu.py keeps this file honest without a GPU.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from metatransformer_amd.encoder import SEED_ATTN_DROP, SEED_BRANCH1, SEED_BRANCH2, SEED_MLP_HIDDEN
from oracle import block_oracle as bo

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PATH_XOR = 0xD1B54A32D192ED03


def u01(seed: int, idx) -> np.ndarray:
    """u01_hash(seed, idx) for an array of indices: float32 in [0, 1) with 24 random bits"""
    base = (int(seed) + GOLDEN) & MASK64                      # seed + GOLDEN, wrapped (negative int64 seeds: two's complement)
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = idx * np.uint64(GOLDEN) + np.uint64(base)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def keep(seed: int, idx, p: float) -> np.ndarray:
    """bool: the element is kept (p = 0 keeps everything: u >= 0)"""
    return u01(seed, idx) >= np.float32(p)


def scale_f32(p: float) -> np.float32:
    """1 / (1 - p) as the kernels form it: fp32 operands, correctly rounded fp32 division (1 for p = 0)"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)


def attn_keep(seed: int, B: int, H: int, N: int, p: float, items: Optional[Sequence[int]] = None) -> np.ndarray:
    """keep mask of the attention probabilities: bool [B, H, N, N], or [len(items), N, N] for the listed flat items b * H + h"""
    qk = (np.arange(N, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :])
    todo = range(B * H) if items is None else items
    out = np.empty((len(todo), N, N), dtype=bool)
    for j, it in enumerate(todo):
        assert 0 <= int(it) < B * H
        out[j] = keep(seed, qk + np.uint64(int(it) * N * N), p)
    return out.reshape(B, H, N, N) if items is None else out


def dropout_keep(seed: int, rows: int, cols: int, p: float) -> np.ndarray:
    """element-wise keep mask of me_dropout_add: bool [rows, cols]"""
    return keep(seed, np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols), p)


def path_keep(seed: int, n_samples: int, p: float) -> np.ndarray:
    """per-sample keep mask of me_dropout_add's drop-path: bool [n_samples]"""
    return keep((int(seed) & MASK64) ^ PATH_XOR, np.arange(n_samples, dtype=np.uint64), p)


def dropout_add_scale(seed: int, rows: int, cols: int, rows_per_sample: int, p_drop: float, p_path: float) -> np.ndarray:
    """the factor me_dropout_add puts on v[r, c], in the kernel's own fp32 arithmetic: path scale first, then times the keep scale"""
    k = np.ones((rows, cols), dtype=np.float32)
    if p_path > 0:
        n_samples = -(-rows // rows_per_sample)
        pk = path_keep(seed, n_samples, p_path)[np.arange(rows) // rows_per_sample]
        k = k * np.where(pk, scale_f32(p_path), np.float32(0.0))[:, None]
    if p_drop > 0:
        k = np.where(dropout_keep(seed, rows, cols, p_drop), k * scale_f32(p_drop), np.float32(0.0))
    return k.astype(np.float32)


def _f64(mask: np.ndarray, p: float) -> torch.Tensor:
    """bool keep mask -> float64 factor keep / (1 - p), with p as the kernels see it (fp32)"""
    return torch.from_numpy(mask.astype(np.float64)) / (1.0 - float(np.float32(p)))


def attention_masked(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, factor: Optional[torch.Tensor]):
    """float64 attention with dropout on the normalised probabilities: O = (softmax(S) * factor) @ V, lse = logsumexp(S)
    (unmasked).  q, k, v [..., N, hd]; factor [..., N, N] or None."""
    s = (q @ k.transpose(-2, -1)) * scale
    a = torch.softmax(s, dim=-1)
    if factor is not None:
        a = a * factor
    return a @ v, torch.logsumexp(s, dim=-1)


def attention_qkv_masked(qkv: torch.Tensor, B: int, N: int, H: int, hd: int, scale: float, p: float, seed: int):
    """the library's layout: qkv [B * N, 3 * H * hd] -> (out [B * N, H * hd], lse [B, H, N]), differentiable"""
    q, k, v = qkv.double().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    factor = _f64(attn_keep(seed, B, H, N, p), p) if p > 0 else None
    o, lse = attention_masked(q, k, v, scale, factor)
    return o.transpose(1, 2).reshape(B * N, H * hd), lse


def _branch(t: torch.Tensor, seed: int, n_per_sample: int, p_drop: float, p_path: float) -> torch.Tensor:
    """drop_path(dropout(t)) of one residual branch, t [M, C]"""
    M, C = t.shape
    if p_drop > 0:
        t = t * _f64(dropout_keep(seed, M, C, p_drop), p_drop)
    if p_path > 0:
        pk = path_keep(seed, M // n_per_sample, p_path)
        t = t * _f64(np.repeat(pk, n_per_sample), p_path)[:, None]
    return t


def block_forward_masked(x: torch.Tensor, sd: Dict[str, torch.Tensor], heads: int, p_drop: float, p_path: float, p_attn: float,
                         seed: int, gamma1: Optional[torch.Tensor] = None, gamma2: Optional[torch.Tensor] = None,
                         window: Optional[tuple] = None, eps: float = 1e-5) -> torch.Tensor:
    """Training-mode Block.forward in float64 with the masks where encoder.py applies them:
        x1 = x  + path1 * keep1 * gamma1 * proj(attn_drop(softmax) @ v)       attention probabilities: seed + SEED_ATTN_DROP
                                                                              branch 1 (dropout and drop-path): seed + SEED_BRANCH1
        y  = x1 + path2 * keep2 * gamma2 * fc2(keep_h * gelu(fc1(LN2(x1))))   hidden activation: seed + SEED_MLP_HIDDEN
                                                                              branch 2: seed + SEED_BRANCH2
    window = (H, W, window_size): windowed attention (zero-padded grid, bo.windowed_attention); its mask is indexed over the
    windowed batch of B * n_windows items of ws * ws tokens.  Differentiable by torch autograd in x and every entry of sd."""
    B, N, C = x.shape
    hd = C // heads
    scale = hd ** -0.5
    x2 = x.double().reshape(B * N, C)
    p = {k: v.double() for k, v in sd.items()}
    qkv = bo.linear(bo.layer_norm(x2, p["norm1.weight"], p["norm1.bias"], eps), p["attn.qkv.weight"], p.get("attn.qkv.bias"))
    if window is None:
        o, _ = attention_qkv_masked(qkv, B, N, heads, hd, scale, p_attn, seed + SEED_ATTN_DROP)
    else:
        gh_, gw_, ws = window
        gh, gw = -(-gh_ // ws), -(-gw_ // ws)
        grid = qkv.new_zeros(B, gh * ws, gw * ws, 3 * C)
        grid[:, :gh_, :gw_] = qkv.reshape(B, gh_, gw_, 3 * C)
        wins = grid.reshape(B, gh, ws, gw, ws, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(B * gh * gw * ws * ws, 3 * C)
        ow, _ = attention_qkv_masked(wins, B * gh * gw, ws * ws, heads, hd, scale, p_attn, seed + SEED_ATTN_DROP)
        o = ow.reshape(B, gh, gw, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, gh * ws, gw * ws, C)[:, :gh_, :gw_]
        o = o.reshape(B * N, C)
    t1 = bo.linear(o, p["attn.proj.weight"], p["attn.proj.bias"])
    x1 = x2 + _branch(t1 if gamma1 is None else gamma1.double() * t1, seed + SEED_BRANCH1, N, p_drop, p_path)
    h = bo.gelu_erf(bo.linear(bo.layer_norm(x1, p["norm2.weight"], p["norm2.bias"], eps), p["mlp.fc1.weight"], p["mlp.fc1.bias"]))
    if p_drop > 0:
        h = h * _f64(dropout_keep(seed + SEED_MLP_HIDDEN, B * N, h.shape[1], p_drop), p_drop)
    t2 = bo.linear(h, p["mlp.fc2.weight"], p["mlp.fc2.bias"])
    y = x1 + _branch(t2 if gamma2 is None else gamma2.double() * t2, seed + SEED_BRANCH2, N, p_drop, p_path)
    return y.reshape(B, N, C)


def block_seed(manual_seed: int) -> int:
    """the seed Block.forward draws as its first use of torch's CPU generator after torch.manual_seed(manual_seed)"""
    torch.manual_seed(manual_seed)
    return int(torch.empty((), dtype=torch.int64).random_().item())
