"""The hyperspectral tokenizer and classifier on the HIP path (Hyper-spectrum/train.py:80-125, Hyper-spectrum/metatransformer.py:111-165).

The reference builds, on the CPU and in float64 numpy, for EVERY labelled pixel of a scene before training starts: the mirror-padded
cube (``mirror_hsi``), a ``patch x patch`` window per pixel (``gain_neighborhood_pixel``) and ``band_patch`` circularly shifted copies of
it side by side (``gain_neighborhood_band``) -- ``patch^2 band_patch`` times the cube -- and feeds ``[B, bands, patch^2 band_patch]``
batches of it through ``nn.Linear``, a cls token and a position embedding.  Here the cube stays on the device as it is and a batch is a
list of pixel coordinates:

  neighborhood_tokens(cube, points, patch, band_patch)   the reference's gathered tensor for those pixels (me_hsi_gather, bit-exact)
  HyperSpectralEmbed(bands, patch, near_band, embed_dim)  the tokenizer: ``forward(cube, points)`` runs the fused kernels
      (me_hsi_embed_fwd: the gathered tensor is never written; backward me_hsi_embed_wgrad regenerates it; ``route`` below names
      the alternatives), ``forward(x)`` with an already gathered ``x [B, n <= bands, K]`` is the reference's call form
  HyperSpectralClassifier(...)                            the reference's MetaTransformer: tokenizer + Block stack + LayerNorm / Linear
      head on the cls token, with the reference's constructor and state-dict keys

Parameter names and shapes are the reference's (``patch_to_embedding.weight [C, K]``, ``cls_token [1, 1, C]``, ``pos_embedding
[1, bands + 1, C]``).  The feature order inside K -- the lower band groups of a ``patch > 1`` window come reversed -- is the
reference's own and is kept, since trained weights depend on it (include/metaenc.h states the formula).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
import torch.nn as nn

from . import _capi, ops
from ._capi import MetaEncError, check, dtype_code, ptr, stream_ptr
from .data2seq import _DropoutFn, _boundary_dtypes
from .linear import linear, pad_to as _pad_to      # (neighborhood_tokens has a `pad_to` argument)
from .weight_cache import _WeightCache

# which route HyperSpectralEmbed.forward(cube, points) takes (DESIGN.md 7g has the timings behind the default):
#   "fused"     me_hsi_embed_fwd, backward me_hsi_embed_wgrad: the gathered tensor is never written
#   "gathered"  this library's unfused route: me_hsi_gather into a K-padded buffer, me_gemm, the cls / position rows added afterwards;
#               backward a TN me_gemm on the saved gathered tensor
#   "auto"      bf16 arithmetic: "fused".  fp32 arithmetic: the forward that measured faster there -- me_hsi_gather + me_gemm with the
#               bias, the position rows and the cls-row offset in the GEMM's epilogue -- and the fused backward (nothing is saved)
DEFAULT_ROUTE = "auto"
ROUTES = ("auto", "fused", "gathered")


def _check_geometry(who: str, H: int, W: int, bands: int, patch: int, band_patch: int) -> int:
    if patch < 1 or patch % 2 != 1:
        raise MetaEncError(f"{who}: patch={patch} must be odd and positive")
    if band_patch < 1 or band_patch % 2 != 1:
        raise MetaEncError(f"{who}: band_patch={band_patch} must be odd and positive")
    if band_patch > bands:
        raise MetaEncError(f"{who}: band_patch={band_patch} exceeds bands={bands}")
    if H is not None and patch // 2 > min(H, W):
        raise MetaEncError(f"{who}: patch={patch} needs patch // 2 <= min(H, W) = {min(H, W)} (one reflection)")
    return patch * patch * band_patch


def _prepare(who: str, cube: torch.Tensor, points: torch.Tensor, patch: int, band_patch: int):
    """(descriptor, cube, points) -- the tensors are returned because the descriptor only holds their addresses"""
    if not isinstance(cube, torch.Tensor) or not cube.is_cuda:
        raise MetaEncError(f"{who}: the cube must be a CUDA tensor (no CPU fallback)")
    if cube.dim() != 3:
        raise MetaEncError(f"{who}: cube {tuple(cube.shape)} must be [H, W, bands]")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
        raise MetaEncError(f"{who}: points must be [B >= 1, 2] (row, col)")
    if points.is_floating_point():
        raise MetaEncError(f"{who}: points must be integers (got {points.dtype})")
    if points.device != cube.device:
        raise MetaEncError(f"{who}: points are on {points.device}, the cube on {cube.device}: move them first (no implicit copies)")
    H, W, bands = cube.shape
    _check_geometry(who, H, W, bands, patch, band_patch)
    if cube.dtype == torch.float64 or cube.dtype == torch.float16:
        cube = cube.float()
    if cube.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"{who}: cube dtype {cube.dtype} unsupported (fp32, bf16; fp64 / fp16 are converted)")
    if cube.stride(2) != 1 or cube.stride(1) < bands or cube.stride(0) < (W - 1) * cube.stride(1) + bands:
        cube = cube.contiguous()
    pts = points.to(torch.int32).contiguous()
    d = _capi.HsiDesc()
    d.cube, d.cube_dtype, d.row_stride, d.pix_stride = cube.data_ptr(), dtype_code(cube.dtype), cube.stride(0), cube.stride(1)
    d.H, d.W, d.bands = H, W, bands
    d.points, d.B, d.patch, d.band_patch = pts.data_ptr(), pts.shape[0], patch, band_patch
    return d, cube, pts


def neighborhood_tokens(cube: torch.Tensor, points: torch.Tensor, patch: int, band_patch: int, out_dtype: Optional[torch.dtype] = None,
                        pad_to: int = 1) -> torch.Tensor:
    """The reference's gathered tensor ``[B, bands, patch^2 band_patch]`` for the pixels ``points [B, 2]`` (row, col) of ``cube
    [H, W, bands]``: mirror_hsi + gain_neighborhood_pixel + gain_neighborhood_band + the transpose of train.py, as one integer-indexed
    copy on the device (bit-exact in the cube's dtype).  ``pad_to`` rounds the row length up with zero columns (a view of the first K
    is returned when it is 1)."""
    lib = _capi.load()
    d, cube, pts = _prepare("neighborhood_tokens", cube, points, patch, band_patch)
    K = patch * patch * band_patch
    odt = out_dtype or cube.dtype
    ld = (K + pad_to - 1) // pad_to * pad_to
    B, bands = pts.shape[0], cube.shape[2]
    out = (torch.zeros if ld != K else torch.empty)((B, bands, ld), dtype=odt, device=cube.device)
    check(lib.me_hsi_gather(ctypes.byref(d), ptr(out), dtype_code(odt), ld, stream_ptr()), "me_hsi_gather")
    return out


def hsi_embed_wgrad(cube, points, patch, band_patch, dy, want=("dw", "dbias", "dcls", "dpos"), into=None, beta: float = 0.0):
    """me_hsi_embed_wgrad: ``dy [B, bands + 1, C]`` (fp32 or bf16) -> dict of the fp32 gradients named in ``want`` (``dw [C, K]``, ``dbias
    [C]``, ``dcls [C]``, ``dpos [bands + 1, C]``).  ``into``: name -> fp32 tensor to write (with ``beta`` != 0: to accumulate) into."""
    lib = _capi.load()
    d, cube, pts = _prepare("hsi_embed_wgrad", cube, points, patch, band_patch)
    B, bands = pts.shape[0], cube.shape[2]
    K = patch * patch * band_patch
    if dy.dim() != 3 or dy.shape[0] != B or dy.shape[1] != bands + 1 or dy.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"hsi_embed_wgrad: dy {tuple(dy.shape)} {dy.dtype} must be [{B}, {bands + 1}, C] fp32 or bf16")
    C = dy.shape[2]
    dy = dy.contiguous()
    shapes = {"dw": (C, K), "dbias": (C,), "dcls": (C,), "dpos": (bands + 1, C)}
    res = {}
    for n in want:
        t = (into or {}).get(n)
        if t is None:
            if beta != 0.0:
                raise MetaEncError(f"hsi_embed_wgrad: beta={beta} needs `into['{n}']` to accumulate into")
            t = torch.empty(shapes[n], dtype=torch.float32, device=dy.device)
        elif t.dtype != torch.float32 or tuple(t.shape) != shapes[n] or t.stride(-1) != 1 or t.device != dy.device:
            raise MetaEncError(f"hsi_embed_wgrad: into['{n}'] must be an fp32 tensor {shapes[n]} with unit inner stride on {dy.device}")
        res[n] = t
    nbytes = lib.me_hsi_embed_wgrad_workspace(ctypes.byref(d), C)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dy.device)
    dw, dpos = res.get("dw"), res.get("dpos")
    check(lib.me_hsi_embed_wgrad(ctypes.byref(d), ptr(dy), dtype_code(dy.dtype), C, C, ptr(dw), dw.stride(0) if dw is not None else K,
                                 ptr(res.get("dbias")), ptr(res.get("dcls")), ptr(dpos), dpos.stride(0) if dpos is not None else C,
                                 float(beta), ptr(ws), nbytes, stream_ptr()), "me_hsi_embed_wgrad")
    return res


class _HsiEmbedFn(torch.autograd.Function):
    """me_hsi_embed_fwd / me_hsi_embed_wgrad: the cube is data (no gradient); weight, bias, cls and pos get theirs"""

    @staticmethod
    def forward(ctx, cube, points, weight, bias, cls, pos, wc, patch, band_patch, odt, gemm_forward=False):
        lib = _capi.load()
        d, cube, pts = _prepare("HyperSpectralEmbed", cube, points, patch, band_patch)
        B, bands = pts.shape[0], cube.shape[2]
        C, K = weight.shape
        wc = wc.contiguous()
        b32 = ops._f32(bias.detach()).contiguous()
        c32 = ops._f32(cls.detach()).reshape(C).contiguous()
        p32 = ops._f32(pos.detach()).reshape(-1, C)[:bands + 1].contiguous()
        kdt = torch.bfloat16 if odt == torch.float16 else odt
        out = torch.empty((B, bands + 1, C), dtype=kdt, device=cube.device)
        if gemm_forward:
            # token rows by me_gemm on the gathered, K-padded tensor: bias, pos[j + 1] (residual, row j of every pixel) and the
            # one-row offset behind the cls token are its epilogue; row 0 of every pixel is parameter-sized glue
            x = neighborhood_tokens(cube, pts, patch, band_patch, out_dtype=wc.dtype, pad_to=8)
            wp = _pad_to(wc, 1)
            ops.gemm(x.reshape(B * bands, wp.shape[1]), wp, out=out.view(B * (bands + 1), C), bias=b32, residual=p32[1:], res_row_mod=bands,
                     out_group=(bands, bands + 1, 1))
            out[:, 0] = (c32 + p32[0]).to(kdt)
        else:
            check(lib.me_hsi_embed_fwd(ctypes.byref(d), ptr(wc), dtype_code(wc.dtype), K, ptr(b32), ptr(c32), ptr(p32), C, ptr(out),
                                       dtype_code(kdt), C, C, stream_ptr()), "me_hsi_embed_fwd")
        ctx.save_for_backward(cube, pts)
        ctx.meta = (patch, band_patch, weight.dtype, bias.dtype, cls.dtype, tuple(cls.shape), pos.dtype, tuple(pos.shape))
        return out if kdt == odt else ops.cast(out, odt)

    @staticmethod
    def backward(ctx, dy):
        cube, pts = ctx.saved_tensors
        patch, band_patch, wdt, bdt, cdt, cshape, pdt, pshape = ctx.meta
        ng = ctx.needs_input_grad
        names = [n for n, need in zip(("dw", "dbias", "dcls", "dpos"), ng[2:6]) if need]
        if not names:
            return (None,) * 11
        if dy.dtype == torch.float16:
            dy = ops.cast(dy.contiguous(), torch.bfloat16)
        g = hsi_embed_wgrad(cube, pts, patch, band_patch, dy, want=names)
        dpos = g.get("dpos")
        if dpos is not None:
            rows = dpos.shape[0]
            full = dpos.new_zeros(pshape)                      # the reference slices pos_embedding[:, :n + 1]: rows beyond get zero
            full.view(-1, pshape[-1])[:rows] = dpos
            dpos = full.to(pdt)
        cast = lambda t, dt: None if t is None else t.to(dt)      # noqa: E731
        dcls = g.get("dcls")
        return (None, None, cast(g.get("dw"), wdt), cast(g.get("dbias"), bdt), None if dcls is None else dcls.reshape(cshape).to(cdt), dpos,
                None, None, None, None, None)


class _HsiTokenizer(nn.Module):
    """the parameters and the token path shared by HyperSpectralEmbed and HyperSpectralClassifier (registration order = the reference's)"""

    def _init_tokenizer(self, bands: int, patch: int, near_band: int, dim: int, emb_dropout: float) -> None:
        K = _check_geometry(type(self).__name__, None, None, bands, patch, near_band)
        if dim <= 0 or dim % 8 != 0:
            raise MetaEncError(f"{type(self).__name__}: embed dim {dim} must be a positive multiple of 8")
        self.bands, self.patch, self.near_band, self.embed_dim = bands, patch, near_band, dim
        self.pos_embedding = nn.Parameter(torch.randn(1, bands + 1, dim))
        self.patch_to_embedding = nn.Linear(K, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.route = DEFAULT_ROUTE
        self._wcache = _WeightCache()

    def _tokens(self, x: torch.Tensor, points: Optional[torch.Tensor] = None) -> torch.Tensor:
        who = type(self).__name__
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise MetaEncError(f"{who} runs on MI355X only (CPU tensor given; no CPU fallback)")
        w = self.patch_to_embedding.weight
        if w.device != x.device:
            raise MetaEncError(f"{who}: parameters are on {w.device}, the input on {x.device}")
        cdt, odt = _boundary_dtypes(w)
        C, K = w.shape
        if self.route not in ROUTES:
            raise MetaEncError(f"{who}: route {self.route!r} (one of {ROUTES})")
        if points is not None and self.route != "gathered":
            if x.dim() == 3 and x.shape[2] != self.bands:
                raise MetaEncError(f"{who}: the cube has {x.shape[2]} bands, the tokenizer was built for {self.bands}")
            wc = self._wcache.fwd("patch_to_embedding", w, cdt)
            y = _HsiEmbedFn.apply(x, points, w, self.patch_to_embedding.bias, self.cls_token, self.pos_embedding, wc, self.patch,
                                  self.near_band, odt, self.route == "auto" and cdt == torch.float32)
            n = self.bands
        else:
            if points is not None:
                if x.dim() == 3 and x.shape[2] != self.bands:
                    raise MetaEncError(f"{who}: the cube has {x.shape[2]} bands, the tokenizer was built for {self.bands}")
                x = neighborhood_tokens(x, points, self.patch, self.near_band, out_dtype=cdt, pad_to=8)
            elif x.dim() != 3 or x.shape[2] != K or x.shape[1] > self.bands or x.shape[1] < 1:
                raise MetaEncError(f"{who}: gathered input {tuple(x.shape)} must be [B, n <= {self.bands}, {K}] "
                                   "(or call forward(cube, points))")
            if x.requires_grad:
                raise MetaEncError(f"{who}: gradient w.r.t. the gathered tokens is not implemented (they are data); detach the input")
            B, n = x.shape[:2]
            # (x and W zero-padded to 8 columns inside; the gathered tokens are data: no dgrad)
            y = linear(x.reshape(B * n, x.shape[2]), w, self.patch_to_embedding.bias, compute_dtype=cdt).reshape(B, n, C)
            # cls row and position rows: parameter-sized glue with autograd's own backward (x += pos_embedding[:, :n + 1])
            y = torch.cat([self.cls_token.float().expand(B, 1, C), y], dim=1) + self.pos_embedding[:, :n + 1].float()
            y = y.to(odt)
        p = float(self.dropout.p) if self.training else 0.0
        if p > 0:
            seed = int(torch.empty((), dtype=torch.int64).random_().item())
            y = _DropoutFn.apply(y, n + 1, p, seed)
        return y


class HyperSpectralEmbed(_HsiTokenizer):
    """The tokenizer of Hyper-spectrum/metatransformer.py:146-159 with its input pipeline (train.py:80-125) folded in.

    ``forward(cube [H, W, bands], points [B, 2])`` -> ``[B, bands + 1, C]``: row 0 is ``cls_token + pos_embedding[0]``, row j + 1 the
    projected band-neighbourhood token of band j plus ``pos_embedding[j + 1]``; then Dropout(emb_dropout) in training mode.
    ``forward(x [B, n <= bands, K])`` takes the reference's already gathered tensor instead (``neighborhood_tokens`` makes it).
    fp32 parameters -> exact fp32 arithmetic; bf16 parameters or autocast -> bf16 MFMA with fp32 accumulation."""

    def __init__(self, bands: int, patch: int = 1, near_band: int = 1, embed_dim: int = 768, emb_dropout: float = 0.):
        super().__init__()
        self._init_tokenizer(bands, patch, near_band, embed_dim, emb_dropout)

    def forward(self, x: torch.Tensor, points: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._tokens(x, points)


class HyperSpectralClassifier(_HsiTokenizer):
    """Hyper-spectrum/metatransformer.py:111-165 (``MetaTransformer``): the reference's constructor and state-dict keys
    (``pos_embedding``, ``patch_to_embedding.*``, ``cls_token``, ``transformer.{i}.*``, ``mlp_head.0.*``, ``mlp_head.1.*``).
    ``image_size`` is the spatial patch, ``num_patches`` the band count.  The reference replaces its own Transformer by the frozen
    12-block encoder loaded from a checkpoint file; here ``encoder=`` takes that stack (an nn.Sequential of Blocks, used as it is),
    and ``encoder=None`` builds ``depth`` Blocks of width ``dim`` with ``heads`` heads and an ``mlp_dim`` hidden layer -- no file is
    read.  ``forward(cube, points)`` or ``forward(x)`` -> logits ``[B, num_classes]`` from the cls token.  ``mode='CAF'`` raises: the
    reference discards the Transformer that would have used it (metatransformer.py:143)."""

    def __init__(self, image_size, near_band, num_patches, num_classes, dim, depth, heads, mlp_dim, pool="cls", channels=1, dim_head=16,
                 dropout=0., emb_dropout=0., mode="ViT", encoder: Optional[nn.Module] = None):
        super().__init__()
        if mode != "ViT":
            raise MetaEncError(f"HyperSpectralClassifier: mode {mode!r} is not supported (the reference's forward never runs its CAF "
                               "Transformer: metatransformer.py:143 replaces it)")
        if pool not in ("cls", "mean"):
            raise MetaEncError(f"HyperSpectralClassifier: pool {pool!r} (cls / mean; the reference's forward reads the cls token either way)")
        self._init_tokenizer(num_patches, image_size, near_band, dim, emb_dropout)
        if encoder is None:
            from .encoder import build_encoder
            if depth < 1 or mlp_dim < 1:
                raise MetaEncError(f"HyperSpectralClassifier: depth={depth}, mlp_dim={mlp_dim}")
            encoder = build_encoder(depth, dim, heads, mlp_ratio=(mlp_dim + 0.5) / dim)      # Block takes int(dim * mlp_ratio) = mlp_dim
        self.transformer = encoder
        self.pool = pool
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, num_classes))

    def forward(self, x: torch.Tensor, points: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .heads import _LayerNormFn, pool_tokens
        t = self.transformer(self._tokens(x, points))
        ln, fc = self.mlp_head[0], self.mlp_head[1]
        f = _LayerNormFn.apply(pool_tokens(t, "cls"), ln.weight, ln.bias, ln.eps)
        return linear(f, fc.weight, fc.bias)
