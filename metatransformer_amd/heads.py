"""Task heads behind the encoder and encoder checkpoint I/O.

Heads restated from the reference pipelines, with the reference parameter names so their checkpoints load strict=True:
  * ``ClassifierHead``  -- Video/models/modeling_finetune.py:445-454 + :395: ``fc_norm(x.mean(1))`` (use_mean_pooling) or
    ``norm(x)[:, 0]``, dropout, ``head`` Linear;
  * ``ClsHead``         -- PointCloud/openpoints/models/classification/cls_base.py:77-136: optional 'max' / 'avg' global
    features over the token axis, then Linear(+BatchNorm1d+ReLU)(+Dropout) blocks and a final Linear.
Token pooling, LayerNorm and every Linear (forward, dgrad, wgrad, bias gradient) run in libmetaenc.so; BatchNorm1d / ReLU /
Dropout on the [B, 256] head activations are PyTorch glue, as the north star prescribes for the heads.

Checkpoint I/O: ``load_encoder_checkpoint`` / ``save_encoder_checkpoint`` move between the reference's wire format (a bare
OrderedDict of ``{i}.norm1.weight ...`` fp32 tensors, README.md:125-135, optionally prefixed ``blocks.`` / ``module.`` /
``encoder.``, or the Video key set) and the device-resident packed layout (``pack_encoder``: one flat fp32 master buffer
whose slices ARE the parameters, its bf16 mirror for the forward GEMMs and the pre-transposed bf16 copies for dgrad).
"""
from __future__ import annotations

import math
import re
from collections import OrderedDict
from typing import Optional

import torch
import torch.nn as nn

from . import _capi, ops
from ._capi import MetaEncError, check, dtype_code, ptr, stream_ptr
from .encoder import Block, convert_video_state_dict
from .linear import linear      # noqa: F401  (heads.linear: the name its call sites and the documents use)

_POOL = {"mean": _capi.ME_POOL_MEAN, "avg": _capi.ME_POOL_MEAN, "max": _capi.ME_POOL_MAX, "cls": _capi.ME_POOL_FIRST,
         "first": _capi.ME_POOL_FIRST}


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        if x.dim() != 3 or not x.is_cuda:
            raise MetaEncError("pool_tokens: [B, N, C] CUDA tokens required (no CPU fallback)")
        x = x.contiguous()
        B, N, C = x.shape
        if x.dtype == torch.float16:
            x = ops.cast(x, torch.bfloat16)
        out = torch.empty(B, C, dtype=torch.float32, device=x.device)
        need = x.requires_grad and mode == _capi.ME_POOL_MAX
        arg = torch.empty(B, C, dtype=torch.int32, device=x.device) if (need or mode == _capi.ME_POOL_MAX) else None
        check(_capi.load().me_pool_tokens(ptr(x), dtype_code(x.dtype), ptr(out), ptr(arg), B, N, C, mode, stream_ptr()),
              "me_pool_tokens")
        ctx.mode, ctx.shape, ctx.dtype = mode, (B, N, C), x.dtype
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        B, N, C = ctx.shape
        dx = torch.empty(B, N, C, dtype=ctx.dtype, device=dy.device)
        dyc = dy.float().contiguous()
        check(_capi.load().me_pool_tokens_bwd(ptr(dyc), ptr(arg), ptr(dx), dtype_code(dx.dtype), B, N, C, ctx.mode, stream_ptr()),
              "me_pool_tokens_bwd")
        return dx, None


def pool_tokens(x: torch.Tensor, mode: str = "mean") -> torch.Tensor:
    """[B, N, C] -> [B, C] fp32: 'mean' (x.mean(1)), 'max' (x.max(1)[0]) or 'cls' (x[:, 0])."""
    if mode not in _POOL:
        raise MetaEncError(f"pool_tokens: mode {mode!r} (mean / max / cls)")
    return _PoolFn.apply(x, _POOL[mode])


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        x = x.contiguous()
        y, mean, rstd = ops.layernorm_fwd(x, w, b, eps, torch.float32, save_stats=True)
        ctx.save_for_backward(x, mean, rstd, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w = ctx.saved_tensors
        dx, dg, db = ops.layernorm_bwd(dy.float().contiguous(), x, mean, rstd, w, None, x.dtype, True)
        return dx, dg.to(w.dtype), db.to(w.dtype), None


class ClassifierHead(nn.Module):
    """The Video / Image classification tail (Video/models/modeling_finetune.py:395, 445-454): parameters ``fc_norm.*``
    (use_mean_pooling=True) or ``norm.*``, and ``head.*``."""

    def __init__(self, embed_dim=768, num_classes=400, use_mean_pooling=True, norm_layer=None, head_drop_rate=0.0, init_scale=0.0):
        super().__init__()
        from functools import partial
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        self.use_mean_pooling = use_mean_pooling
        if use_mean_pooling:
            self.fc_norm = norm_layer(embed_dim)
        else:
            self.norm = norm_layer(embed_dim)
        self.head_dropout = nn.Dropout(head_drop_rate)
        self.head = nn.Linear(embed_dim, num_classes)
        if init_scale:
            self.head.weight.data.mul_(init_scale)
            self.head.bias.data.mul_(init_scale)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        ln = self.fc_norm if self.use_mean_pooling else self.norm
        # LayerNorm is per token, so norm(x)[:, 0] == norm(x[:, 0]): pool first, normalise B rows instead of B*N
        f = pool_tokens(x, "mean" if self.use_mean_pooling else "cls")
        f = _LayerNormFn.apply(f, ln.weight, ln.bias, ln.eps)
        return linear(self.head_dropout(f), self.head.weight, self.head.bias)


class ClsHead(nn.Module):
    """openpoints ClsHead (cls_base.py:77-136).  ``global_feat`` e.g. 'max,avg' pools the token axis and concatenates;
    blocks follow create_linearblock: nn.Sequential(Linear, [BatchNorm1d], [ReLU]) -> keys ``head.{i}.0.weight`` ..."""

    def __init__(self, num_classes: int, in_channels: int, mlps=(256,), norm_args=None, act_args=None, dropout: float = 0.5,
                 global_feat: Optional[str] = None, point_dim: int = 2):
        super().__init__()
        self.global_feat = global_feat.split(",") if global_feat is not None else None
        self.point_dim = point_dim
        act_args = {"act": "relu"} if act_args is None else act_args
        cin = len(self.global_feat) * in_channels if self.global_feat is not None else in_channels
        dims = [cin] + list(mlps or []) + [num_classes]
        heads = []
        for i in range(len(dims) - 2):
            blk = [nn.Linear(dims[i], dims[i + 1], bias=not (norm_args and "bn" in norm_args.get("norm", "")))]
            if norm_args and "bn" in norm_args.get("norm", ""):
                blk.append(nn.BatchNorm1d(dims[i + 1]))
            elif norm_args and "ln" in norm_args.get("norm", ""):
                blk.append(nn.LayerNorm(dims[i + 1]))
            if act_args:
                blk.append(nn.ReLU(inplace=True))
            heads.append(nn.Sequential(*blk))
            if dropout:
                heads.append(nn.Dropout(dropout))
        heads.append(nn.Sequential(nn.Linear(dims[-2], dims[-1])))
        self.head = nn.Sequential(*heads)

    def forward(self, end_points: torch.Tensor) -> torch.Tensor:
        f = end_points
        if self.global_feat is not None:
            if f.dim() != 3:
                raise MetaEncError("ClsHead(global_feat=...) expects 3-D features")
            if self.point_dim == 2:                 # the reference's channel-first [B, C, N] convention
                f = f.transpose(1, 2)
            f = torch.cat([pool_tokens(f.contiguous(), "max" if "max" in g else "mean") for g in self.global_feat], dim=1)
        for m in self.head:
            if isinstance(m, nn.Sequential):
                lin = m[0]
                f = linear(f, lin.weight, lin.bias)
                for sub in list(m)[1:]:
                    f = sub(f)
            else:
                f = m(f)
        return f


# ----------------------------------------------------------------------------------------------------- checkpoint I/O

_BLOCK_KEY = re.compile(r"(?:^|\.)(\d+\.(?:norm1|norm2|attn|mlp|gamma_?[12])\b.*)$")


def _strip(sd):
    """keep the encoder blocks' entries and drop whatever wraps them (module. / backbone. / encoder. / blocks. ...):
    'module.blocks.3.attn.qkv.weight' -> '3.attn.qkv.weight'; patch_embed / head / pos_embed entries are not the encoder's"""
    out = OrderedDict()
    for k, v in sd.items():
        m = _BLOCK_KEY.search(k)
        if m:
            out[m.group(1)] = v
    return out


def load_encoder_checkpoint(encoder: nn.Sequential, source, strict: bool = True, map_location="cpu") -> nn.Sequential:
    """``source``: a path to the reference's .pth (torch.load -> bare state dict or {'model' / 'state_dict': ...}) or a state
    dict.  Accepts the wire format of README.md:125-135, wrapper prefixes, the Video key set (q_bias / v_bias / gamma_1 /
    gamma_2) and fp16 / bf16 tensors; non-encoder keys (patch_embed, head, ...) are ignored unless strict demands every
    encoder key is present.  Loads with the reference's own ``load_state_dict(strict=True)`` call."""
    sd = torch.load(source, map_location=map_location, weights_only=True) if isinstance(source, (str, bytes)) or hasattr(source, "read") else source
    for k in ("model", "state_dict", "module"):
        if isinstance(sd, dict) and k in sd and isinstance(sd[k], dict):
            sd = sd[k]
    sd = convert_video_state_dict(_strip(OrderedDict(sd)))
    want = encoder.state_dict()
    sd = OrderedDict((k, v.to(want[k].dtype) if k in want else v) for k, v in sd.items())
    encoder.load_state_dict(sd, strict=strict)
    return encoder


def save_encoder_checkpoint(encoder: nn.Sequential, path, dtype: torch.dtype = torch.float32) -> None:
    """Writes the reference wire format: a bare OrderedDict of CPU tensors under the timm key names."""
    sd = OrderedDict((k, v.detach().to("cpu", dtype)) for k, v in encoder.state_dict().items())
    torch.save(sd, path)


def pack_encoder(encoder: nn.Sequential, device=None, warm: bool = True):
    """Device-resident packed layout of an encoder's weights: returns a parallel.FlatParams whose flat fp32 buffer holds
    every parameter (each nn.Parameter becomes a view of it, no-decay parameters first) and, with ``warm``, builds the
    compute-dtype copies the kernels read (bf16 forward copies and transposed dgrad copies, one batched launch)."""
    from . import parallel
    if device is not None:
        encoder.to(device)
    if not all(isinstance(b, Block) for b in encoder):
        raise MetaEncError("pack_encoder: an nn.Sequential of Blocks is required")
    for p in encoder.parameters():
        p.requires_grad_(True)
    flat = parallel.FlatParams(encoder.named_parameters(), no_decay=parallel.no_decay_rule)
    if warm:
        for b in encoder:
            b._wcache.bind(b)
            # the dtype the Block will compute in (compute_dtype may be the STRING "fp32_3xbf16", which is not a torch dtype)
            cdt = torch.float32 if b.compute_dtype == "fp32_3xbf16" else (b.compute_dtype or torch.bfloat16)
            # (which copies a compute mode reads is the cache's knowledge: the same call builds them for the kernels, _BlockFn._desc)
            b._wcache.operands(b._wcache.weights(), cdt, b.uses_3xbf16(cdt, torch.float32), True)
    return flat


# ----------------------------------------------------------------------------------------------------- point-cloud tokenizer

def furthest_point_sample(p: torch.Tensor, m: int) -> torch.Tensor:
    """[B, n, 3] fp32 -> [B, m] int32 indices (me_fps; idx[:, 0] = 0 as in the reference kernel)."""
    if p.dim() != 3 or p.shape[2] != 3 or not p.is_cuda:
        raise MetaEncError("furthest_point_sample: [B, n, 3] CUDA points required (no CPU fallback)")
    p = p.float().contiguous()
    B, n, _ = p.shape
    idx = torch.empty(B, m, dtype=torch.int32, device=p.device)
    tmp = torch.empty(B, n, dtype=torch.float32, device=p.device)
    check(_capi.load().me_fps(ptr(p), ptr(idx), ptr(tmp), B, n, m, stream_ptr()), "me_fps")
    return idx


def knn_indices(support: torch.Tensor, query: torch.Tensor, k: int) -> torch.Tensor:
    """[B, n, 3], [B, m, 3] -> [B, m, k] int32: the k nearest support points of each query, nearest first (me_knn)."""
    support, query = support.float().contiguous(), query.float().contiguous()
    B, n, _ = support.shape
    m = query.shape[1]
    idx = torch.empty(B, m, k, dtype=torch.int32, device=support.device)
    check(_capi.load().me_knn(ptr(support), ptr(query), ptr(idx), B, n, m, k, stream_ptr()), "me_knn")
    return idx


class PointPatchEmbed(nn.Module):
    """openpoints PointPatchEmbed (group_embed.py:60-172) for the configuration the Meta-Transformer point-cloud pipelines
    use (cfgs/modelnet40ply2048/metatransformer.yaml:19-33): FPS subsampling, KNN grouping, feature_type 'dp' (relative
    xyz), conv-norm-act blocks with BatchNorm2d + ReLU, max reduction.  Parameter names follow the reference's
    ``conv1.{i}.0.weight`` ([out, in, 1, 1] Conv2d) / ``conv1.{i}.1.*`` (BatchNorm2d) layout, so its checkpoints load.

    forward(p) returns the reference's ``[p, center_p], [x, out_f]`` with out_f channel-first [B, C, S]; ``tokens(p)`` gives
    the [B, S, C] token layout the encoder consumes.  FPS / KNN / grouping, every 1x1 convolution (a GEMM over B*S*k rows)
    and the max reductions run in libmetaenc.so; BatchNorm / ReLU are PyTorch glue."""

    def __init__(self, sample_ratio=0.25, group_size=32, in_channels=3, layers=4, embed_dim=768, channels=(128, 256, 512),
                 subsample="fps", group="knn", feature_type="dp", norm_args=None, reduction="max"):
        super().__init__()
        if subsample != "fps" or "knn" not in group or feature_type != "dp" or reduction != "max":
            raise MetaEncError("PointPatchEmbed: fps + knn + feature_type 'dp' + max reduction is the implemented configuration")
        self.sample_ratio, self.group_size = sample_ratio, group_size
        ch = [3] + list(channels) + [embed_dim]
        layers = len(ch) - 1
        half = layers // 2

        def block(cin, cout, last):
            mods = [nn.Conv2d(cin, cout, 1, bias=last)]
            if not last:
                mods += [nn.BatchNorm2d(cout), nn.ReLU(inplace=True)]
            return nn.Sequential(*mods)
        self.conv1 = nn.Sequential(*[block(ch[i], ch[i + 1], i == half - 1) for i in range(half)])
        ch2 = list(ch)
        ch2[half] *= 2
        self.conv2 = nn.Sequential(*[block(ch2[i], ch2[i + 1], i == layers - 1) for i in range(half, layers)])
        self.out_channels = ch[-1]

    def _mlp(self, seq: nn.Sequential, f: torch.Tensor) -> torch.Tensor:
        for blk in seq:
            conv = blk[0]
            f = linear(f, _w2d(conv), conv.bias)                  # (the xyz layer: 3 weight columns on rows padded to 8)
            if len(blk) > 1:
                bn = blk[1]
                f = torch.nn.functional.batch_norm(f, bn.running_mean, bn.running_var, bn.weight, bn.bias, bn.training, bn.momentum, bn.eps)
                f = torch.relu_(f)
        return f

    def tokens(self, p: torch.Tensor):
        B, n, _ = p.shape
        S, k = int(n * self.sample_ratio), self.group_size
        p = p.float().contiguous()
        idx = furthest_point_sample(p, S)
        center = torch.gather(p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        nbr = knn_indices(p, center, k)
        rows = torch.empty(B * S * k, 8, dtype=torch.float32, device=p.device)
        check(_capi.load().me_group_relative(ptr(p), ptr(center), ptr(nbr), ptr(rows), B, n, S, k, 8, stream_ptr()), "me_group_relative")
        f = self._mlp(self.conv1, rows)                                               # [B*S*k, C1]
        C1 = f.shape[1]
        pooled = pool_tokens(f.reshape(B * S, k, C1), "max")                          # [B*S, C1]
        f = torch.cat([pooled.unsqueeze(1).expand(-1, k, -1), f.reshape(B * S, k, C1)], dim=2).reshape(B * S * k, 2 * C1)
        f = self._mlp(self.conv2, f.contiguous())
        out = pool_tokens(f.reshape(B * S, k, f.shape[1]), "max").reshape(B, S, -1)
        return out, center, idx, nbr

    def forward(self, p: torch.Tensor, x: Optional[torch.Tensor] = None):
        out, center, _, _ = self.tokens(p)
        return [p, center], [x, out.transpose(1, 2)]


# ----------------------------------------------------------------------------------------------------- P3Embed

_GROUP_MODE = {"dp_fj": _capi.ME_GROUP_DP_FJ, "dp_df": _capi.ME_GROUP_DP_DF, "dp_fj_df": _capi.ME_GROUP_DP_FJ_DF}


def _group_width(mode: int, C: int) -> int:
    return 3 + {_capi.ME_GROUP_DP: 0, _capi.ME_GROUP_DP_FJ: C, _capi.ME_GROUP_DP_DF: C, _capi.ME_GROUP_DP_FJ_DF: 2 * C}[mode]


class _GroupFeaturesFn(torch.autograd.Function):
    """rows [B*m*k, cols] fp32 = me_group_features(p, f, ctr, nbr); backward: df by me_group_features_bwd (the points carry
    no gradient)"""

    @staticmethod
    def forward(ctx, p, f, ctr, nbr, mode, cols):
        B, n, _ = p.shape
        m, k = nbr.shape[1], nbr.shape[2]
        C = f.shape[2] if f is not None else 0
        rows = torch.empty(B * m * k, cols, dtype=torch.float32, device=p.device)
        check(_capi.load().me_group_features(ptr(p), ptr(f), dtype_code(f.dtype) if f is not None else _capi.ME_F32, ptr(ctr),
                                             ptr(nbr), ptr(rows), B, n, m, k, C, cols, mode, stream_ptr()), "me_group_features")
        ctx.save_for_backward(ctr, nbr)
        ctx.meta = (B, n, m, k, C, cols, mode, f.dtype if f is not None else None)
        return rows

    @staticmethod
    def backward(ctx, drows):
        ctr, nbr = ctx.saved_tensors
        B, n, m, k, C, cols, mode, fdt = ctx.meta
        if fdt is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        lib = _capi.load()
        df = torch.empty(B, n, C, dtype=fdt, device=drows.device)
        ws = torch.empty(max(1, int(lib.me_group_features_bwd_workspace(B, n, m, k, C))), dtype=torch.uint8, device=drows.device)
        d = drows.float().contiguous()
        check(lib.me_group_features_bwd(ptr(d), ptr(ctr), ptr(nbr), ptr(df), dtype_code(fdt), B, n, m, k, C, cols, mode, ptr(ws),
                                        ws.numel(), stream_ptr()), "me_group_features_bwd")
        return None, df, None, None, None, None


def group_features(p: torch.Tensor, f: Optional[torch.Tensor], ctr: torch.Tensor, nbr: torch.Tensor, feature_type: str = "dp_df",
                   cols: Optional[int] = None) -> torch.Tensor:
    """The grouped GEMM operand rows of P3Embed: points [B, n, 3], token-major features [B, n, C] (fp32 / bf16), centre
    indices [B, m] and neighbour indices [B, m, k] (int32) -> rows [B*m*k, cols] fp32, row (b, s, j) =
    [p[nbr] - p[ctr] | feature part | 0 ...] with the feature part of ``feature_type`` ('dp': none, 'dp_fj': f[nbr], 'dp_df':
    f[nbr] - f[ctr], 'dp_fj_df': both); cols defaults to the width rounded up to a multiple of 8.  Differentiable in f."""
    mode = _capi.ME_GROUP_DP if feature_type == "dp" else _GROUP_MODE.get(feature_type)
    if mode is None:
        raise MetaEncError(f"group_features: feature_type {feature_type!r} (dp / dp_fj / dp_df / dp_fj_df)")
    if p.dim() != 3 or p.shape[2] != 3 or not p.is_cuda or nbr.dim() != 3 or ctr.shape != nbr.shape[:2]:
        raise MetaEncError("group_features: CUDA points [B, n, 3], ctr [B, m], nbr [B, m, k] required (no CPU fallback)")
    if mode == _capi.ME_GROUP_DP:
        f = None
    elif f is None or f.dim() != 3 or f.shape[:2] != p.shape[:2]:
        raise MetaEncError(f"group_features: feature_type {feature_type!r} needs token-major features [B, n, C]")
    else:
        f = f.contiguous() if f.dtype in (torch.float32, torch.bfloat16) else f.float().contiguous()
    width = _group_width(mode, f.shape[2] if f is not None else 0)
    cols = cols if cols is not None else (width + 7) // 8 * 8
    if cols % 8 or cols < width:
        raise MetaEncError(f"group_features: cols {cols} (a multiple of 8 >= {width})")
    return _GroupFeaturesFn.apply(p.float().contiguous(), f, ctr.to(torch.int32).contiguous(), nbr.to(torch.int32).contiguous(),
                                  mode, cols)


class LayerNorm2d(nn.LayerNorm):
    """openpoints LayerNorm2d (layers/norm.py:12-20): a LayerNorm over the channels; it ignores norm_args (eps 1e-5)."""

    def __init__(self, num_channels, **kwargs):
        super().__init__(num_channels)


def _norm_2d(norm_args, channels):
    """create_norm(norm_args, channels, dimension='2d') (layers/norm.py:74-97) for the norms P3Embed runs: 'bn' / 'bn2d'
    (BatchNorm2d) and 'ln2d'"""
    if norm_args is None:
        return None
    if isinstance(norm_args, dict):
        kw = dict(norm_args)
        norm = kw.pop("norm", None)
    else:
        norm, kw = norm_args, {}
    if norm is None:
        return None
    norm = str(norm).lower()
    if "2d" not in norm:
        norm += "2d"
    if norm == "bn2d":
        return nn.BatchNorm2d(channels, **kw)
    if norm == "ln2d":
        return LayerNorm2d(channels, **kw)
    raise MetaEncError(f"P3Embed: norm_args {norm_args!r} (bn / bn2d / ln2d are implemented)")


def _batch_norm_rows(norm, f: torch.Tensor) -> torch.Tensor:
    """BatchNorm1d / BatchNorm2d over the rows of token-major [rows, C] (== over (B, C, N[, k]) channel-first), tracking the
    running statistics in training mode as the module itself does"""
    momentum = norm.momentum
    if norm.training and norm.track_running_stats:
        norm.num_batches_tracked.add_(1)
        if momentum is None:
            momentum = 1.0 / float(norm.num_batches_tracked)
    use_batch = norm.training or norm.running_mean is None
    return torch.nn.functional.batch_norm(f, norm.running_mean, norm.running_var, norm.weight, norm.bias, use_batch,
                                          momentum if momentum is not None else 0.0, norm.eps)


class P3Embed(nn.Module):
    """openpoints P3Embed, the progressive point patch embed (group_embed.py:176-286) of the ScanObjectNN / ShapeNetPart /
    S3DIS / ScanNet Meta-Transformer recipes: per stage FPS to N // 4 centres of the previous stage's points, KNN grouping,
    the 'dp_df' (or 'dp_fj' / 'dp_fj_df') grouped features, conv1 (1x1 convolutions), max over the group, conv2 on
    [pooled | conv1 output], max over the group.  Parameters ``convs.{stage}.{0|1}.{i}.{0|1}.*`` as create_convblock2d makes
    them (no bias where a norm follows), so the reference's checkpoints load strict=True.

    forward(p [B, N, 3], f [B, C, N]) returns the reference's (out_p, out_f) lists, out_f channel-first [B, C_s, S_s].  Inside,
    features stay token-major [rows, C]: FPS / KNN / grouping, every 1x1 convolution (exact-fp32 GEMM), LayerNorm2d and the
    max reductions run in libmetaenc.so; BatchNorm2d and ReLU are PyTorch glue.  conv2's first layer runs on cat(pool, fj) as
    fj W_b^T + broadcast(pool W_a^T): the concatenation is never built and that GEMM is half as long."""

    def __init__(self, sample_ratio=0.0625, scale=4, group_size=32, in_channels=3, layers=4, embed_dim=256, subsample="fps",
                 group="ballquery", normalize_dp=False, radius=0.1, feature_type="dp_df", relative_xyz=True,
                 norm_args={"norm": "bn1d"}, act_args={"act": "relu"}, conv_args={"order": "conv-norm-act"}, reduction="max",
                 **kwargs):
        super().__init__()
        if subsample.lower() != "fps":
            raise MetaEncError(f"P3Embed: subsample {subsample!r} (fps is implemented; random subsampling is not)")
        if "knn" not in group.lower():
            raise MetaEncError(f"P3Embed: group {group!r} (knn is implemented; ball query is not)")
        if normalize_dp:
            raise MetaEncError("P3Embed: normalize_dp=True is not implemented")
        if not relative_xyz:
            raise MetaEncError("P3Embed: relative_xyz=False is not implemented")
        if feature_type not in _GROUP_MODE:
            raise MetaEncError(f"P3Embed: feature_type {feature_type!r} (dp_df / dp_fj / dp_fj_df are implemented)")
        act = act_args.get("act") if isinstance(act_args, dict) else act_args
        if act is None or str(act).lower() != "relu":
            raise MetaEncError(f"P3Embed: act_args {act_args!r} (relu is implemented)")
        order = (conv_args or {}).get("order", "conv-norm-act")
        if order != "conv-norm-act" or set(conv_args or {}) - {"order"}:
            raise MetaEncError(f"P3Embed: conv_args {conv_args!r} (order conv-norm-act, no other options)")
        if reduction in ("mean", "avg", "meanpool", "avgpool"):
            self.reduction = "mean"
        elif reduction == "max":
            self.reduction = "max"
        else:
            raise MetaEncError(f"P3Embed: reduction {reduction!r} (max / mean)")
        if layers < 2 or layers % 2:
            raise MetaEncError(f"P3Embed: layers={layers} (an even number >= 2)")
        self.sample_ratio, self.group_size, self.feature_type = sample_ratio, group_size, feature_type
        self.mode = _GROUP_MODE[feature_type]
        chmap = {"dp_fj": lambda x: 3 + x, "dp_df": lambda x: x + 3, "dp_fj_df": lambda x: 2 * x + 3}[feature_type]   # CHANNEL_MAP

        def block(cin, cout, with_norm):
            norm = _norm_2d(norm_args, cout) if with_norm else None
            mods = [nn.Conv2d(cin, cout, 1, bias=norm is None)]
            if norm is not None:
                mods.append(norm)
            if with_norm:
                mods.append(nn.ReLU(inplace=True))
            return nn.Sequential(*mods)

        stages = int(math.log(1 / sample_ratio, scale))
        embed_dim = int(embed_dim // 2 ** (stages - 1))
        self.convs = nn.ModuleList()
        self.channel_list = [in_channels]
        half = layers // 2
        for _ in range(stages):
            channels = [chmap(in_channels)] + [embed_dim] * half + [embed_dim * 2] * (half - 1) + [embed_dim]
            conv1 = nn.Sequential(*[block(channels[i], channels[i + 1], i != half - 1) for i in range(half)])
            channels[half] *= 2
            conv2 = nn.Sequential(*[block(channels[i], channels[i + 1], True) for i in range(half, layers)])
            self.convs.append(nn.ModuleList([conv1, conv2]))
            self.channel_list.append(embed_dim)
            in_channels = embed_dim
            embed_dim *= 2
        self.out_channels = channels[-1]

    @staticmethod
    def _norm_act(blk: nn.Sequential, f: torch.Tensor) -> torch.Tensor:
        if len(blk) == 1:
            return f
        norm = blk[1]
        if isinstance(norm, LayerNorm2d):
            f = _LayerNormFn.apply(f, norm.weight, norm.bias, norm.eps)
        else:                                       # BatchNorm2d over (B, C, S, k) == batch_norm over the rows of [rows, C]
            f = _batch_norm_rows(norm, f)
        return torch.relu(f)

    def _stage(self, convs, cur_p: torch.Tensor, cur_f: torch.Tensor, S: int):
        B = cur_p.shape[0]
        k = self.group_size
        idx = furthest_point_sample(cur_p, S)
        center_p = torch.gather(cur_p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        nbr = knn_indices(cur_p, center_p, k)
        f = group_features(cur_p, cur_f, idx, nbr, self.feature_type)                 # [B*S*k, cols]
        conv1, conv2 = convs
        for blk in conv1:
            f = self._norm_act(blk, linear(f, _w2d(blk[0]), blk[0].bias))
        C1 = f.shape[1]
        pooled = pool_tokens(f.reshape(B * S, k, C1), self.reduction)                 # [B*S, C1]
        first = conv2[0]
        w = first[0].weight.reshape(first[0].out_channels, 2 * C1)
        # cat([pool.expand(k), fj]) @ W^T == fj @ W_b^T + broadcast(pool @ W_a^T)
        g = linear(f, w[:, C1:].contiguous(), None).reshape(B * S, k, -1) + linear(pooled, w[:, :C1].contiguous(), first[0].bias).unsqueeze(1)
        f = self._norm_act(first, g.reshape(B * S * k, -1))
        for blk in list(conv2)[1:]:
            f = self._norm_act(blk, linear(f, _w2d(blk[0]), blk[0].bias))
        out = pool_tokens(f.reshape(B * S, k, f.shape[1]), self.reduction).reshape(B, S, -1)
        return center_p, out

    def forward(self, p: torch.Tensor, f: Optional[torch.Tensor] = None):
        if p.dim() != 3 or p.shape[2] != 3 or not p.is_cuda:
            raise MetaEncError("P3Embed: [B, N, 3] CUDA points required (no CPU fallback)")
        if f is None:
            raise MetaEncError("P3Embed: features f [B, C, N] are required (the reference's grouping gathers them)")
        N = p.shape[1]
        out_p, out_f = [p], [f]
        cur_p, cur_f = p.float().contiguous(), f.transpose(1, 2).float().contiguous()        # token-major [B, N, C]
        for convs in self.convs:
            N = N // 4
            cur_p, cur_f = self._stage(convs, cur_p, cur_f, N)
            out_p.append(cur_p)
            out_f.append(cur_f.transpose(1, 2))
        return out_p, out_f


# ----------------------------------------------------------------------------------------------------- point segmentation decoder

def _three_nn(unknown: torch.Tensor, known: torch.Tensor, want_dist: bool):
    if unknown.dim() != 3 or known.dim() != 3 or unknown.shape[2] != 3 or known.shape[2] != 3 or unknown.shape[0] != known.shape[0]:
        raise MetaEncError("three_nn: unknown [B, n, 3] and known [B, m, 3] points required")
    if not (unknown.is_cuda and known.is_cuda):
        raise MetaEncError("three_nn: CUDA points required (no CPU fallback)")
    u, k = unknown.detach().float().contiguous(), known.detach().float().contiguous()
    B, n, _ = u.shape
    m = k.shape[1]
    idx = torch.empty(B, n, 3, dtype=torch.int32, device=u.device)
    w = torch.empty(B, n, 3, dtype=torch.float32, device=u.device)
    dist = torch.empty(B, n, 3, dtype=torch.float32, device=u.device) if want_dist else None
    check(_capi.load().me_three_nn(ptr(u), ptr(k), ptr(idx), ptr(w), ptr(dist), B, n, m, stream_ptr()), "me_three_nn")
    return idx, w, dist


def three_nn(unknown: torch.Tensor, known: torch.Tensor):
    """upsampling.three_nn: [B, n, 3], [B, m, 3] -> (dist [B, n, 3] fp32, idx [B, n, 3] int32), the 3 nearest known points of
    every unknown point in the (squared distance, index) order (me_three_nn).  No gradient, as in the reference."""
    idx, _, dist = _three_nn(unknown, known, True)
    return dist, idx


def three_nn_weights(unknown: torch.Tensor, known: torch.Tensor):
    """(idx [B, n, 3] int32, weight [B, n, 3] fp32): three_nn and three_interpolation's inverse-distance weights in one kernel"""
    idx, w, _ = _three_nn(unknown, known, False)
    return idx, w


class _InterpolateFn(torch.autograd.Function):
    """token-major three_interpolate: out [B*n, C] fp32 = interp(feats [B*m, C]), or base [B*n, C] += interp(feats) in place
    (base is then the output, so the skip GEMM's result absorbs the interpolation without a second [B*n, C] buffer).  The
    gradient goes to feats (me_three_interpolate_bwd) and passes through to base; indices and weights carry none."""

    @staticmethod
    def forward(ctx, feats, idx, weight, base, B, n, m):
        f = feats.float().contiguous()
        C = f.shape[1]
        if base is None:
            out, acc = torch.empty(B * n, C, dtype=torch.float32, device=f.device), 0
        else:
            if base.dtype != torch.float32 or not base.is_contiguous() or base.shape != (B * n, C):
                raise MetaEncError("three_interpolate: the accumulation target must be contiguous fp32 [B*n, C]")
            out, acc = base, 1
            ctx.mark_dirty(base)
        check(_capi.load().me_three_interpolate(ptr(f), C, ptr(idx), ptr(weight), ptr(out), C, 0, B, n, m, C, acc, stream_ptr()),
              "me_three_interpolate")
        ctx.save_for_backward(idx, weight)
        ctx.meta = (B, n, m, C, feats.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        idx, weight = ctx.saved_tensors
        B, n, m, C, fdt = ctx.meta
        df = None
        if ctx.needs_input_grad[0]:
            lib = _capi.load()
            d = dout.float().contiguous()
            df = torch.empty(B * m, C, dtype=torch.float32, device=d.device)
            ws = torch.empty(max(1, int(lib.me_three_interpolate_bwd_workspace(B, n, m))), dtype=torch.uint8, device=d.device)
            check(lib.me_three_interpolate_bwd(ptr(d), C, 0, ptr(idx), ptr(weight), ptr(df), C, B, n, m, C, ptr(ws), ws.numel(),
                                               stream_ptr()), "me_three_interpolate_bwd")
            df = df.to(fdt)
        return df, None, None, dout if ctx.needs_input_grad[3] else None, None, None, None


def _interpolate_rows(feats: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor, base: Optional[torch.Tensor] = None):
    """feats [B, m, C] -> [B*n, C] fp32 (added onto base [B*n, C] when given)"""
    B, m, C = feats.shape
    return _InterpolateFn.apply(feats.reshape(B * m, C), idx, weight, base, B, idx.shape[1], m)


def three_interpolation(unknown_xyz: torch.Tensor, known_xyz: torch.Tensor, know_feat: torch.Tensor) -> torch.Tensor:
    """upsampling.three_interpolation: unknown [B, n, 3], known [B, m, 3], features [B, C, m] -> [B, C, n] fp32 (fp32 under
    autocast too, as the reference's custom_fwd(cast_inputs=float32)).  Differentiable in the features only."""
    if know_feat.dim() != 3 or known_xyz.dim() != 3 or know_feat.shape[2] != known_xyz.shape[1]:
        raise MetaEncError("three_interpolation: features [B, C, m] for known points [B, m, 3] required")
    if not know_feat.is_cuda:
        raise MetaEncError("three_interpolation: CUDA tensors required (no CPU fallback)")
    idx, w = three_nn_weights(unknown_xyz, known_xyz)
    B, n = idx.shape[:2]
    out = _interpolate_rows(know_feat.transpose(1, 2).float(), idx, w)
    return out.view(B, n, -1).transpose(1, 2)


class LayerNorm1d(nn.LayerNorm):
    """openpoints LayerNorm1d (layers/norm.py:23-31): a LayerNorm over the channels; it ignores norm_args (eps 1e-5)."""

    def __init__(self, num_channels, **kwargs):
        super().__init__(num_channels)


def _norm_1d(norm_args, channels, who):
    """create_norm(norm_args, channels, dimension='1d') (layers/norm.py:74-97) for 'bn' / 'bn1d' (BatchNorm1d) and 'ln' / 'ln1d'
    (LayerNorm1d)"""
    if norm_args is None:
        return None
    if isinstance(norm_args, dict):
        kw = dict(norm_args)
        norm = kw.pop("norm", None)
    else:
        norm, kw = norm_args, {}
    if norm is None:
        return None
    norm = str(norm).lower()
    if "1d" not in norm:
        norm += "1d"
    if norm == "bn1d":
        return nn.BatchNorm1d(channels, **kw)
    if norm == "ln1d":
        return LayerNorm1d(channels, **kw)
    raise MetaEncError(f"{who}: norm_args {norm_args!r} (bn / bn1d / ln1d are implemented)")


def _act_1d(act_args, who):
    if act_args is None:
        return None
    act = act_args.get("act") if isinstance(act_args, dict) else act_args
    if act is None:
        return None
    act = str(act).lower()
    if act == "relu":
        return nn.ReLU(inplace=True)
    if act == "gelu":
        return nn.GELU()
    raise MetaEncError(f"{who}: act_args {act_args!r} (relu / gelu are implemented)")


def _check_conv_args(conv_args, who):
    order = (conv_args or {}).get("order", "conv-norm-act")
    if order != "conv-norm-act":
        raise MetaEncError(f"{who}: conv order {order!r} (conv-norm-act is implemented)")


def _convblock1d(cin, cout, norm_args=None, act_args=None, order="conv-norm-act", who="create_convblock1d"):
    """create_convblock1d (layers/conv.py:65-103), order conv-norm-act: Conv1d k=1 (no bias where a norm follows), norm, act"""
    _check_conv_args({"order": order}, who)
    norm = _norm_1d(norm_args, cout, who)
    mods = [nn.Conv1d(cin, cout, 1, bias=norm is None)]
    if norm is not None:
        mods.append(norm)
    act = _act_1d(act_args, who)
    if act is not None:
        mods.append(act)
    return nn.Sequential(*mods)


def _w2d(conv) -> torch.Tensor:
    """the [out, in] matrix of a k = 1 convolution (Conv1d / Conv2d)"""
    return conv.weight.reshape(conv.out_channels, conv.in_channels)


def _lin(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [rows, K] W^T (+ b) on the exact-fp32 GEMM"""
    return linear(x.float(), w, b)


def _post(blk: nn.Sequential, f: torch.Tensor) -> torch.Tensor:
    """the norm / activation behind a conv block's Conv1d, on token-major rows"""
    for mod in list(blk)[1:]:
        if isinstance(mod, nn.BatchNorm1d):
            f = _batch_norm_rows(mod, f)
        elif isinstance(mod, nn.LayerNorm):
            f = _LayerNormFn.apply(f, mod.weight, mod.bias, mod.eps)
        elif isinstance(mod, nn.ReLU):
            f = torch.relu(f)
        elif isinstance(mod, nn.GELU):
            f = torch.nn.functional.gelu(f)
        else:
            raise MetaEncError(f"conv block: {type(mod).__name__} is not implemented")
    return f


def _need_cuda(t: torch.Tensor, who: str):
    if not t.is_cuda:
        raise MetaEncError(f"{who}: CUDA tensors required (no CPU fallback)")


class FeaturePropogation(nn.Module):
    """openpoints FeaturePropogation (backbone/pointnext.py:173-226, the reference spelling), upsample branch:
    convs(cat(f_skip, three_interpolation(p_dense, p_sparse, f_sparse))), or convs(interp) without a skip; convs are
    create_convblock1d blocks (Conv1d k=1, BatchNorm1d, ReLU) with keys ``convs.{j}.{0|1}.*``.

    The first conv never sees the concatenation: interpolation is linear, so with W = [W_a | W_b]
    cat(f_skip, interp(f_sparse)) W^T = f_skip W_a^T + interp(f_sparse W_b^T); the W_b GEMM runs on the sparse points and
    me_three_interpolate adds its result onto the skip GEMM's output in place."""

    def __init__(self, mlp, upsample=True, norm_args={"norm": "bn1d"}, act_args={"act": "relu"}):
        super().__init__()
        if not upsample:
            raise MetaEncError("FeaturePropogation: upsample=False (the PointNet++ global branch) is not implemented")
        self.convs = nn.Sequential(*[_convblock1d(mlp[i], mlp[i + 1], norm_args=norm_args, act_args=act_args,
                                                  who="FeaturePropogation") for i in range(len(mlp) - 1)])

    def rows(self, p1: torch.Tensor, f1: Optional[torch.Tensor], p2: torch.Tensor, f2: torch.Tensor,
             cloud: Optional[torch.Tensor] = None) -> torch.Tensor:
        """token-major core: dense points p1 [B, n, 3] with skip features f1 [B, n, Cs] (or None), sparse points p2 [B, m, 3] with
        features f2 [B, m, Cin]; ``cloud`` [B, Cc] are per-cloud channels in front of the skip (the part decoder's class
        branch).  Returns [B*n, C_out] fp32."""
        _need_cuda(p1, "FeaturePropogation")
        B, n, _ = p1.shape
        m, Cin = f2.shape[1], f2.shape[2]
        Cs = f1.shape[2] if f1 is not None else 0
        Cc = cloud.shape[1] if cloud is not None else 0
        conv = self.convs[0][0]
        if conv.in_channels != Cc + Cs + Cin:
            raise MetaEncError(f"FeaturePropogation: the first conv takes {conv.in_channels} channels, given {Cc} + {Cs} + {Cin}")
        w = _w2d(conv)
        idx, wt = three_nn_weights(p1, p2)
        z = _lin(f2.reshape(B * m, Cin), w[:, Cc + Cs:])                         # the interpolated part, on the sparse rows
        y = _lin(f1.reshape(B * n, Cs), w[:, Cc:Cc + Cs], conv.bias) if Cs else None
        f = _interpolate_rows(z.view(B, m, -1), idx, wt, y)
        if cloud is not None:                                                     # [B, C]: constant over the cloud
            g = _lin(cloud, w[:, :Cc], conv.bias if y is None else None)
            f = (f.view(B, n, -1) + g.unsqueeze(1)).view(B * n, -1)
        elif y is None and conv.bias is not None:
            f = f + conv.bias
        f = _post(self.convs[0], f)
        for blk in list(self.convs)[1:]:
            f = _post(blk, _lin(f, _w2d(blk[0]), blk[0].bias))
        return f

    def forward(self, pf1, pf2=None):
        if pf2 is None:
            raise MetaEncError("FeaturePropogation: the global branch (pf2=None) needs upsample=False, which is not implemented")
        (p1, f1), (p2, f2) = pf1, pf2
        B, n = p1.shape[:2]
        out = self.rows(p1, f1.transpose(1, 2) if f1 is not None else None, p2, f2.transpose(1, 2))
        return out.view(B, n, -1).transpose(1, 2)


def _cat_global(g: Optional[torch.Tensor], f: torch.Tensor) -> torch.Tensor:
    """cat(broadcast(g [B, G]), f [B, N, C]) channel-first -> [B, G + C, N] (the reference's decoder output)"""
    if g is None:
        return f.transpose(1, 2)
    return torch.cat((g.unsqueeze(2).expand(-1, -1, f.shape[1]), f.transpose(1, 2)), dim=1)


class _ViTDecoderBase(nn.Module):
    """what PointViTDecoder and PointViTPartDecoder (backbone/pointvit.py:177-393) share"""

    def _build(self, encoder_channel_list, decoder_layers, n_decoder_stages, scale, channel_scaling, sampler, global_feat,
               progressive_input, kwargs, cls_branch=None):
        who = type(self).__name__
        if str(sampler).lower() != "fps":
            raise MetaEncError(f"{who}: sampler {sampler!r} (fps is implemented; random sampling is not)")
        _check_conv_args(kwargs.get("conv_args"), who)
        self.decoder_layers = decoder_layers
        self.global_feat = global_feat.split(",") if global_feat is not None else None
        num_global_feat = len(self.global_feat) if self.global_feat is not None else 0
        self.in_channels = encoder_channel_list[-1]
        self.scale = scale
        self.n_decoder_stages = n_decoder_stages
        if progressive_input:
            skip_dim = [self.in_channels // 2 ** i for i in range(n_decoder_stages - 1, 0, -1)]
        else:
            skip_dim = [0 for _ in range(n_decoder_stages - 1)]
        skip_channels = [encoder_channel_list[0]] + skip_dim
        fp_channels = [self.in_channels * channel_scaling]
        for _ in range(n_decoder_stages - 1):
            fp_channels.insert(0, fp_channels[0] * channel_scaling)
        if cls_branch is not None:                  # the part decoder's convc, registered before the decoder as in the reference
            skip_channels[0] += cls_branch()
        decoder = [[] for _ in range(n_decoder_stages)]
        for i in range(-1, -n_decoder_stages - 1, -1):
            mlp = [skip_channels[i] + self.in_channels] + [fp_channels[i]] * self.decoder_layers
            decoder[i] = nn.Sequential(FeaturePropogation(mlp))
            self.in_channels = fp_channels[i]
        self.decoder = nn.Sequential(*decoder)
        self.out_channels = fp_channels[-n_decoder_stages] * (num_global_feat + 1)

    def _run(self, p, f, cloud=None):
        """the shared forward on the caller's lists (mutated as the reference mutates them) -> (global [B, G*C] or None,
        f_out [B, N, C] token-major)"""
        who = type(self).__name__
        _need_cuda(p[0], who)
        if len(p) != self.n_decoder_stages + 1:     # the FPS resampling path: new point sets, no skip features
            for i in range(self.n_decoder_stages - 1):
                pos = p[i]
                idx = furthest_point_sample(pos, pos.shape[1] // self.scale).long()
                p.insert(1, torch.gather(pos, 1, idx.unsqueeze(-1).expand(-1, -1, 3)))
                f.insert(1, None)
        cur = f[-1].transpose(1, 2)                                          # [B, 1 + S, C] token-major
        cls_token = cur[:, 0].float()
        cur = cur[:, 1:]
        f[-1] = cur.transpose(1, 2)
        L = len(self.decoder)
        for i in range(-1, -L - 1, -1):
            skip = f[i - 1]
            rows = self.decoder[i][0].rows(p[i - 1], skip.transpose(1, 2).float() if skip is not None else None, p[i],
                                           cur.float(), cloud if i == -L else None)
            cur = rows.view(p[i - 1].shape[0], p[i - 1].shape[1], -1)
            f[i - 1] = cur.transpose(1, 2)
        if self.global_feat is None:
            return None, cur
        gs = []
        for token_type in self.global_feat:
            if "cls" in token_type:
                gs.append(cls_token)
            elif "max" in token_type:
                gs.append(pool_tokens(cur, "max"))
            elif token_type in ("avg", "mean"):
                gs.append(pool_tokens(cur, "mean"))
        if not gs:
            raise MetaEncError(f"{who}: global_feat {','.join(self.global_feat)!r} names none of cls / max / avg / mean")
        return torch.cat(gs, dim=1), cur


class PointViTDecoder(_ViTDecoderBase):
    """openpoints PointViTDecoder (backbone/pointvit.py:177-263), the decoder of the S3DIS / ScanNet recipes: per stage a
    FeaturePropogation from the coarser point set onto the finer one (keys ``decoder.{s}.0.convs.{j}.{0|1}.*``), then the
    optional global features (cls token / max / avg over the points) in front of every point's.

    forward(p, f) returns the reference's [B, C_out, N]; forward_split(p, f) returns (global [B, G*C] or None, f_out
    [B, N, C] token-major) and with SegHead.forward_split skips the materialised concatenation.  three_nn, the interpolation
    and every 1x1 convolution (exact-fp32 GEMM), LayerNorm and pooling run in libmetaenc.so; BatchNorm1d and ReLU are torch
    glue.  fp32 throughout, autocast included."""

    def __init__(self, encoder_channel_list, decoder_layers=2, n_decoder_stages=2, scale=4, channel_scaling=1, sampler="fps",
                 global_feat=None, progressive_input=False, **kwargs):
        super().__init__()
        self._build(encoder_channel_list, decoder_layers, n_decoder_stages, scale, channel_scaling, sampler, global_feat,
                    progressive_input, kwargs)

    def forward_split(self, p, f):
        return self._run(p, f)

    def forward(self, p, f):
        return _cat_global(*self.forward_split(p, f))


class PointViTPartDecoder(_ViTDecoderBase):
    """openpoints PointViTPartDecoder (backbone/pointvit.py:266-393), the ShapeNetPart decoder, cls_map 'pointnet2': the shape
    class one-hot [B, 16] goes through ``convc`` (Conv1d 16 -> 64 with bias, then the recipe's activation) and joins the
    skip features of the last stage.  The one-hot is constant over a cloud, so convc and its share of the last stage's first
    conv run once per cloud and are broadcast.  Interfaces as PointViTDecoder, with cls_label [B, 1]."""

    def __init__(self, encoder_channel_list, decoder_layers=2, n_decoder_stages=2, scale=4, channel_scaling=1, sampler="fps",
                 global_feat=None, progressive_input=False, cls_map="pointnet2", num_classes=16, **kwargs):
        super().__init__()
        if cls_map != "pointnet2":
            raise MetaEncError(f"PointViTPartDecoder: cls_map {cls_map!r} (pointnet2 is implemented; curvenet is not)")
        self.cls_map, self.num_classes = cls_map, num_classes
        act_args = kwargs.get("act_args", {"act": "relu"})

        def cls_branch():
            self.convc = nn.Sequential(_convblock1d(16, 64, norm_args=None, act_args=act_args, who="PointViTPartDecoder"))
            return 64
        self._build(encoder_channel_list, decoder_layers, n_decoder_stages, scale, channel_scaling, sampler, global_feat,
                    progressive_input, kwargs, cls_branch)

    def forward_split(self, p, f, cls_label):
        _need_cuda(p[0], "PointViTPartDecoder")
        B = p[0].shape[0]
        one_hot = torch.zeros(B, self.num_classes, device=p[0].device).scatter_(1, cls_label.long().reshape(B, -1), 1)
        blk = self.convc[0]
        cloud = _post(blk, _lin(one_hot, _w2d(blk[0]), blk[0].bias))                  # [B, 64]: convc on every point alike
        return self._run(p, f, cloud)

    def forward(self, p, f, cls_label):
        return _cat_global(*self.forward_split(p, f, cls_label))


class SegHead(nn.Module):
    """openpoints SegHead (segmentation/base_seg.py:92-149): optional global features (max / avg over the points) appended
    to every point's, create_convblock1d blocks with Dropout between them, a final Conv1d with bias; keys
    ``head.{0|2}.*``.  forward(end_points [B, C, N]) -> logits [B, num_classes, N].

    forward_split(global, f) takes the decoder's split output instead of cat(broadcast(global), f): everything constant over
    a cloud (the decoder's global features, and the head's own pooled ones) meets its share of the first conv once per
    cloud, so only f [B, N, C] runs the per-point GEMM."""

    def __init__(self, num_classes, in_channels, mlps=None, norm_args={"norm": "bn1d"}, act_args={"act": "relu"}, dropout=0.5,
                 global_feat=None, **kwargs):
        super().__init__()
        _check_conv_args(kwargs.get("conv_args"), "SegHead")
        if global_feat is not None:
            self.global_feat = global_feat.split(",")
            multiplier = len(self.global_feat) + 1
        else:
            self.global_feat = None
            multiplier = 1
        in_channels *= multiplier
        if mlps is None:
            mlps = [in_channels, in_channels] + [num_classes]
        else:
            mlps = [in_channels] + (list(mlps) if isinstance(mlps, (list, tuple)) else [mlps]) + [num_classes]
        heads = []
        for i in range(len(mlps) - 2):
            heads.append(_convblock1d(mlps[i], mlps[i + 1], norm_args=norm_args, act_args=act_args, who="SegHead"))
            if dropout:
                heads.append(nn.Dropout(dropout))
        heads.append(_convblock1d(mlps[-2], mlps[-1], act_args=None, who="SegHead"))
        self.head = nn.Sequential(*heads)

    def forward_split(self, global_feat: Optional[torch.Tensor], f: torch.Tensor) -> torch.Tensor:
        """global [B, G] (or None) and token-major f [B, N, C] stand for end_points = cat(broadcast(global), f) -> logits
        [B, num_classes, N]"""
        _need_cuda(f, "SegHead")
        B, N, C = f.shape
        f = f.float().contiguous()
        G = global_feat.shape[1] if global_feat is not None else 0
        cloud = [global_feat.float()] if global_feat is not None else []
        for feat_type in self.global_feat or []:
            mode = "max" if "max" in feat_type else "mean" if feat_type in ("avg", "mean") else None
            if mode is None:
                continue
            if global_feat is not None:
                cloud.append(global_feat.float())                     # pooled over the points, a broadcast is itself
            cloud.append(pool_tokens(f, mode))
        pools = sum(1 for t in self.global_feat or [] if "max" in t or t in ("avg", "mean"))
        conv = self.head[0][0]
        if conv.in_channels != (G + C) * (1 + pools):
            raise MetaEncError(f"SegHead: the first conv takes {conv.in_channels} channels, given {G} global + {C} per point")
        w = _w2d(conv)
        y = _lin(f.reshape(B * N, C), w[:, G:G + C], conv.bias)
        if cloud:
            g = _lin(torch.cat(cloud, dim=1), torch.cat([w[:, :G], w[:, G + C:]], dim=1))
            y = (y.view(B, N, -1) + g.unsqueeze(1)).view(B * N, -1)
        y = _post(self.head[0], y)
        for mod in list(self.head)[1:]:
            y = mod(y) if isinstance(mod, nn.Dropout) else _post(mod, _lin(y, _w2d(mod[0]), mod[0].bias))
        return y.view(B, N, -1).transpose(1, 2).contiguous()

    def forward(self, end_points: torch.Tensor) -> torch.Tensor:
        return self.forward_split(None, end_points.transpose(1, 2))
