"""Multi-scale deformable attention and the ViT-Adapter interaction blocks (Image detection / segmentation backbones).

Restated from the reference with its constructor arguments, parameter names and forward signatures, so that the
``interactions.*`` part of a ViT-Adapter checkpoint loads ``strict=True``:
  * ``ms_deform_attn`` / ``MSDeformAttn``  -- Image/detection/ops/functions/ms_deform_attn_func.py:19-46 and
    ops/modules/ms_deform_attn.py:28-130 (the reference ships the sampling core as a CUDA extension only);
  * ``get_reference_points``, ``deform_inputs``, ``ConvFFN``, ``DWConv``, ``Extractor``, ``Injector``, ``InteractionBlock`` --
    Image/{detection,segmentation}/mmdet_custom|mmseg_custom/models/backbones/adapter_modules.py:13-191.
The sampling core (forward, and the three gradients) is me_ms_deform_attn_fwd / _bwd of libmetaenc.so; every Linear runs on the
library's GEMMs (heads.linear) and every LayerNorm on its LayerNorm kernels.  Softmax, the location arithmetic, the depth-wise
3x3 convolution, GELU behind it and DropPath are PyTorch glue.  ``InteractionBlock.forward`` takes ``blocks`` = a slice of this
package's layer-scale / windowed ``Block``s, as vit_adapter.py:107 slices the encoder.

The backbone around them -- ``SpatialPriorModule`` (adapter_modules.py:194-246) and ``ViTAdapter`` (vit_adapter.py:19-132) -- keeps
every image tensor as token rows [B*H*W, C] (row order (b, y, x)): ``conv3x3_rows`` (me_conv3x3_gather + the GEMMs of heads.linear,
me_conv3x3_scatter for the input gradient), ``max_pool3x3s2_rows``, ``resize_rows_batched`` and ``conv_transpose2x2_rows`` are
the kernels of csrc/conv_rows.hip.  SyncBatchNorm (called on the [rows, C] tensor), ReLU, the level-embed adds and the one
permute to channel-first at the very end are PyTorch glue.
"""
from __future__ import annotations

import ctypes
import math
from functools import partial
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as cp

from . import _capi, ops
from ._capi import MetaEncError, check, dtype_code, ptr, stream_ptr
from .data2seq import PatchEmbed
from .encoder import Block
from .heads import _LayerNormFn
from .linear import linear

MAX_LEVELS = 8          # me_ms_deform_attn_*: levels per call
MAX_HEAD_DIM = 128      # ... channels per head (a multiple of 4)


def _host_levels(spatial_shapes, level_start_index) -> Tuple[List[Tuple[int, int]], List[int]]:
    """(H, W) per level and the level starts as host integers.  A CUDA tensor costs one device synchronisation here."""
    def rows(t, who):
        if isinstance(t, torch.Tensor):
            if t.dtype.is_floating_point or t.dtype == torch.bool:
                raise MetaEncError(f"ms_deform_attn: {who} must hold integers (got {t.dtype})")
            t = t.detach().cpu().tolist()
        return t
    shp = rows(spatial_shapes, "spatial_shapes")
    st = rows(level_start_index, "level_start_index")
    try:
        shapes = [(int(h), int(w)) for h, w in shp]
        starts = [int(s) for s in st]
    except (TypeError, ValueError) as e:
        raise MetaEncError("ms_deform_attn: spatial_shapes must be [L, 2] (H, W) pairs and level_start_index [L] integers") from e
    if len(shapes) != len(starts):
        raise MetaEncError(f"ms_deform_attn: level_start_index has {len(starts)} entries for {len(shapes)} spatial_shapes")
    return shapes, starts


def _require_one_gpu(who: str, **tensors) -> None:
    """every given tensor (None entries are skipped) on one and the same CUDA device, or a MetaEncError naming the offender"""
    first = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise MetaEncError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise MetaEncError(f"{who}: {name} is a CPU tensor: CUDA tensors required (no CPU fallback)")
        if first is None:
            first = (name, t.device)
        elif t.device != first[1]:
            raise MetaEncError(f"{who}: {name} is on {t.device} but {first[0]} is on {first[1]}")


def _c_levels(shapes, starts):
    L = len(shapes)
    flat = [v for hw in shapes for v in hw]
    return (ctypes.c_int32 * max(2 * L, 1))(*flat), (ctypes.c_int32 * max(L, 1))(*starts)


def _msda_backward(value, shapes, starts, loc, attn, dout, need_value: bool, need_query: bool, dvalue: Optional[torch.Tensor] = None):
    """me_ms_deform_attn_bwd on contiguous fp32 tensors -> (dvalue, dloc, dattn), None for what was not asked for.  ``dvalue``
    may be a caller-owned contiguous fp32 buffer of value's shape (every element of it is written)."""
    lib = _capi.load()
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    if value.numel() == 0 or loc.numel() == 0:               # an empty problem: no sample, every gradient zero
        dv = (torch.zeros_like(value) if dvalue is None else dvalue.zero_()) if need_value else None
        return dv, (torch.zeros_like(loc) if need_query else None), (torch.zeros_like(attn) if need_query else None)
    if need_value and dvalue is None:
        dvalue = torch.empty_like(value)
    dloc = torch.empty_like(loc) if need_query else None
    dattn = torch.empty_like(attn) if need_query else None
    if not (need_value or need_query):
        return None, None, None
    cs, cl = _c_levels(shapes, starts)
    ws = None
    if need_value:
        ws = torch.empty(max(16, int(lib.me_ms_deform_attn_bwd_workspace(N, S, M, Lq, L, P))), dtype=torch.uint8, device=value.device)
    check(lib.me_ms_deform_attn_bwd(ptr(value), cs, cl, ptr(loc), ptr(attn), ptr(dout), ptr(dvalue) if need_value else 0, ptr(dloc),
                                    ptr(dattn), N, S, M, D, Lq, L, P, ptr(ws), ws.numel() if ws is not None else 0, stream_ptr()),
          "me_ms_deform_attn_bwd")
    return (dvalue if need_value else None), dloc, dattn


class _MSDeformAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, loc, attn, shapes, starts):
        v, lo, aw = value.float().contiguous(), loc.float().contiguous(), attn.float().contiguous()
        N, S, M, D = v.shape
        Lq, L, P = lo.shape[1], lo.shape[3], lo.shape[4]
        out = torch.empty(N, Lq, M * D, dtype=torch.float32, device=v.device)
        cs, cl = _c_levels(shapes, starts)
        check(_capi.load().me_ms_deform_attn_fwd(ptr(v), cs, cl, ptr(lo), ptr(aw), ptr(out), N, S, M, D, Lq, L, P, stream_ptr()),
              "me_ms_deform_attn_fwd")
        ctx.save_for_backward(v, lo, aw)
        ctx.levels = (shapes, starts)
        ctx.dtypes = (value.dtype, loc.dtype, attn.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        v, lo, aw = ctx.saved_tensors
        shapes, starts = ctx.levels
        need_q = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dv, dl, da = _msda_backward(v, shapes, starts, lo, aw, dout.float().contiguous(), ctx.needs_input_grad[0], need_q)
        vdt, ldt, adt = ctx.dtypes
        return (dv.to(vdt) if dv is not None else None, dl.to(ldt) if dl is not None and ctx.needs_input_grad[1] else None,
                da.to(adt) if da is not None and ctx.needs_input_grad[2] else None, None, None)


def ms_deform_attn(value: torch.Tensor, spatial_shapes, level_start_index, sampling_locations: torch.Tensor,
                   attention_weights: torch.Tensor, im2col_step=None) -> torch.Tensor:
    """MSDeformAttnFunction.apply (ops/functions/ms_deform_attn_func.py:19-46), same argument order; ``im2col_step`` is accepted
    and ignored.  value [N, S, M, D], sampling_locations [N, Lq, M, L, P, 2] ((x, y) in [0, 1] over the level),
    attention_weights [N, Lq, M, L, P] -> [N, Lq, M * D] fp32; gradients for value, sampling_locations and attention_weights
    (the value gradient is deterministic: no float atomics).  bf16 / fp16 inputs are cast to fp32 and the result is fp32, as the
    reference's custom_fwd(cast_inputs=torch.float32) does.

    ``spatial_shapes`` [L, 2] = (H_l, W_l) and ``level_start_index`` [L] may be lists, CPU tensors or CUDA tensors; the kernel
    takes them as host arrays, so a CUDA tensor costs one device synchronisation per call (``deform_inputs`` returns CPU tensors).
    L <= 8, D a multiple of 4 up to 128."""
    del im2col_step
    for name, t, nd in (("value", value, 4), ("sampling_locations", sampling_locations, 6), ("attention_weights", attention_weights, 5)):
        if not isinstance(t, torch.Tensor) or t.dim() != nd:
            raise MetaEncError(f"ms_deform_attn: {name} must be a {nd}-dimensional tensor"
                               + (f" (got shape {tuple(t.shape)})" if isinstance(t, torch.Tensor) else ""))
        if not t.is_floating_point():
            raise MetaEncError(f"ms_deform_attn: {name} must be a floating-point tensor (got {t.dtype})")
    N, S, M, D = value.shape
    if sampling_locations.shape[0] != N or sampling_locations.shape[2] != M or sampling_locations.shape[5] != 2:
        raise MetaEncError(f"ms_deform_attn: sampling_locations {tuple(sampling_locations.shape)} must be [N, Lq, M, L, P, 2] for value "
                           f"{tuple(value.shape)}")
    if tuple(attention_weights.shape) != tuple(sampling_locations.shape[:5]):
        raise MetaEncError(f"ms_deform_attn: attention_weights {tuple(attention_weights.shape)} must be [N, Lq, M, L, P] = "
                           f"{tuple(sampling_locations.shape[:5])}")
    shapes, starts = _host_levels(spatial_shapes, level_start_index)
    if len(shapes) != sampling_locations.shape[3]:
        raise MetaEncError(f"ms_deform_attn: spatial_shapes has {len(shapes)} levels, sampling_locations has {sampling_locations.shape[3]}")
    if len(shapes) > MAX_LEVELS:
        raise MetaEncError(f"ms_deform_attn: spatial_shapes has {len(shapes)} levels (at most {MAX_LEVELS})")
    if D % 4 != 0 or D > MAX_HEAD_DIM:
        raise MetaEncError(f"ms_deform_attn: value has D = {D} channels per head (a multiple of 4, at most {MAX_HEAD_DIM})")
    _require_one_gpu("ms_deform_attn", value=value, sampling_locations=sampling_locations, attention_weights=attention_weights)
    return _MSDeformAttnFn.apply(value, sampling_locations, attention_weights, tuple(shapes), tuple(starts))


def _layernorm(norm: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """an nn.LayerNorm on the library's kernel (any other norm_layer the caller chose runs as it is)"""
    if type(norm) is not nn.LayerNorm:
        return norm(x)
    return _LayerNormFn.apply(x.float() if x.dtype == torch.float16 else x, norm.weight, norm.bias, norm.eps)


def _lin(layer: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    return linear(x, layer.weight, layer.bias)


class MSDeformAttn(nn.Module):
    """The reference's MSDeformAttn module (ops/modules/ms_deform_attn.py) by interface: constructor arguments, the four
    nn.Linear parameters ``sampling_offsets`` / ``attention_weights`` / ``value_proj`` / ``output_proj``, their initial values and
    the forward signature.  Per query and head it predicts L x P sampling offsets and softmax weights, samples the projected
    values there (me_ms_deform_attn_fwd / _bwd) and projects the result back.  The Linears run on the library's GEMMs; softmax
    and the location arithmetic are PyTorch glue."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4, ratio=1.0):
        super().__init__()
        width = int(d_model * ratio)                         # channels of the value / sampled side
        if d_model % n_heads or width % n_heads:
            raise MetaEncError(f"MSDeformAttn: d_model = {d_model} and int(d_model * ratio) = {width} must both split into n_heads = {n_heads}")
        if (width // n_heads) % 4 or width // n_heads > MAX_HEAD_DIM:
            raise MetaEncError(f"MSDeformAttn: {width // n_heads} channels per head (a multiple of 4, at most {MAX_HEAD_DIM}, is what "
                               f"the kernels take)")
        if not 1 <= n_levels <= MAX_LEVELS:
            raise MetaEncError(f"MSDeformAttn: n_levels = {n_levels} (1 .. {MAX_LEVELS})")
        self.d_model, self.ratio = d_model, ratio
        self.n_levels, self.n_heads, self.n_points = n_levels, n_heads, n_points
        self.im2col_step = 64                                # kept for callers that read it; the kernels have no such step
        samples = n_heads * n_levels * n_points
        self.sampling_offsets = nn.Linear(d_model, 2 * samples)
        self.attention_weights = nn.Linear(d_model, samples)
        self.value_proj = nn.Linear(d_model, width)
        self.output_proj = nn.Linear(width, d_model)
        self._reset_parameters()

    @torch.no_grad()
    def _reset_parameters(self):
        """Queries start out ignoring their content: zero offset / weight matrices, zero weight biases (uniform softmax), and an
        offset bias that sends head m along the direction of angle 2 pi m / n_heads (scaled so its larger component is 1), point
        p of every level p + 1 steps out.  The two projections are xavier-uniform with zero bias."""
        M, L, P = self.n_heads, self.n_levels, self.n_points
        angle = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
        direction = torch.stack([angle.cos(), angle.sin()], -1)
        direction = direction / direction.abs().amax(-1, keepdim=True)
        steps = torch.arange(1, P + 1, dtype=torch.float32)
        self.sampling_offsets.bias.copy_((direction[:, None, None, :] * steps[None, None, :, None]).expand(M, L, P, 2).reshape(-1))
        for zeroed in (self.sampling_offsets.weight, self.attention_weights.weight, self.attention_weights.bias,
                       self.value_proj.bias, self.output_proj.bias):
            zeroed.zero_()
        nn.init.xavier_uniform_(self.value_proj.weight)
        nn.init.xavier_uniform_(self.output_proj.weight)

    def _locations(self, reference_points: torch.Tensor, offsets: torch.Tensor, shapes) -> torch.Tensor:
        """[N, Lq, M, L, P, 2] normalised sample positions.  Reference points [N, Lq, L, 2]: the offsets are in pixels of their
        level; [N, Lq, L, 4] = (cx, cy, w, h) boxes: the offsets are in units of half a box side / n_points."""
        ref = reference_points.to(offsets.dtype)[:, :, None, :, None, :]
        cols = ref.shape[-1]
        if cols == 2:
            pixels = torch.tensor([(w, h) for h, w in shapes], dtype=offsets.dtype, device=offsets.device)
            return ref + offsets / pixels[:, None, :]
        if cols == 4:
            return ref[..., :2] + offsets * (ref[..., 2:] * (0.5 / self.n_points))
        raise MetaEncError(f"MSDeformAttn: reference_points must end in 2 (points) or 4 (boxes) columns, got {cols}")

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index, input_padding_mask=None):
        """query [N, Lq, C]; reference_points [N, Lq, L, 2] in [0, 1] or [N, Lq, L, 4]; input_flatten [N, sum_l H_l W_l, C];
        input_spatial_shapes [L, 2] (H, W) and input_level_start_index [L] as in ms_deform_attn; input_padding_mask
        [N, sum_l H_l W_l], True on padding -> [N, Lq, C]"""
        _require_one_gpu("MSDeformAttn", query=query, input_flatten=input_flatten, reference_points=reference_points,
                         input_padding_mask=input_padding_mask)
        shapes, starts = _host_levels(input_spatial_shapes, input_level_start_index)
        M, L, P = self.n_heads, self.n_levels, self.n_points
        rows = sum(h * w for h, w in shapes)
        if len(shapes) != L or rows != input_flatten.shape[1]:
            raise MetaEncError(f"MSDeformAttn: input_spatial_shapes gives {len(shapes)} levels of {rows} rows in all; the module has "
                               f"n_levels = {L} and input_flatten {input_flatten.shape[1]} rows")
        N, Lq = query.shape[:2]
        value = _lin(self.value_proj, input_flatten)
        if input_padding_mask is not None:
            value = value * (~input_padding_mask).to(value.dtype).unsqueeze(-1)
        weights = F.softmax(_lin(self.attention_weights, query).view(N, Lq, M, L * P), dim=-1)
        offsets = _lin(self.sampling_offsets, query).view(N, Lq, M, L, P, 2)
        sampled = _MSDeformAttnFn.apply(value.view(N, rows, M, -1), self._locations(reference_points, offsets, shapes),
                                        weights.view(N, Lq, M, L, P), tuple(shapes), tuple(starts))
        return _lin(self.output_proj, sampled)


def _pixel_centres(h: int, w: int, device) -> torch.Tensor:
    """[h w, 2] = ((j + 0.5) / w, (i + 0.5) / h), row-major"""
    ys = torch.linspace(0.5, h - 0.5, h, dtype=torch.float32, device=device) / h
    xs = torch.linspace(0.5, w - 0.5, w, dtype=torch.float32, device=device) / w
    return torch.stack((xs.repeat(h), ys.repeat_interleave(w)), -1)


def get_reference_points(spatial_shapes, device):
    """The pixel centres of every level in normalised (x, y), levels concatenated: [1, sum_l H_l W_l, 1, 2] fp32
    (adapter_modules.get_reference_points by interface)."""
    return torch.cat([_pixel_centres(int(h), int(w), device) for h, w in spatial_shapes])[None, :, None, :]


def _level_tensors(shapes):
    """(spatial_shapes [L, 2], level_start_index [L]) as int64 CPU tensors"""
    areas = [h * w for h, w in shapes]
    return torch.tensor(shapes, dtype=torch.long), torch.tensor([sum(areas[:l]) for l in range(len(areas))], dtype=torch.long)


def deform_inputs(x: torch.Tensor):
    """For an image batch x [B, C, h, w]: (deform_inputs1, deform_inputs2), each [reference_points, spatial_shapes,
    level_start_index] (adapter_modules.deform_inputs by interface).  The first serves the injector: queries on the stride-16
    grid, values on the stride 8 / 16 / 32 pyramid; the second the extractor, the other way round.  reference_points live on x's
    device; the shape tensors stay on the CPU (int64), where ms_deform_attn wants them: no synchronisation per call."""
    h, w = x.shape[-2:]
    vit = [(h // 16, w // 16)]
    pyramid = [(h // s, w // s) for s in (8, 16, 32)]
    return ([get_reference_points(vit, x.device), *_level_tensors(pyramid)],
            [get_reference_points(pyramid, x.device), *_level_tensors(vit)])


class DropPath(nn.Module):
    """stochastic depth per sample (what timm calls DropPath): PyTorch glue, identity in eval mode or at probability 0"""

    def __init__(self, drop_prob: float = 0.):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * (mask / keep)


class DWConv(nn.Module):
    """One depth-wise 3x3 convolution (parameter ``dwconv``) shared by the three pyramid levels of the token rows [B, 21 n, C]:
    16 n rows of the 2H x 2W grid, 4 n of H x W, n of H/2 x W/2.  PyTorch glue."""

    def __init__(self, dim=768):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=3, padding=1, groups=dim)

    def forward(self, x, H, W):
        B, rows, C = x.shape
        grids = ((2 * H, 2 * W), (H, W), (H // 2, W // 2))
        if sum(h * w for h, w in grids) != rows:
            raise MetaEncError(f"DWConv: {rows} token rows are not the 2H x 2W + H x W + H/2 x W/2 pyramid of H = {H}, W = {W}")
        out = []
        for part, (h, w) in zip(x.split([h * w for h, w in grids], dim=1), grids):
            out.append(self.dwconv(part.transpose(1, 2).reshape(B, C, h, w)).flatten(2).transpose(1, 2))
        return torch.cat(out, dim=1)


class ConvFFN(nn.Module):
    """Linear -> depth-wise convolution over the pyramid -> activation -> Linear, dropout behind the activation and at the end
    (parameters ``fc1``, ``dwconv``, ``fc2``).  The two Linears run on the library's GEMMs."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        hidden = hidden_features if hidden_features else in_features
        self.fc1 = nn.Linear(in_features, hidden)
        self.dwconv = DWConv(hidden)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden, out_features if out_features else in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x, H, W):
        hidden = self.drop(self.act(self.dwconv(_lin(self.fc1, x), H, W)))
        return self.drop(_lin(self.fc2, hidden))


_ADAPTER_NORM = partial(nn.LayerNorm, eps=1e-6)


class _DeformCrossAttention(nn.Module):
    """What Injector and Extractor share: ``query_norm``, ``feat_norm`` and ``attn`` (an MSDeformAttn in which the normalised
    queries sample the normalised features), and the optional recomputation of the whole step in backward."""

    def __init__(self, dim, num_heads, n_points, n_levels, deform_ratio, norm_layer, with_cp):
        super().__init__()
        self.with_cp = bool(with_cp)
        self.query_norm, self.feat_norm = norm_layer(dim), norm_layer(dim)
        self.attn = MSDeformAttn(dim, n_levels, num_heads, n_points, deform_ratio)

    def _attend(self, query, feat, reference_points, spatial_shapes, level_start_index):
        return self.attn(_layernorm(self.query_norm, query), reference_points, _layernorm(self.feat_norm, feat), spatial_shapes,
                         level_start_index)

    def _run(self, step, query, feat):
        """step(query, feat), under torch.utils.checkpoint when with_cp is set and a gradient is wanted"""
        if self.with_cp and query.requires_grad:
            return cp.checkpoint(step, query, feat, use_reentrant=True)
        return step(query, feat)


class Extractor(_DeformCrossAttention):
    """The pyramid tokens (query) gather from the ViT tokens (feat): query += attn, then query += drop_path(ConvFFN(ffn_norm(query)))
    when with_cffn (adapter_modules.Extractor by interface; parameters query_norm, feat_norm, attn, ffn, ffn_norm)."""

    def __init__(self, dim, num_heads=6, n_points=4, n_levels=1, deform_ratio=1.0, with_cffn=True, cffn_ratio=0.25, drop=0.,
                 drop_path=0., norm_layer=_ADAPTER_NORM, with_cp=False):
        super().__init__(dim, num_heads, n_points, n_levels, deform_ratio, norm_layer, with_cp)
        self.with_cffn = bool(with_cffn)
        if self.with_cffn:
            self.ffn = ConvFFN(dim, int(dim * cffn_ratio), drop=drop)
            self.ffn_norm = norm_layer(dim)
            self.drop_path = DropPath(drop_path) if drop_path > 0 else nn.Identity()

    def forward(self, query, reference_points, feat, spatial_shapes, level_start_index, H, W):
        def step(q, f):
            q = q + self._attend(q, f, reference_points, spatial_shapes, level_start_index)
            if not self.with_cffn:
                return q
            return q + self.drop_path(self.ffn(_layernorm(self.ffn_norm, q), H, W))
        return self._run(step, query, feat)


class Injector(_DeformCrossAttention):
    """The ViT tokens (query) gather from the pyramid tokens (feat) and take the result in through a learnt per-channel scale:
    query + gamma * attn (adapter_modules.Injector by interface; parameters query_norm, feat_norm, attn, gamma)."""

    def __init__(self, dim, num_heads=6, n_points=4, n_levels=1, deform_ratio=1.0, norm_layer=_ADAPTER_NORM, init_values=0.,
                 with_cp=False):
        super().__init__(dim, num_heads, n_points, n_levels, deform_ratio, norm_layer, with_cp)
        self.gamma = nn.Parameter(torch.full((dim,), float(init_values)))

    def forward(self, query, reference_points, feat, spatial_shapes, level_start_index):
        def step(q, f):
            return torch.addcmul(q, self.gamma, self._attend(q, f, reference_points, spatial_shapes, level_start_index))
        return self._run(step, query, feat)


class InteractionBlock(nn.Module):
    """One ViT-Adapter interaction (adapter_modules.InteractionBlock by interface): ``injector`` (3 pyramid levels into the ViT
    tokens), the caller's encoder blocks as ``blk(x, H, W)``, ``extractor`` (ViT tokens into the pyramid) and, with
    extra_extractor, two more in ``extra_extractors``."""

    def __init__(self, dim, num_heads=6, n_points=4, norm_layer=_ADAPTER_NORM, drop=0., drop_path=0., with_cffn=True,
                 cffn_ratio=0.25, init_values=0., deform_ratio=1.0, extra_extractor=False, with_cp=False):
        super().__init__()
        shared = dict(num_heads=num_heads, n_points=n_points, deform_ratio=deform_ratio, norm_layer=norm_layer, with_cp=with_cp)
        ffn = dict(with_cffn=with_cffn, cffn_ratio=cffn_ratio, drop=drop, drop_path=drop_path)
        self.injector = Injector(dim, n_levels=3, init_values=init_values, **shared)
        self.extractor = Extractor(dim, n_levels=1, **shared, **ffn)
        self.extra_extractors = nn.Sequential(Extractor(dim, **shared, **ffn), Extractor(dim, **shared, **ffn)) if extra_extractor else None

    def forward(self, x, c, blocks: Sequence[nn.Module], deform_inputs1, deform_inputs2, H, W):
        x = self.injector(x, deform_inputs1[0], c, deform_inputs1[1], deform_inputs1[2])
        for blk in blocks:
            x = blk(x, H, W)
        for extractor in (self.extractor, *(self.extra_extractors or ())):
            c = extractor(c, deform_inputs2[0], x, deform_inputs2[1], deform_inputs2[2], H, W)
        return x, c


# ----------------------------------------------------------------------------- image tensors as token rows (csrc/conv_rows.hip)
def conv_out_size(n: int, stride: int = 1) -> int:
    """output length of a 3-tap window with padding 1 over n positions (Conv2d(3, stride, 1), MaxPool2d(3, 2, 1))"""
    return (int(n) - 1) // int(stride) + 1


def interpolate_geometry(n: int, scale_factor: float) -> Tuple[int, float]:
    """(output length, source scale) of F.interpolate(scale_factor=f, align_corners=False) without recompute_scale_factor:
    floor(n * f) outputs sampled at (o + 0.5) / f - 0.5 -- 1 / f, not n / floor(n * f), which differs where n * f is not whole"""
    if not scale_factor > 0:
        raise MetaEncError(f"interpolate_geometry: scale_factor = {scale_factor} must be positive")
    return int(math.floor(float(n) * float(scale_factor))), 1.0 / float(scale_factor)


def _rows(who: str, x, B: int, H: int, W: int, multiple: int = 4) -> torch.Tensor:
    """x as a contiguous fp32 / bf16 [B*H*W, C] CUDA tensor (fp16 is converted to fp32), or a MetaEncError"""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise MetaEncError(f"{who}: x must be token rows [B*H*W, C]" + (f" (got shape {tuple(x.shape)})" if isinstance(x, torch.Tensor) else ""))
    if not x.is_cuda:
        raise MetaEncError(f"{who}: x is a CPU tensor: CUDA tensors required (no CPU fallback)")
    if min(int(B), int(H), int(W)) < 1 or x.shape[0] != int(B) * int(H) * int(W):
        raise MetaEncError(f"{who}: x has {x.shape[0]} rows, B * H * W = {B} * {H} * {W} expected")
    if x.dtype == torch.float16:
        x = x.float()
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"{who}: x must be float32, bfloat16 or float16 (got {x.dtype})")
    if x.shape[1] % multiple:
        raise MetaEncError(f"{who}: C = {x.shape[1]} must be a multiple of {multiple}")
    return x.contiguous()


def conv3x3_kpad(cin: int) -> int:
    """columns of the unfolded matrix: 9 cin rounded up to the GEMM's K granule (8)"""
    return (9 * int(cin) + 7) // 8 * 8


class _Conv3x3UnfoldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B, H, W, stride):
        Cin = x.shape[1]
        Kpad = conv3x3_kpad(Cin)
        cols = torch.empty(B * conv_out_size(H, stride) * conv_out_size(W, stride), Kpad, dtype=x.dtype, device=x.device)
        check(_capi.load().me_conv3x3_gather(ptr(x), dtype_code(x.dtype), ptr(cols), B, H, W, Cin, stride, Kpad, stream_ptr()),
              "me_conv3x3_gather")
        ctx.geom = (B, H, W, Cin, stride, Kpad, x.dtype)
        return cols

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dcols):
        B, H, W, Cin, stride, Kpad, dt = ctx.geom
        dcols = dcols.contiguous()
        if dcols.dtype not in (torch.float32, torch.bfloat16):
            dcols = dcols.float()
        dx = torch.empty(B * H * W, Cin, dtype=dt, device=dcols.device)
        check(_capi.load().me_conv3x3_scatter(ptr(dcols), dtype_code(dcols.dtype), ptr(dx), dtype_code(dt), B, H, W, Cin, stride, Kpad,
                                              stream_ptr()), "me_conv3x3_scatter")
        return dx, None, None, None, None


CONV_K_CHUNK = 128      # fp32 contractions longer than this run as several me_gemm calls accumulating into the output (linear's k_chunk)


def conv3x3_rows(x: torch.Tensor, weight: torch.Tensor, B: int, H: int, W: int, stride: int = 1,
                 bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Conv2d(Cin, Cout, 3, stride, padding=1) on rows: x [B*H*W, Cin] -> fp32 [B*Ho*Wo, Cout], Ho = conv_out_size(H, stride).
    ``weight`` keeps its checkpoint shape [Cout, Cin, 3, 3].  The rows are unfolded by me_conv3x3_gather into (dy, dx, c) columns
    and contracted on me_gemm with the dtype policy of heads.linear (fp32 rows: exact fp32 GEMM, K taken 128 columns at a time to
    keep the accumulation chains short; bf16 rows: bf16 GEMM; weight gradient on the split-K TN kernel);
    the input gradient is me_conv3x3_scatter, deterministic.  Any Cin (the RGB stem has 3); Cout as heads.linear takes it."""
    if stride not in (1, 2):
        raise MetaEncError(f"conv3x3_rows: stride = {stride} (1 or 2)")
    x = _rows("conv3x3_rows", x, B, H, W, multiple=1)
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3):
        raise MetaEncError(f"conv3x3_rows: weight must be [Cout, {x.shape[1]}, 3, 3]"
                           + (f" (got {tuple(weight.shape)})" if isinstance(weight, torch.Tensor) else ""))
    _require_one_gpu("conv3x3_rows", x=x, weight=weight, bias=bias)
    Cout, Cin = weight.shape[:2]
    cols = _Conv3x3UnfoldFn.apply(x, int(B), int(H), int(W), int(stride))
    return linear(cols, weight.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin), bias, k_chunk=CONV_K_CHUNK)


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B, H, W):
        C = x.shape[1]
        rows = B * conv_out_size(H, 2) * conv_out_size(W, 2)
        y = torch.empty(rows, C, dtype=x.dtype, device=x.device)
        idx = torch.empty(rows, C, dtype=torch.int8, device=x.device)
        check(_capi.load().me_maxpool3x3s2_rows(ptr(x), dtype_code(x.dtype), ptr(y), dtype_code(y.dtype), ptr(idx), B, H, W, C,
                                                stream_ptr()), "me_maxpool3x3s2_rows")
        ctx.save_for_backward(idx)
        ctx.geom = (B, H, W, C, x.dtype)
        ctx.mark_non_differentiable(idx)
        return y, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _didx):
        (idx,) = ctx.saved_tensors
        B, H, W, C, dt = ctx.geom
        dy = dy.contiguous()
        if dy.dtype not in (torch.float32, torch.bfloat16):
            dy = dy.float()
        dx = torch.empty(B * H * W, C, dtype=dt, device=dy.device)
        check(_capi.load().me_maxpool3x3s2_rows_bwd(ptr(dy), dtype_code(dy.dtype), ptr(idx), ptr(dx), dtype_code(dt), B, H, W, C,
                                                    stream_ptr()), "me_maxpool3x3s2_rows_bwd")
        return dx, None, None, None


def max_pool3x3s2_rows(x: torch.Tensor, B: int, H: int, W: int, return_indices: bool = False):
    """MaxPool2d(3, 2, 1) on rows: x [B*H*W, C] -> [B*Ho*Wo, C] of x's dtype, Ho = conv_out_size(H, 2).  With return_indices also
    the winning tap dy * 3 + dx per element (int8; the first tap in (dy, dx) order on ties).  C a multiple of 4."""
    x = _rows("max_pool3x3s2_rows", x, B, H, W)
    y, idx = _MaxPoolFn.apply(x, int(B), int(H), int(W))
    return (y, idx) if return_indices else y


class _ResizeRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, B, h, w, H, W, sy, sx):
        C = x.shape[1]
        y = torch.empty(B * H * W, C, dtype=x.dtype, device=x.device)
        check(_capi.load().me_resize_rows_batched(ptr(x), dtype_code(x.dtype), ptr(y), dtype_code(y.dtype), B, h, w, H, W, C, sy, sx,
                                                  stream_ptr()), "me_resize_rows_batched")
        ctx.geom = (B, h, w, H, W, C, sy, sx, x.dtype)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        B, h, w, H, W, C, sy, sx, dt = ctx.geom
        dy = dy.contiguous()
        if dy.dtype not in (torch.float32, torch.bfloat16):
            dy = dy.float()
        dx = torch.empty(B * h * w, C, dtype=dt, device=dy.device)
        check(_capi.load().me_resize_rows_batched_bwd(ptr(dy), dtype_code(dy.dtype), ptr(dx), dtype_code(dt), B, h, w, H, W, C, sy, sx,
                                                      stream_ptr()), "me_resize_rows_batched_bwd")
        return dx, None, None, None, None, None, None, None


def resize_rows_batched(x: torch.Tensor, B: int, h: int, w: int, scale_factor: Optional[float] = None, size=None) -> torch.Tensor:
    """Bilinear F.interpolate(align_corners=False) on rows: x [B*h*w, C] -> [B*H*W, C] of x's dtype.  Exactly one of
    ``scale_factor`` (H = floor(h * f), sampled with 1 / f: interpolate_geometry) and ``size`` = (H, W) (sampled with h / H).
    C a multiple of 4; the gradient is me_resize_rows_batched_bwd, deterministic."""
    if (scale_factor is None) == (size is None):
        raise MetaEncError("resize_rows_batched: give exactly one of scale_factor and size")
    x = _rows("resize_rows_batched", x, B, h, w)
    if size is not None:
        try:
            H, W = (int(v) for v in size)
        except (TypeError, ValueError) as e:
            raise MetaEncError("resize_rows_batched: size must be (H, W)") from e
        if H < 1 or W < 1:
            raise MetaEncError(f"resize_rows_batched: size = ({H}, {W}) must be positive")
        sy, sx = h / H, w / W
    else:
        (H, sy), (W, sx) = interpolate_geometry(h, scale_factor), interpolate_geometry(w, scale_factor)
        if H < 1 or W < 1:
            raise MetaEncError(f"resize_rows_batched: scale_factor = {scale_factor} leaves no output for a {h} x {w} grid")
    return _ResizeRowsFn.apply(x, int(B), int(h), int(w), H, W, float(sy), float(sx))


class _Upsample2xFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y4, bias, add, B, h, w):
        C = y4.shape[1] // 4
        out = torch.empty(B * 4 * h * w, C, dtype=torch.float32, device=y4.device)
        b32 = bias.detach().float().contiguous() if bias is not None else None
        check(_capi.load().me_upsample2x_rows(ptr(y4), dtype_code(y4.dtype), ptr(b32), ptr(add), dtype_code(add.dtype) if add is not None else 0,
                                              ptr(out), _capi.ME_F32, B, h, w, C, stream_ptr()), "me_upsample2x_rows")
        ctx.geom = (B, h, w, C, y4.dtype, bias.dtype if bias is not None else None, add.dtype if add is not None else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        B, h, w, C, ydt, bdt, adt = ctx.geom
        dout = dout.float().contiguous()
        dy4 = None
        if ctx.needs_input_grad[0]:
            dy4 = torch.empty(B * h * w, 4 * C, dtype=ydt, device=dout.device)
            check(_capi.load().me_upsample2x_rows_bwd(ptr(dout), _capi.ME_F32, ptr(dy4), dtype_code(ydt), B, h, w, C, stream_ptr()),
                  "me_upsample2x_rows_bwd")
        db = ops.colsum(dout).to(bdt) if bdt is not None and ctx.needs_input_grad[1] else None
        da = dout.to(adt) if adt is not None and ctx.needs_input_grad[2] else None
        return dy4, db, da, None, None, None


def conv_transpose2x2_rows(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], B: int, h: int, w: int,
                           add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvTranspose2d(Cin, Cout, 2, 2) on rows, plus an optional second operand: x [B*h*w, Cin] -> fp32 [B*2h*2w, Cout] =
    up(x) + bias (+ add, [B*2h*2w, Cout]).  ``weight`` keeps its checkpoint shape [Cin, Cout, 2, 2].  One GEMM (heads.linear
    against the weight as [(ky, kx, cout), cin]), then me_upsample2x_rows moves every row's four Cout-wide segments to its four
    children; backward is the inverse permutation, me_colsum for the bias and the GEMMs of heads.linear."""
    x = _rows("conv_transpose2x2_rows", x, B, h, w, multiple=8)
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4 or weight.shape[0] != x.shape[1] or tuple(weight.shape[2:]) != (2, 2):
        raise MetaEncError(f"conv_transpose2x2_rows: weight must be [{x.shape[1]}, Cout, 2, 2]"
                           + (f" (got {tuple(weight.shape)})" if isinstance(weight, torch.Tensor) else ""))
    Cin, Cout = weight.shape[:2]
    if Cout % 4:
        raise MetaEncError(f"conv_transpose2x2_rows: Cout = {Cout} must be a multiple of 4")
    if bias is not None and tuple(bias.shape) != (Cout,):
        raise MetaEncError(f"conv_transpose2x2_rows: bias must be [{Cout}] (got {tuple(bias.shape)})")
    if add is not None:
        if not isinstance(add, torch.Tensor) or tuple(add.shape) != (4 * x.shape[0], Cout):
            raise MetaEncError(f"conv_transpose2x2_rows: add must be [{4 * x.shape[0]}, {Cout}] rows of the 2h x 2w grid")
        add = (add.float() if add.dtype not in (torch.float32, torch.bfloat16) else add).contiguous()
    _require_one_gpu("conv_transpose2x2_rows", x=x, weight=weight, bias=bias, add=add)
    y4 = linear(x, weight.permute(2, 3, 1, 0).reshape(4 * Cout, Cin), None)
    return _Upsample2xFn.apply(y4, bias, add, int(B), int(h), int(w))


def _autocast_rows(rows: torch.Tensor) -> torch.Tensor:
    """under torch.autocast the convolutions and their Linears compute in bf16, as Block and PatchEmbed do (fp16 autocast runs on
    the bf16 kernels too); outside it the rows' own dtype decides"""
    if torch.is_autocast_enabled() and rows.dtype != torch.bfloat16:
        return rows.to(torch.bfloat16)
    return rows


def _check_image(who: str, x) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise MetaEncError(f"{who}: expected an image batch [B, C, H, W]" + (f", got shape {tuple(x.shape)}" if isinstance(x, torch.Tensor) else ""))
    if not x.is_cuda:
        raise MetaEncError(f"{who}: input is a CPU tensor: CUDA tensors required (no CPU fallback)")
    if not x.is_floating_point():
        raise MetaEncError(f"{who}: input must be a floating-point tensor (got {x.dtype})")


def _image_rows(who: str, x) -> torch.Tensor:
    """a channel-first image batch [B, C, H, W] as rows [B*H*W, C] (the one layout change on the way in)"""
    _check_image(who, x)
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _rows_to_image(rows: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    return rows.view(B, H, W, rows.shape[-1]).permute(0, 3, 1, 2).contiguous()


class SpatialPriorModule(nn.Module):
    """The convolutional stem that gives the adapter its 1/4 .. 1/32 pyramid (adapter_modules.SpatialPriorModule by interface:
    constructor, state-dict keys ``stem.{0,1,3,4,6,7}``, ``conv{2,3,4}.{0,1}``, ``fc{1..4}`` with the convolution weights in their
    [Cout, Cin, k, k] checkpoint shape, and the return values).  Everything between the input image and the results stays in
    rows: the 3x3 convolutions are conv3x3_rows, the pool max_pool3x3s2_rows, the four 1x1 convolutions heads.linear.  The norms
    are the nn.SyncBatchNorm modules themselves, called on [rows, C] (channel at dim 1): batch statistics, running-statistic
    updates and the cross-rank synchronisation are PyTorch's; ReLU is PyTorch glue.  Under torch.autocast every convolution
    reads bf16 rows (bf16 GEMM, fp32 result), so the norms and the pool stay fp32."""

    def __init__(self, inplanes=64, embed_dim=384):
        super().__init__()
        def conv(cin, cout, stride):
            return [nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False), nn.SyncBatchNorm(cout), nn.ReLU(inplace=True)]
        self.stem = nn.Sequential(*conv(3, inplanes, 2), *conv(inplanes, inplanes, 1), *conv(inplanes, inplanes, 1),
                                  nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        self.conv2 = nn.Sequential(*conv(inplanes, 2 * inplanes, 2))
        self.conv3 = nn.Sequential(*conv(2 * inplanes, 4 * inplanes, 2))
        self.conv4 = nn.Sequential(*conv(4 * inplanes, 4 * inplanes, 2))
        self.fc1 = nn.Conv2d(inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)
        self.fc2 = nn.Conv2d(2 * inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)
        self.fc3 = nn.Conv2d(4 * inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)
        self.fc4 = nn.Conv2d(4 * inplanes, embed_dim, kernel_size=1, stride=1, padding=0, bias=True)

    @staticmethod
    def _unit(seq, at, rows, B, H, W):
        """convolution seq[at], norm seq[at + 1], ReLU -> (rows, Ho, Wo)"""
        s = seq[at].stride[0]
        y = F.relu(seq[at + 1](conv3x3_rows(_autocast_rows(rows), seq[at].weight, B, H, W, s)))
        return y, conv_out_size(H, s), conv_out_size(W, s)

    @staticmethod
    def _fc(fc, rows):
        return linear(_autocast_rows(rows), fc.weight.reshape(fc.weight.shape[0], -1), fc.bias)

    def forward_rows(self, x):
        """x [B, 3, H, W] -> (c1 rows [B*H1*W1, D], c2 [B, H2 W2, D], c3, c4, (H1, W1)): forward() with c1 left as rows of the
        stride-4 grid"""
        rows = _image_rows("SpatialPriorModule", x)
        if rows.dtype == torch.float16:
            rows = rows.float()
        B, _, H, W = x.shape
        y, H, W = self._unit(self.stem, 0, rows.contiguous(), B, H, W)
        y, H, W = self._unit(self.stem, 3, y, B, H, W)
        y, H, W = self._unit(self.stem, 6, y, B, H, W)
        c1 = max_pool3x3s2_rows(y, B, H, W)
        H1, W1 = conv_out_size(H, 2), conv_out_size(W, 2)
        c2, H2, W2 = self._unit(self.conv2, 0, c1, B, H1, W1)
        c3, H3, W3 = self._unit(self.conv3, 0, c2, B, H2, W2)
        c4, _, _ = self._unit(self.conv4, 0, c3, B, H3, W3)
        D = self.fc1.weight.shape[0]
        return (self._fc(self.fc1, c1), self._fc(self.fc2, c2).view(B, -1, D), self._fc(self.fc3, c3).view(B, -1, D),
                self._fc(self.fc4, c4).view(B, -1, D), (H1, W1))

    def forward(self, x):
        """-> (c1 [B, D, H/4, W/4] channel-first, c2 [B, H/8 W/8, D], c3 [B, H/16 W/16, D], c4 [B, H/32 W/32, D] tokens)"""
        c1, c2, c3, c4, (H1, W1) = self.forward_rows(x)
        return _rows_to_image(c1, x.shape[0], H1, W1), c2, c3, c4


class _PosResizeFn(torch.autograd.Function):
    """the bicubic resize of the pos-embed grid (me_resize_rows) with a gradient: the resize is a fixed linear map R, so
    d table = R^T d pos, with R itself read off the kernel (the identity table resized) and the product on me_gemm TN"""

    _matrices = {}      # (h, w, H, W, device) -> R, zero-padded to multiples of 8 both ways

    @staticmethod
    def forward(ctx, table, hw, HW):
        ctx.geom = (hw, HW, table.dtype)
        return ops.resize_rows(table.detach().float().contiguous(), hw, HW, "bicubic")

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpos):
        (h, w), (H, W), dt = ctx.geom
        n, N = h * w, H * W
        npad, Npad = (n + 7) // 8 * 8, (N + 7) // 8 * 8
        key = (h, w, H, W, dpos.device)
        R = _PosResizeFn._matrices.get(key)
        if R is None:
            eye = torch.zeros(n, npad, dtype=torch.float32, device=dpos.device)
            eye.fill_diagonal_(1.0)
            R = torch.zeros(Npad, npad, dtype=torch.float32, device=dpos.device)
            R[:N] = ops.resize_rows(eye, (h, w), (H, W), "bicubic")
            if len(_PosResizeFn._matrices) >= 8:          # a training run sees a handful of image sizes; keep the cache small
                _PosResizeFn._matrices.clear()
            _PosResizeFn._matrices[key] = R
        d = torch.zeros(Npad, dpos.shape[1], dtype=torch.float32, device=dpos.device)
        d[:N] = dpos
        return ops.gemm(R, d, op=_capi.ME_GEMM_TN, out_dtype=torch.float32)[:n].to(dt), None, None


class _AdapterPatchEmbed(PatchEmbed):
    """PatchEmbed for images of any size that the patch divides (the backbone runs at the data pipeline's sizes)"""

    def _check_input(self, x):
        p = self.patch_size[0]
        if x.shape[-2] % p or x.shape[-1] % p:
            raise MetaEncError(f"ViTAdapter: image {x.shape[-2]} x {x.shape[-1]} is not a multiple of the patch size {p}")


class _Checkpointed:
    """blk(x, H, W) recomputed in backward (the with_cp of the reference's Block); a plain callable, not a registered module"""

    def __init__(self, blk):
        self.blk = blk

    def __call__(self, x, H, W):
        if x.requires_grad:
            return cp.checkpoint(self.blk, x, H, W, use_reentrant=False)
        return self.blk(x, H, W)


class ViTAdapter(nn.Module):
    """The ViT-Adapter backbone of the Image detection and segmentation recipes (vit_adapter.ViTAdapter on TIMMVisionTransformer,
    by interface): constructor arguments, state-dict keys (``pos_embed``, ``patch_embed.proj.*``, ``blocks.*``, ``level_embed``,
    ``spm.*``, ``interactions.*``, ``up.*``, ``norm{1..4}.*``; no ``cls_token``), initial distributions and the forward:
    image [B, 3, H, W] (H and W multiples of 32) -> [f1, f2, f3, f4], channel-first fp32 maps of ``embed_dim`` channels at
    strides 4, 8, 16 and 32.

    The spatial prior module, the up-sampling ``up`` (conv_transpose2x2_rows, with the ``+ c1`` fused), the three bilinear
    resizes of the ViT tokens (resize_rows_batched) and the four output norms all work on token rows; the four results are
    permuted to channel-first once, at the end.  The encoder blocks are this package's ``Block``s, the interactions its
    ``InteractionBlock``s.  The SyncBatchNorm modules run as they are, on [rows, C].

    ``pretrained`` is a state dict (or an object with one under ``state_dict`` / ``model``) or a path for torch.load; it is
    loaded non-strict, a ``pos_embed`` of another grid size resized first, as TIMMVisionTransformer.init_weights does.
    As in the reference the position grid is ``pretrain_size // 16`` squared and the pyramid strides assume ``patch_size`` 16.

    The two reference copies differ in three places.  The segmentation copy (mmseg_custom) takes ``pretrained`` and ``with_cp``
    explicitly and hands ``with_cp`` to the interaction blocks too (here: always).  And with ``add_vit_feature`` it adds, to
    f1 .. f4, the ViT tokens as they stand after interaction 1 .. 4 (so it needs exactly four interactions), where the
    detection copy adds the final tokens to all four: ``vit_feature_per_interaction=True`` selects the segmentation form."""

    def __init__(self, pretrain_size=224, num_heads=12, conv_inplane=64, n_points=4, deform_num_heads=6, init_values=0.,
                 interaction_indexes=None, with_cffn=True, cffn_ratio=0.25, deform_ratio=1.0, add_vit_feature=True, pretrained=None,
                 use_extra_extractor=True, with_cp=False, img_size=None, patch_size=16, in_chans=3, residual_indices=(), embed_dim=768,
                 depth=12, mlp_ratio=4., qkv_bias=True, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., layer_scale=True,
                 norm_layer=None, act_layer=None, window_attn=False, window_size=14, vit_feature_per_interaction=False):
        super().__init__()
        if patch_size != 16:
            raise MetaEncError(f"ViTAdapter: patch_size = {patch_size}: the pyramid strides and the position grid assume 16, as the reference's do")
        if in_chans != 3:
            raise MetaEncError(f"ViTAdapter: in_chans = {in_chans}: the spatial prior module reads 3 channels")
        if residual_indices:
            raise MetaEncError("ViTAdapter: residual_indices (ResBottleneckBlock in the encoder) is not implemented")
        if not interaction_indexes:
            raise MetaEncError("ViTAdapter: interaction_indexes = [[first block, last block], ...] is required")
        img_size = pretrain_size if img_size is None else img_size
        if img_size != pretrain_size:
            raise MetaEncError(f"ViTAdapter: img_size = {img_size} and pretrain_size = {pretrain_size} must agree (one position table)")
        for first, last in interaction_indexes:
            if not 0 <= first <= last < depth:
                raise MetaEncError(f"ViTAdapter: interaction_indexes entry [{first}, {last}] is not a block range of depth {depth}")
        if vit_feature_per_interaction and add_vit_feature and len(interaction_indexes) != 4:
            raise MetaEncError("ViTAdapter: vit_feature_per_interaction needs exactly four interactions")
        norm_layer = norm_layer or _ADAPTER_NORM
        act_layer = act_layer or nn.GELU
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 1
        self.norm_layer, self.act_layer = norm_layer, act_layer
        self.drop_path_rate, self.drop_rate = drop_path_rate, drop_rate
        self.img_size, self.patch_size = (img_size, img_size), patch_size
        self.interpolate_mode = "bicubic"
        self.pretrain_size = (pretrain_size, pretrain_size)
        self.interaction_indexes = [list(p) for p in interaction_indexes]
        self.add_vit_feature = bool(add_vit_feature)
        self.vit_feature_per_interaction = bool(vit_feature_per_interaction)
        self.with_cp = bool(with_cp)
        self.cls_token = None
        windowed = list(window_attn) if isinstance(window_attn, (list, tuple)) else [window_attn] * depth
        sizes = list(window_size) if isinstance(window_size, (list, tuple)) else [window_size] * depth
        if len(windowed) != depth or len(sizes) != depth:
            raise MetaEncError(f"ViTAdapter: window_attn / window_size lists must have depth = {depth} entries")
        self.patch_embed = _AdapterPatchEmbed(img_size=img_size, patch_size=patch_size, in_c=in_chans, embed_dim=embed_dim)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + self.num_tokens, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.Sequential(*[Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                                            attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, act_layer=act_layer,
                                            windowed=bool(windowed[i]), window_size=sizes[i] if sizes[i] else 14, layer_scale=layer_scale)
                                      for i in range(depth)])
        self.num_block = depth
        self._cp_blocks = [_Checkpointed(b) for b in self.blocks] if self.with_cp else None
        self.level_embed = nn.Parameter(torch.zeros(3, embed_dim))
        self.spm = SpatialPriorModule(inplanes=conv_inplane, embed_dim=embed_dim)
        n = len(self.interaction_indexes)
        self.interactions = nn.Sequential(*[
            InteractionBlock(dim=embed_dim, num_heads=deform_num_heads, n_points=n_points, init_values=init_values,
                             drop_path=drop_path_rate, norm_layer=norm_layer, with_cffn=with_cffn, cffn_ratio=cffn_ratio,
                             deform_ratio=deform_ratio, extra_extractor=(i == n - 1 and bool(use_extra_extractor)), with_cp=with_cp)
            for i in range(n)])
        self.up = nn.ConvTranspose2d(embed_dim, embed_dim, 2, 2)
        self.norm1, self.norm2 = nn.SyncBatchNorm(embed_dim), nn.SyncBatchNorm(embed_dim)
        self.norm3, self.norm4 = nn.SyncBatchNorm(embed_dim), nn.SyncBatchNorm(embed_dim)
        self.up.apply(self._init_weights)
        self.spm.apply(self._init_weights)
        self.interactions.apply(self._init_weights)
        self.apply(self._init_deform_weights)
        nn.init.normal_(self.level_embed)
        self.init_weights(pretrained)

    def _init_weights(self, m):
        """Linear: truncated normal(std 0.02), zero bias; LayerNorm / BatchNorm2d: one and zero; Conv2d / ConvTranspose2d:
        normal(0, sqrt(2 / fan_out)) with fan_out = k k out_channels / groups, zero bias (vit_adapter.py:58-71)"""
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.LayerNorm, nn.BatchNorm2d)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels // m.groups
            m.weight.data.normal_(0, math.sqrt(2.0 / fan_out))
            if m.bias is not None:
                m.bias.data.zero_()

    def _init_deform_weights(self, m):
        if isinstance(m, MSDeformAttn):
            m._reset_parameters()

    def init_weights(self, pretrained=None):
        """load ``pretrained`` (None: nothing) non-strict; returns load_state_dict's (missing, unexpected) report"""
        if pretrained is None:
            return None
        if isinstance(pretrained, (str, bytes)) or hasattr(pretrained, "__fspath__"):
            pretrained = torch.load(pretrained, map_location="cpu", weights_only=True)
        if isinstance(pretrained, nn.Module):
            pretrained = pretrained.state_dict()
        if not isinstance(pretrained, dict):
            raise MetaEncError(f"ViTAdapter: pretrained must be a state dict or a path (got {type(pretrained).__name__})")
        for key in ("state_dict", "model"):
            if key in pretrained and isinstance(pretrained[key], dict):
                pretrained = pretrained[key]
        sd = dict(pretrained)
        pe = sd.get("pos_embed")
        if pe is not None and pe.shape != self.pos_embed.shape:
            side = int(math.sqrt(pe.shape[1] - 1))
            if side * side != pe.shape[1] - 1 or pe.shape[-1] != self.embed_dim:
                raise MetaEncError(f"ViTAdapter: pretrained pos_embed {tuple(pe.shape)} is not a cls row plus a square grid of width {self.embed_dim}")
            g = self.img_size[0] // self.patch_size
            grid = pe[:, 1:].float().reshape(1, side, side, -1).permute(0, 3, 1, 2)
            grid = F.interpolate(grid, size=(g, g), mode="bicubic", align_corners=False)      # (a one-off at load time, on the CPU)
            sd["pos_embed"] = torch.cat([pe[:, :1].float(), grid.flatten(2).transpose(1, 2)], dim=1)
        return self.load_state_dict(sd, strict=False)

    def _get_pos_embed(self, H, W):
        """the position table without its cls row, resampled (bicubic) from the pretrain grid to H x W: [1, H W, D]"""
        g = (self.pretrain_size[0] // 16, self.pretrain_size[1] // 16)
        table = self.pos_embed[0, 1:]
        if g == (H, W):
            return table.unsqueeze(0)
        return _PosResizeFn.apply(table, g, (H, W)).unsqueeze(0)

    def _add_level_embed(self, c2, c3, c4):
        return c2 + self.level_embed[0], c3 + self.level_embed[1], c4 + self.level_embed[2]

    def forward(self, x):
        _check_image("ViTAdapter", x)
        B, Cimg, Himg, Wimg = x.shape
        if Cimg != 3:
            raise MetaEncError(f"ViTAdapter: the image has {Cimg} channels, 3 expected")
        if Himg % 32 or Wimg % 32 or min(Himg, Wimg) < 32:
            raise MetaEncError(f"ViTAdapter: image {Himg} x {Wimg}: height and width must be multiples of 32")
        d1, d2 = deform_inputs(x)
        c1, c2, c3, c4, _ = self.spm.forward_rows(x)
        c2, c3, c4 = self._add_level_embed(c2, c3, c4)
        n2, n3 = c2.shape[1], c3.shape[1]
        c = torch.cat([c2, c3, c4], dim=1)
        H, W = Himg // 16, Wimg // 16
        tok = self.patch_embed(x)
        D = tok.shape[-1]
        tok = self.pos_drop(tok.float() + self._get_pos_embed(H, W))
        outs = []
        for layer, (first, last) in zip(self.interactions, self.interaction_indexes):
            blocks = self._cp_blocks[first:last + 1] if self.with_cp and torch.is_grad_enabled() else self.blocks[first:last + 1]
            tok, c = layer(tok, c, blocks, d1, d2, H, W)
            outs.append(tok)
        c2 = c[:, :n2].reshape(-1, D)
        c3 = c[:, n2:n2 + n3].reshape(-1, D)
        c4 = c[:, n2 + n3:].reshape(-1, D)
        c1 = conv_transpose2x2_rows(_autocast_rows(c2), self.up.weight, self.up.bias, B, 2 * H, 2 * W, add=c1)
        if self.add_vit_feature:
            x1, x2, x3, x4 = (t.reshape(-1, D).float() for t in (outs if self.vit_feature_per_interaction else [tok] * 4))
            c1 = c1 + resize_rows_batched(x1, B, H, W, scale_factor=4)
            c2 = c2 + resize_rows_batched(x2, B, H, W, scale_factor=2)
            c3 = c3 + x3
            c4 = c4 + resize_rows_batched(x4, B, H, W, scale_factor=0.5)
        f1 = _rows_to_image(self.norm1(c1), B, 4 * H, 4 * W)
        f2 = _rows_to_image(self.norm2(c2), B, 2 * H, 2 * W)
        f3 = _rows_to_image(self.norm3(c3), B, H, W)
        f4 = _rows_to_image(self.norm4(c4), B, H // 2, W // 2)
        return [f1, f2, f3, f4]
