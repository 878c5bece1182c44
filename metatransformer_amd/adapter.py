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

from . import _capi
from ._capi import MetaEncError, check, ptr, stream_ptr
from .heads import _LayerNormFn, linear

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
