"""VideoMAE masked pre-training on the HIP path (Video/models/modeling_pretrain.py:28-360, Video/engine_for_pretraining.py:57-113).

The reference embeds every tubelet of a clip and throws the masked 90 % away (``x[~mask]``), and builds the per-patch normalised pixel
target of the whole clip from five full-size temporaries.  Here only what is used is touched:

  PretrainVisionTransformerEncoder   me_tubelet_gather writes the tubelets of the VISIBLE tokens as GEMM rows (10 % of the clip at the
      usual mask ratio), one me_gemm projects them with the bias and the gathered position rows as its epilogue, then the Blocks
  PretrainVisionTransformerDecoder   Blocks, then ``norm`` + ``head`` on the decoded rows only
  PretrainVisionTransformer          encoder -> ``encoder_to_decoder`` -> me_mae_assemble_fwd (visible tokens + position rows, mask tokens
      + position rows, one launch) -> decoder
  mae_reconstruction_loss            me_mae_loss: target and masked mean-squared error of the decoded patches in one pass

Constructor arguments, attribute names and ``forward(x, mask, decode_mask=None)`` are the reference's; ``convert_video_state_dict`` of a
reference state dict loads with ``strict=True`` and ``to_video_state_dict`` gives the reference keys back.

Index lists: ``vis_idx`` / ``dec_idx`` are built on the device from the bool masks by a stable sort -- ascending position, which is what
boolean indexing yields.  Their lengths are shapes, so ONE host read of the per-sample counts happens per call (``token_indices``);
unequal counts raise, as the reference's ``reshape(B, -1, C)`` would fail.  Everything else stays on the stream.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _capi, ops
from ._capi import MetaEncError, check, dtype_code, ptr, stream_ptr
from .data2seq import VideoPatchEmbed, _boundary_dtypes, video_sinusoid_table
from .encoder import Block
from .linear import linear, pad_to, wgrad

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


# ----------------------------------------------------------------------------------------------------------------- index lists

def _check_mask(who: str, m: torch.Tensor, B: int, N: int, device, name: str) -> torch.Tensor:
    if not isinstance(m, torch.Tensor) or not m.is_cuda:
        raise MetaEncError(f"{who}: {name} must be a CUDA tensor (no CPU fallback)")
    if m.device != device:
        raise MetaEncError(f"{who}: {name} is on {m.device}, the clip on {device}: move it first (no implicit copies)")
    if m.dtype != torch.bool:
        raise MetaEncError(f"{who}: {name} must be a bool tensor (got {m.dtype})")
    if m.dim() != 2 or m.shape[0] != B or m.shape[1] != N:
        raise MetaEncError(f"{who}: {name} {tuple(m.shape)} must be [{B}, {N}] (one entry per tubelet)")
    return m


def token_indices(who: str, *selections: torch.Tensor):
    """For each bool ``[B, N]`` selection the int32 ``[B, n]`` list of its True positions, ascending per sample (a stable sort of the
    flags: the order boolean indexing yields).  The counts of all selections are read to the host in ONE copy -- they are the shapes of
    what follows; a selection whose samples disagree raises."""
    counts = torch.stack([s.sum(dim=1) for s in selections]).tolist()           # the one host read
    out = []
    for s, c in zip(selections, counts):
        if min(c) != max(c):
            raise MetaEncError(f"{who}: the samples select different numbers of tokens ({sorted(set(int(v) for v in c))}); "
                               "every sample of a batch must keep the same count")
        order = torch.sort((~s).to(torch.uint8), dim=1, stable=True).indices
        out.append(order[:, :int(c[0])].to(torch.int32).contiguous())
    return out


def mae_index_lists(mask: torch.Tensor, decode_mask: Optional[torch.Tensor] = None, who: str = "mae_index_lists"):
    """(vis_idx [B, Nvis], dec_idx [B, Ndec], w [B, Ndec] fp32) of a pre-training step: the visible positions ``~mask``, the decoded
    positions ``mask`` -- or ``~decode_mask`` when a decoder mask is given (modeling_pretrain.py:341) -- and the loss weights
    ``mask[decoded positions]`` (engine_for_pretraining.py:104: ``cal_loss_mask``)."""
    dec = mask if decode_mask is None else ~decode_mask
    vis_idx, dec_idx = token_indices(who, ~mask, dec)
    w = torch.gather(mask, 1, dec_idx.long()).to(torch.float32)
    return vis_idx, dec_idx, w


# ----------------------------------------------------------------------------------------------------------------- the kernels

def _clip(who: str, video: torch.Tensor) -> torch.Tensor:
    if not isinstance(video, torch.Tensor) or not video.is_cuda:
        raise MetaEncError(f"{who} runs on MI355X only (CPU tensor given; no CPU fallback)")
    if video.dim() != 5:
        raise MetaEncError(f"{who}: clip {tuple(video.shape)} must be [B, C, T, H, W]")
    if video.requires_grad:
        raise MetaEncError(f"{who}: gradient w.r.t. the clip is not implemented (pre-training needs none); detach the input")
    if video.dtype == torch.float16:
        video = ops.cast(video.contiguous(), torch.bfloat16)
    elif video.dtype == torch.float64:
        video = video.float()
    if video.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"{who}: clip dtype {video.dtype} unsupported (fp32, bf16; fp64 / fp16 are converted)")
    return video.contiguous()


def _idx(who: str, idx: torch.Tensor, device) -> torch.Tensor:
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2 or idx.is_floating_point() or idx.dtype == torch.bool:
        raise MetaEncError(f"{who}: an index list must be an integer tensor [B, n]")
    if idx.device != device:
        raise MetaEncError(f"{who}: the index list is on {idx.device}, the data on {device}: move it first (no implicit copies)")
    return idx.to(torch.int32).contiguous()


def tubelet_gather(video: torch.Tensor, idx: torch.Tensor, tubelet: Tuple[int, int, int], out_dtype: Optional[torch.dtype] = None,
                   pad_cols_to: int = 1, pad_rows_to: int = 1) -> torch.Tensor:
    """me_tubelet_gather: rows ``[B * n, Cin kt kh kw]`` of the tubelets ``idx [B, n]`` of ``video [B, Cin, T, H, W]``, columns in the
    order of the flattened Conv3d weight.  ``pad_cols_to`` / ``pad_rows_to`` round the matrix up with zero columns / rows (the GEMM's
    granules); the result then has the padded shape."""
    who = "tubelet_gather"
    video = _clip(who, video)
    idx = _idx(who, idx, video.device)
    B, Cin, T, H, W = video.shape
    kt, kh, kw = (int(v) for v in tubelet)
    if idx.shape[0] != B:
        raise MetaEncError(f"{who}: index list {tuple(idx.shape)} for a batch of {B}")
    K, M = Cin * kt * kh * kw, B * idx.shape[1]
    Kp, Mp = -(-K // pad_cols_to) * pad_cols_to, -(-M // pad_rows_to) * pad_rows_to
    odt = out_dtype or video.dtype
    out = (torch.zeros if (Kp != K or Mp != M) else torch.empty)((Mp, Kp), dtype=odt, device=video.device)
    check(_capi.load().me_tubelet_gather(ptr(video), dtype_code(video.dtype), ptr(idx), ptr(out), dtype_code(odt), Kp, B, Cin, T, H, W, kt, kh, kw,
                                         idx.shape[1], stream_ptr()), "me_tubelet_gather")
    return out


def take_rows(table: torch.Tensor, idx: torch.Tensor, add: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """me_take_rows: ``out[b, j] = table[idx[b, j]] (+ add)`` -> ``[B, n, C]``; table ``[rows, C]`` fp32 or bf16, add ``[C]``."""
    who = "take_rows"
    if not isinstance(table, torch.Tensor) or not table.is_cuda or table.dim() != 2 or table.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"{who}: the table must be a CUDA fp32 / bf16 matrix [rows, C]")
    idx = _idx(who, idx, table.device)
    table = table if table.stride(1) == 1 else table.contiguous()
    rows, C = table.shape
    a32 = None if add is None else ops._f32(add.detach()).reshape(-1).contiguous()
    if a32 is not None and a32.numel() != C:
        raise MetaEncError(f"{who}: add has {a32.numel()} elements, the table {C} columns")
    B, n = idx.shape
    out = torch.empty((B, n, C), dtype=out_dtype or table.dtype, device=table.device)
    check(_capi.load().me_take_rows(ptr(table), dtype_code(table.dtype), table.stride(0), rows, ptr(idx), ptr(a32), ptr(out), dtype_code(out.dtype), C,
                                    B, n, C, stream_ptr()), "me_take_rows")
    return out


def mae_assemble(xv: torch.Tensor, pos: torch.Tensor, vis_idx: torch.Tensor, dec_idx: torch.Tensor, mask_token: torch.Tensor,
                 out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """me_mae_assemble_fwd: ``cat(xv + pos[vis_idx], mask_token + pos[dec_idx])`` -> ``[B, Nvis + Ndec, Cd]`` (no autograd)."""
    who = "mae_assemble"
    if not isinstance(xv, torch.Tensor) or not xv.is_cuda or xv.dim() != 3 or xv.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"{who}: xv must be CUDA fp32 / bf16 tokens [B, Nvis, Cd]")
    xv = xv.contiguous()
    B, Nvis, Cd = xv.shape
    vis_idx, dec_idx = _idx(who, vis_idx, xv.device), _idx(who, dec_idx, xv.device)
    p32 = ops._f32(pos.detach()).reshape(-1, Cd).contiguous()
    t32 = ops._f32(mask_token.detach()).reshape(Cd).contiguous()
    if tuple(vis_idx.shape) != (B, Nvis) or dec_idx.shape[0] != B:
        raise MetaEncError(f"{who}: vis_idx {tuple(vis_idx.shape)} / dec_idx {tuple(dec_idx.shape)} for xv {tuple(xv.shape)}")
    Ndec = dec_idx.shape[1]
    out = torch.empty((B, Nvis + Ndec, Cd), dtype=out_dtype or xv.dtype, device=xv.device)
    check(_capi.load().me_mae_assemble_fwd(ptr(xv), dtype_code(xv.dtype), Cd, ptr(p32), Cd, p32.shape[0], ptr(vis_idx), ptr(dec_idx), ptr(t32),
                                           ptr(out), dtype_code(out.dtype), Cd, B, Nvis, Ndec, Cd, stream_ptr()), "me_mae_assemble_fwd")
    return out


def mae_assemble_bwd(dx_full: torch.Tensor, Nvis: int, dxv_dtype: Optional[torch.dtype] = None, want_dxv: bool = True, want_dmask: bool = True):
    """me_mae_assemble_bwd: ``dx_full [B, Nvis + Ndec, Cd]`` -> (dxv ``[B, Nvis, Cd]`` or None, dmask_token fp32 ``[Cd]`` or None)."""
    if not dx_full.is_cuda or dx_full.dim() != 3 or dx_full.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError("mae_assemble_bwd: dx_full must be CUDA fp32 / bf16 [B, Nvis + Ndec, Cd]")
    lib = _capi.load()
    dx_full = dx_full.contiguous()
    B, Nf, Cd = dx_full.shape
    Ndec = Nf - Nvis
    if Nvis < 0 or Ndec < 0:
        raise MetaEncError(f"mae_assemble_bwd: Nvis={Nvis} of {Nf} rows")
    dxv = torch.empty((B, Nvis, Cd), dtype=dxv_dtype or dx_full.dtype, device=dx_full.device) if want_dxv else None
    dmask = torch.empty(Cd, dtype=torch.float32, device=dx_full.device) if want_dmask else None
    nbytes = lib.me_mae_assemble_bwd_workspace(B, Ndec, Cd) if want_dmask else 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dx_full.device)
    check(lib.me_mae_assemble_bwd(ptr(dx_full), dtype_code(dx_full.dtype), Cd, ptr(dxv), dtype_code(dxv.dtype) if want_dxv else 0, Cd, ptr(dmask), B,
                                  Nvis, Ndec, Cd, ptr(ws), nbytes, stream_ptr()), "me_mae_assemble_bwd")
    return dxv, dmask


_stat_cache = {}


def _channel_stats(mean, std, Cin: int, device):
    key = (tuple(float(v) for v in mean), tuple(float(v) for v in std), str(device))
    if key not in _stat_cache:
        if len(key[0]) != Cin or len(key[1]) != Cin:
            raise MetaEncError(f"mae loss: mean / std have {len(key[0])} / {len(key[1])} entries, the clip {Cin} channels")
        _stat_cache[key] = (torch.tensor(key[0], dtype=torch.float32, device=device), torch.tensor(key[1], dtype=torch.float32, device=device))
    return _stat_cache[key]


def mae_loss_terms(pred: torch.Tensor, video: torch.Tensor, dec_idx: torch.Tensor, w: torch.Tensor, tubelet: Tuple[int, int, int],
                   normalize_target: bool = True, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, grad_scale: Optional[torch.Tensor] = None,
                   want_loss: bool = True, want_labels: bool = False, want_dpred: bool = False) -> dict:
    """me_mae_loss as it is (no autograd): dict with ``loss`` (fp32 scalar) and ``tok_loss`` fp32 ``[B, Ndec]`` (want_loss), ``wsum``
    (fp32 scalar), ``labels`` fp32 ``[B, Ndec, cols]`` (want_labels) and ``dpred`` in pred's dtype (want_dpred; scaled by the device
    scalar ``grad_scale`` when given).  ``pred [B, Ndec, kt kh kw Cin]`` fp32 or bf16, ``w [B, Ndec]`` the loss weights."""
    who = "mae_loss"
    video = _clip(who, video)
    B, Cin, T, H, W = video.shape
    kt, kh, kw = (int(v) for v in tubelet)
    cols = kt * kh * kw * Cin
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda or pred.device != video.device:
        raise MetaEncError(f"{who}: pred must be a CUDA tensor on the clip's device (no CPU fallback)")
    dec_idx = _idx(who, dec_idx, video.device)
    Ndec = dec_idx.shape[1]
    if pred.dim() != 3 or tuple(pred.shape) != (B, Ndec, cols):
        raise MetaEncError(f"{who}: pred {tuple(pred.shape)} must be [{B}, {Ndec}, {cols}] (decoded tokens x kt kh kw C)")
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise MetaEncError(f"{who}: pred dtype {pred.dtype} unsupported (fp32, bf16)")
    pred = pred.contiguous()
    w32 = w.to(torch.float32).contiguous()
    if tuple(w32.shape) != (B, Ndec) or w32.device != video.device:
        raise MetaEncError(f"{who}: weights {tuple(w32.shape)} on {w32.device} must be [{B}, {Ndec}] on {video.device}")
    m, s = _channel_stats(mean, std, Cin, video.device)
    dev = video.device
    tok = torch.empty((B, Ndec), dtype=torch.float32, device=dev) if want_loss else None
    scalars = torch.zeros(2, dtype=torch.float32, device=dev)
    labels = torch.empty((B, Ndec, cols), dtype=torch.float32, device=dev) if want_labels else None
    dpred = torch.empty_like(pred) if want_dpred else None
    g = None
    if grad_scale is not None:
        g = grad_scale.detach().to(torch.float32).reshape(1).contiguous()
    check(_capi.load().me_mae_loss(ptr(video), dtype_code(video.dtype), B, Cin, T, H, W, kt, kh, kw, ptr(m), ptr(s), ptr(dec_idx), ptr(w32), Ndec,
                                   ptr(pred), dtype_code(pred.dtype), cols, 1 if normalize_target else 0, ptr(g), ptr(tok), ptr(scalars), ptr(labels),
                                   cols, ptr(dpred), cols, stream_ptr()), "me_mae_loss")
    res = {"wsum": scalars[1]}
    if want_loss:
        res["loss"], res["tok_loss"] = scalars[0], tok
    if want_labels:
        res["labels"] = labels
    if want_dpred:
        res["dpred"] = dpred
    return res


# ----------------------------------------------------------------------------------------------------------------- autograd

class _VisibleEmbedFn(torch.autograd.Function):
    """tubelet projection of the visible tokens: me_tubelet_gather -> me_gemm (bias and the gathered position rows in its epilogue).
    Backward: dW = dY^T X as one TN GEMM on the SAVED gathered matrix, db = colsum(dY); the clip and the position table are data."""

    @staticmethod
    def forward(ctx, video, vis_idx, weight, bias, pos, tubelet, cdt, odt):
        B, Nvis = vis_idx.shape
        C = weight.shape[0]
        K = weight[0].numel()
        M = B * Nvis
        xg = tubelet_gather(video, vis_idx, tubelet, out_dtype=cdt, pad_cols_to=8, pad_rows_to=8)       # zero rows / columns pad to the GEMM granules
        wc = pad_to(ops.cast(weight.detach().reshape(C, K).contiguous(), cdt), 1)
        pos_rows = take_rows(ops._f32(pos.detach()).reshape(-1, C), vis_idx, out_dtype=torch.float32).view(M, C)
        kdt = torch.bfloat16 if odt == torch.float16 else odt
        b32 = None if bias is None else ops._f32(bias.detach()).contiguous()
        y = ops.gemm(xg[:M], wc, bias=b32, residual=pos_rows, out_dtype=kdt)
        ctx.save_for_backward(xg)
        ctx.meta = (M, K, tuple(weight.shape), weight.dtype, None if bias is None else bias.dtype)
        y = y if kdt == odt else ops.cast(y, odt)
        return y.view(B, Nvis, C)

    @staticmethod
    def backward(ctx, dy):
        (xg,) = ctx.saved_tensors
        M, K, wshape, wdt, bdt = ctx.meta
        C = wshape[0]
        d2 = dy.reshape(M, C).contiguous()
        if d2.dtype == torch.float16:
            d2 = ops.cast(d2, torch.bfloat16)
        d2 = pad_to(ops.cast(d2, xg.dtype), 0)      # (xg came from the gather with its rows padded already)
        need_b = bdt is not None and ctx.needs_input_grad[3]
        dw = db = None
        if ctx.needs_input_grad[2]:
            dw, db = wgrad(d2, xg, bias=need_b)
            dw = dw[:, :K].reshape(wshape).to(wdt)
        elif need_b:
            db = ops.colsum(d2)
        return None, None, dw, db.to(bdt) if need_b else None, None, None, None, None


class _AssembleFn(torch.autograd.Function):
    """me_mae_assemble_fwd / _bwd; the position table is data (the reference adds a detached copy)"""

    @staticmethod
    def forward(ctx, xv, mask_token, pos, vis_idx, dec_idx, odt):
        xdt = xv.dtype
        if xv.dtype == torch.float16:
            xv = ops.cast(xv.contiguous(), torch.bfloat16)
        kdt = torch.bfloat16 if odt == torch.float16 else odt
        out = mae_assemble(xv, pos, vis_idx, dec_idx, mask_token, out_dtype=kdt)
        ctx.meta = (xv.shape[1], xdt, mask_token.dtype, tuple(mask_token.shape))
        return out if kdt == odt else ops.cast(out, odt)

    @staticmethod
    def backward(ctx, dy):
        Nvis, xdt, tdt, tshape = ctx.meta
        if dy.dtype == torch.float16:
            dy = ops.cast(dy.contiguous(), torch.bfloat16)
        kdt = torch.bfloat16 if xdt == torch.float16 else xdt
        dxv, dmask = mae_assemble_bwd(dy, Nvis, dxv_dtype=kdt, want_dxv=ctx.needs_input_grad[0], want_dmask=ctx.needs_input_grad[1])
        if dxv is not None and kdt != xdt:
            dxv = ops.cast(dxv, xdt)
        return dxv, None if dmask is None else dmask.reshape(tshape).to(tdt), None, None, None, None


class _NormFn(torch.autograd.Function):
    """nn.LayerNorm on me_layernorm_fwd / _bwd with the output in the compute dtype"""

    @staticmethod
    def forward(ctx, x, w, b, eps, odt):
        x = x.contiguous()
        if x.dtype == torch.float16:
            x = ops.cast(x, torch.bfloat16)
        y, mean, rstd = ops.layernorm_fwd(x, w, b, eps, odt, save_stats=True)
        ctx.save_for_backward(x, mean, rstd, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, w = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.dtype not in (torch.float32, torch.bfloat16):
            dy = dy.float()
        dx, dg, db = ops.layernorm_bwd(dy, x, mean, rstd, w, None, x.dtype, True)
        return dx, dg.to(w.dtype), db.to(w.dtype), None, None


class _MaeLossFn(torch.autograd.Function):
    """me_mae_loss.  Forward: the loss only.  Backward: the same pass again with the upstream scalar on the device, writing dpred
    (nothing of pred's size is kept between the two)."""

    @staticmethod
    def forward(ctx, pred, video, dec_idx, w, tubelet, normalize_target, mean, std):
        pdt = pred.dtype
        if pred.dtype == torch.float16:
            pred = ops.cast(pred.contiguous(), torch.bfloat16)
        res = mae_loss_terms(pred, video, dec_idx, w, tubelet, normalize_target, mean, std)
        ctx.save_for_backward(pred, video, dec_idx, w)
        ctx.meta = (tubelet, normalize_target, mean, std, pdt)
        return res["loss"].clone()

    @staticmethod
    def backward(ctx, g):
        pred, video, dec_idx, w = ctx.saved_tensors
        tubelet, normalize_target, mean, std, pdt = ctx.meta
        dpred = mae_loss_terms(pred, video, dec_idx, w, tubelet, normalize_target, mean, std, grad_scale=g, want_loss=False, want_dpred=True)["dpred"]
        return (dpred if dpred.dtype == pdt else ops.cast(dpred, pdt)), None, None, None, None, None, None, None


def mae_reconstruction_loss(pred: torch.Tensor, video: torch.Tensor, mask: torch.Tensor, decode_mask: Optional[torch.Tensor] = None,
                            patch_size: int = 16, tubelet_size: int = 2, normalize_target: bool = True, mean=IMAGENET_DEFAULT_MEAN,
                            std=IMAGENET_DEFAULT_STD) -> torch.Tensor:
    """The pre-training loss of engine_for_pretraining.py:66-105 as one fp32 scalar: ``pred [B, Ndec, tubelet patch^2 C]`` (the model's
    output) against the per-patch normalised pixels (``normalize_target``: per channel, unbiased variance, ``/(std + 1e-6)``) of the
    decoded tokens of ``video`` -- the data loader's normalised clip, un-normalised with ``mean`` / ``std`` -- averaged over the
    columns and then over the decoded tokens that ``mask`` covers (``decode_mask`` given: the decoded tokens are ``~decode_mask`` and
    the visible ones among them weigh 0).  The gradient goes to ``pred`` only.  No weight at all gives loss 0 and a zero gradient."""
    who = "mae_reconstruction_loss"
    if not isinstance(video, torch.Tensor) or not video.is_cuda or not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise MetaEncError(f"{who} runs on MI355X only (CPU tensor given; no CPU fallback)")
    if video.dim() != 5:
        raise MetaEncError(f"{who}: clip {tuple(video.shape)} must be [B, C, T, H, W]")
    B, _, T, H, W = video.shape
    N = (T // tubelet_size) * (H // patch_size) * (W // patch_size)
    mask = _check_mask(who, mask, B, N, video.device, "mask")
    if decode_mask is not None:
        decode_mask = _check_mask(who, decode_mask, B, N, video.device, "decode_mask")
    _, dec_idx, w = mae_index_lists(mask, decode_mask, who)
    return _MaeLossFn.apply(pred, video, dec_idx, w, (tubelet_size, patch_size, patch_size), bool(normalize_target), tuple(mean), tuple(std))


# ----------------------------------------------------------------------------------------------------------------- the modules

def _init_weights(m: nn.Module) -> None:
    if isinstance(m, nn.Linear):
        nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


def _make_blocks(who, embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale, drop_rate, attn_drop_rate, drop_path_rate, norm_layer,
                 init_values, with_cp, cos_attn) -> nn.ModuleList:
    if cos_attn:
        raise MetaEncError(f"{who}: cos_attn=True (CosAttention, modeling_finetune.py:81-139) has no HIP kernel yet")
    if with_cp:
        raise MetaEncError(f"{who}: with_cp=True (activation checkpointing) is not supported: the Blocks save what their own backward needs")
    if init_values is None:
        raise MetaEncError(f"{who}: init_values=None is not a configuration (the reference's Block compares it with 0 and fails); "
                           "pass 0. for no layer scale")
    dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
    return nn.ModuleList([Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                                attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, layer_scale=init_values > 0)
                          for i in range(depth)])


def _set_layer_scale(blocks, init_values) -> None:
    for blk in blocks:
        if blk.layer_scale:
            nn.init.constant_(blk.gamma1, init_values)
            nn.init.constant_(blk.gamma2, init_values)


def _stream_dtype(param: torch.Tensor, odt: torch.dtype) -> torch.dtype:
    """dtype of the token stream between the Blocks: fp32 while the parameters are (autocast changes the arithmetic, not the stream)"""
    return torch.float32 if param.dtype == torch.float32 else odt


def _norm(x: torch.Tensor, ln: nn.LayerNorm, odt: torch.dtype) -> torch.Tensor:
    return _NormFn.apply(x, ln.weight, ln.bias, ln.eps, torch.bfloat16 if odt == torch.float16 else odt)


class PretrainVisionTransformerEncoder(nn.Module):
    """modeling_pretrain.py:28-144: tubelet embed of the visible tokens + position rows, Blocks, ``norm``, ``head``.
    ``forward(x [B, C, T, H, W], mask [B, N] bool)`` -> ``[B, Nvis, embed_dim]`` (``num_classes`` when > 0); True in ``mask`` = masked."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=0, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=False,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=None, tubelet_size=2,
                 use_learnable_pos_emb=False, with_cp=False, all_frames=16, cos_attn=False):
        super().__init__()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = VideoPatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim, num_frames=all_frames,
                                           tubelet_size=tubelet_size)
        num_patches = self.patch_embed.num_patches
        self.with_cp = with_cp
        if use_learnable_pos_emb:
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        else:
            self.register_buffer("pos_embed", video_sinusoid_table(num_patches, embed_dim), persistent=False)
        self.blocks = _make_blocks("PretrainVisionTransformerEncoder", embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale, drop_rate,
                                   attn_drop_rate, drop_path_rate, norm_layer, init_values, with_cp, cos_attn)
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        if use_learnable_pos_emb:
            nn.init.trunc_normal_(self.pos_embed, std=.02, a=-.02, b=.02)
        self.apply(_init_weights)
        _set_layer_scale(self.blocks, init_values)

    def get_num_layers(self):
        return len(self.blocks)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=""):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def _masks(self, x, mask, who):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise MetaEncError(f"{who} runs on MI355X only (CPU tensor given; no CPU fallback)")
        if x.dim() != 5:
            raise MetaEncError(f"{who}: clip {tuple(x.shape)} must be [B, C, T, H, W]")
        pe = self.patch_embed
        kt, kh, kw = pe.geom[:3]
        B, _, T, H, W = x.shape
        if (H, W) != tuple(pe.img_size) or x.shape[1] != pe.proj.weight.shape[1] or (T // kt) * (H // kh) * (W // kw) != pe.num_patches:
            raise MetaEncError(f"{who}: clip {tuple(x.shape)} does not match the model ({pe.proj.weight.shape[1]} channels, "
                               f"{pe.num_patches} tubelets of {kt} x {kh} x {kw} at {pe.img_size[0]} x {pe.img_size[1]})")
        if pe.proj.weight.device != x.device:
            raise MetaEncError(f"{who}: parameters are on {pe.proj.weight.device}, the clip on {x.device}")
        return _check_mask(who, mask, B, pe.num_patches, x.device, "mask")

    def _features(self, x, vis_idx, cdt, odt):
        """tubelet embed of the visible tokens, Blocks, norm.  The token stream between the Blocks has the PARAMETERS' dtype: fp32
        parameters under autocast keep an fp32 residual stream (bf16 arithmetic inside the Blocks), as when fp32 tokens are handed to
        a Block under autocast.  ``norm`` writes that dtype too, so the Linears behind the two final norms (``head`` /
        ``encoder_to_decoder``, and the decoder's ``head``) compute in it: fp32 parameters give them fp32 arithmetic under autocast as
        well, like the fp32 LayerNorm + Linear of ClassifierHead -- an exception to "autocast -> bf16" that costs 1.7 ms of a 92.6 ms
        Base step at B = 32.  bf16 parameters run them in bf16."""
        pe = self.patch_embed
        who = type(self).__name__
        if self.pos_embed.shape[1] != pe.num_patches:
            raise MetaEncError(f"{who}: use_learnable_pos_emb=True holds {self.pos_embed.shape[1]} position rows for {pe.num_patches} tubelets "
                               "(the reference's own forward fails on that sum, modeling_pretrain.py:68-69, 127)")
        if vis_idx.shape[1] == 0:
            raise MetaEncError(f"{who}: the mask leaves no visible token")
        x = _clip(who, x)
        t = _VisibleEmbedFn.apply(x, vis_idx, pe.proj.weight, pe.proj.bias, self.pos_embed, tuple(pe.geom[:3]), cdt, _stream_dtype(pe.proj.weight, odt))
        for blk in self.blocks:
            t = blk(t)
        return _norm(t, self.norm, _stream_dtype(self.norm.weight, odt))

    def forward_features(self, x, mask):
        mask = self._masks(x, mask, type(self).__name__)
        cdt, odt = _boundary_dtypes(self.patch_embed.proj.weight)
        (vis_idx,) = token_indices(type(self).__name__, ~mask)
        return self._features(x, vis_idx, cdt, odt)

    def _head(self, t):
        return t if isinstance(self.head, nn.Identity) else linear(t, self.head.weight, self.head.bias)

    def forward(self, x, mask):
        return self._head(self.forward_features(x, mask))


class PretrainVisionTransformerDecoder(nn.Module):
    """modeling_pretrain.py:147-236: Blocks, then ``head(norm(.))`` on the last ``return_token_num`` rows (all rows when it is 0)."""

    def __init__(self, patch_size=16, num_classes=768, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=False, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=None, num_patches=196, tubelet_size=2,
                 with_cp=False, cos_attn=False):
        super().__init__()
        self.num_classes = num_classes
        assert num_classes == 3 * tubelet_size * patch_size ** 2
        self.num_features = self.embed_dim = embed_dim
        self.patch_size = patch_size
        self.with_cp = with_cp
        self.blocks = _make_blocks("PretrainVisionTransformerDecoder", embed_dim, depth, num_heads, mlp_ratio, qkv_bias, qk_scale, drop_rate,
                                   attn_drop_rate, drop_path_rate, norm_layer, init_values, with_cp, cos_attn)
        self.norm = norm_layer(embed_dim)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        self.apply(_init_weights)
        _set_layer_scale(self.blocks, init_values)

    def get_num_layers(self):
        return len(self.blocks)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token"}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=""):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def forward(self, x, return_token_num):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise MetaEncError("PretrainVisionTransformerDecoder runs on MI355X only (CPU tensor given; no CPU fallback)")
        for blk in self.blocks:
            x = blk(x)
        if return_token_num > 0:
            x = x[:, -return_token_num:].contiguous()      # only the decoded rows are normalised and projected
        cdt, odt = _boundary_dtypes(self.norm.weight)
        # the prediction meets an fp32 target: with fp32 parameters norm and head stay fp32 under autocast too (see _features)
        x = _norm(x, self.norm, _stream_dtype(self.norm.weight, odt))
        return x if isinstance(self.head, nn.Identity) else linear(x, self.head.weight, self.head.bias)


class PretrainVisionTransformer(nn.Module):
    """modeling_pretrain.py:239-360.  ``forward(x, mask, decode_mask=None)`` -> ``[B, Ndec, decoder_num_classes]`` fp32: the decoded
    positions are ``mask``, or ``~decode_mask`` when a decoder mask is given (the reference's own convention, :341)."""

    def __init__(self, img_size=224, patch_size=16, encoder_in_chans=3, encoder_num_classes=0, encoder_embed_dim=768, encoder_depth=12,
                 encoder_num_heads=12, decoder_num_classes=1536, decoder_embed_dim=512, decoder_depth=8, decoder_num_heads=8, mlp_ratio=4.,
                 qkv_bias=False, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=0.,
                 use_learnable_pos_emb=False, tubelet_size=2, num_classes=0, in_chans=0, with_cp=False, all_frames=16, cos_attn=False):
        super().__init__()
        self.encoder = PretrainVisionTransformerEncoder(
            img_size=img_size, patch_size=patch_size, in_chans=encoder_in_chans, num_classes=encoder_num_classes, embed_dim=encoder_embed_dim,
            depth=encoder_depth, num_heads=encoder_num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop_rate=drop_rate,
            attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer, init_values=init_values,
            tubelet_size=tubelet_size, use_learnable_pos_emb=use_learnable_pos_emb, with_cp=with_cp, all_frames=all_frames, cos_attn=cos_attn)
        self.decoder = PretrainVisionTransformerDecoder(
            patch_size=patch_size, num_patches=self.encoder.patch_embed.num_patches, num_classes=decoder_num_classes, embed_dim=decoder_embed_dim,
            depth=decoder_depth, num_heads=decoder_num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop_rate=drop_rate,
            attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate, norm_layer=norm_layer, init_values=init_values,
            tubelet_size=tubelet_size, with_cp=with_cp, cos_attn=cos_attn)
        self.encoder_to_decoder = nn.Linear(encoder_embed_dim, decoder_embed_dim, bias=False)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, decoder_embed_dim))
        self.register_buffer("pos_embed", video_sinusoid_table(self.encoder.patch_embed.num_patches, decoder_embed_dim), persistent=False)
        nn.init.trunc_normal_(self.mask_token, std=.02, a=-.02, b=.02)

    def get_num_layers(self):
        return len(self.encoder.blocks)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"pos_embed", "cls_token", "mask_token"}

    def forward(self, x, mask, decode_mask=None):
        who = type(self).__name__
        enc = self.encoder
        mask = enc._masks(x, mask, who)
        if decode_mask is not None:
            decode_mask = _check_mask(who, decode_mask, mask.shape[0], mask.shape[1], x.device, "decode_mask")
        cdt, odt = _boundary_dtypes(enc.patch_embed.proj.weight)
        vis_idx, dec_idx, _ = mae_index_lists(mask, decode_mask, who)
        x_vis = enc._head(enc._features(x, vis_idx, cdt, odt))                                  # [B, Nvis, C_e]
        x_vis = linear(x_vis, self.encoder_to_decoder.weight, None)                             # [B, Nvis, C_d] fp32
        # the visible tokens keep their shuffled order; the position rows are gathered to match (modeling_pretrain.py:347-356)
        x_full = _AssembleFn.apply(x_vis, self.mask_token, self.pos_embed, vis_idx, dec_idx, _stream_dtype(self.mask_token, odt))
        return self.decoder(x_full, dec_idx.shape[1])
