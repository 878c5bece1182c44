"""Time-Series forecast decoder and forecaster on the HIP path.

Restates the trainable side of the reference's forecast recipe (Time-Series/models/MetaTransformer.py:46-70,80-88,119-122):

  ``FullAttention``   Time-Series/layers/SelfAttention_Family.py:48-75      softmax(scale Q K^T [causal]) V, attention dropout
  ``AttentionLayer``  Time-Series/layers/SelfAttention_Family.py:179-211    query / key / value / out projections around it
  ``DecoderLayer``    Time-Series/layers/Transformer_EncDec.py:83-116       causal self-attention, cross-attention, k=1 conv MLP, post-norm
  ``Decoder``         Time-Series/layers/Transformer_EncDec.py:119-135      the layers, a final LayerNorm and Linear(d_model, c_out)
  ``Forecaster``      Time-Series/models/MetaTransformer.py (forecast tasks) two DataEmbeddings, the frozen encoder, the decoder

Constructor signatures, parameter names and shapes are the reference's, so its state dicts load strict=True.

What runs where.  Every projection is me_gemm: ONE GEMM on the concatenated query | key | value weights for self-attention, one for
query and one on key | value for cross-attention.  me_attention_qkv_fwd / _bwd (csrc/attention_qkv.hip) read Q, K, V in place from those
GEMM outputs through their row strides and write dQ, dK, dV straight into one packed gradient buffer: no permute or copy between a
projection and the attention, forward or backward.  The out-projection GEMM fuses bias and residual; LayerNorm is me_layernorm_*; conv1
(a k=1 Conv1d) is a GEMM with bias + GELU that saves gelu' for backward (ME_GEMM_SAVE_GELU_GRAD), conv2 a GEMM with the residual; the
final projection to c_out (7 in the recipes: not a multiple of 8) goes through heads.linear's padded-N route.

Precision.  fp32 inputs run the exact-fp32 kernels.  Under bf16 / fp16 autocast (or with bf16 / fp16 inputs) GEMM operands and attention
run in bf16; the residual stream, LayerNorm and every result handed back stay fp32.

Training mode.  ``Decoder.forward`` draws ONE int64 seed from torch's CPU generator (as Block does) whenever a dropout is active;
layer i uses seed + i * SEED_LAYER_STRIDE + site, with the sites below.  Every mask is u01_hash(seed', index) of csrc/common.h,
regenerated in backward.  The attention probabilities are indexed ((b*H + h)*Nq + q)*Nk + k, the layer dropouts r * cols + c
(me_dropout_add).  eval() or dropout = 0 is deterministic and draws nothing.
"""
from __future__ import annotations

from math import sqrt
from typing import Optional

import torch
import torch.nn as nn

from . import heads, ops
from ._capi import ME_ACT_GELU, ME_GEMM_AUX_IS_FACTOR, ME_GEMM_SAVE_GELU_GRAD, MetaEncError
from .data2seq import DataEmbedding
from .encoder import Block
from .linear import linear, wgrad

# per-site seed offsets inside one decoder layer (DecoderLayer.forward, Transformer_EncDec.py:98-116)
SEED_SELF_ATTN_DROP = 1       # FullAttention.dropout of the self-attention: on the probabilities, inside the kernel
SEED_SELF_BRANCH = 2          # x + dropout(self_attention(x))
SEED_CROSS_ATTN_DROP = 3      # FullAttention.dropout of the cross-attention
SEED_CROSS_BRANCH = 4         # x + dropout(cross_attention(x, cross))
SEED_MLP_HIDDEN = 5           # dropout(activation(conv1(y)))
SEED_MLP_BRANCH = 6           # dropout(conv2(...))
SEED_LAYER_STRIDE = 8         # layer i: seed + i * SEED_LAYER_STRIDE + site


def _draw_seed() -> int:
    return int(torch.empty((), dtype=torch.int64).random_().item())


def _compute_dtype(x: torch.Tensor) -> torch.dtype:
    if not x.is_cuda:
        raise MetaEncError("the Time-Series decoder runs on MI355X only (CPU tensor given; no CPU fallback)")
    if torch.is_autocast_enabled():
        acast = torch.get_autocast_dtype("cuda")
        if acast not in (torch.bfloat16, torch.float16, torch.float32):
            raise MetaEncError(f"autocast dtype {acast} unsupported")
        return torch.float32 if acast == torch.float32 else torch.bfloat16
    if x.dtype == torch.float32:
        return torch.float32
    if x.dtype in (torch.bfloat16, torch.float16):
        return torch.bfloat16
    raise MetaEncError(f"unsupported input dtype {x.dtype}")


def _masked_grad(dy2: torch.Tensor, rows: int, p: float, seed: int, cdt: torch.dtype) -> torch.Tensor:
    """the gradient entering dropout(t), in the compute dtype (the same mask, regenerated)"""
    return ops.dropout_add(dy2, None, rows, p, 0.0, seed, out_dtype=cdt) if p > 0 else ops.cast(dy2, cdt)


class _LinFn(torch.autograd.Function):
    """y = [res +] dropout_p(x W^T + b) on me_gemm; bias and (without dropout) the residual ride in the GEMM epilogue."""

    @staticmethod
    def forward(ctx, x, w, b, res, cdt, out_dtype, p, seed, rows):
        N, K = w.shape
        xc = ops.cast(x.reshape(-1, K).contiguous(), cdt)
        wc = w.detach().to(cdt).contiguous()
        bc = b.detach().float() if b is not None else None
        res2 = res.reshape(-1, N).contiguous() if res is not None else None
        if p > 0:
            y = ops.dropout_add(ops.gemm(xc, wc, bias=bc, out_dtype=out_dtype), res2, rows, p, 0.0, seed, out_dtype=out_dtype)
        else:
            y = ops.gemm(xc, wc, bias=bc, residual=res2, out_dtype=out_dtype)
        ctx.save_for_backward(xc, wc)
        ctx.meta = (x.shape, x.dtype, w.dtype, b is not None, res is not None, res.shape if res is not None else None, cdt, p, seed, rows)
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        xshape, xdt, wdt, has_b, has_res, rshape, cdt, p, seed, rows = ctx.meta
        ng = ctx.needs_input_grad
        dy2 = dy.reshape(-1, wc.shape[0]).contiguous()
        d = _masked_grad(dy2, rows, p, seed, cdt)
        dx = dw = db = None
        if ng[0]:
            dx = ops.gemm(d, ops.transpose_cast(wc, cdt), out_dtype=xdt if xdt in (torch.float32, torch.bfloat16) else torch.float32)
            dx = dx.reshape(xshape).to(xdt)
        if ng[1] or (has_b and ng[2]):
            dw, db = wgrad(d, xc, bias=has_b and ng[2], fused_bias=True)
            dw = dw.to(wdt) if ng[1] else None
            db = db.to(wdt) if db is not None else None
        dres = dy.reshape(rshape) if has_res and ng[3] else None
        return dx, dw, db, dres, None, None, None, None, None


class _MlpFn(torch.autograd.Function):
    """y = x + dropout(conv2(dropout(gelu(conv1(x))))) -- DecoderLayer's k=1 convolutions as two GEMMs (Transformer_EncDec.py:112-114)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, cdt, p, seed_hidden, seed_branch, rows):
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        xc = ops.cast(x2, cdt)
        w1c, w2c = w1.detach().to(cdt).contiguous(), w2.detach().to(cdt).contiguous()
        gp = torch.empty((x2.shape[0], w1.shape[0]), dtype=cdt, device=x.device)          # gelu'(conv1 pre-activation)
        a = ops.gemm(xc, w1c, bias=b1.detach().float(), act=ME_ACT_GELU, preact=gp, flags=ME_GEMM_SAVE_GELU_GRAD)
        if p > 0:
            a = ops.dropout_add(a, None, rows, p, 0.0, seed_hidden)
            y = ops.dropout_add(ops.gemm(a, w2c, bias=b2.detach().float(), out_dtype=torch.float32), x2, rows, p, 0.0, seed_branch)
        else:
            y = ops.gemm(a, w2c, bias=b2.detach().float(), residual=x2, out_dtype=torch.float32)
        ctx.save_for_backward(xc, gp, a, w1c, w2c)
        ctx.meta = (x.shape, w1.dtype, cdt, p, seed_hidden, seed_branch, rows)
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        xc, gp, a, w1c, w2c = ctx.saved_tensors
        xshape, wdt, cdt, p, seed_hidden, seed_branch, rows = ctx.meta
        dy2 = dy.reshape(-1, xshape[-1]).float().contiguous()
        d = _masked_grad(dy2, rows, p, seed_branch, cdt)
        dh = ops.gemm(d, ops.transpose_cast(w2c, cdt), aux=gp, flags=ME_GEMM_AUX_IS_FACTOR)      # (d W2) * gelu'
        if p > 0:
            dh = ops.dropout_add(dh, None, rows, p, 0.0, seed_hidden)
        dw2, db2 = wgrad(d, a, bias=True, fused_bias=True)
        dw1, db1 = wgrad(dh, xc, bias=True, fused_bias=True)
        dx = ops.gemm(dh, ops.transpose_cast(w1c, cdt), residual=dy2, out_dtype=torch.float32)
        return dx.reshape(xshape), dw1.to(wdt), db1.to(wdt), dw2.to(wdt), db2.to(wdt), None, None, None, None, None


class _AttnFn(torch.autograd.Function):
    """me_attention_qkv_fwd / _bwd on projection outputs, read and written in place.  layout: 'packed3' (a = [B*N, 3C] = q | k | v),
    'q_kv' (a = q [B*Nq, C], b = [B*Nk, 2C] = k | v) or 'separate' (a, b, c).  The gradients come back in the same packing."""

    @staticmethod
    def _views(layout, a, b, c, C):
        if layout == "packed3":
            return a[:, :C], a[:, C:2 * C], a[:, 2 * C:]
        if layout == "q_kv":
            return a, b[:, :C], b[:, C:]
        return a, b, c

    @staticmethod
    def forward(ctx, a, b, c, layout, B, Nq, Nk, H, scale, causal, p, seed):
        C = a.shape[1] // 3 if layout == "packed3" else a.shape[1]
        q, k, v = _AttnFn._views(layout, a, b, c, C)
        out, lse = ops.attention_qkv_fwd(q, k, v, B, Nq, Nk, H, C // H, scale, causal=causal, need_lse=True, p_drop=p, seed=seed)
        ctx.save_for_backward(a, b, c, out, lse)
        ctx.meta = (layout, B, Nq, Nk, H, C, scale, causal, p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, b, c, out, lse = ctx.saved_tensors
        layout, B, Nq, Nk, H, C, scale, causal, p, seed = ctx.meta
        q, k, v = _AttnFn._views(layout, a, b, c, C)
        da, db, dc = (torch.empty_like(t) if t is not None else None for t in (a, b, c))
        ops.attention_qkv_bwd(q, k, v, out, ops.cast(dout.contiguous(), out.dtype), lse, B, Nq, Nk, H, C // H, scale, causal=causal, p_drop=p,
                              seed=seed, grads=_AttnFn._views(layout, da, db, dc, C))
        return da, db, dc, None, None, None, None, None, None, None, None, None


class FullAttention(nn.Module):
    """softmax(scale * Q K^T) V with TriangularCausalMask when ``mask_flag`` and dropout on the probabilities
    (SelfAttention_Family.py:48-75).  forward takes [B, L, H, E] queries, [B, S, H, E] keys and [B, S, H, E] values, as the reference;
    inside an AttentionLayer the operands are read in place from the projection GEMMs instead (``attend_rows``)."""

    def __init__(self, mask_flag=True, factor=5, scale=None, attention_dropout=0.1, output_attention=False):
        super().__init__()
        if output_attention:
            raise MetaEncError("FullAttention: output_attention=True is not implemented (the fused kernel never forms the [B, H, L, S] matrix)")
        self.scale = scale
        self.mask_flag = mask_flag
        self.output_attention = output_attention
        self.dropout = nn.Dropout(attention_dropout)

    def attend_rows(self, a, b, c, layout, B, L, S, H, seed: Optional[int] = None):
        """the attention on 2-D row operands (see _AttnFn) -> [B*L, H*E]; seed: this site's seed (drawn here when None and needed)"""
        C = a.shape[1] // 3 if layout == "packed3" else a.shape[1]
        if self.mask_flag and L != S:
            raise MetaEncError(f"FullAttention(mask_flag=True): the causal mask needs as many queries as keys (got {L}, {S})")
        p = float(self.dropout.p) if self.training else 0.0
        if p > 0 and seed is None:
            seed = _draw_seed()
        scale = self.scale or 1.0 / sqrt(C // H)
        return _AttnFn.apply(a, b, c, layout, B, L, S, H, float(scale), bool(self.mask_flag), p, seed or 0)

    def forward(self, queries, keys, values, attn_mask=None, tau=None, delta=None):
        if attn_mask is not None:
            raise MetaEncError("FullAttention: an explicit attn_mask is not implemented (mask_flag selects the causal mask; the reference's "
                               "forecast path passes None)")
        B, L, H, E = queries.shape
        S = keys.shape[1]
        if values.shape[-1] != E:
            raise MetaEncError("FullAttention: value head width must equal the key head width")
        cdt = _compute_dtype(queries)
        q, k, v = (t.reshape(-1, H * E).to(cdt).contiguous() for t in (queries, keys, values))
        out = self.attend_rows(q, k, v, "separate", B, L, S, H)
        return out.reshape(B, L, H, E).to(queries.dtype), None


class AttentionLayer(nn.Module):
    """SelfAttention_Family.py:179-211.  forward(queries, keys, values, attn_mask) -> (out [B, L, d_model], None)."""

    def __init__(self, attention, d_model, n_heads, d_keys=None, d_values=None):
        super().__init__()
        d_keys = d_keys or (d_model // n_heads)
        d_values = d_values or (d_model // n_heads)
        if d_keys != d_values:
            raise MetaEncError(f"AttentionLayer: d_keys ({d_keys}) != d_values ({d_values}) is not implemented (one head width per kernel call)")
        self.inner_attention = attention
        self.query_projection = nn.Linear(d_model, d_keys * n_heads)
        self.key_projection = nn.Linear(d_model, d_keys * n_heads)
        self.value_projection = nn.Linear(d_model, d_values * n_heads)
        self.out_projection = nn.Linear(d_values * n_heads, d_model)
        self.n_heads = n_heads

    def attend(self, queries, keys, values, cdt, seed: Optional[int] = None):
        """projections + attention, up to (not including) the out-projection -> [B*L, H*E] in the compute dtype"""
        B, L, _ = queries.shape
        S = keys.shape[1]
        H = self.n_heads
        qp, kp, vp = self.query_projection, self.key_projection, self.value_projection
        lin = lambda x, ws, bs: _LinFn.apply(x, torch.cat(ws) if len(ws) > 1 else ws[0], torch.cat(bs) if len(bs) > 1 else bs[0], None, cdt, cdt,
                                             0.0, 0, 1).reshape(-1, sum(w.shape[0] for w in ws))      # noqa: E731
        if queries is keys and keys is values:
            qkv = lin(queries, [qp.weight, kp.weight, vp.weight], [qp.bias, kp.bias, vp.bias])
            return self.inner_attention.attend_rows(qkv, None, None, "packed3", B, L, S, H, seed)
        q = lin(queries, [qp.weight], [qp.bias])
        if keys is values:
            kv = lin(keys, [kp.weight, vp.weight], [kp.bias, vp.bias])
            return self.inner_attention.attend_rows(q, kv, None, "q_kv", B, L, S, H, seed)
        return self.inner_attention.attend_rows(q, lin(keys, [kp.weight], [kp.bias]), lin(values, [vp.weight], [vp.bias]), "separate", B, L, S,
                                                H, seed)

    def forward(self, queries, keys, values, attn_mask=None, tau=None, delta=None):
        if attn_mask is not None:
            raise MetaEncError("AttentionLayer: an explicit attn_mask is not implemented")
        cdt = _compute_dtype(queries)
        o = self.attend(queries, keys, values, cdt)
        op = self.out_projection
        out = _LinFn.apply(o, op.weight, op.bias, None, cdt, torch.float32, 0.0, 0, 1)
        return out.reshape(queries.shape[0], queries.shape[1], -1), None


def _layer_norm(norm: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    return heads._LayerNormFn.apply(x, norm.weight, norm.bias, norm.eps)


class DecoderLayer(nn.Module):
    """Transformer_EncDec.py:83-116 (post-norm): x = norm1(x + drop(self_attn(x))); x = norm2(x + drop(cross_attn(x, cross)));
    norm3(x + drop(conv2(drop(act(conv1(x)))))).  activation: anything but "relu" is GELU, as in the reference; "relu" raises."""

    def __init__(self, self_attention, cross_attention, d_model, d_ff=None, dropout=0.1, activation="relu"):
        super().__init__()
        if activation == "relu":
            raise MetaEncError('DecoderLayer: activation="relu" is not implemented (the GEMM epilogue has GELU only; every recipe of the '
                               'reference passes "gelu")')
        d_ff = d_ff or 4 * d_model
        self.self_attention = self_attention
        self.cross_attention = cross_attention
        self.conv1 = nn.Conv1d(in_channels=d_model, out_channels=d_ff, kernel_size=1)
        self.conv2 = nn.Conv1d(in_channels=d_ff, out_channels=d_model, kernel_size=1)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self.activation = "gelu"

    def _stochastic(self) -> bool:
        return self.training and (self.dropout.p > 0 or self.self_attention.inner_attention.dropout.p > 0
                                  or self.cross_attention.inner_attention.dropout.p > 0)

    def forward(self, x, cross, x_mask=None, cross_mask=None, tau=None, delta=None, seed: Optional[int] = None):
        """seed: this layer's base seed (Decoder passes its own + i * SEED_LAYER_STRIDE); drawn here when the layer is called on its own"""
        if x_mask is not None or cross_mask is not None:
            raise MetaEncError("DecoderLayer: explicit masks are not implemented (the reference's forecast path passes None)")
        cdt = _compute_dtype(x)
        if seed is None:
            seed = _draw_seed() if self._stochastic() else 0
        B, L, C = x.shape
        p = float(self.dropout.p) if self.training else 0.0
        x = x.float()                                             # fp32 residual stream
        sa, ca = self.self_attention, self.cross_attention
        o = sa.attend(x, x, x, cdt, seed + SEED_SELF_ATTN_DROP)
        x = _LinFn.apply(o, sa.out_projection.weight, sa.out_projection.bias, x.reshape(B * L, C), cdt, torch.float32, p, seed + SEED_SELF_BRANCH, L)
        x = _layer_norm(self.norm1, x).reshape(B, L, C)
        o = ca.attend(x, cross, cross, cdt, seed + SEED_CROSS_ATTN_DROP)
        x = _LinFn.apply(o, ca.out_projection.weight, ca.out_projection.bias, x.reshape(B * L, C), cdt, torch.float32, p, seed + SEED_CROSS_BRANCH,
                         L)
        x = _layer_norm(self.norm2, x)
        y = _MlpFn.apply(x, self.conv1.weight.squeeze(-1), self.conv1.bias, self.conv2.weight.squeeze(-1), self.conv2.bias, cdt, p,
                         seed + SEED_MLP_HIDDEN, seed + SEED_MLP_BRANCH, L)
        return _layer_norm(self.norm3, y).reshape(B, L, C)


class Decoder(nn.Module):
    """Transformer_EncDec.py:119-135: the layers, then ``norm`` and ``projection`` when given."""

    def __init__(self, layers, norm_layer=None, projection=None):
        super().__init__()
        self.layers = nn.ModuleList(layers)
        self.norm = norm_layer
        self.projection = projection

    def forward(self, x, cross, x_mask=None, cross_mask=None, tau=None, delta=None):
        cdt = _compute_dtype(x)
        seed = _draw_seed() if any(l._stochastic() for l in self.layers) else 0
        for i, layer in enumerate(self.layers):
            x = layer(x, cross, x_mask=x_mask, cross_mask=cross_mask, tau=tau, delta=delta, seed=seed + i * SEED_LAYER_STRIDE)
        if self.norm is not None:
            x = _layer_norm(self.norm, x.float()).reshape(x.shape)
        if self.projection is not None:
            x = linear(x.to(cdt), self.projection.weight, self.projection.bias)      # (fp32 result; N padded to a multiple of 8 inside)
        return x


class Forecaster(nn.Module):
    """The forecast model of Time-Series/models/MetaTransformer.py: children ``enc_embedding``, ``encoder`` (the package's Blocks, frozen:
    requires_grad=False as :40-41), ``dec_embedding``, ``decoder``.  forward(x_enc, x_mark_enc, x_dec, x_mark_dec) -> [B, pred_len, c_out]."""

    def __init__(self, enc_in, dec_in, c_out, pred_len, d_model=768, n_heads=8, d_ff=2048, d_layers=1, embed="timeF", freq="h", dropout=0.1,
                 activation="gelu", depth=12, num_heads=12):
        super().__init__()
        self.pred_len = pred_len
        self.enc_embedding = DataEmbedding(enc_in, d_model, embed, freq, dropout)
        self.encoder = nn.Sequential(*[Block(dim=d_model, num_heads=num_heads, mlp_ratio=4., qkv_bias=True, norm_layer=nn.LayerNorm,
                                             act_layer=nn.GELU) for _ in range(depth)])
        for prm in self.encoder.parameters():
            prm.requires_grad = False
        self.dec_embedding = DataEmbedding(dec_in, d_model, embed, freq, dropout)
        self.decoder = Decoder(
            [DecoderLayer(AttentionLayer(FullAttention(True, attention_dropout=dropout, output_attention=False), d_model, n_heads),
                          AttentionLayer(FullAttention(False, attention_dropout=dropout, output_attention=False), d_model, n_heads),
                          d_model, d_ff, dropout=dropout, activation=activation) for _ in range(d_layers)],
            norm_layer=nn.LayerNorm(d_model), projection=nn.Linear(d_model, c_out, bias=True))

    def forecast(self, x_enc, x_mark_enc, x_dec, x_mark_dec):
        enc_out = self.encoder(self.enc_embedding(x_enc, x_mark_enc))
        return self.decoder(self.dec_embedding(x_dec, x_mark_dec), enc_out, x_mask=None, cross_mask=None)

    def forward(self, x_enc, x_mark_enc, x_dec, x_mark_dec, mask=None):
        return self.forecast(x_enc, x_mark_enc, x_dec, x_mark_dec)[:, -self.pred_len:, :]
