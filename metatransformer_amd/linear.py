"""y = x W^T + b on me_gemm, with gradients: the one place that knows the GEMM's granules.

me_gemm moves 16-byte rows: an NT product wants its reduction K, a TN product its two operand widths, a multiple of 8 (bf16; 4 in fp32, and
8 serves both).  ``pad_to`` is the one spelling of that padding, ``wgrad`` the one weight-gradient call (dW = dY^T x on the TN kernel, with
the bias gradient), ``linear`` the differentiable F.linear that heads, adapter, data2seq and hyperspectral share (``heads.linear`` is this
function).  The Functions that fuse more into the GEMM epilogue (timeseries._LinFn / _MlpFn, data2seq._TimeFeatFn,
video_mae._VisibleEmbedFn) keep their forward and take their weight gradients from ``wgrad``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _capi, ops
from ._capi import ME_GEMM_TN, MetaEncError, check, dtype_code, ptr, stream_ptr


def pad_to(t: torch.Tensor, dim: int, multiple: int = 8) -> torch.Tensor:
    """t with dimension ``dim`` zero-padded up to a multiple of ``multiple``; t itself where it already is one"""
    short = -t.shape[dim] % multiple
    if not short:
        return t
    shape = list(t.shape)
    shape[dim] = short
    return torch.cat([t, t.new_zeros(shape)], dim=dim)


def wgrad(d: torch.Tensor, x: torch.Tensor, *, bias: bool = False, fused_bias: bool = False):
    """(dW [N, K] fp32 = d^T x, db [N] fp32 or None) from d [M, N] and x [M, K] of one compute dtype, N and K multiples of the granule (8; 4
    serves fp32: data2seq._TSEmbedFn's unfolded columns).

    The row count M, the TN product's reduction, is zero-padded to a multiple of 8 on both operands when it is not one.  The bias gradient
    comes one of two ways, which add in different orders:
      * ``fused_bias=False``: ``ops.colsum(d)``, a pass of its own over d as given, before the row pad (heads.linear and through it
        adapter.conv3x3_rows and hyperspectral's gathered route; video_mae._VisibleEmbedFn, which pads d itself next to its saved rows);
      * ``fused_bias=True``: the column sums of the padded d from the TN kernel's own operand fragments where it can fuse them
        (``ops.gemm(..., want_colsum_a=True)``: timeseries._LinFn / _MlpFn).

    Do the kernels need the row pad?  No.  me_gemm's fill_params checks M, N, lda, ldb of a TN problem and not K, and none of the three
    loaders needs it: TnLoader (gemm.hip, the generic kernel, all of fp32) tests every reduction row against K and stages zeros past it;
    TnStager2 (gemm_stage.h, the K-step-32 kernel) has no such test but g2b_supported sends it whole steps only (K % 32 == 0); the g3 TN
    stage (gemm3_core.h) reads rows past K as zeros through its buffer descriptors' bounds check.  The pad stays all the same: K is what
    plan_gemm chooses the kernel and its split over the reduction by (bf16, 25 rows: the generic kernel as they are, the K-step-32 kernel
    once padded to 32), so the same data without it can sum in another order."""
    dp, xp = pad_to(d, 0), pad_to(x, 0)
    if bias and fused_bias:
        return ops.gemm(dp, xp, op=ME_GEMM_TN, out_dtype=torch.float32, want_colsum_a=True)
    dw = ops.gemm(dp, xp, op=ME_GEMM_TN, out_dtype=torch.float32)
    return dw, ops.colsum(d) if bias else None


def _gemm_nt_chunked(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor], step: int) -> torch.Tensor:
    """fp32 [M, N] = a [M, K] b [N, K]^T (+ bias) on me_gemm NT.  The exact-fp32 kernel adds all K products of an output into
    one accumulator, so its rounding error grows like sqrt(K); a 3x3 convolution has K = 9 Cin up to 2304.  The operands are
    therefore contracted ``step`` columns at a time, each call adding its partial sum to the output (beta = 1): the long
    chain becomes K / step short ones plus K / step additions of partial sums.  (The descriptor is built here: ops.gemm takes
    whole matrices, a chunk is a column window of a wider one.)"""
    lib = _capi.load()
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    es = a.element_size()
    bias = bias.detach().float().contiguous() if bias is not None else None
    for k0 in range(0, K, step):
        d = _capi.GemmDesc()
        d.op, d.ab_dtype = _capi.ME_GEMM_NT, dtype_code(a.dtype)
        d.M, d.N, d.K = M, N, min(step, K - k0)
        d.A, d.lda = ptr(a) + k0 * es, K
        d.B, d.ldb = ptr(b) + k0 * es, K
        d.C, d.ldc, d.c_dtype = ptr(out), N, _capi.ME_F32
        d.alpha, d.beta = 1.0, 0.0 if k0 == 0 else 1.0
        if bias is not None and k0 == 0:
            d.bias = ptr(bias)
        ws = None
        need = lib.me_gemm_workspace_bytes(ctypes.byref(d))
        if need:
            ws = torch.empty(need, dtype=torch.uint8, device=a.device)
            d.workspace, d.workspace_bytes = ptr(ws), need
        check(lib.me_gemm(ctypes.byref(d), stream_ptr()), "me_gemm (k_chunk)")
    return out


def _gemm_nt(a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor], k_chunk: Optional[int]) -> torch.Tensor:
    if k_chunk and a.dtype == torch.float32:      # (bf16 operands, whose own rounding is 2^-9, take one call)
        return _gemm_nt_chunked(a, b, bias, k_chunk)
    return ops.gemm(a, b, bias=bias, out_dtype=torch.float32)


class _LinearFn(torch.autograd.Function):
    """y [rows, N] fp32 = x W^T + b on me_gemm in the compute dtype ``cdt`` (exact fp32 MFMA or bf16 MFMA); N (class counts such as 174) and
    K (3 coordinates, 27 band neighbours) are padded to multiples of 8 in here.  Backward: dx = dY W (skipped where x is data), (dW, db) =
    wgrad."""

    @staticmethod
    def forward(ctx, x, w, b, cdt, k_chunk):
        N, K = w.shape
        xc = ops.cast(pad_to(x.reshape(-1, x.shape[-1]), 1).contiguous(), cdt)
        wc = pad_to(pad_to(w.detach().to(cdt), 0), 1).contiguous()
        bc = pad_to(b.detach().float(), 0) if b is not None else None
        y = _gemm_nt(xc, wc, bc, k_chunk)
        ctx.save_for_backward(xc, wc if ctx.needs_input_grad[0] else None)
        ctx.meta = (N, K, x.shape, x.dtype, w.dtype, b.dtype if b is not None else None, k_chunk)
        # never a VIEW of a tensor made in here: the reference's ClsHead puts nn.ReLU(inplace=True) straight behind its Linear
        # (cls_base.py:112-118 with norm_args=None), and autograd refuses in-place writes to a custom Function's view output
        return y if y.shape[1] == N else y[:, :N].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        xc, wc = ctx.saved_tensors
        N, K, xshape, xdt, wdt, bdt, k_chunk = ctx.meta
        ng = ctx.needs_input_grad
        d2 = pad_to(dy.to(xc.dtype), 1).contiguous()
        dx = dw = db = None
        if ng[0]:
            dx = _gemm_nt(d2, ops.transpose_cast(wc, wc.dtype), None, k_chunk)[:, :xshape[-1]].reshape(xshape).to(xdt)
        need_b = bdt is not None and ng[2]
        if ng[1] or need_b:
            dw, db = wgrad(d2, xc, bias=need_b)
            dw = dw[:N, :K].to(wdt) if ng[1] else None
            db = db[:N].to(bdt) if need_b else None
        return dx, dw, db, None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], *, compute_dtype: Optional[torch.dtype] = None,
           k_chunk: Optional[int] = None) -> torch.Tensor:
    """F.linear on the HIP GEMM: fp32 result [..., out_features], differentiable in x, weight and bias.

    ``compute_dtype``: what x and weight are cast to; by default bf16 / fp16 input -> bf16, anything else -> exact fp32.  Any in_features and
    out_features: both are zero-padded to the GEMM's granule of 8 inside.  x may be wider than the weight by such padding already (the
    gather kernels write their rows 8 columns wide); the weight and its gradient keep their own width.  ``k_chunk``: fp32 operands are
    contracted that many columns at a time, forward and dgrad (_gemm_nt_chunked; adapter.conv3x3_rows passes its CONV_K_CHUNK)."""
    if not x.is_cuda:
        raise MetaEncError("linear: CUDA tensors only (no CPU fallback)")
    K = weight.shape[1]
    if not K <= x.shape[-1] <= (K + 7) // 8 * 8:
        raise MetaEncError(f"linear: x has {x.shape[-1]} columns, the weight {K} (x may be wider by zero padding up to a multiple of 8 only)")
    if compute_dtype is None:
        compute_dtype = torch.bfloat16 if x.dtype in (torch.bfloat16, torch.float16) else torch.float32
    y = _LinearFn.apply(x, weight, bias, compute_dtype, k_chunk)            # [rows, out_features]
    return y if x.dim() == 2 else y.reshape(*x.shape[:-1], weight.shape[0])
