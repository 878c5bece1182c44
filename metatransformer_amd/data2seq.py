"""Data2Seq tokenizers on the HIP path: ``Data2Seq(modality, dim)(data) -> [B, N, dim]``.

Mirrors the reference's tokenizer plugin point (Data2Seq/Data2Seq.py:19-55, README.md:113-122) for the
modalities whose tokenizers are on the north-star path:

  image        Data2Seq/Image.py:8-28        Conv2d(3, C, k16, s16)           -> MFMA GEMM gathering its own patches
  audio        Data2Seq/Acoustic.py:5-23     Conv2d(1, C, k16, stride 10x10)  -> overlapping gather + GEMM
               (as written the reference class cannot be constructed -- it double-tuples patch_size; the working
               construction is Audio/src/models/ast_models.py:86, which this follows)
  video        Video/models/modeling_finetune.py:263-297  Conv3d(3, C, k=s=(2,16,16)) tubelets
               (Data2Seq/Video.py is broken in the reference)
  time-series  Data2Seq/Time_Series.py:109-126  Conv1d k3 circular + sinusoid PE + temporal-embedding gathers (embed_type='fixed'), or
               + Linear on float time features (embed_type='timeF', Time-Series/layers/Embed.py:96-106: what Time-Series/run.py
               defaults to); the decoder side of that recipe is timeseries.py
  graph        Data2Seq/Graph.py:43-305      TokenGT GraphFeatureTokenizer: node / edge embedding sums, node identifiers, type id
               -> one GEMM over the node rows + one assembly kernel (graph preprocessing -- Laplacian eigenvectors, the
               collator -- stays with the caller)

Parameter names follow the reference modules (``proj.weight`` / ``proj.bias``;
``value_embedding.tokenConv.weight``; ``atom_encoder.weight`` ...), so their state_dicts interchange.  ``Data2Seq("hyper", dim,
bands=, patch=, near_band=)`` builds hyperspectral.HyperSpectralEmbed (the working tokenizer of Hyper-spectrum/train.py and
metatransformer.py; Data2Seq/Hyper_Spectrum.py itself is broken glue).  The text tokenizer of the reference is CLIP and out of scope
(SURVEY.md 2.1 row 1).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi, ops
from ._capi import MetaEncError, check, dtype_code, ptr, stream_ptr
from .linear import linear, pad_to, wgrad


def _boundary_dtypes(weight: torch.Tensor):
    """(compute dtype, output dtype) at a tokenizer's boundary, the rule Block follows: fp32 parameters -> exact fp32
    kernels; bf16 (parameters or autocast) -> bf16 MFMA kernels; fp16 (``.half()`` models, ``torch.autocast(float16)`` --
    Audio/src/traintest.py) is a STORAGE dtype of the boundary only: tensors are converted by me_cast, the kernels compute
    in bf16 and the result goes back out as fp16."""
    dt = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else weight.dtype
    if dt == torch.float16:
        return torch.bfloat16, torch.float16
    if dt in (torch.bfloat16, torch.float32):
        return dt, dt
    raise MetaEncError(f"tokenizer dtype {dt} unsupported (fp32, bf16, fp16)")


class _PatchEmbedFn(torch.autograd.Function):
    """conv-as-GEMM through me_patch_embed: for bf16 compute on the reference's image / tubelet geometries the patch gather runs
    inside the MFMA GEMM's operand stager (no gathered matrix in memory); bias, optional pos-embed add and the cls-token row offset
    are the GEMM's epilogue.  Backward: me_patch_embed_wgrad gathers the same patches inside the weight-gradient kernel."""

    @staticmethod
    def forward(ctx, x, weight, bias, pos, geom, cdt, prefix_rows, odt=None):
        kt, kh, kw, st, sh, sw = geom
        B = x.shape[0]
        Cout = weight.shape[0]
        x_dtype = x.dtype
        x = x.contiguous()
        if x.dtype == torch.float16:                      # fp16 is converted at the boundary (me_cast), never computed in
            x = ops.cast(x, torch.bfloat16)
        if cdt == torch.bfloat16 and x.dtype == torch.float32 and ops.patch_embed_fused(x, geom, cdt, Cout, x_dtype=cdt):
            # the gather rounds the pixels to bf16 either way: one vectorised cast pass, then the fused kernel reads them where they lie
            x = ops.cast(x, cdt)
        w2 = ops.cast(weight.detach().reshape(Cout, -1).contiguous(), cdt)
        pos2 = None
        if pos is not None:
            pos2 = pos.detach().reshape(-1, Cout)
        y, tps = ops.patch_embed(x, w2, bias, pos2, geom, prefix_rows, cdt)
        out_tps = tps + prefix_rows
        ctx.save_for_backward(x, weight)
        ctx.meta = (geom, cdt, tps, out_tps, prefix_rows, bias is not None, pos is not None, x_dtype)
        if odt is not None and odt != y.dtype:
            y = ops.cast(y, odt)
        return y.reshape(B, out_tps, Cout)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        geom, cdt, tps, out_tps, prefix_rows, has_bias, has_pos, x_dtype = ctx.meta
        kt, kh, kw, st, sh, sw = geom
        B = x.shape[0]
        Cout = weight.shape[0]
        dy = dy.contiguous()
        if prefix_rows:
            dy = dy[:, prefix_rows:, :].contiguous()
        dy2 = ops.cast(dy.reshape(B * tps, Cout), cdt)
        ng = ctx.needs_input_grad
        dW = db = dx = dpos = None
        want_db = bool(ng[2] and has_bias)
        if ng[1]:
            wdt = torch.float32 if weight.dtype == torch.float16 else weight.dtype
            dW, db = ops.patch_embed_wgrad(x, geom, dy2, wdt, want_db)
            dW = ops.cast(dW, weight.dtype).reshape(weight.shape)
            if db is not None:
                db = db.to(weight.dtype)
        elif want_db:
            db = ops.colsum(dy2).to(weight.dtype)
        if ng[0]:
            wT = ops.transpose_cast(weight.detach().reshape(Cout, -1).contiguous(), cdt)     # [K, Cout]
            dcols = ops.gemm(dy2, wT)                                                        # [B*tps, K]
            dx = ops.unpatchify_add(dcols, tuple(x.shape), kt, kh, kw, st, sh, sw)
            if dx.dtype != x_dtype:
                dx = ops.cast(dx, x_dtype)
        if has_pos and ng[3]:
            raise MetaEncError("gradient w.r.t. a fused pos-embed is not implemented; add it outside the tokenizer")
        return dx, dW, db, dpos, None, None, None, None


class _ConvPatchEmbed(nn.Module):
    geom = (1, 16, 16, 1, 16, 16)

    def forward(self, x: torch.Tensor, pos_embed: Optional[torch.Tensor] = None, prefix_rows: int = 0) -> torch.Tensor:
        if not x.is_cuda:
            raise MetaEncError(f"{type(self).__name__} runs on MI355X only (CPU tensor given; no CPU fallback)")
        self._check_input(x)
        cdt, odt = _boundary_dtypes(self.proj.weight)
        return _PatchEmbedFn.apply(x, self.proj.weight, self.proj.bias, pos_embed, self.geom, cdt, prefix_rows, odt)

    def _check_input(self, x):
        pass


class PatchEmbed(_ConvPatchEmbed):
    """2D Image to Patch Embedding -- Data2Seq/Image.py:4-28 (same constructor, same parameter names)."""

    def __init__(self, img_size=224, patch_size=16, in_c=3, embed_dim=768, norm_layer=None):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.grid_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_c, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        if norm_layer is not None:
            raise MetaEncError("norm_layer is unused by the reference forward (Data2Seq/Image.py:27) and unsupported")
        self.norm = nn.Identity()
        self.geom = (1, patch_size, patch_size, 1, patch_size, patch_size)

    def _check_input(self, x):
        B, C, H, W = x.shape
        assert H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."


class AcousticPatchEmbed(_ConvPatchEmbed):
    """Spectrogram patch embed, Conv2d(in_chans, C, k=(16,16), stride=(fstride,tstride)) -- Data2Seq/Acoustic.py:5-23,
    Audio/src/models/ast_models.py:86."""

    def __init__(self, img_size=224, patch_size=16, in_chans=1, embed_dim=768, fstride=10, tstride=10):
        super().__init__()
        self.patch_size = (patch_size, patch_size)
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=(fstride, tstride))
        self.geom = (1, patch_size, patch_size, 1, fstride, tstride)

    @staticmethod
    def num_tokens(F: int, T: int, patch: int = 16, fstride: int = 10, tstride: int = 10) -> int:
        return ((F - patch) // fstride + 1) * ((T - patch) // tstride + 1)


class VideoPatchEmbed(_ConvPatchEmbed):
    """Tubelet embed, Conv3d(3, C, k=s=(tubelet,16,16)) -- Video/models/modeling_finetune.py:263-297."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, num_frames=16, tubelet_size=2):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.tubelet_size = tubelet_size
        self.patch_size = (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2 * (num_frames // tubelet_size)
        self.proj = nn.Conv3d(in_chans, embed_dim, kernel_size=(tubelet_size, patch_size, patch_size),
                              stride=(tubelet_size, patch_size, patch_size))
        self.geom = (tubelet_size, patch_size, patch_size, tubelet_size, patch_size, patch_size)

    def _check_input(self, x):
        B, C, T, H, W = x.shape
        assert H == self.img_size[0] and W == self.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."


def sinusoid_table(n: int, d_model: int) -> torch.Tensor:
    """PositionalEmbedding / FixedEmbedding table -- Data2Seq/Time_Series.py:12-23,49-57 (host-side constant)."""
    pe = torch.zeros(n, d_model).float()
    position = torch.arange(0, n).float().unsqueeze(1)
    div_term = (torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model)).exp()
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def video_sinusoid_table(n_position: int, d_hid: int) -> torch.Tensor:
    """get_sinusoid_encoding_table -- Video/models/modeling_finetune.py:302-318 (float64 math, float32 result)."""
    pos = torch.arange(n_position, dtype=torch.float64).unsqueeze(1)
    j = torch.arange(d_hid, dtype=torch.float64)
    angle = pos / torch.pow(torch.tensor(10000.0, dtype=torch.float64), 2 * torch.div(j, 2, rounding_mode="floor") / d_hid)
    tab = angle.clone()
    tab[:, 0::2] = torch.sin(angle[:, 0::2])
    tab[:, 1::2] = torch.cos(angle[:, 1::2])
    return tab.float().unsqueeze(0)


class _TokenConv(nn.Module):
    def __init__(self, c_in, d_model):
        super().__init__()
        self.tokenConv = nn.Conv1d(c_in, d_model, kernel_size=3, padding=1, padding_mode="circular", bias=False)
        nn.init.kaiming_normal_(self.tokenConv.weight, mode="fan_in", nonlinearity="leaky_relu")


class _FixedEmb(nn.Module):
    def __init__(self, c_in, d_model):
        super().__init__()
        self.emb = nn.Embedding(c_in, d_model)
        self.emb.weight = nn.Parameter(sinusoid_table(c_in, d_model), requires_grad=False)


class _Temporal(nn.Module):
    SIZES = (("month", 13), ("day", 32), ("weekday", 7), ("hour", 24), ("minute", 4))   # mark column order 0..4

    def __init__(self, d_model, freq="h"):
        super().__init__()
        if freq == "t":
            self.minute_embed = _FixedEmb(4, d_model)
        self.hour_embed = _FixedEmb(24, d_model)
        self.weekday_embed = _FixedEmb(7, d_model)
        self.day_embed = _FixedEmb(32, d_model)
        self.month_embed = _FixedEmb(13, d_model)

    def tables(self):
        names = ["month", "day", "weekday", "hour"] + (["minute"] if hasattr(self, "minute_embed") else [])
        return [getattr(self, f"{n}_embed").emb.weight for n in names]


class _PosEmb(nn.Module):
    def __init__(self, d_model, max_len=5000):
        super().__init__()
        self.register_buffer("pe", sinusoid_table(max_len, d_model).unsqueeze(0))


class _TimeFeature(nn.Module):
    """TimeFeatureEmbedding (Time-Series/layers/Embed.py:96-106): Linear(d_inp, d_model, bias=False) on float time features"""
    D_INP = {"h": 4, "t": 5, "s": 6, "m": 1, "a": 1, "w": 2, "d": 3, "b": 3}      # features per time stamp, by sampling frequency

    def __init__(self, d_model, freq="h"):
        super().__init__()
        if freq not in self.D_INP:
            raise MetaEncError(f"DataEmbedding(embed_type='timeF'): unknown freq {freq!r} (one of {sorted(self.D_INP)})")
        self.embed = nn.Linear(self.D_INP[freq], d_model, bias=False)


class DataEmbedding(nn.Module):
    """Time-series DataEmbedding -- Data2Seq/Time_Series.py:109-126 / Time-Series/layers/Embed.py:109-126.
    forward(x [B,L,c_in], x_mark or None) -> [B,L,C].
    ``embed_type='fixed'`` (x_mark [B,L,4|5] calendar indices): the three terms (circular Conv1d k3, temporal table gathers indexed by
    ``x_mark.long()``, positional slice ``pe[:, :L]``) are one fused kernel; the gathers are integer-indexed and bit-exact.
    ``embed_type='timeF'`` (x_mark [B,L,d_inp] float time features, d_inp by ``freq``; the Time-Series recipes' default): the same
    kernel forms the value and positional terms, the temporal term ``embed(x_mark)`` is a GEMM on features and weight zero-padded to 8
    columns with that embedding as its fused residual.  Gradients go to the Conv1d weight and to ``temporal_embedding.embed.weight``.
    Dropout(p) is applied in training mode (me_dropout_add, one int64 seed per call from torch's CPU generator), identity in eval."""

    def __init__(self, c_in, d_model, embed_type="fixed", freq="h", dropout=0.1):
        super().__init__()
        if embed_type not in ("fixed", "timeF"):
            raise MetaEncError("embed_type must be 'fixed' (the Data2Seq default) or 'timeF' (the Time-Series recipes' default)")
        self.embed_type = embed_type
        self.value_embedding = _TokenConv(c_in, d_model)
        self.position_embedding = _PosEmb(d_model)
        self.temporal_embedding = _Temporal(d_model, freq) if embed_type == "fixed" else _TimeFeature(d_model, freq)
        self.dropout = nn.Dropout(p=dropout)
        self.d_model = d_model

    def forward(self, x: torch.Tensor, x_mark: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not x.is_cuda:
            raise MetaEncError("DataEmbedding runs on MI355X only (CPU tensor given; no CPU fallback)")
        if x.requires_grad:
            raise MetaEncError("DataEmbedding: gradient w.r.t. the input series is not implemented (no reference pipeline "
                               "needs it); detach the input")
        B, L, cin = x.shape
        pe = self.position_embedding.pe[0]
        if L > pe.shape[0]:
            raise MetaEncError(f"sequence length {L} exceeds positional table {pe.shape[0]}")
        marks, tabs = None, []
        timef = self.embed_type == "timeF"
        if x_mark is not None and timef:
            d_inp = self.temporal_embedding.embed.in_features
            if x_mark.dim() != 3 or tuple(x_mark.shape[:2]) != (B, L) or x_mark.shape[-1] != d_inp:
                raise MetaEncError(f"x_mark must be [B, L, {d_inp}] time features for this freq, got {tuple(x_mark.shape)}")
            if x_mark.device != x.device:
                raise MetaEncError(f"x_mark is on {x_mark.device}, the series on {x.device}: move it first (no implicit copies)")
        elif x_mark is not None:
            tabs = [t.detach().float().contiguous() for t in self.temporal_embedding.tables()]
            if x_mark.shape[-1] < len(tabs):
                raise MetaEncError(f"x_mark has {x_mark.shape[-1]} columns, need {len(tabs)}")
            if x_mark.device != x.device:
                raise MetaEncError(f"x_mark is on {x_mark.device}, the series on {x.device}: move it first (no implicit copies; "
                                   "a host pointer handed to the kernel would fault the GPU)")
            marks = x_mark[..., :len(tabs)].long().to(torch.int32).contiguous()      # == x.long() (Time_Series.py:83)
        acast = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None
        if acast not in (None, torch.bfloat16, torch.float16, torch.float32):
            raise MetaEncError(f"autocast dtype {acast} unsupported")
        out_dtype = torch.bfloat16 if acast in (torch.bfloat16, torch.float16) else torch.float32      # fp16: bf16 compute, cast out
        p = float(self.dropout.p) if self.training else 0.0
        seed = int(torch.empty((), dtype=torch.int64).random_().item()) if p > 0 else 0
        if timef:      # value + positional from the fused kernel, + embed(x_mark) by a GEMM with that as residual, then the dropout
            y = _TSEmbedFn.apply(x.detach().float().contiguous(), self.value_embedding.tokenConv.weight, None, [], pe.contiguous(), out_dtype,
                                 0.0, 0)
            if x_mark is not None:
                y = _TimeFeatFn.apply(x_mark.detach().float().reshape(B * L, -1), self.temporal_embedding.embed.weight, y)
            if p > 0:
                y = _DropoutFn.apply(y, L, p, seed)
            return y.to(torch.float16) if acast == torch.float16 else y
        y = _TSEmbedFn.apply(x.detach().float().contiguous(), self.value_embedding.tokenConv.weight, marks, tabs,
                             pe.contiguous(), out_dtype, p, seed)
        return y.to(torch.float16) if acast == torch.float16 else y


class _TSEmbedFn(torch.autograd.Function):
    """DataEmbedding.forward (Data2Seq/Time_Series.py:118-126): value + temporal + positional embedding, Dropout(p).
    Backward: the only trainable tensor of the default (embed_type='fixed') configuration is the Conv1d weight;
    dW[C, cin, 3] = dY^T unfold(x) as one TN GEMM on the circularly unfolded input (me_timeseries_unfold)."""

    @staticmethod
    def forward(ctx, xf, weight, marks, tabs, pe, out_dtype, p, seed):
        lib = _capi.load()
        B, L, cin = xf.shape
        C = weight.shape[0]
        w = weight.detach().float().contiguous()
        out = torch.empty((B, L, C), dtype=out_dtype, device=xf.device)
        err = torch.zeros(1, dtype=torch.int32, device=xf.device)
        n_mark, tab_arr, rows_arr = len(tabs), None, None
        if marks is not None:
            tab_arr = (ctypes.c_void_p * n_mark)(*[t.data_ptr() for t in tabs])
            rows_arr = (ctypes.c_int32 * n_mark)(*[t.shape[0] for t in tabs])
        check(lib.me_timeseries_embed(ptr(xf), ptr(w), ptr(marks), n_mark if marks is not None else 0, tab_arr, rows_arr, ptr(pe),
                                      ptr(out), dtype_code(out_dtype), B, L, cin, C, ptr(err), stream_ptr()),
              "me_timeseries_embed")
        if marks is not None and int(err.item()) != 0:
            raise IndexError("x_mark holds an index outside its embedding table (nn.Embedding would raise too)")
        if p > 0:      # nn.Dropout(p) of Time_Series.py:126, training mode
            out = ops.dropout_add(out, None, L, p, 0.0, seed)
        ctx.save_for_backward(xf)
        ctx.meta = (p, seed, weight.dtype, weight.shape)
        return out

    @staticmethod
    def backward(ctx, dy):
        (xf,) = ctx.saved_tensors
        p, seed, wdt, wshape = ctx.meta
        if not ctx.needs_input_grad[1]:
            return (None,) * 8
        lib = _capi.load()
        B, L, cin = xf.shape
        C = wshape[0]
        dy2 = dy.contiguous()
        if p > 0:
            dy2 = ops.dropout_add(dy2, None, L, p, 0.0, seed)
        dy2 = ops.cast(dy2.reshape(B * L, C), torch.float32)
        ncols = (3 * cin + 3) // 4 * 4
        xu = torch.empty((B * L, ncols), dtype=torch.float32, device=xf.device)
        check(lib.me_timeseries_unfold(ptr(xf), ptr(xu), B, L, cin, ncols, stream_ptr()), "me_timeseries_unfold")
        dw = wgrad(dy2, xu)[0][:, :3 * cin].reshape(C, cin, 3).to(wdt)                 # [C, ncols] -> the Conv1d's [C, cin, 3]
        return (None, dw, None, None, None, None, None, None)


class _TimeFeatFn(torch.autograd.Function):
    """emb + feats W^T: the temporal term of DataEmbedding(embed_type='timeF').  feats [M, d_inp] fp32 and W [C, d_inp] are zero-padded to 8
    columns (one 16-byte bf16 row of the GEMM's operands); emb [B, L, C] is the GEMM's fused residual and fixes the compute dtype (bf16 under
    autocast, exact fp32 otherwise).  Backward: dW = dY^T feats (TN GEMM), d emb = dY."""

    @staticmethod
    def forward(ctx, feats, weight, emb):
        C, d_inp = weight.shape
        cdt = emb.dtype
        fc = pad_to(feats, 1).to(cdt).contiguous()
        wc = pad_to(weight.detach().float(), 1).to(cdt).contiguous()
        y = ops.gemm(fc, wc, residual=emb.reshape(-1, C).contiguous(), out_dtype=cdt)
        ctx.save_for_backward(fc)
        ctx.meta = (d_inp, weight.dtype, emb.shape)
        return y.reshape(emb.shape)

    @staticmethod
    def backward(ctx, dy):
        (fc,) = ctx.saved_tensors
        d_inp, wdt, eshape = ctx.meta
        dw = None
        if ctx.needs_input_grad[1]:
            dw = wgrad(ops.cast(dy.reshape(-1, eshape[-1]).contiguous(), fc.dtype), fc)[0][:, :d_inp].to(wdt)
        return None, dw, dy if ctx.needs_input_grad[2] else None


class _DropoutFn(torch.autograd.Function):
    """nn.Dropout(p) in training mode on me_dropout_add; backward regenerates the mask from the seed"""

    @staticmethod
    def forward(ctx, x, rows_per_sample, p, seed):
        ctx.meta = (rows_per_sample, p, seed)
        return ops.dropout_add(x.contiguous(), None, rows_per_sample, p, 0.0, seed)

    @staticmethod
    def backward(ctx, dy):
        rows_per_sample, p, seed = ctx.meta
        return ops.dropout_add(dy.contiguous(), None, rows_per_sample, p, 0.0, seed), None, None, None


def _graph_desc(node_data, edge_data, edge_index, offsets, atom, edge, graph_token, null_token, order, Z, perturb, dims):
    d = _capi.GraphDesc()
    d.node_data, d.edge_data, d.edge_index, d.offsets = ptr(node_data), ptr(edge_data), ptr(edge_index), ptr(offsets)
    d.atom, d.edge, d.graph_token, d.null_token = ptr(atom), ptr(edge), ptr(graph_token), ptr(null_token)
    d.order, d.Z, d.perturb = ptr(order), ptr(Z), ptr(perturb)
    d.B, d.T, d.C, d.Fn, d.Fe, d.Sn, d.Se, d.max_n = dims
    d.atom_rows, d.edge_rows = atom.shape[0], edge.shape[0]
    return d


def _f32c(t):
    return None if t is None else t.detach().float().contiguous()


class _GraphTokensFn(torch.autograd.Function):
    """me_graph_tokens_fwd / _bwd (include/metaenc.h): the whole padded batch in one launch; backward gathers along inverted
    index lists (deterministic).  Z has its rows padded to a multiple of 8 for the weight-gradient GEMM that follows."""

    @staticmethod
    def forward(ctx, atom, edge, graph_token, null_token, order, Z, perturb, node_data, edge_data, edge_index, offsets, dims, out_dtype):
        lib = _capi.load()
        B, T, C = dims[:3]
        par = [_f32c(t) for t in (atom, edge, graph_token, null_token, order, Z, perturb)]
        d = _graph_desc(node_data, edge_data, edge_index, offsets, *par, dims)
        dev = node_data.device
        out = torch.empty((B, T + 2, C), dtype=out_dtype, device=dev)
        pidx = torch.empty((B, T, 2), dtype=torch.int64, device=dev)
        pmask = torch.empty((B, T + 2), dtype=torch.bool, device=dev)
        check(lib.me_graph_tokens_fwd(ctypes.byref(d), ptr(out), dtype_code(out_dtype), ptr(pidx), ptr(pmask), stream_ptr()),
              "me_graph_tokens_fwd")
        ctx.save_for_backward(node_data, edge_data, edge_index, offsets, par[0], par[1], par[2], par[3])
        ctx.meta = (dims, tuple(None if t is None else (t.dtype, tuple(t.shape)) for t in (atom, edge, graph_token, null_token, order, Z, perturb)))
        ctx.mark_non_differentiable(pidx, pmask)
        return out, pmask, pidx

    @staticmethod
    def backward(ctx, dout, _dmask, _didx):
        lib = _capi.load()
        node_data, edge_data, edge_index, offsets, atom, edge, graph_token, null_token = ctx.saved_tensors
        dims, meta = ctx.meta
        dev = dout.device
        dout = dout.contiguous()
        if dout.dtype != torch.float32:
            dout = ops.cast(dout, torch.float32)
        grads = []
        for need, m in zip(ctx.needs_input_grad[:7], meta):
            grads.append(torch.empty(m[1], dtype=torch.float32, device=dev) if need and m is not None else None)
        dZ = grads[5]
        if dZ is not None and dZ.shape[0] > dims[5]:
            dZ[dims[5]:].zero_()                                  # the zero rows Z was padded with
        d = _graph_desc(node_data, edge_data, edge_index, offsets, atom, edge, graph_token, null_token, None, None, None, dims)
        nbytes = lib.me_graph_tokens_bwd_workspace(ctypes.byref(d))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib.me_graph_tokens_bwd(ctypes.byref(d), ptr(dout), *[ptr(g) for g in grads],
                                      _capi.ME_GRAPH_BWD_INDEX | _capi.ME_GRAPH_BWD_GATHER, ptr(ws), nbytes, stream_ptr()),
              "me_graph_tokens_bwd")
        grads = [g if g is None or g.dtype == m[0] else g.to(m[0]) for g, m in zip(grads, meta)]
        return (*grads, None, None, None, None, None, None)


def _init_graph_params(module, n_layers):
    """Data2Seq/Graph.py:34-40: Linear weights N(0, 0.02 / sqrt(n_layers)), Embedding tables N(0, 0.02) -- row 0 included: the
    padding rows are overwritten with noise, and read like any other row."""
    if isinstance(module, nn.Linear):
        module.weight.data.normal_(mean=0.0, std=0.02 / math.sqrt(n_layers))
        if module.bias is not None:
            module.bias.data.zero_()
    if isinstance(module, nn.Embedding):
        module.weight.data.normal_(mean=0.0, std=0.02)


class GraphFeatureTokenizer(nn.Module):
    """TokenGT graph tokenizer -- Data2Seq/Graph.py:43-305 (= Graph/metatransformer/modules/tokenizer.py): same constructor,
    same state-dict keys, same initialisation.  ``forward(batched_data, perturb=None)`` takes the collator's dict (``node_data
    [Sn, Fn]``, ``edge_data [Se, Fe]``, ``edge_index [2, Se]`` int64, ``node_num`` / ``edge_num`` Python lists, ``lap_eigvec
    [Sn, k']``; ``in_degree`` / ``out_degree`` / ``lap_eigval`` are accepted and unused, as in the reference) and returns
    ``(padded_feature [B, 2+T, C], padding_mask [B, 2+T] bool, padded_index [B, T, 2] int64)``.

    The identifier Linears act on cat(P[u], P[v]), so W cat(P[u], P[v]) = W_a P[u] + W_b P[v]: all identifier kinds go through ONE
    GEMM over the Sn node rows (Z = [P_rand | P_orf | P_lap] [W_a ; W_b]^T, [Sn, 2C]) and a token gathers two projected rows; the
    [B, T, 2D] index embeddings are never built.  The rest -- embedding sums, perturbation, type id, special tokens, padding, index
    and mask -- is one kernel (me_graph_tokens_fwd).  Backward is deterministic (me_graph_tokens_bwd).  Under torch.autocast the
    GEMM takes bf16 operands (fp32 result); the tokens are fp32, or bf16 for bf16 parameters.

    ``node_ids={"rand": [Sn, rand_node_id_dim], "orf": [Sn, orf_node_id_dim]}`` replaces the random draws (reproducible tokens).
    Still PyTorch glue, on the input's device: the uniform draw and F.normalize of the rand identifiers, the batched QR of the orf
    identifiers, pad / truncate to the configured widths, the training-mode eigenvector Dropout2d and random sign flip.
    Preconditions, as in the reference: table indices inside their tables, edge_index inside each graph's node range."""

    def __init__(self, num_atoms=1, num_edges=1, rand_node_id=1, rand_node_id_dim=768, orf_node_id=1, orf_node_id_dim=768,
                 lap_node_id=1, lap_node_id_k=1, lap_node_id_sign_flip=1, lap_node_id_eig_dropout=1, type_id=1, hidden_dim=1,
                 n_layers=1):
        super().__init__()
        self.encoder_embed_dim = hidden_dim
        self.atom_encoder = nn.Embedding(num_atoms, hidden_dim, padding_idx=0)
        self.edge_encoder = nn.Embedding(num_edges, hidden_dim, padding_idx=0)
        self.graph_token = nn.Embedding(1, hidden_dim)
        self.null_token = nn.Embedding(1, hidden_dim)
        self.rand_node_id, self.rand_node_id_dim = rand_node_id, rand_node_id_dim
        self.orf_node_id, self.orf_node_id_dim = orf_node_id, orf_node_id_dim
        self.lap_node_id, self.lap_node_id_k, self.lap_node_id_sign_flip = lap_node_id, lap_node_id_k, lap_node_id_sign_flip
        self.type_id = type_id
        if rand_node_id:
            self.rand_encoder = nn.Linear(2 * rand_node_id_dim, hidden_dim, bias=False)
        if lap_node_id:
            self.lap_encoder = nn.Linear(2 * lap_node_id_k, hidden_dim, bias=False)
            self.lap_eig_dropout = nn.Dropout2d(p=lap_node_id_eig_dropout) if lap_node_id_eig_dropout > 0 else None
        if orf_node_id:
            self.orf_encoder = nn.Linear(2 * orf_node_id_dim, hidden_dim, bias=False)
        if type_id:
            self.order_encoder = nn.Embedding(2, hidden_dim)
        self.apply(lambda m: _init_graph_params(m, n_layers=n_layers))

    # ---- host-side checks and index arrays (Python lists and shapes only: no device synchronisation)
    def _check(self, bd, perturb, node_ids):
        who = "GraphFeatureTokenizer"
        for k in ("node_data", "edge_data", "edge_index", "node_num", "edge_num"):
            if k not in bd:
                raise MetaEncError(f"{who}: batched_data has no '{k}'")
        node_data, edge_data, edge_index = bd["node_data"], bd["edge_data"], bd["edge_index"]
        for k in ("node_data", "edge_data", "edge_index"):
            t = bd[k]
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise MetaEncError(f"{who}: {k} must be a CUDA tensor (no CPU fallback)")
            if t.dtype != torch.int64:
                raise MetaEncError(f"{who}: {k} must be int64 (got {t.dtype})")
            if t.device != node_data.device:
                raise MetaEncError(f"{who}: {k} is on {t.device}, node_data on {node_data.device}")
        if self.atom_encoder.weight.device != node_data.device:
            raise MetaEncError(f"{who}: parameters are on {self.atom_encoder.weight.device}, node_data on {node_data.device}")
        node_num, edge_num = [int(v) for v in bd["node_num"]], [int(v) for v in bd["edge_num"]]
        if len(node_num) == 0 or len(node_num) != len(edge_num):
            raise MetaEncError(f"{who}: node_num / edge_num must be non-empty lists of one length (got {len(node_num)}, {len(edge_num)})")
        if min(node_num) < 0 or min(edge_num) < 0:
            raise MetaEncError(f"{who}: node_num / edge_num hold a negative count")
        if node_data.dim() != 2 or sum(node_num) != node_data.size(0):
            raise MetaEncError(f"{who}: node_data {tuple(node_data.shape)} must be [sum(node_num) = {sum(node_num)}, features]")
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or sum(edge_num) != edge_index.size(1):
            raise MetaEncError(f"{who}: edge_index {tuple(edge_index.shape)} must be [2, sum(edge_num) = {sum(edge_num)}]")
        if edge_data.dim() != 2 or sum(edge_num) != edge_data.size(0):
            raise MetaEncError(f"{who}: edge_data {tuple(edge_data.shape)} must be [sum(edge_num) = {sum(edge_num)}, features]")
        Sn, max_n, B = sum(node_num), max(node_num), len(node_num)
        if self.lap_node_id:
            lap = bd.get("lap_eigvec")
            if not isinstance(lap, torch.Tensor) or not lap.is_cuda:
                raise MetaEncError(f"{who}: lap_eigvec must be a CUDA tensor (no CPU fallback)")
            if not lap.is_floating_point():
                raise MetaEncError(f"{who}: lap_eigvec must be a floating-point tensor (got {lap.dtype})")
            if lap.dim() != 2 or lap.size(0) != Sn:
                raise MetaEncError(f"{who}: lap_eigvec {tuple(lap.shape)} must have one row per node ({Sn})")
        if perturb is not None:
            if not isinstance(perturb, torch.Tensor) or not perturb.is_cuda:
                raise MetaEncError(f"{who}: perturb must be a CUDA tensor (no CPU fallback)")
            if tuple(perturb.shape) != (B, max_n, self.encoder_embed_dim):
                raise MetaEncError(f"{who}: perturb {tuple(perturb.shape)} must be [B, max(node_num), C] = "
                                   f"({B}, {max_n}, {self.encoder_embed_dim})")
        for kind, width in (("rand", self.rand_node_id_dim), ("orf", self.orf_node_id_dim)):
            t = (node_ids or {}).get(kind)
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or tuple(t.shape) != (Sn, width)):
                raise MetaEncError(f"{who}: node_ids['{kind}'] must be a CUDA tensor [{Sn}, {width}]")
        unknown = set(node_ids or {}) - {"rand", "orf"}
        if unknown:
            raise MetaEncError(f"{who}: node_ids has unknown kinds {sorted(unknown)} (rand, orf)")
        return node_num, edge_num

    @staticmethod
    def _node_places(node_num, device):
        """(graph of node [Sn], b * max_n + local number [Sn]) built on the host"""
        max_n = max(node_num)
        graph, flat = [], []
        for b, n in enumerate(node_num):
            graph.extend([b] * n)
            flat.extend(range(b * max_n, b * max_n + n))
        both = torch.tensor([graph, flat], dtype=torch.int64).to(device, non_blocking=True)
        return both[0], both[1]

    def _identifiers(self, bd, node_num, node_ids):
        """[(kind, P [Sn, D] fp32, Linear weight [C, 2D])] in the reference's order of addition"""
        node_ids = node_ids or {}
        dev = bd["node_data"].device
        Sn, B, max_n = sum(node_num), len(node_num), max(node_num)
        places = None
        out = []
        if self.rand_node_id:
            p = node_ids.get("rand")
            if p is None:
                p = F.normalize(torch.rand(Sn, self.rand_node_id_dim, device=dev, dtype=torch.float32), p=2, dim=1)
            out.append(("rand", p.float(), self.rand_encoder.weight))
        if self.orf_node_id:
            p = node_ids.get("orf")
            if p is None:
                places = places or self._node_places(node_num, dev)
                q, _ = torch.linalg.qr(torch.randn(B, max_n, max_n, device=dev), mode="reduced")
                orf = F.normalize(q.transpose(2, 1), p=2, dim=2).reshape(B * max_n, max_n).index_select(0, places[1])
                if self.orf_node_id_dim > max_n:
                    orf = F.pad(orf, (0, self.orf_node_id_dim - max_n), value=0.0)
                else:
                    orf = orf[..., :self.orf_node_id_dim]
                p = F.normalize(orf, p=2, dim=1)
            out.append(("orf", p.float(), self.orf_encoder.weight))
        if self.lap_node_id:
            eig = bd["lap_eigvec"].float()
            k = eig.size(-1)
            eig = F.pad(eig, (0, self.lap_node_id_k - k), value=0.0) if self.lap_node_id_k > k else eig[:, :self.lap_node_id_k]
            if self.lap_eig_dropout is not None:
                eig = self.lap_eig_dropout(eig[..., None, None]).view(eig.size())
            if self.lap_node_id_sign_flip and self.training:
                places = places or self._node_places(node_num, dev)
                sign = torch.rand(B, eig.size(1), device=dev, dtype=eig.dtype)
                sign = torch.where(sign >= 0.5, 1.0, -1.0).to(eig.dtype)
                eig = eig * sign.index_select(0, places[0])
            out.append(("lap", eig, self.lap_encoder.weight))
        return out

    @torch.no_grad()
    def node_identifiers(self, batched_data, node_ids=None):
        """the [Sn, D] node identifiers a forward would use, by kind (fresh draws where node_ids gives none)"""
        node_num, _ = self._check(batched_data, None, node_ids)
        return {kind: p for kind, p, _ in self._identifiers(batched_data, node_num, node_ids)}

    def _project(self, ids, Sn):
        """Z [Sn padded to 8, 2C]: one GEMM for every identifier kind, K = the widths side by side (padded to a multiple of 8)"""
        C = self.encoder_embed_dim
        dev = ids[0][1].device
        cdt = torch.bfloat16 if torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") in (torch.bfloat16, torch.float16) \
            else torch.float32
        K = sum(p.shape[1] for _, p, _ in ids)
        Kp, rows = (K + 7) // 8 * 8, (Sn + 7) // 8 * 8
        P = torch.zeros((rows, Kp), dtype=cdt, device=dev)
        ws, at = [], 0
        for _, p, w in ids:
            D = p.shape[1]
            P[:Sn, at:at + D] = p
            ws.append(w.view(C, 2, D).permute(1, 0, 2).reshape(2 * C, D))          # [W_a ; W_b]
            at += D
        W = ws[0] if len(ws) == 1 else torch.cat(ws, dim=1)
        # the dtype policy of heads.linear (fp32 rows -> the exact fp32 MFMA, bf16 rows -> bf16 MFMA, fp32 result either way); the identifiers
        # carry no gradient, so backward is the one TN GEMM dW = dZ^T P
        return linear(P, W, None, compute_dtype=cdt)

    def forward(self, batched_data, perturb=None, node_ids=None):
        node_num, edge_num = self._check(batched_data, perturb, node_ids)
        node_data, edge_data, edge_index = (batched_data[k].contiguous() for k in ("node_data", "edge_data", "edge_index"))
        dev = node_data.device
        B, Sn, Se, max_n = len(node_num), sum(node_num), sum(edge_num), max(node_num)
        T = max(n + e for n, e in zip(node_num, edge_num))
        C = self.encoder_embed_dim
        if C % 4 != 0:
            raise MetaEncError(f"GraphFeatureTokenizer: hidden_dim {C} must be a multiple of 4")
        offs = [0]
        for n in node_num:
            offs.append(offs[-1] + n)
        offs.append(0)
        for e in edge_num:
            offs.append(offs[-1] + e)
        offsets = torch.tensor(offs, dtype=torch.int32).to(dev, non_blocking=True)
        ids = self._identifiers(batched_data, node_num, node_ids)
        Z = self._project(ids, Sn) if ids and Sn > 0 else None
        wdt = self.atom_encoder.weight.dtype
        if wdt not in (torch.float32, torch.bfloat16):
            raise MetaEncError(f"GraphFeatureTokenizer: parameter dtype {wdt} unsupported (fp32, bf16)")
        dims = (B, T, C, node_data.shape[1], edge_data.shape[1], Sn, Se, max_n)
        order = self.order_encoder.weight if self.type_id else None
        return _GraphTokensFn.apply(self.atom_encoder.weight, self.edge_encoder.weight, self.graph_token.weight, self.null_token.weight,
                                    order, Z, perturb, node_data, edge_data, edge_index, offsets, dims, wdt)


class Data2Seq(nn.Module):
    """``Data2Seq(modality, dim)`` dispatcher -- API shape of Data2Seq/Data2Seq.py:19-55 (which itself does not run
    as written: SURVEY.md appendix A).  Multi-modal use concatenates along tokens exactly as README.md:118-122:
    ``features = torch.concat([image_tokenizer(img), ts_tokenizer(ts), audio_tokenizer(spec)], dim=1)``."""

    def __init__(self, modality: str, dim: int, **kw):
        super().__init__()
        self.modality = modality
        if modality == "image":
            self.embed = PatchEmbed(embed_dim=dim, **kw)
        elif modality == "audio":
            self.embed = AcousticPatchEmbed(embed_dim=dim, **kw)
        elif modality == "video":
            self.embed = VideoPatchEmbed(embed_dim=dim, **kw)
        elif modality == "time-series":
            self.embed = DataEmbedding(c_in=kw.pop("c_in", 1), d_model=dim, **kw)
        elif modality == "graph":       # Data2Seq/Data2Seq.py:32: both identifier widths follow dim, everything else default
            self.embed = GraphFeatureTokenizer(rand_node_id_dim=dim, orf_node_id_dim=dim, **kw)
        elif modality == "hyper":       # Hyper-spectrum/metatransformer.py:111-118; the reference's defaults there are not runnable
            from .hyperspectral import HyperSpectralEmbed
            missing = [k for k in ("bands", "patch", "near_band") if k not in kw]
            if missing:
                raise MetaEncError(f"Data2Seq('hyper', dim): keyword(s) {missing} required (bands, patch, near_band)")
            self.embed = HyperSpectralEmbed(embed_dim=dim, **kw)
        else:
            raise MetaEncError(f"modality '{modality}' has no HIP tokenizer (in scope: image, audio, video, time-series, graph, hyper)")

    def forward(self, data, *args, **kw):
        return self.embed(data, *args, **kw)
