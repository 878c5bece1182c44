"""The audio recipe from waveform to logits on the HIP path (Audio/src/dataloader.py:98-205, Audio/src/models/ast_models.py:35-167).

The reference's audio tokenizer is the filterbank itself: ``torchaudio.compliance.kaldi.fbank(waveform, htk_compat=True,
sample_frequency=sr, use_energy=False, window_type='hanning', num_mel_bins=..., dither=0.0, frame_shift=10)`` (Data2Seq/Data2Seq.py:38-45),
one clip at a time on the CPU inside the dataloader, followed by cut / pad to ``target_length``, the SpecAug masks and
``(x - mean) / (2 std)``.  Here a batch of padded waveforms stays on the device:

  KaldiFbank(sample_frequency, num_mel_bins, target_length, norm_mean, norm_std)
      ``forward(wave [B, n], lengths, mix, freq_mask, time_mask)`` -> ``[B, target_length, num_mel_bins]``: one me_fbank call (mean
      removal and mix-up, framing, pre-emphasis, Hann window, power spectrum, mel filters, log, cut / pad, masks, normalisation)
  mel_filterbank / fbank_tables      the float64 builders of the tables me_fbank reads (the library keeps none)
  specaug_bands                      the bands torchaudio's FrequencyMasking / TimeMasking would draw, as int32 ``[B, 2]`` tensors
  ASTModel(label_dim, fstride, tstride, input_fdim, input_tdim, ...)
      the reference's classifier with its constructor and state-dict keys, on AcousticPatchEmbed, this package's Blocks and the
      fused LayerNorm / Linear of heads.py; ``encoder=`` takes the Block stack the reference loads from a file inside ``__init__``

The dataloader's ``noise=True`` branch (uniform noise, ``torch.roll``) is two torch ops on the result and stays with the caller; file
decoding, resampling and ``audioset_pretrain`` are out of scope.
"""
from __future__ import annotations

import ctypes
import math
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from . import _capi, ops
from ._capi import MetaEncError, check, dtype_code, ptr, stream_ptr
from .data2seq import AcousticPatchEmbed, _PatchEmbedFn, _boundary_dtypes

FRAMES_PER_WORKGROUP = _capi.ME_FBANK_RUN      # output rows one workgroup of me_fbank owns
LOW_FREQ = 20.0                    # Kaldi's default low edge of the mel filters


def frame_geometry(sample_frequency: int):
    """(win, shift, padded): 25 ms frames every 10 ms, transformed at the next power of two"""
    win, shift = int(sample_frequency * 0.025), int(sample_frequency * 0.010)
    if win < 2 or shift < 1:
        raise MetaEncError(f"sample_frequency {sample_frequency} gives a {win}-sample window")
    padded = 1 << (win - 1).bit_length()
    return win, shift, padded


def mel_filterbank(sample_frequency: int = 16000, num_mel_bins: int = 128) -> torch.Tensor:
    """float64 ``[num_mel_bins, padded / 2]``: Kaldi's triangular filters (htk_compat, low edge 20 Hz, high edge Nyquist) over the FFT
    bins below Nyquist; the Nyquist bin's weight is 0 and has no column."""
    if num_mel_bins < 1:
        raise MetaEncError(f"num_mel_bins={num_mel_bins}")
    _, _, padded = frame_geometry(sample_frequency)
    mel_lo = 1127.0 * math.log(1.0 + LOW_FREQ / 700.0)
    mel_hi = 1127.0 * math.log(1.0 + 0.5 * sample_frequency / 700.0)
    delta = (mel_hi - mel_lo) / (num_mel_bins + 1)
    left = mel_lo + torch.arange(num_mel_bins, dtype=torch.float64)[:, None] * delta
    center = left + delta
    right = center + delta
    freq = torch.arange(padded // 2, dtype=torch.float64) * (sample_frequency / padded)
    m = (1127.0 * torch.log(1.0 + freq / 700.0))[None, :]
    return torch.clamp_min(torch.minimum((m - left) / (center - left), (right - m) / (right - center)), 0.0)


def fbank_tables(sample_frequency: int = 16000, num_mel_bins: int = 128) -> dict:
    """The tables of me_fbank in float64 (the caller rounds them once to fp32): ``window [win]`` = hann_window(win, periodic=False),
    ``twiddle [padded, 2]`` = (cos, -sin)(2 pi n / padded), ``mel_range`` int32 ``[n_mel, 2]`` = (first bin, count) of every filter's
    non-zero weights, ``mel_weight [n_mel, mel_ld]`` = those weights from the first bin on; plus ``win``, ``shift``, ``padded``."""
    win, shift, padded = frame_geometry(sample_frequency)
    n = torch.arange(win, dtype=torch.float64)
    window = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / (win - 1))
    ang = 2.0 * math.pi * torch.arange(padded, dtype=torch.float64) / padded
    twiddle = torch.stack([torch.cos(ang), -torch.sin(ang)], dim=1)
    banks = mel_filterbank(sample_frequency, num_mel_bins)
    # against the fp32 value the kernel multiplies with: a weight that rounds to zero belongs to no range
    nz = banks.float() != 0
    count = nz.sum(1)
    first = torch.where(count > 0, nz.float().argmax(1), torch.zeros_like(count))
    last = torch.where(count > 0, banks.shape[1] - 1 - nz.flip(1).float().argmax(1), first - 1)
    span = last - first + 1
    mel_ld = max(int(span.max()), 1)
    weight = torch.zeros(num_mel_bins, mel_ld, dtype=torch.float64)
    for b in range(num_mel_bins):
        c = int(span[b])
        weight[b, :c] = banks[b, int(first[b]):int(first[b]) + c]
    return {"win": win, "shift": shift, "padded": padded, "window": window, "twiddle": twiddle,
            "mel_range": torch.stack([first, span], dim=1).to(torch.int32), "mel_weight": weight}


def specaug_bands(B: int, n_freq: int, n_time: int, freqm: int, timem: int, generator: Optional[torch.Generator] = None):
    """(freq_mask, time_mask), int32 ``[B, 2]`` each: the ``[start, end)`` bands torchaudio's ``mask_along_axis`` draws for
    FrequencyMasking(freqm) / TimeMasking(timem) (dataloader.py:186-198), one pair per clip: ``value = rand * param``,
    ``start = int(rand * (size - value))``, ``end = start + int(value)``.  A parameter of 0 gives empty bands."""
    def draw(size: int, param: int) -> torch.Tensor:
        if param < 0 or param > size:
            raise MetaEncError(f"specaug_bands: mask parameter {param} outside [0, {size}]")
        value = torch.rand(B, generator=generator, dtype=torch.float64) * param
        start = (torch.rand(B, generator=generator, dtype=torch.float64) * (size - value)).long()
        return torch.stack([start, start + value.long()], dim=1).to(torch.int32)
    return draw(n_freq, freqm), draw(n_time, timem)


class KaldiFbank(nn.Module):
    """Waveforms to (normalised, masked, padded) log-mel filterbanks, a batch per call: ``forward(wave [B, n] fp32, lengths=None,
    mix=None, freq_mask=None, time_mask=None)`` -> ``[B, target_length, num_mel_bins]`` (``target_length=None``: the frame count of the
    longest clip, which costs one host read of ``lengths``).  ``lengths`` int32 ``[B]``: samples of every clip (the rest of a row is
    padding and is never read); ``mix = (wave2, lengths2, lam [B])``: the mix-up partner of dataloader.py:105-127; ``freq_mask`` /
    ``time_mask`` int32 ``[B, 2]``: ``[start, end)`` bands set to zero before the normalisation (``specaug_bands`` draws them).
    ``norm_mean`` / ``norm_std`` both None: no normalisation (the reference's ``skip_norm``).  No parameters, no gradient."""

    def __init__(self, sample_frequency: int = 16000, num_mel_bins: int = 128, target_length: Optional[int] = None,
                 norm_mean: Optional[float] = None, norm_std: Optional[float] = None, out_dtype: torch.dtype = torch.float32):
        super().__init__()
        if (norm_mean is None) != (norm_std is None):
            raise MetaEncError("KaldiFbank: give norm_mean and norm_std together (or neither)")
        if norm_std is not None and float(norm_std) == 0.0:
            raise MetaEncError("KaldiFbank: norm_std = 0")
        if target_length is not None and target_length < 0:
            raise MetaEncError(f"KaldiFbank: target_length={target_length}")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise MetaEncError(f"KaldiFbank: out_dtype {out_dtype} (float32 or bfloat16)")
        self.sample_frequency, self.num_mel_bins, self.target_length = int(sample_frequency), int(num_mel_bins), target_length
        self.norm_mean, self.norm_std, self.out_dtype = norm_mean, norm_std, out_dtype
        t = fbank_tables(self.sample_frequency, self.num_mel_bins)
        self.win, self.shift, self.padded = t["win"], t["shift"], t["padded"]
        for name in ("window", "twiddle", "mel_weight"):
            self.register_buffer(name, t[name].float().contiguous(), persistent=False)
        self.register_buffer("mel_range", t["mel_range"].contiguous(), persistent=False)

    def num_frames(self, length: int) -> int:
        return 1 + (length - self.win) // self.shift if length >= self.win else 0

    @staticmethod
    def _wave(who: str, wave, dev=None) -> torch.Tensor:
        if not isinstance(wave, torch.Tensor) or not wave.is_cuda:
            raise MetaEncError(f"{who} runs on MI355X only (CPU tensor given; no CPU fallback)")
        if wave.dim() != 2:
            raise MetaEncError(f"{who}: waveforms {tuple(wave.shape)} must be [B, samples]")
        if dev is not None and wave.device != dev:
            raise MetaEncError(f"{who}: tensors on {wave.device} and {dev}: move them first (no implicit copies)")
        wave = wave.detach()
        if wave.dtype != torch.float32:
            wave = wave.float()
        return wave if wave.stride(1) == 1 and wave.stride(0) >= wave.shape[1] else wave.contiguous()

    @staticmethod
    def _ints(who: str, name: str, t, shape, dev) -> Optional[torch.Tensor]:
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or tuple(t.shape) != shape:
            raise MetaEncError(f"{who}: {name} must be an integer tensor of shape {shape}")
        if t.device != dev:
            raise MetaEncError(f"{who}: {name} is on {t.device}, the waveforms on {dev}: move it first (no implicit copies)")
        return t.to(torch.int32).contiguous()

    @torch.no_grad()
    def forward(self, wave, lengths=None, mix=None, freq_mask=None, time_mask=None) -> torch.Tensor:
        who = "KaldiFbank"
        lib = _capi.load()
        wave = self._wave(who, wave)
        dev = wave.device
        if self.window.device != dev:
            raise MetaEncError(f"{who}: its tables are on {self.window.device}, the waveforms on {dev}: move the module first")
        B, n = wave.shape
        lengths = self._ints(who, "lengths", lengths, (B,), dev)
        d = _capi.FbankDesc()
        d.wave, d.ld_wave, d.lengths, d.B, d.n_samples = ptr(wave), wave.stride(0) if B else n, ptr(lengths), B, n
        if mix is not None:
            wave2, lengths2, lam = mix
            wave2 = self._wave(who, wave2, dev)
            if wave2.shape[0] != B:
                raise MetaEncError(f"{who}: the mix-up partner has {wave2.shape[0]} clips, the batch {B}")
            lengths2 = self._ints(who, "lengths2", lengths2, (B,), dev)
            if not isinstance(lam, torch.Tensor) or tuple(lam.shape) != (B,) or lam.device != dev:
                raise MetaEncError(f"{who}: lam must be a [{B}] tensor on {dev}")
            lam = lam.detach().float().contiguous()
            d.wave2, d.ld_wave2, d.lengths2, d.lam, d.n_samples2 = ptr(wave2), wave2.stride(0) if B else wave2.shape[1], ptr(lengths2), ptr(lam), wave2.shape[1]
        freq_mask = self._ints(who, "freq_mask", freq_mask, (B, 2), dev)
        time_mask = self._ints(who, "time_mask", time_mask, (B, 2), dev)
        L = self.target_length
        if L is None:
            longest = n if lengths is None or B == 0 else min(max(int(lengths.max()), 0), n)
            L = self.num_frames(longest)
        out = torch.empty((B, L, self.num_mel_bins), dtype=self.out_dtype, device=dev)
        d.win, d.shift, d.padded, d.n_mel, d.mel_ld, d.target_length = self.win, self.shift, self.padded, self.num_mel_bins, self.mel_weight.shape[1], L
        d.window, d.twiddle, d.mel_range, d.mel_weight = ptr(self.window), ptr(self.twiddle), ptr(self.mel_range), ptr(self.mel_weight)
        d.freq_mask, d.time_mask = ptr(freq_mask), ptr(time_mask)
        if self.norm_mean is not None:
            d.normalize, d.norm_mean, d.norm_std = 1, float(self.norm_mean), float(self.norm_std)
        d.out, d.out_dtype, d.ld_out = ptr(out), dtype_code(self.out_dtype), self.num_mel_bins
        nbytes = lib.me_fbank_workspace_bytes(ctypes.byref(d))
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        check(lib.me_fbank(ctypes.byref(d), ptr(ws), nbytes, stream_ptr()), "me_fbank")
        return out


def _transpose_clips(x: torch.Tensor) -> torch.Tensor:
    """``[B, rows, cols]`` -> ``[B, cols, rows]`` contiguous: me_transpose_cast_batched, ME_TC_BATCH clips per launch"""
    lib = _capi.load()
    B, rows, cols = x.shape
    x = x.contiguous()
    y = torch.empty((B, cols, rows), dtype=x.dtype, device=x.device)
    for i in range(0, B, _capi.ME_TC_BATCH):
        tb = _capi.TcBatch()
        tb.n, tb.src_dtype, tb.dst_dtype = min(_capi.ME_TC_BATCH, B - i), dtype_code(x.dtype, True), dtype_code(x.dtype, True)
        for k in range(tb.n):
            tb.item[k].src, tb.item[k].dst, tb.item[k].rows, tb.item[k].cols = x[i + k].data_ptr(), y[i + k].data_ptr(), rows, cols
        check(lib.me_transpose_cast_batched(ctypes.byref(tb), stream_ptr()), "me_transpose_cast_batched")
    return y


class _SpecToImageFn(torch.autograd.Function):
    """``[B, T, F]`` -> ``[B, 1, F, T]`` contiguous, the layout the patch embed gathers from (ast_models.py:152-153's unsqueeze and
    transpose, which the reference's Conv2d reads through strides)"""

    @staticmethod
    def forward(ctx, x):
        return _transpose_clips(x).unsqueeze(1)

    @staticmethod
    def backward(ctx, dy):
        return _transpose_clips(dy.squeeze(1))


class _AddPosFn(torch.autograd.Function):
    """tokens ``[B, N, C]`` + pos ``[1, N, C]`` (me_add_rows); the position gradient is the sum over the batch (me_colsum)"""

    @staticmethod
    def forward(ctx, x, pos):
        B, N, C = x.shape
        ctx.meta = (tuple(pos.shape), pos.dtype)
        p = pos.detach().reshape(N, C).contiguous()
        if p.dtype == torch.float16:
            p = p.float()
        return ops.add_rows(x.contiguous(), p)

    @staticmethod
    def backward(ctx, dy):
        pshape, pdt = ctx.meta
        dpos = None
        if ctx.needs_input_grad[1]:
            d2 = dy.contiguous().reshape(dy.shape[0], -1)
            if d2.dtype == torch.float16:
                d2 = ops.cast(d2, torch.bfloat16)
            dpos = ops.colsum(d2).reshape(pshape).to(pdt)
        return dy, dpos


class _ASTBackbone(nn.Module):
    """the attributes of the timm VisionTransformer that ast_models.py keeps under ``self.v``"""

    def __init__(self, dim: int, patch: int, fstride: int, tstride: int, num_patches: int, encoder: nn.Module):
        super().__init__()
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, dim))
        self.pos_drop = nn.Dropout(0.0)
        self.patch_embed = AcousticPatchEmbed(patch_size=patch, in_chans=1, embed_dim=dim, fstride=fstride, tstride=tstride)
        self.patch_embed.num_patches = num_patches
        self.blocks = encoder
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.head = nn.Linear(dim, 1000)                       # timm's ImageNet head: a key of the state dict, never called
        self.dist_token = nn.Parameter(torch.zeros(1, 1, dim))


class ASTModel(nn.Module):
    """Audio/src/models/ast_models.py:35-167 with the reference's constructor, attribute names and state-dict keys (``v.cls_token``,
    ``v.dist_token``, ``v.pos_embed``, ``v.patch_embed.proj.*``, ``v.blocks.{i}.*``, ``v.norm.*``, ``v.head.*``, ``mlp_head.{0,1}.*``).
    ``encoder=`` is the stack of this package's Blocks that the reference loads from a checkpoint file inside ``__init__`` (default:
    ``build_encoder(12, 768, 12)`` with LayerNorm eps 1e-6, untrained); no file is read.

    ``forward(x [B, time frames, frequency bins])`` -> ``[B, label_dim]`` does what the reference's forward does, as it is written:
    the patch embed reads ``x`` as ``[B, 1, F, T]``; with ``imagenet_pretrain=True`` its weight is the channel-summed patch-32 weight
    ``[C, 1, 32, 32]`` applied at stride ``(fstride, tstride)``, with ``False`` a 16 x 16 one; ``v.pos_embed`` has ``(f_dim - 1)(t_dim -
    1)`` rows, ``f_dim, t_dim`` the 16 x 16 patch counts of ``get_shape``; cls and dist tokens are parameters that are NOT
    concatenated; then ``+ pos_embed``, the Blocks, ``v.norm``, the mean of tokens 0 and 1, ``mlp_head``.  Where the reference dies on a
    broadcast -- the token count differs from the position rows -- this raises MetaEncError with both numbers.  As in the reference,
    everything under ``v`` except ``pos_embed`` and ``patch_embed.proj.weight`` is frozen.  ``audioset_pretrain=True`` raises (it needs
    a download).  The reference's ``@autocast()`` is ``torch.autocast('cuda', torch.bfloat16)`` around the call: bf16 arithmetic on an
    fp32 token stream; the two LayerNorms and the Linear behind the pooled pair stay fp32 (2 rows per clip)."""

    def __init__(self, label_dim=527, fstride=10, tstride=10, input_fdim=224, input_tdim=1024, imagenet_pretrain=True,
                 audioset_pretrain=False, model_size="base384", verbose=True, encoder: Optional[nn.Module] = None):
        super().__init__()
        if audioset_pretrain:
            raise MetaEncError("ASTModel: audioset_pretrain=True needs the reference's AudioSet checkpoint download and is not supported; "
                               "load such weights with load_state_dict")
        if encoder is None:
            from .encoder import build_encoder
            encoder = build_encoder(12, 768, 12, norm_layer=partial(nn.LayerNorm, eps=1e-6))
        if len(encoder) < 1:
            raise MetaEncError("ASTModel: the encoder holds no Block")
        dim = encoder[0].norm1.weight.shape[0]
        self.original_embedding_dim = dim
        self.fstride, self.tstride, self.input_fdim, self.input_tdim = fstride, tstride, input_fdim, input_tdim
        self.patch = 32 if imagenet_pretrain else 16
        f_dim, t_dim = self.get_shape(fstride, tstride, input_fdim, input_tdim)
        num_patches = (f_dim - 1) * (t_dim - 1)
        if num_patches < 2:
            raise MetaEncError(f"ASTModel: a {input_fdim} x {input_tdim} input gives {num_patches} position rows; the forward averages tokens 0 and 1")
        if verbose:
            print("---------------AST Model Summary---------------")
            print(f"ImageNet pretraining: {imagenet_pretrain}, AudioSet pretraining: {audioset_pretrain}")
            print(f"frequncey stride={fstride:d}, time stride={tstride:d}")
            print(f"number of patches={num_patches:d}")
        self.v = _ASTBackbone(dim, self.patch, fstride, tstride, num_patches, encoder)
        nn.init.trunc_normal_(self.v.pos_embed, std=.02)
        for name, p in self.v.named_parameters():
            if name not in ("pos_embed", "patch_embed.proj.weight"):
                p.requires_grad = False
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, label_dim))

    def get_shape(self, fstride, tstride, input_fdim=224, input_tdim=1024):
        """the output grid of a 16 x 16 convolution at these strides (the reference runs one to find out)"""
        if input_fdim < 16 or input_tdim < 16:
            raise MetaEncError(f"ASTModel: input {input_fdim} x {input_tdim} is smaller than a 16 x 16 patch")
        return (input_fdim - 16) // fstride + 1, (input_tdim - 16) // tstride + 1

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .heads import _LayerNormFn, linear, pool_tokens
        who = "ASTModel"
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise MetaEncError(f"{who}: the input must be a [batch, time frames, frequency bins] tensor")
        B, T, F = x.shape
        k = self.patch
        tokens = ((F - k) // self.fstride + 1) * ((T - k) // self.tstride + 1) if F >= k and T >= k else 0
        rows = self.v.pos_embed.shape[1]
        if tokens != rows:
            raise MetaEncError(f"{who}: a [{T} frames, {F} bins] input gives {tokens} tokens through the {k} x {k} patch embed at stride "
                               f"({self.fstride}, {self.tstride}), but v.pos_embed holds {rows} rows (the reference fails on this broadcast)")
        if not x.is_cuda:
            raise MetaEncError(f"{who} runs on MI355X only (CPU tensor given; no CPU fallback)")
        pe = self.v.patch_embed
        w = pe.proj.weight
        if w.device != x.device:
            raise MetaEncError(f"{who}: parameters are on {w.device}, the input on {x.device}")
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float() if x.dtype != torch.float16 else ops.cast(x.contiguous(), torch.bfloat16)
        cdt, odt = _boundary_dtypes(w)
        sdt = torch.float32 if w.dtype == torch.float32 else odt      # the token stream stays fp32 while the parameters are
        img = _SpecToImageFn.apply(x.contiguous())
        t = _PatchEmbedFn.apply(img, w, pe.proj.bias, None, pe.geom, cdt, 0, sdt)
        t = self.v.pos_drop(_AddPosFn.apply(t, self.v.pos_embed))
        for blk in self.v.blocks:
            t = blk(t)
        C = t.shape[-1]
        ln, (ln2, fc) = self.v.norm, self.mlp_head
        # LayerNorm is per token: only tokens 0 and 1 are normalised
        pair = _LayerNormFn.apply(t[:, :2].reshape(B * 2, C), ln.weight, ln.bias, ln.eps)
        f = pool_tokens(pair.reshape(B, 2, C), "mean")
        return linear(_LayerNormFn.apply(f, ln2.weight, ln2.bias, ln2.eps), fc.weight, fc.bias)
