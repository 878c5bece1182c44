"""The Kaldi filterbank of the Audio recipe restated in torch, and the inputs the audio tests share.

``torchaudio.compliance.kaldi.fbank(waveform, htk_compat=True, sample_frequency=sr, use_energy=False, window_type='hanning',
num_mel_bins=n, dither=0.0, frame_shift=10)`` as Audio/src/dataloader.py:98-205 calls it, with the steps around it (mean removal,
mix-up, cut / pad, SpecAug bands, normalisation), written out step by step in the dtype asked for -- float64 is the reference, float32
its own rounding error (the yardstick of the device kernel's bound).  The transform is ``torch.fft.rfft``.  A plain module (like
ew_cases.py): it imports nothing of the package, its tables are built here."""
from __future__ import annotations

import math

import torch

EPS = 1.1920929e-07                     # fp32 machine epsilon: the floor under the log
PREEMPH = 0.97
LOW_FREQ = 20.0


def geometry(sr: int):
    """(win, shift, padded): 25 ms window, 10 ms shift, next power of two"""
    win, shift = int(sr * 0.025), int(sr * 0.010)
    padded = 1
    while padded < win:
        padded *= 2
    return win, shift, padded


def num_frames(length: int, sr: int) -> int:
    win, shift, _ = geometry(sr)
    return 1 + (length - win) // shift if length >= win else 0


def mel(f):
    return 1127.0 * torch.log(1.0 + f / 700.0)


def mel_banks(sr: int, n_mel: int) -> torch.Tensor:
    """float64 [n_mel, padded / 2]: the triangular weights of the FFT bins below Nyquist (the Nyquist bin's is 0 and is left out)"""
    _, _, padded = geometry(sr)
    lo = 1127.0 * math.log(1.0 + LOW_FREQ / 700.0)
    hi = 1127.0 * math.log(1.0 + 0.5 * sr / 700.0)
    delta = (hi - lo) / (n_mel + 1)
    b = torch.arange(n_mel, dtype=torch.float64)[:, None]
    left = lo + b * delta
    center = left + delta
    right = center + delta
    m = mel(torch.arange(padded // 2, dtype=torch.float64) * (sr / padded))[None, :]
    return torch.minimum((m - left) / (center - left), (right - m) / (right - center)).clamp_min(0.0)


def hann(win: int) -> torch.Tensor:
    return 0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(win, dtype=torch.float64) / (win - 1))


def empty_filters(sr: int, n_mel: int) -> torch.Tensor:
    """bool [n_mel]: filters narrower than one FFT bin"""
    return mel_banks(sr, n_mel).sum(1) == 0


def remove_mean(wave: torch.Tensor) -> torch.Tensor:
    return wave - wave.mean() if wave.numel() else wave


def mix(wave: torch.Tensor, wave2: torch.Tensor, lam: float) -> torch.Tensor:
    """dataloader.py:105-127 on two 1-D waves of the working dtype"""
    a, c = remove_mean(wave), remove_mean(wave2)
    if c.numel() < a.numel():
        c = torch.cat([c, c.new_zeros(a.numel() - c.numel())])
    else:
        c = c[:a.numel()]
    lam_t = torch.tensor(lam, dtype=torch.float32).to(wave.dtype)          # lam reaches the device as an fp32 number
    x = lam_t * a + (1 - lam_t) * c
    return remove_mean(x)


def fbank_raw(x: torch.Tensor, sr: int, n_mel: int) -> torch.Tensor:
    """steps 2-6 on a clip whose mean is already removed: [T, n_mel] log-mel energies in x's dtype"""
    dt = x.dtype
    win, shift, padded = geometry(sr)
    T = num_frames(x.numel(), sr)
    if T == 0:
        return x.new_zeros(0, n_mel)
    f = x.unfold(0, win, shift)[:T].clone()                                # [T, win]
    f = f - f.mean(dim=1, keepdim=True)
    prev = torch.cat([f[:, :1], f[:, :-1]], dim=1)
    f = f - torch.tensor(PREEMPH, dtype=dt) * prev
    f = f * hann(win).to(dt)
    f = torch.nn.functional.pad(f, (0, padded - win))
    spec = torch.fft.rfft(f)
    power = (spec.real ** 2 + spec.imag ** 2)[:, :padded // 2]
    energy = power @ mel_banks(sr, n_mel).to(dt).t()
    return torch.log(energy.clamp_min(torch.tensor(EPS, dtype=dt)))


def finish(raw: torch.Tensor, target_length, freq_band=None, time_band=None, norm=None) -> torch.Tensor:
    """steps 7-9"""
    T, n_mel = raw.shape
    L = T if target_length is None else target_length
    out = raw.new_zeros(L, n_mel)
    out[:min(T, L)] = raw[:L]
    if freq_band is not None:
        out[:, freq_band[0]:freq_band[1]] = 0
    if time_band is not None:
        out[time_band[0]:time_band[1]] = 0
    if norm is not None:
        mean, std = (torch.tensor(v, dtype=torch.float32).to(raw.dtype) for v in norm)
        out = (out - mean) / (2 * std)
    return out


def fbank(wave: torch.Tensor, sr: int, n_mel: int, target_length=None, dtype=torch.float64, wave2=None, lam=None, freq_band=None,
          time_band=None, norm=None) -> torch.Tensor:
    """all nine steps for ONE clip (1-D fp32 wave, already cut to its length) in `dtype`"""
    w = wave.to(dtype)
    x = remove_mean(w) if wave2 is None else mix(w, wave2.to(dtype), lam)
    return finish(fbank_raw(x, sr, n_mel), target_length, freq_band, time_band, norm)


def make_wave(n: int, sr: int, seed: int) -> torch.Tensor:
    """0.1 Gaussian noise + 0.3 sin(440 Hz) + 0.05 sin(3 kHz), fp32: the noise floor keeps every non-empty filter off cancellation"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    x = 0.1 * torch.randn(n, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.05 * torch.sin(2 * math.pi * 3000.0 * t)
    return x.float()
