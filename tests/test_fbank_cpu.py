"""CPU: the Kaldi filterbank restatement (tests/fbank_cases.py) checks itself, the package's float64 table builders agree with it,
specaug_bands keeps torchaudio's ranges, and ASTModel's host side (constructor, keys, geometry errors) is the reference's."""
import math

import pytest
import torch

import fbank_cases as fc
import metatransformer_amd as M
from metatransformer_amd import audio


@pytest.mark.parametrize("sr", [16000, 8000])
def test_frame_counts_at_the_edges(sr):
    win, shift, padded = fc.geometry(sr)
    assert (win, shift, padded) == ({16000: (400, 160, 512), 8000: (200, 80, 256)}[sr]) == audio.frame_geometry(sr)
    for length, frames in ((win - 1, 0), (win, 1), (win + shift - 1, 1), (win + shift, 2)):
        assert fc.num_frames(length, sr) == frames
        assert fc.fbank(fc.make_wave(length, sr, 0), sr, 8).shape == (frames, 8)
        assert M.KaldiFbank(sr, 8).num_frames(length) == frames


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_silent_and_constant_clips_are_log_eps_everywhere(dtype):
    for wave in (torch.zeros(2000), torch.full((2000,), 0.37)):
        out = fc.fbank(wave, 16000, 128, dtype=dtype)
        assert out.shape == (11, 128)
        assert torch.equal(out, torch.full_like(out, math.log(fc.EPS)))


def test_a_tone_peaks_in_the_filter_nearest_to_it():
    sr, n_mel = 16000, 128
    t = torch.arange(4000, dtype=torch.float64) / sr
    out = fc.fbank(torch.sin(2 * math.pi * 1000.0 * t).float(), sr, n_mel)
    lo, hi = (1127.0 * math.log(1.0 + f / 700.0) for f in (fc.LOW_FREQ, sr / 2))
    centers = lo + (torch.arange(n_mel, dtype=torch.float64) + 1) * (hi - lo) / (n_mel + 1)
    want = int((centers - 1127.0 * math.log(1.0 + 1000.0 / 700.0)).abs().argmin())
    assert all(int(row.argmax()) == want for row in out)


def test_empty_filter_counts():
    """filters narrower than one FFT bin: 1 of 128 and 16 of 224 at 16 kHz; they yield exactly log(eps)"""
    assert int(fc.empty_filters(16000, 128).sum()) == 1
    assert int(fc.empty_filters(16000, 224).sum()) == 16
    assert int(fc.empty_filters(8000, 64).sum()) == 0
    out = fc.fbank(fc.make_wave(2000, 16000, 3), 16000, 224, dtype=torch.float32)
    empty = fc.empty_filters(16000, 224)
    assert torch.equal(out[:, empty], torch.full_like(out[:, empty], math.log(fc.EPS)))
    assert bool((out[:, ~empty] > math.log(fc.EPS) + 1).all())


def test_cut_pad_masks_and_normalisation_of_the_restatement():
    w = fc.make_wave(2000, 16000, 4)
    raw = fc.fbank(w, 16000, 16)
    out = fc.fbank(w, 16000, 16, target_length=14, freq_band=(2, 5), time_band=(1, 3), norm=(-4.0, 4.5))
    cell = (0.0 - (-4.0)) / (2 * 4.5)
    assert out.shape == (14, 16) and torch.allclose(out[11:], torch.full((3, 16), cell, dtype=torch.float64))
    assert torch.allclose(out[:, 2:5], torch.full((14, 3), cell, dtype=torch.float64)) and torch.allclose(out[1:3], torch.full((2, 16), cell, dtype=torch.float64))
    assert torch.allclose(out[4:11, 6:], (raw[4:, 6:] + 4.0) / 9.0)
    assert torch.equal(fc.fbank(w, 16000, 16, target_length=5), raw[:5])


@pytest.mark.parametrize("sr,n_mel", [(16000, 128), (16000, 224), (8000, 64), (16000, 23)])
def test_table_builders_equal_the_restatement(sr, n_mel):
    win, shift, padded = fc.geometry(sr)
    banks = fc.mel_banks(sr, n_mel)
    got = M.mel_filterbank(sr, n_mel)
    assert got.dtype == torch.float64 and got.shape == (n_mel, padded // 2)
    assert torch.equal(got.float(), banks.float())
    t = M.fbank_tables(sr, n_mel)
    assert (t["win"], t["shift"], t["padded"]) == (win, shift, padded)
    assert t["window"].dtype == torch.float64 and torch.equal(t["window"].float(), fc.hann(win).float())
    assert torch.equal(t["window"].float(), torch.hann_window(win, periodic=False, dtype=torch.float64).float())
    n = torch.arange(padded, dtype=torch.float64)
    w = torch.polar(torch.ones_like(n), -2 * math.pi * n / padded)
    assert torch.allclose(t["twiddle"][:, 0], w.real, atol=1e-15, rtol=0) and torch.allclose(t["twiddle"][:, 1], w.imag, atol=1e-15, rtol=0)
    # the (first bin, count) ranges and the packed weights unpack to the dense matrix
    rng, wt = t["mel_range"], t["mel_weight"]
    assert rng.dtype == torch.int32 and rng.shape == (n_mel, 2) and wt.shape[0] == n_mel and wt.shape[1] == int(rng[:, 1].max())
    dense = torch.zeros_like(banks)
    for b in range(n_mel):
        first, count = int(rng[b, 0]), int(rng[b, 1])
        assert 0 <= first and first + count <= padded // 2
        dense[b, first:first + count] = wt[b, :count]
        assert bool((wt[b, count:] == 0).all())
    assert torch.equal(dense.float(), banks.float())
    assert int((rng[:, 1] == 0).sum()) == int(fc.empty_filters(sr, n_mel).sum())


def test_specaug_bands_stay_inside_the_axis():
    g = torch.Generator().manual_seed(0)
    fm, tm = M.specaug_bands(4096, 128, 1024, 48, 192, generator=g)
    for band, size, param in ((fm, 128, 48), (tm, 1024, 192)):
        assert band.dtype == torch.int32 and band.shape == (4096, 2)
        start, end = band[:, 0].long(), band[:, 1].long()
        assert bool((start >= 0).all()) and bool((end <= size).all()) and bool((end >= start).all())
        assert bool((end - start < param).all()) and int((end - start).max()) > param // 2
    fm, tm = M.specaug_bands(8, 128, 1024, 0, 0)
    assert bool((fm[:, 0] == fm[:, 1]).all()) and bool((tm[:, 0] == tm[:, 1]).all())
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    assert all(torch.equal(a, b) for a, b in zip(M.specaug_bands(16, 64, 100, 10, 20, g1), M.specaug_bands(16, 64, 100, 10, 20, g2)))
    with pytest.raises(M.MetaEncError):
        M.specaug_bands(2, 64, 100, 65, 0)


def _small_ast(**kw):
    return M.ASTModel(label_dim=35, verbose=False, encoder=M.build_encoder(2, 64, 2), **kw)


def test_ast_model_constructor_and_state_dict_keys():
    m = _small_ast(input_fdim=224, input_tdim=224)
    assert m.v.pos_embed.shape == (1, 400, 64)                     # (21 - 1) * (21 - 1) rows from the 16 x 16 counts of get_shape
    assert m.get_shape(10, 10, 224, 224) == (21, 21) and m.get_shape(10, 10, 128, 1024) == (12, 101)
    assert m.v.patch_embed.proj.weight.shape == (64, 1, 32, 32) and m.v.patch_embed.proj.stride == (10, 10)
    assert _small_ast(input_fdim=224, input_tdim=224, imagenet_pretrain=False).v.patch_embed.proj.weight.shape == (64, 1, 16, 16)
    keys = set(m.state_dict())
    block = {f"v.blocks.{i}.{k}" for i in range(2) for k in M.build_encoder(1, 64, 2)[0].state_dict()}
    assert keys == block | {"v.cls_token", "v.dist_token", "v.pos_embed", "v.patch_embed.proj.weight", "v.patch_embed.proj.bias", "v.norm.weight",
                            "v.norm.bias", "v.head.weight", "v.head.bias", "mlp_head.0.weight", "mlp_head.0.bias", "mlp_head.1.weight",
                            "mlp_head.1.bias"}
    assert m.v.cls_token.shape == m.v.dist_token.shape == (1, 1, 64) and m.mlp_head[1].weight.shape == (35, 64)
    assert m.v.norm.eps == 1e-6 and m.mlp_head[0].eps == 1e-5
    # the reference trains pos_embed, the patch weight and the head; the rest of v is frozen (ast_models.py:66-70)
    assert {n for n, p in m.named_parameters() if p.requires_grad} == {"v.pos_embed", "v.patch_embed.proj.weight", "mlp_head.0.weight",
                                                                       "mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"}
    full = M.ASTModel(verbose=False)                                # the reference's defaults: Base encoder, eps 1e-6, 527 labels
    assert len(full.v.blocks) == 12 and full.v.blocks[0].eps == 1e-6 and full.mlp_head[1].weight.shape == (527, 768)
    assert full.v.pos_embed.shape == (1, 20 * 100, 768)
    m2 = _small_ast(input_fdim=224, input_tdim=224)
    m2.load_state_dict(m.state_dict(), strict=True)


def test_ast_model_errors():
    with pytest.raises(M.MetaEncError, match="audioset_pretrain"):
        M.ASTModel(audioset_pretrain=True, verbose=False, encoder=M.build_encoder(1, 64, 2))
    with pytest.raises(M.MetaEncError, match="no CPU fallback"):
        _small_ast(input_fdim=224, input_tdim=224)(torch.zeros(1, 224, 224))
    with pytest.raises(M.MetaEncError, match="no CPU fallback"):
        M.KaldiFbank()(torch.zeros(1, 16000))
    # 128 bins x 1024 frames with the 32 x 32 patch embed: 10 * 100 tokens against (12 - 1) * (101 - 1) position rows
    with pytest.raises(M.MetaEncError, match=r"1000 tokens.*1100 rows"):
        _small_ast(input_fdim=128, input_tdim=1024)(torch.zeros(1, 1024, 128))
    with pytest.raises(M.MetaEncError, match=r"45 tokens.*32 rows"):
        _small_ast(input_fdim=64, input_tdim=104, imagenet_pretrain=False)(torch.zeros(1, 104, 64))
