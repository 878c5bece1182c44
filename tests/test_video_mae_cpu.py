"""CPU: the VideoMAE pre-training cases, restatements, names and argument checks (no kernel runs).

The fixture tests/golden/video_mae.npz comes from the reference's own model (tools/make_video_mae_golden.py); the float64
restatements of tests/video_mae_cases.py, which the GPU tests use as their reference, are tied here to an einops formulation of the
target (Video/engine_for_pretraining.py:75-98) and to that fixture."""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn
from einops import rearrange

from conftest import GOLDEN, TOL_F32, check_close, rel_err

import metatransformer_amd as M
import video_mae_cases as vc
from metatransformer_amd import _capi, build as me_build, parallel


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "video_mae.npz"), allow_pickle=False)


def einops_labels(clip: torch.Tensor, patch: int, normalize: bool) -> torch.Tensor:
    """engine_for_pretraining.py:75-95, as written there, on whatever dtype `clip` has"""
    mean = torch.as_tensor(vc.MEAN, dtype=clip.dtype)[None, :, None, None, None]
    std = torch.as_tensor(vc.STD, dtype=clip.dtype)[None, :, None, None, None]
    unnorm = clip * std + mean
    if not normalize:
        return rearrange(unnorm, "b c (t p0) (h p1) (w p2) -> b (t h w) (p0 p1 p2 c)", p0=2, p1=patch, p2=patch)
    sq = rearrange(unnorm, "b c (t p0) (h p1) (w p2) -> b (t h w) (p0 p1 p2) c", p0=2, p1=patch, p2=patch)
    norm = (sq - sq.mean(dim=-2, keepdim=True)) / (sq.var(dim=-2, unbiased=True, keepdim=True).sqrt() + 1e-6)
    return rearrange(norm, "b n p c -> b n (p c)")


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", list(vc.CASES))
def test_restated_labels_equal_the_einops_formulation(case, normalize):
    rng = np.random.default_rng(5)
    c = vc.CASES[case]
    clip = torch.from_numpy(rng.standard_normal((2, 3, c["frames"], c["img"], c["img"])))
    kt, kh, kw = vc.tubelet(case)
    got = vc.labels_restate(clip, kt, kh, kw, normalize)
    want = einops_labels(clip, c["patch"], normalize)
    assert got.shape == want.shape == (2, vc.n_tokens(case), 3 * kt * kh * kw)
    assert float((got - want).abs().max()) < 1e-12
    # the gather's column order is the Conv3d weight's: a tubelet row times a flattened filter is the convolution's output
    w = torch.from_numpy(rng.standard_normal((4, 3, kt, kh, kw)))
    idx = torch.arange(vc.n_tokens(case)).repeat(2, 1)
    rows = vc.gather_restate(clip, idx, kt, kh, kw)
    conv = torch.nn.functional.conv3d(clip, w, stride=(kt, kh, kw)).flatten(2).transpose(1, 2)
    assert float((rows @ w.reshape(4, -1).t() - conv).abs().max()) < 1e-10


def test_low_contrast_patch_tells_the_eps_forms_apart():
    """eps on the standard deviation (the reference) against eps on the variance and no eps: on the low-contrast patch the reference
    arithmetic in fp32 stays within TOL_F32 of float64, either mistake is several times TOL_F32 away"""
    case = "p8"
    kt, kh, kw = vc.tubelet(case)
    clip = torch.from_numpy(vc.low_contrast_clip(case))
    row = lambda t: t[0, 1]                                        # noqa: E731  (the low-contrast token)
    ref = row(vc.labels_restate(clip, kt, kh, kw))
    f32 = row(einops_labels(clip, vc.CASES[case]["patch"], True))
    assert f32.dtype == torch.float32
    scale = float(ref.abs().max())
    e32 = float((f32.double() - ref).abs().max()) / scale
    e_none = float((row(vc.labels_restate(clip, kt, kh, kw, eps_mode="none")) - ref).abs().max()) / scale
    e_var = float((row(vc.labels_restate(clip, kt, kh, kw, eps_mode="var")) - ref).abs().max()) / scale
    print(f"low-contrast patch: fp32 reference {e32:.2e}, no eps {e_none:.2e}, eps on the variance {e_var:.2e}")
    assert e32 < TOL_F32 < e_none / 3 and TOL_F32 < e_var / 3
    # elsewhere the three agree far below the bound: only this patch separates them
    others = vc.labels_restate(clip, kt, kh, kw)[1]
    assert float((vc.labels_restate(clip, kt, kh, kw, eps_mode="none")[1] - others).abs().max()) < 1e-4 * float(others.abs().max())


@pytest.mark.parametrize("variant", list(vc.VARIANTS))
def test_restated_model_equals_the_fixture(gold, variant):
    case, with_dm, _ = vc.VARIANTS[variant]
    assert np.array_equal(vc.make_clip(case), gold[f"{case}/clip"])
    mask, dmask = vc.make_masks(case)
    assert np.array_equal(mask, gold[f"{case}/mask"]) and np.array_equal(dmask, gold[f"{case}/decode_mask"])
    sd = vc.fixture_state_dict(gold, variant)
    clip = torch.from_numpy(gold[f"{case}/clip"])
    dm = dmask if with_dm else None
    y = vc.model_restate(sd, case, clip, mask, dm)
    check_close(y, torch.from_numpy(gold[f"{variant}/out"]), 1e-5, f"{variant} restated forward")
    check_close(vc.model_restate(sd, case, clip, mask, dm, encoder_only=True), torch.from_numpy(gold[f"{variant}/enc"]), 1e-5, f"{variant} encoder")
    assert float(gold[f"{variant}/out_ref_err"]) < TOL_F32 / 100
    # the loss of the fixture is the restated one on the restated labels
    vis_idx, dec_idx, w = vc.index_lists(mask, dm)
    kt, kh, kw = vc.tubelet(case)
    labels = vc.take(vc.labels_restate(clip, kt, kh, kw), dec_idx)
    loss, _, _ = vc.loss_restate(y, labels, w)
    assert abs(float(loss) - float(gold[f"{variant}/loss"])) < 1e-9 * float(gold[f"{variant}/loss"])
    if with_dm:
        assert float(w.min()) == 0.0 and float(w.max()) == 1.0           # cal_loss_mask has a zero in it
        assert dec_idx.shape[1] == (vc.CASES[case]["masked"] + 1) // 2 + 1
    else:
        assert float(w.min()) == 1.0 and dec_idx.shape[1] == vc.CASES[case]["masked"]
    assert vis_idx.shape[1] == vc.n_tokens(case) - vc.CASES[case]["masked"]


@pytest.mark.parametrize("variant", ["p8", "p8_ls_dm", "p16"])
def test_state_dict_keys_are_the_reference(gold, variant):
    case, _, init_values = vc.VARIANTS[variant]
    ref_sd = vc.fixture_state_dict(gold, variant)
    assert [(k, tuple(s)) for k, s in json.loads(str(gold[f"{case}/keys"]))] == [(k, tuple(v.shape)) for k, v in ref_sd.items() if "gamma" not in k]
    m = M.PretrainVisionTransformer(norm_layer=partial(nn.LayerNorm, eps=vc.MODEL["eps"]), **vc.model_kwargs(case, init_values))
    m.load_state_dict(M.convert_video_state_dict(ref_sd), strict=True)
    back = M.to_video_state_dict(m.state_dict())
    assert set(back) == set(ref_sd)
    for k, v in ref_sd.items():
        assert torch.equal(back[k], v), k
    assert "pos_embed" not in m.state_dict() and "encoder.pos_embed" not in m.state_dict()      # sinusoid tables are not parameters
    assert torch.equal(m.pos_embed[0], vc.sinusoid_table(vc.n_tokens(case), vc.MODEL["dec_dim"]))
    assert m.encoder.blocks[0].layer_scale == (init_values > 0) and m.encoder.blocks[0].eps == vc.MODEL["eps"]
    bad = dict(M.convert_video_state_dict(ref_sd))
    bad["decoder.pos_embed"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad, strict=True)


def test_constructors_follow_the_reference():
    enc = M.PretrainVisionTransformerEncoder(img_size=32, patch_size=16, embed_dim=32, depth=1, num_heads=2, init_values=0., all_frames=4,
                                             use_learnable_pos_emb=True)
    assert isinstance(enc.pos_embed, nn.Parameter) and tuple(enc.pos_embed.shape) == (1, 9, 32) and "pos_embed" in enc.state_dict()
    assert isinstance(enc.head, nn.Identity) and enc.get_num_layers() == 1 and enc.patch_embed.proj.weight.shape == (32, 3, 2, 16, 16)
    assert enc.no_weight_decay() == {"pos_embed", "cls_token"}
    dec = M.PretrainVisionTransformerDecoder(patch_size=8, num_classes=384, embed_dim=32, depth=1, num_heads=2, init_values=0.1)
    assert dec.no_weight_decay() == {"pos_embed", "cls_token"} and float(dec.blocks[0].gamma1.detach()[0]) == pytest.approx(0.1)
    with pytest.raises(AssertionError):
        M.PretrainVisionTransformerDecoder(patch_size=8, num_classes=100, embed_dim=32, depth=1, num_heads=2, init_values=0.)
    m = M.PretrainVisionTransformer(**vc.model_kwargs("p16"))
    assert m.no_weight_decay() == {"pos_embed", "cls_token", "mask_token"} and tuple(m.mask_token.shape) == (1, 1, 32)
    assert m.encoder_to_decoder.bias is None and float(m.mask_token.detach().abs().max()) <= 0.02
    E = M.MetaEncError
    for kw, what in ((dict(cos_attn=True), "cos_attn"), (dict(with_cp=True), "with_cp"), (dict(init_values=None), "init_values")):
        with pytest.raises(E, match=what):
            M.PretrainVisionTransformer(**{**vc.model_kwargs("p16"), **kw})
    with pytest.raises(E, match="init_values"):
        M.PretrainVisionTransformerEncoder(img_size=32, embed_dim=32, depth=1, num_heads=2, all_frames=4)       # the reference's default, None
    # no device route from CPU tensors
    clip, mask = torch.zeros(2, 3, 4, 32, 32), torch.zeros(2, 8, dtype=torch.bool)
    with pytest.raises(E, match="no CPU fallback"):
        m(clip, mask)
    with pytest.raises(E, match="no CPU fallback"):
        m.encoder(clip, mask)
    with pytest.raises(E, match="no CPU fallback"):
        M.mae_reconstruction_loss(torch.zeros(2, 6, 1536), clip, mask)


def test_no_decay_rule_takes_the_models_skip_set():
    """Video/optim_factory.py:67-68: 1-D, `.bias`, `.scale` and the names of no_weight_decay(); the default call is what it was"""
    m = M.PretrainVisionTransformer(**vc.model_kwargs("p16", 0.1))
    named = dict(m.named_parameters())
    rule = partial(parallel.no_decay_rule, skip=m.no_weight_decay())
    assert not parallel.no_decay_rule("mask_token", named["mask_token"]) and rule("mask_token", named["mask_token"])
    for k, p in named.items():
        want = p.dim() == 1 or k.endswith(".bias") or k == "mask_token"
        assert rule(k, p) == want, k
        assert parallel.no_decay_rule(k, p) == (p.dim() == 1 or k.endswith(".bias")), k
    w = nn.Parameter(torch.zeros(2, 2))
    assert parallel.no_decay_rule("attn.scale", w) and not parallel.no_decay_rule("attn.scales", w)


def test_library_rejects_bad_arguments_before_any_launch():
    me_build.build(verbose=False)
    lib = _capi.load()
    F32 = _capi.ME_F32
    a = 4096                                                         # an aligned address; never dereferenced: the checks fail first
    assert lib.me_tubelet_gather(a, F32, a, a, F32, 100, 2, 3, 4, 32, 32, 2, 16, 16, 2, None) != 0 and b"ld_out" in lib.me_last_error()
    assert lib.me_tubelet_gather(a, F32, a, a, F32, 1536, 2, 3, 4, 8, 32, 2, 16, 16, 2, None) != 0 and b"larger than the clip" in lib.me_last_error()
    assert lib.me_tubelet_gather(a, _capi.ME_F16, a, a, F32, 1536, 2, 3, 4, 32, 32, 2, 16, 16, 2, None) != 0 and b"video_dtype" in lib.me_last_error()
    assert lib.me_take_rows(a, F32, 16, 8, a, None, a, F32, 32, 2, 3, 32, None) != 0 and b"ld_table" in lib.me_last_error()
    assert lib.me_mae_assemble_fwd(a, F32, 32, a, 16, 8, a, a, a, a, F32, 32, 2, 2, 6, 32, None) != 0 and b"ld_pos" in lib.me_last_error()
    assert lib.me_mae_assemble_bwd_workspace(2, 6, 32) == 12 * 32 * 4 and lib.me_mae_assemble_bwd_workspace(32, 1408, 384) == 256 * 384 * 4
    assert lib.me_mae_assemble_bwd_workspace(2, 0, 32) == 0
    assert lib.me_mae_assemble_bwd(a, F32, 32, a, F32, 32, a, 2, 2, 6, 32, None, 0, None) != 0 and b"workspace" in lib.me_last_error()
    loss = lambda **kw: lib.me_mae_loss(a, F32, 2, kw.get("Cin", 3), 4, 32, 32, kw.get("kt", 2), 16, 16, a, a, a, a, 6, a, F32,     # noqa: E731
                                        kw.get("ld", 1536), 1, None, a, kw.get("scalars", a), None, 0, None, 0, None)
    assert loss(ld=1000) != 0 and b"ld_pred" in lib.me_last_error()
    assert loss(scalars=None) != 0 and b"scalars" in lib.me_last_error()
    assert loss(Cin=17, ld=1 << 20) != 0 and b"at most 16" in lib.me_last_error()
    assert lib.me_mae_loss(a, F32, 2, 3, 4, 32, 32, 1, 1, 1, a, a, a, a, 6, a, F32, 3, 1, None, a, a, None, 0, None, 0, None) != 0
    assert b"two pixels" in lib.me_last_error()
