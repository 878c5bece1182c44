"""CPU: the hyperspectral tokenizer's cases, restatement, names and argument checks (no kernel runs).

The fixture tests/golden/hyperspectral.npz comes from the reference's own functions (tools/make_hyperspectral_golden.py); the
restatement of tests/hyperspectral_cases.py, which the GPU tests use as their float64 reference on shapes the fixture does not hold,
is tied to it here."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TOL_F32, check_close

import hyperspectral_cases as hc
import metatransformer_amd as M
from metatransformer_amd import _capi, build as me_build


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hyperspectral.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    me_build.build(verbose=False)
    return _capi.load()


@pytest.mark.parametrize("name", list(hc.SMALL))
def test_restatement_equals_the_reference_gather(gold, name):
    H, W, bands, p, bp = hc.SMALL[name]
    cube, pts = torch.from_numpy(gold[f"{name}/cube"]), torch.from_numpy(gold[f"{name}/points"])
    assert np.array_equal(hc.make_cube(name), gold[f"{name}/cube"]) and np.array_equal(hc.make_points(name), gold[f"{name}/points"])
    want = torch.from_numpy(gold[f"{name}/gathered"])
    assert tuple(want.shape) == (pts.shape[0], bands, p * p * bp)
    assert torch.equal(hc.restate(cube, pts, p, bp), want)
    # the cases hold what the issue lists: four corners, the centre, a duplicate
    got = {tuple(r) for r in pts.tolist()}
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)} <= got and len(got) < pts.shape[0]


@pytest.mark.parametrize("name", list(hc.SMALL))
def test_reference_call_form_in_plain_torch_matches_the_fixture(gold, name):
    params = {k: gold[f"{name}/param/{k}"] for k in hc.make_params(name, hc.SMALL_C)}
    for k, v in hc.make_params(name, hc.SMALL_C).items():
        assert np.array_equal(v, params[k]), k
    x = torch.from_numpy(gold[f"{name}/gathered"])
    want = torch.from_numpy(gold[f"{name}/out"])
    check_close(hc.embed_reference(x.double(), params), want, TOL_F32, f"{name} float64")
    check_close(hc.embed_reference(x, params), want, TOL_F32, f"{name} float32")
    n = max(1, x.shape[1] // 2)              # the reference's forward takes any n <= bands and slices pos_embedding[:, :n + 1]
    check_close(hc.embed_reference(x[:, :n].double(), params), want[:, :n + 1], TOL_F32, f"{name} first {n} bands")


def test_state_dict_keys_and_shapes_are_the_reference(gold):
    c = json.loads(str(gold["cls/config"]))
    assert c == hc.CLASSIFIER
    H, W, bands, p, bp = hc.SMALL[c["case"]]
    want = [(k, tuple(s)) for k, s in json.loads(str(gold["cls/keys"]))]
    m = M.HyperSpectralClassifier(image_size=p, near_band=bp, num_patches=bands, num_classes=c["num_classes"], dim=c["dim"], depth=c["depth"],
                                  heads=c["heads"], mlp_dim=c["mlp_dim"])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    m.load_state_dict({k: torch.from_numpy(gold["cls/sd/" + k]) for k, _ in want}, strict=True)
    bad = {k: torch.from_numpy(gold["cls/sd/" + k]) for k, _ in want}
    bad["to_patch.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad, strict=True)
    emb = M.HyperSpectralEmbed(bands=200, patch=7, near_band=3)
    assert [(k, tuple(v.shape)) for k, v in emb.state_dict().items()] == [
        ("pos_embedding", (1, 201, 768)), ("cls_token", (1, 1, 768)), ("patch_to_embedding.weight", (768, 147)), ("patch_to_embedding.bias", (768,))]
    d2s = M.Data2Seq("hyper", 64, bands=13, patch=3, near_band=3)
    assert isinstance(d2s.embed, M.HyperSpectralEmbed) and d2s.embed.patch_to_embedding.weight.shape == (64, 27)
    # an encoder handed in is used as it is (the frozen-encoder recipe), whatever depth / heads / mlp_dim say
    enc = M.build_encoder(1, 64, 4)
    assert M.HyperSpectralClassifier(3, 3, 13, 5, 64, 12, 12, 1024, encoder=enc).transformer is enc


def test_constructor_and_argument_errors():
    E = M.MetaEncError
    for kw in (dict(bands=13, patch=2), dict(bands=13, near_band=4), dict(bands=3, near_band=5), dict(bands=13, patch=0),
               dict(bands=13, embed_dim=60), dict(bands=13, near_band=0)):
        with pytest.raises(E):
            M.HyperSpectralEmbed(**kw)
    with pytest.raises(E, match="CAF"):
        M.HyperSpectralClassifier(3, 3, 13, 5, 64, 2, 4, 128, mode="CAF")
    with pytest.raises(E, match="pool"):
        M.HyperSpectralClassifier(3, 3, 13, 5, 64, 2, 4, 128, pool="max")
    for kw in (dict(), dict(bands=13), dict(bands=13, patch=3)):
        with pytest.raises(E, match="required"):
            M.Data2Seq("hyper", 64, **kw)
    emb = M.HyperSpectralEmbed(bands=13, patch=3, near_band=3, embed_dim=64)
    with pytest.raises(E, match="no CPU fallback"):
        emb(torch.zeros(9, 11, 13), torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(E, match="no CPU fallback"):
        emb(torch.zeros(2, 13, 27))
    with pytest.raises(E, match="no CPU fallback"):
        M.neighborhood_tokens(torch.zeros(9, 11, 13), torch.zeros(2, 2, dtype=torch.int64), 3, 3)


def _desc(H=9, W=11, bands=13, patch=3, bp=3, B=2, dt=_capi.ME_F32):
    d = _capi.HsiDesc()
    d.cube, d.cube_dtype, d.row_stride, d.pix_stride = 4096, dt, W * bands, bands      # (aligned addresses; never dereferenced: the checks fail first)
    d.H, d.W, d.bands, d.points, d.B, d.patch, d.band_patch = H, W, bands, 8192, B, patch, bp
    return d


def test_library_rejects_bad_geometry_before_any_launch(lib):
    def gather(d):
        return lib.me_hsi_gather(ctypes.byref(d), 16384, _capi.ME_F32, d.patch * d.patch * d.band_patch, None)

    def fwd(d, C):
        return lib.me_hsi_embed_fwd(ctypes.byref(d), 4096, _capi.ME_F32, d.patch * d.patch * d.band_patch, 4096, 4096, 4096, C, 16384,
                                    _capi.ME_F32, C, C, None)
    for d, what in ((_desc(patch=4), b"patch=4"), (_desc(bp=2), b"band_patch=2"), (_desc(H=2, W=11, patch=7), b"min(H, W)"),
                    (_desc(bands=3, bp=5), b"exceeds bands"), (_desc(dt=_capi.ME_F16), b"cube_dtype")):
        assert gather(d) != 0 and what in lib.me_last_error(), what
        assert fwd(d, 64) != 0 and what in lib.me_last_error(), what
    for C in (60, 4, 0):
        assert fwd(_desc(), C) != 0 and b"multiple of 8" in lib.me_last_error()
        assert lib.me_hsi_embed_wgrad(ctypes.byref(_desc()), 4096, _capi.ME_F32, 64, C, 4096, 27, None, None, None, 64, 0.0, 4096, 1 << 30, None) != 0
        assert b"multiple of 8" in lib.me_last_error()
    d = _desc()
    d.pix_stride = 12                                                        # pixels overlap
    assert gather(d) != 0 and b"strides" in lib.me_last_error()
    assert lib.me_hsi_embed_wgrad_workspace(ctypes.byref(_desc(B=5)), 64) >= (5 * 64 * 27 + 14 * 64) * 4
    assert lib.me_hsi_embed_wgrad(ctypes.byref(_desc()), 4096, _capi.ME_F32, 64, 64, 4096, 27, None, None, None, 64, 0.0, None, 0, None) != 0
    assert b"workspace" in lib.me_last_error()
