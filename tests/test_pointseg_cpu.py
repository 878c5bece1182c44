"""The point segmentation decoder and head (pointvit.py:177-393, pointnext.py:173-226, base_seg.py:92-149) built on CPU: their
state-dict keys and shapes equal the reference's for the S3DIS / ScanNet / ShapeNetPart recipes at full width (recorded in
tests/golden/pointseg.npz by tools/make_pointseg_golden.py), the fixture's state dicts load strict=True, and the options
that are not implemented raise MetaEncError naming the option.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import metatransformer_amd as M
from metatransformer_amd import MetaEncError

RECIPES = ["s3dis", "scannet", "shapenetpart"]
CASES = ["s3dis", "part", "resample"]


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "pointseg.npz"))


def _build(r):
    dec = getattr(M, r["decoder"])(**r["dec"])
    return dec, M.SegHead(in_channels=dec.out_channels, **r["head"])


@pytest.mark.parametrize("name", RECIPES)
def test_recipe_state_dict_keys_and_shapes(z, name):
    dec, head = _build(json.loads(str(z[f"recipe/{name}/config"])))
    got = [("decoder." + k, tuple(v.shape)) for k, v in dec.state_dict().items()] + \
          [("head." + k, tuple(v.shape)) for k, v in head.state_dict().items()]
    assert got == [(k, tuple(s)) for k, s in json.loads(str(z[f"recipe/{name}/keys"]))]
    assert dec.out_channels == int(z[f"recipe/{name}/out_channels"])


def test_out_channels():
    assert M.PointViTDecoder([7, 384, 768], global_feat="cls,max", progressive_input=True).out_channels == 2304
    assert M.PointViTPartDecoder([7, 384, 768], global_feat="cls,max,avg", progressive_input=True).out_channels == 3072
    assert M.PointViTDecoder([7, 384, 768]).out_channels == 768


def test_reference_layout():
    dec = M.PointViTDecoder([7, 384, 768], global_feat="cls,max", progressive_input=True)
    assert dec.decoder[1][0].convs[0][0].weight.shape == (768, 384 + 768, 1)        # the coarsest stage: skip 384 (progressive)
    assert dec.decoder[0][0].convs[0][0].weight.shape == (768, 7 + 768, 1)
    assert dec.decoder[0][0].convs[0][0].bias is None and isinstance(dec.decoder[0][0].convs[0][1], torch.nn.BatchNorm1d)
    part = M.PointViTPartDecoder([7, 384, 768], global_feat="cls,max,avg", progressive_input=True)
    assert part.convc[0][0].weight.shape == (64, 16, 1) and part.convc[0][0].bias is not None
    assert part.decoder[0][0].convs[0][0].weight.shape == (768, 64 + 7 + 768, 1)
    head = M.SegHead(13, 2304, mlps=[256], norm_args={"norm": "ln1d", "eps": 1e-6})
    assert isinstance(head.head[0][1], M.heads.LayerNorm1d) and head.head[0][1].eps == 1e-5   # LayerNorm1d ignores its kwargs
    assert isinstance(head.head[1], torch.nn.Dropout) and head.head[2][0].bias is not None
    head = M.SegHead(20, 2304, global_feat="max", norm_args={"norm": "bn"})
    assert head.head[0][0].weight.shape == (4608, 4608, 1) and isinstance(head.head[0][1], torch.nn.BatchNorm1d)


@pytest.mark.parametrize("name", CASES)
def test_fixture_case_state_dict_loads_strict(z, name):
    dec, head = _build(json.loads(str(z[f"{name}/config"])))
    for prefix, mod in (("decoder.", dec), ("head.", head)):
        pre = f"{name}/w/{prefix}"
        mod.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}, strict=True)


@pytest.mark.parametrize("make,word", [
    (lambda: M.FeaturePropogation([16, 32, 32], upsample=False), "upsample"),
    (lambda: M.PointViTPartDecoder([7, 48, 96], cls_map="curvenet"), "cls_map"),
    (lambda: M.PointViTDecoder([7, 48, 96], sampler="random"), "sampler"),
    (lambda: M.PointViTPartDecoder([7, 48, 96], sampler="random"), "sampler"),
    (lambda: M.PointViTDecoder([7, 48, 96], conv_args={"order": "norm-act-conv"}), "order"),
    (lambda: M.SegHead(13, 96, conv_args={"order": "conv-act-norm"}), "order"),
    (lambda: M.SegHead(13, 96, norm_args={"norm": "in1d"}), "norm_args"),
])
def test_unsupported_options_raise(make, word):
    with pytest.raises(MetaEncError, match=word):
        make()


def test_cpu_tensors_raise():
    p = [torch.rand(1, 64, 3), torch.rand(1, 16, 3), torch.rand(1, 4, 3)]
    f = [torch.rand(1, 7, 64), torch.rand(1, 48, 16), torch.rand(1, 96, 5)]
    with pytest.raises(MetaEncError, match="CUDA"):
        M.PointViTDecoder([7, 48, 96], progressive_input=True)(p, f)
    with pytest.raises(MetaEncError, match="CUDA"):
        M.SegHead(13, 96)(torch.rand(1, 96, 64))
    with pytest.raises(MetaEncError, match="CUDA"):
        M.three_interpolation(p[0], p[1], f[1])
    with pytest.raises(MetaEncError, match="CUDA"):
        M.three_nn(p[0], p[1])
