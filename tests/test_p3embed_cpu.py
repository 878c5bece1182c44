"""P3Embed (group_embed.py:176-286) built on CPU: its state-dict keys and shapes equal the reference's for the four
Meta-Transformer recipe configurations (recorded in tests/golden/p3embed.npz by tools/make_p3embed_golden.py), and the
options it does not implement raise MetaEncError naming the option.  No GPU."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from metatransformer_amd import MetaEncError, P3Embed

RECIPES = ["scanobjectnn", "shapenetpart", "s3dis", "scannet"]


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "p3embed.npz"))


@pytest.mark.parametrize("name", RECIPES)
def test_recipe_state_dict_keys_and_shapes(z, name):
    kw = json.loads(str(z[f"recipe/{name}/config"]))
    want = [(k, tuple(s)) for k, s in json.loads(str(z[f"recipe/{name}/keys"]))]
    mod = P3Embed(**kw)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == want


@pytest.mark.parametrize("name", ["bn1", "ln2"])
def test_fixture_case_state_dict_loads_strict(z, name):
    import torch
    kw = json.loads(str(z[f"{name}/config"]))
    mod = P3Embed(**kw)
    prefix = f"{name}/w/"
    mod.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}, strict=True)


def test_channel_arithmetic():
    m = P3Embed(sample_ratio=0.0625, in_channels=7, embed_dim=768, group="knn", norm_args={"norm": "ln2d"})
    assert m.channel_list == [7, 384, 768] and m.out_channels == 768 and len(m.convs) == 2
    assert m.convs[0][0][0][0].weight.shape == (384, 10, 1, 1)          # dp_df: 3 + 7 input channels
    assert m.convs[1][0][0][0].weight.shape == (768, 387, 1, 1)
    assert m.convs[0][0][1][0].bias is not None and m.convs[0][0][0][0].bias is None      # no bias where a norm follows
    m = P3Embed(sample_ratio=0.25, in_channels=3, embed_dim=768, group="knn", norm_args="bn")
    assert m.channel_list == [3, 768] and m.out_channels == 768 and len(m.convs) == 1
    m = P3Embed(sample_ratio=0.25, in_channels=3, embed_dim=64, group="knn", norm_args="bn", feature_type="dp_fj_df", reduction="avg")
    assert m.convs[0][0][0][0].weight.shape == (64, 9, 1, 1) and m.reduction == "mean"


@pytest.mark.parametrize("kw,word", [
    (dict(group="ballquery"), "group"),
    (dict(subsample="random"), "subsample"),
    (dict(normalize_dp=True), "normalize_dp"),
    (dict(act_args={"act": "gelu"}), "act_args"),
    (dict(feature_type="pi_dp_fj_df"), "feature_type"),
    (dict(feature_type="dp"), "feature_type"),
    (dict(norm_args={"norm": "in2d"}), "norm_args"),
    (dict(reduction="sum"), "reduction"),
    (dict(relative_xyz=False), "relative_xyz"),
])
def test_unsupported_options_raise(kw, word):
    base = dict(sample_ratio=0.25, in_channels=3, embed_dim=64, group="knn", norm_args="bn")
    base.update(kw)
    with pytest.raises(MetaEncError, match=word):
        P3Embed(**base)
