"""CPU: the host side of multi-scale deformable attention and the ViT-Adapter interaction blocks -- constructor / state-dict
parity with the reference (tests/golden/msda.npz, tools/make_msda_golden.py), argument errors."""
import json
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN

import metatransformer_amd as M
from metatransformer_amd import adapter
import msda_cases as mc


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "msda.npz"), allow_pickle=False)


def _interactions(r):
    norm = partial(nn.LayerNorm, eps=1e-6)
    return nn.Sequential(*[M.InteractionBlock(dim=r["dim"], num_heads=r["num_heads"], n_points=r["n_points"], init_values=0.,
                                              drop_path=r["drop_path"], norm_layer=norm, with_cffn=True, cffn_ratio=r["cffn_ratio"],
                                              deform_ratio=r["deform_ratio"], extra_extractor=(i == r["n"] - 1))
                           for i in range(r["n"])])


@pytest.mark.parametrize("recipe", ["det_base", "seg_base"])
def test_interactions_state_dict_matches_the_reference(gold, recipe):
    r = json.loads(str(gold[f"keys/{recipe}/config"]))
    want = [(k, tuple(s)) for k, s in json.loads(str(gold[f"keys/{recipe}/keys"]))]
    inter = _interactions(r)
    got = [(k, tuple(v.shape)) for k, v in inter.state_dict().items()]
    assert got == want
    # a checkpoint with exactly the reference's keys loads strict=True
    sd = {k: torch.zeros(s) for k, s in want}
    inter.load_state_dict(sd, strict=True)


def test_fixture_state_dicts_load_strict():
    b = mc.BLOCK
    ib = M.InteractionBlock(dim=b["dim"], num_heads=b["num_heads"], n_points=b["n_points"], with_cffn=b["with_cffn"],
                            cffn_ratio=b["cffn_ratio"], init_values=b["init_values"], deform_ratio=b["deform_ratio"],
                            extra_extractor=b["extra_extractor"])
    sd = mc.state_dict_arrays([(k, tuple(v.shape)) for k, v in ib.state_dict().items()], "block/interaction")
    ib.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert float(ib.injector.gamma.detach().min()) >= 0.25
    for name, c in mc.MODULE.items():
        m = M.MSDeformAttn(d_model=c["d_model"], n_levels=len(c["shapes"]), n_heads=c["M"], n_points=c["P"], ratio=c["ratio"])
        sd = mc.state_dict_arrays([(k, tuple(v.shape)) for k, v in m.state_dict().items()], "module/" + name)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)


def test_reset_parameters_equals_the_reference(gold):
    c = json.loads(str(gold["init/config"]))
    torch.manual_seed(c.pop("seed"))
    m = M.MSDeformAttn(**c)
    sd = m.state_dict()
    keys = [k[len("init/"):] for k in gold.files if k.startswith("init/") and k != "init/config"]
    assert sorted(keys) == sorted(sd)
    for k in keys:
        assert sd[k].dtype == torch.float32 and np.array_equal(sd[k].numpy(), gold["init/" + k]), k
    assert M.MSDeformAttn().value_proj.weight.shape == (256, 256)          # the reference's defaults


def test_deform_inputs_equal_the_reference(gold):
    h, w = (int(v) for v in gold["points/image_hw"])
    d1, d2 = M.deform_inputs(torch.zeros(1, 3, h, w))
    for tag, d in (("points/1", d1), ("points/2", d2)):
        for name, t in zip(("reference_points", "spatial_shapes", "level_start_index"), d):
            want = gold[f"{tag}/{name}"]
            assert t.device.type == "cpu" and tuple(t.shape) == want.shape and t.numpy().dtype == want.dtype, (tag, name)
            assert np.array_equal(t.numpy(), want), (tag, name)
    pts = M.get_reference_points([(8, 12)], "cpu")
    assert np.array_equal(pts.numpy(), gold["points/1/reference_points"])


def _core(L=1, D=8, M_=2, Lq=3, P=2, N=1):
    shapes = [(2, 3)] * L
    S = 6 * L
    return (torch.zeros(N, S, M_, D), shapes, [6 * l for l in range(L)], torch.zeros(N, Lq, M_, L, P, 2), torch.zeros(N, Lq, M_, L, P))


def test_cpu_tensors_raise():
    v, ss, st, lo, aw = _core()
    with pytest.raises(M.MetaEncError, match=r"value.*CUDA.*no CPU fallback"):
        M.ms_deform_attn(v, ss, st, lo, aw)
    m = M.MSDeformAttn(d_model=32, n_levels=1, n_heads=2, n_points=2)
    with pytest.raises(M.MetaEncError, match=r"CUDA.*no CPU fallback"):
        m(torch.zeros(1, 3, 32), torch.zeros(1, 3, 1, 2), torch.zeros(1, 6, 32), ss, st)


def test_unsupported_arguments_name_the_argument():
    v, ss, st, lo, aw = _core()
    with pytest.raises(M.MetaEncError, match="value"):
        M.ms_deform_attn(v[0], ss, st, lo, aw)
    with pytest.raises(M.MetaEncError, match="sampling_locations"):
        M.ms_deform_attn(v, ss, st, lo[..., :1], aw)
    with pytest.raises(M.MetaEncError, match="attention_weights"):
        M.ms_deform_attn(v, ss, st, lo, aw[:, :2])
    with pytest.raises(M.MetaEncError, match="spatial_shapes"):
        M.ms_deform_attn(v, ss + ss, st + st, lo, aw)
    with pytest.raises(M.MetaEncError, match="level_start_index"):
        M.ms_deform_attn(v, ss, st + st, lo, aw)
    with pytest.raises(M.MetaEncError, match="spatial_shapes"):
        M.ms_deform_attn(v, torch.tensor([[2.0, 3.0]]), st, lo, aw)
    v9, ss9, st9, lo9, aw9 = _core(L=9)
    with pytest.raises(M.MetaEncError, match=r"spatial_shapes.*9 levels"):
        M.ms_deform_attn(v9, ss9, st9, lo9, aw9)
    vd, ssd, std_, lod, awd = _core(D=130)
    with pytest.raises(M.MetaEncError, match=r"value.*130"):
        M.ms_deform_attn(vd, ssd, std_, lod, awd)
    with pytest.raises(M.MetaEncError, match="channels per head"):
        M.MSDeformAttn(d_model=60, n_heads=6)
    assert adapter.MAX_LEVELS == 8 and adapter.MAX_HEAD_DIM == 128
    # im2col_step is accepted (and ignored) as a keyword
    with pytest.raises(M.MetaEncError, match="CUDA"):
        M.ms_deform_attn(v, ss, st, lo, aw, im2col_step=64)


def test_synthesised_locations_stay_clear_of_pixel_boundaries():
    for name in mc.CORE:
        i = mc.core_inputs(name)
        assert mc.check_clear(i["loc"], i["shapes"], name) >= mc.MARGIN
    out = mc.core_inputs("outside")
    px, _ = mc.pixel_coords(out["loc"], out["shapes"])
    assert px.min() < -1.0 and (px[..., 0, :, 0] > out["shapes"][0][1]).any()        # corners outside the level do occur
    pile = mc.core_inputs("pile")
    px, _ = mc.pixel_coords(pile["loc"], pile["shapes"])
    assert np.ptp(np.floor(px[0]).reshape(-1, 2), axis=0).max() == 0            # one 2 x 2 neighbourhood per batch item
