"""GPU: the point-cloud half of SURVEY 8 row f4 pinned to the reference itself.

  * me_fps against the reference's OWN kernel -- PointCloud/openpoints/cpp/pointnet2_batch/src/sampling_gpu.cu:101-258,
    compiled unmodified for gfx950 by oracle/build_ref.py into oracle/_ref/libref_fps.so and run on the same clouds
    (ties, lattices, the block sizes opt_n_threads picks, the S3DIS cloud size); its indices are stored in
    tests/golden/fps_reference.npz (oracle/make_fps_golden.py), and where the library is built the kernel is run again;
  * PointPatchEmbed and ClsHead against tests/golden/pointcloud.npz, written by oracle/make_golden.py from the reference's
    own classes (group_embed.py:60-172, cls_base.py:77-136), parameters loaded with load_state_dict(strict=True).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, TOL_F32, check_close, rel_err
from metatransformer_amd import heads
from oracle import make_fps_golden as mfg

pytestmark = pytest.mark.gpu

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_fps.so")


@pytest.fixture(scope="module")
def ref_fps():
    """(n, m, seed, clouds) -> the reference kernel's indices on mfg.fps_clouds(n, seed)[:clouds], from tests/golden/fps_reference.npz
    (written by oracle/make_fps_golden.py from that kernel).  Where oracle/_ref/libref_fps.so is built, the kernel also runs
    and must still return the stored indices."""
    z = np.load(os.path.join(GOLDEN, "fps_reference.npz"))
    live = mfg.load_kernel() if os.path.isfile(REF_SO) else None

    def want(n, m, seed, keep, p):
        k = mfg.case_key(n, m, seed)
        assert float(p.double().sum()) == float(z[k + "/cloud_sum"]), f"{k}: the seeded cloud differs from the one the fixture was made on"
        idx = torch.from_numpy(z[k + "/idx"])
        if live is not None:
            assert torch.equal(live(p.cuda().contiguous(), m).cpu(), idx), f"{k}: the reference kernel no longer returns the stored indices"
        return idx
    return want


@pytest.mark.parametrize("n,m", [(2, 2), (5, 5), (33, 20), (64, 64), (100, 50), (777, 100), (1024, 256), (2048, 512), (3000, 64),
                                 (8192, 300), (24000, 1500)])
def test_fps_indices_equal_the_reference_kernel(dev, ref_fps, n, m):
    p = mfg.fps_clouds(n, 100 + n)
    want = ref_fps(n, m, 100 + n, 4, p).to(dev)
    got = heads.furthest_point_sample(p.to(dev).contiguous(), m)
    assert got.dtype == torch.int32 and bool((got[:, 0] == 0).all())
    same = torch.equal(got, want)
    if not same:
        b, j = [int(v[0]) for v in torch.nonzero(got != want, as_tuple=True)]
        raise AssertionError(f"n={n} m={m}: first difference at cloud {b}, round {j}: me_fps {int(got[b, j])}, reference kernel {int(want[b, j])}")


def test_fps_memory_resident_form_equals_the_reference_kernel(dev, ref_fps):
    """n beyond the register-resident form (24 576 points): the same rounds with points and temp in memory"""
    p = mfg.fps_clouds(30000, 7)[:3].contiguous()
    assert torch.equal(heads.furthest_point_sample(p.to(dev), 200).cpu(), ref_fps(30000, 200, 7, 3, p))


def test_literal_restatement_equals_the_reference_kernel(dev, ref_fps):
    """oracle.tokenizer_oracle.fps_reference (used on CPU to generate tests/golden/pointcloud.npz) follows the same kernel"""
    from oracle import tokenizer_oracle as to
    for n, m in ((100, 40), (777, 60), (1500, 48)):
        p = mfg.fps_clouds(n, 300 + n)
        assert np.array_equal(to.fps_reference(p.numpy(), m), ref_fps(n, m, 300 + n, 4, p).numpy()), (n, m)


def _load(z, prefix):
    return {k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}


def test_point_patch_embed_equals_the_reference_class(dev):
    z = np.load(os.path.join(GOLDEN, "pointcloud.npz"))
    cfg = json.loads(str(z["ppe/config"]))
    mod = heads.PointPatchEmbed(sample_ratio=cfg["sample_ratio"], group_size=cfg["group_size"], embed_dim=cfg["embed_dim"],
                                channels=tuple(cfg["channels"]), subsample=cfg["subsample"], group=cfg["group"],
                                feature_type=cfg["feature_type"], reduction=cfg["reduction"])
    mod.load_state_dict(_load(z, "ppe/w/"), strict=True)          # the reference module's own state dict
    mod = mod.to(dev).eval()
    p = torch.from_numpy(z["ppe/p"]).to(dev)
    (pp, center), (x, out_f) = mod(p)
    assert x is None and pp is p
    assert torch.equal(center.cpu(), torch.from_numpy(z["ppe/center"]))           # sampled centres: same points, same order
    check_close(out_f, torch.from_numpy(z["ppe/out_f"]), TOL_F32, "PointPatchEmbed out_f")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_cls_head_equals_the_reference_class(dev, tag):
    z = np.load(os.path.join(GOLDEN, "pointcloud.npz"))
    kw = json.loads(str(z[f"cls_{tag}/config"]))
    head = heads.ClsHead(**kw)
    head.load_state_dict(_load(z, f"cls_{tag}/w/"), strict=True)
    head = head.to(dev).eval()
    x = torch.from_numpy(z[f"cls_{tag}/x"]).to(dev)
    check_close(head(x), torch.from_numpy(z[f"cls_{tag}/y"]), TOL_F32, f"ClsHead {tag} logits")
    if tag == "b":
        # the class defaults in TRAINING mode: nn.ReLU(inplace=True) directly behind the Linear (no norm layer in between)
        head.train()
        xr = x.clone().requires_grad_(True)
        y = head(xr)
        (y * torch.from_numpy(z["cls_b/go"]).to(dev)).sum().backward()
        check_close(y, torch.from_numpy(z["cls_b/y_train"]), TOL_F32, "ClsHead b train logits")
        check_close(xr.grad, torch.from_numpy(z["cls_b/dx"]), TOL_F32, "ClsHead b dx")
        for k, p in head.named_parameters():
            assert rel_err(p.grad, torch.from_numpy(z["cls_b/g/" + k])) < TOL_F32, k
