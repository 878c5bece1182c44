"""Write tests/golden/p3embed.npz from the reference's own P3Embed (PointCloud/openpoints/models/layers/group_embed.py:176-286,
loaded unmodified by oracle.ref_loader.reference_pointcloud_modules, which serves its CPU FPS and grouping).

    python tools/make_p3embed_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_p3embed_golden.py --check    # regenerate and compare with the stored fixture, write nothing

Cases (narrow embed_dim keeps the file small):
  * bn1 -- 1 stage, BatchNorm2d (eval, randomised running statistics), in_channels 3, [2, 512] points (the ScanObjectNN form);
  * ln2 -- 2 stages, LayerNorm2d, in_channels 7, [2, 1024] points (the ShapeNetPart / S3DIS / ScanNet form).
Each stores its constructor arguments, the reference's state dict, p, f, the centres of every stage and out_f of every stage.
The clouds are chosen so that every query's k-th and (k+1)-th nearest distances differ by more than 1e-5 (relative): the
neighbour SETS then do not depend on how the distance is rounded (the reference's cdist, me_knn's fmaf chain).
``recipe/<name>`` holds the state-dict key list and shapes of the four full-width recipe configurations.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "p3embed.npz")

COMMON = dict(group_size=32, layers=4, subsample="fps", group="knn", normalize_dp=False, feature_type="dp_df",
              conv_args={"order": "conv-norm-act"}, reduction="max")
# the recipes' embed_args (PointCloud/cfgs/<recipe>/metatransformer.yaml) at their full width
RECIPES = {
    "scanobjectnn": dict(COMMON, sample_ratio=0.25, in_channels=3, embed_dim=768, norm_args="bn"),
    "shapenetpart": dict(COMMON, sample_ratio=0.0625, in_channels=7, embed_dim=768, norm_args={"norm": "bn"}),
    "s3dis": dict(COMMON, sample_ratio=0.0625, in_channels=7, embed_dim=768, norm_args={"norm": "ln2d"}),
    "scannet": dict(COMMON, sample_ratio=0.0625, in_channels=7, embed_dim=768, norm_args={"norm": "ln2d"}),
}
CASES = {
    "bn1": (dict(COMMON, sample_ratio=0.25, in_channels=3, embed_dim=64, norm_args="bn"), (2, 512)),
    "ln2": (dict(COMMON, sample_ratio=0.0625, in_channels=7, embed_dim=64, norm_args={"norm": "ln2d"}), (2, 1024)),
}


def _randomize(mod, g):
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.LayerNorm)):
            m.weight.data.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
            m.bias.data.copy_(0.05 * torch.randn(m.bias.shape, generator=g))
        elif isinstance(m, torch.nn.Conv2d):
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=g) * (m.weight[0].numel() ** -0.5))
            if m.bias is not None:
                m.bias.data.copy_(0.05 * torch.randn(m.bias.shape, generator=g))


def _knn_margin(support: torch.Tensor, query: torch.Tensor, k: int) -> float:
    """smallest relative gap between the k-th and (k+1)-th float64 distance over all queries"""
    d = torch.cdist(query.double(), support.double(), compute_mode="donot_use_mm_for_euclid_dist").pow(2)
    v = d.topk(k + 1, dim=2, largest=False).values
    return float(((v[..., k] - v[..., k - 1]) / v[..., k].clamp_min(1e-30)).min())


def generate() -> dict:
    from oracle import ref_loader
    ge, _ = ref_loader.reference_pointcloud_modules()
    out = {}
    for name, kw in RECIPES.items():
        mod = ge.P3Embed(**kw)
        out[f"recipe/{name}/config"] = json.dumps(kw)
        out[f"recipe/{name}/keys"] = json.dumps([[k, list(v.shape)] for k, v in mod.state_dict().items()])
    for ci, (name, (kw, (B, N))) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(5100 + ci)
        mod = ge.P3Embed(**kw).eval()
        _randomize(mod, g)
        for attempt in range(100):
            p = torch.rand(B, N, 3, generator=g) * 2 - 1
            f = torch.randn(B, kw["in_channels"], N, generator=g)
            with torch.no_grad():
                out_p, out_f = mod(p, f)
            margins = [_knn_margin(out_p[s], out_p[s + 1], kw["group_size"]) for s in range(len(out_p) - 1)]
            if min(margins) > 1e-5:
                break
        else:
            raise RuntimeError(f"{name}: no cloud with separated k-th neighbours")
        out.update({f"{name}/config": json.dumps(kw), f"{name}/p": p.numpy(), f"{name}/f": f.numpy(),
                    f"{name}/stages": np.int64(len(out_p) - 1)})
        for s in range(1, len(out_p)):
            out[f"{name}/center{s}"] = out_p[s].numpy()
            out[f"{name}/out_f{s}"] = out_f[s].numpy()
        for k, v in mod.state_dict().items():
            out[f"{name}/w/{k}"] = v.numpy()
        print(f"  {name}: attempt {attempt}, knn margins {['%.1e' % m for m in margins]}, out_f "
              + ", ".join(str(tuple(out_f[s].shape)) for s in range(1, len(out_f))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the stored fixture instead of writing it")
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = generate()
    if args.check:
        z = np.load(GOLDEN)
        assert sorted(z.files) == sorted(out), sorted(set(z.files) ^ set(out))
        bad = [k for k in out if np.asarray(out[k]).dtype != z[k].dtype or np.asarray(out[k]).tobytes() != z[k].tobytes()]
        assert not bad, f"differs from {GOLDEN}: {bad[:8]}"
        print(f"[check] {GOLDEN}: {len(out)} arrays identical")
        return
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
