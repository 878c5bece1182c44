"""Write tests/golden/pointseg.npz from the reference's own point segmentation decoder and head: PointViTDecoder /
PointViTPartDecoder (PointCloud/openpoints/models/backbone/pointvit.py:177-393), FeaturePropogation (backbone/pointnext.py:173-226),
three_interpolation (layers/upsampling.py) and SegHead (segmentation/base_seg.py:92-149), all four files loaded unmodified.

    python tools/make_pointseg_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_pointseg_golden.py --check    # regenerate and compare with the stored fixture, write nothing

The files are loaded under oracle.ref_loader's mirror of the package (`_ref_op.*`), extended here at run time.  Stubbed, and
only these: the package attributes the files import (taken from the sibling files the mirror already loads), the encoder
Block pointvit.py imports (the decoders do not use it), the absolute `openpoints.models.layers` import of upsampling.py, the
CUDA extension's three_nn_wrapper / three_interpolate_wrapper (the literal CPU restatements below), and torch.cuda.FloatTensor
/ IntTensor (CPU allocations while the fixture is generated).

Cases (eval mode, randomised BatchNorm statistics, narrow widths; weights and inputs are fp16-representable values stored as
float16 to keep the file small):
  * s3dis -- PointViTDecoder([7, 48, 96], global_feat 'cls,max', progressive_input) + SegHead(13, mlps [64], ln1d), [2, 1024],
    p1 / p2 from the reference FPS;
  * part  -- PointViTPartDecoder([7, 32, 64], 'cls,max,avg', progressive_input, act_args gelu as the recipe's merged encoder
    arguments give it) + SegHead(50, mlps [64], bn) with class labels, [2, 256];
  * resample -- PointViTDecoder([7, 32, 64], progressive_input False) on p = [p0, p_centres]: the decoder inserts the FPS
    points itself; + SegHead(13, global_feat 'max', bn), [2, 512];
  * interp/* -- bare three_interpolation on duplicated known points (ties) and with m in {1, 2}.
The clouds are chosen so that among every query's 4 nearest known points (distinct positions, where duplicates are
deliberate) consecutive distances differ by more than 1e-5 (relative): the three_nn order then does not depend on how the
distance is rounded.  ``recipe/<name>/keys`` holds the full-width decoder + head state-dict keys and shapes of the
S3DIS / ScanNet / ShapeNetPart recipes.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointseg.npz")

# the recipes' decoder_args / cls_args (PointCloud/cfgs/<recipe>/metatransformer.yaml) at full width; encoder_channel_list is
# P3Embed's channel_list with the encoder width last (pointvit.py:87-88), in_channels the decoder's out_channels (base_seg.py)
RECIPES = {
    "s3dis": dict(decoder="PointViTDecoder", dec=dict(encoder_channel_list=[7, 384, 768], channel_scaling=1, global_feat="cls,max",
                                                      progressive_input=True),
                  head=dict(num_classes=13, mlps=[256], norm_args={"norm": "ln1d"})),
    "scannet": dict(decoder="PointViTDecoder", dec=dict(encoder_channel_list=[7, 384, 768], channel_scaling=1, global_feat="cls,max",
                                                        progressive_input=True),
                    head=dict(num_classes=20, global_feat="max", norm_args={"norm": "bn"})),
    "shapenetpart": dict(decoder="PointViTPartDecoder", dec=dict(encoder_channel_list=[7, 384, 768], channel_scaling=1,
                                                                 global_feat="cls,max,avg", progressive_input=True,
                                                                 act_args={"act": "gelu"}),
                         head=dict(num_classes=50, mlps=[256], norm_args={"norm": "bn"})),
}
CASES = {
    "s3dis": dict(decoder="PointViTDecoder", dec=dict(encoder_channel_list=[7, 48, 96], global_feat="cls,max", progressive_input=True),
                  head=dict(num_classes=13, mlps=[64], norm_args={"norm": "ln1d"}), B=2, N=1024, resample=False),
    "part": dict(decoder="PointViTPartDecoder", dec=dict(encoder_channel_list=[7, 32, 64], global_feat="cls,max,avg",
                                                         progressive_input=True, act_args={"act": "gelu"}),
                 head=dict(num_classes=50, mlps=[64], norm_args={"norm": "bn"}), B=2, N=256, resample=False),
    "resample": dict(decoder="PointViTDecoder", dec=dict(encoder_channel_list=[7, 32, 64], progressive_input=False),
                     head=dict(num_classes=13, mlps=[64], global_feat="max", norm_args={"norm": "bn"}), B=2, N=512, resample=True),
}
INTERP = {"dup": (2, 512, 64, 8, True), "m1": (2, 300, 1, 5, False), "m2": (2, 300, 2, 12, False)}   # B, n, m, C, duplicated


# ----------------------------------------------------------------------------------------------------- the CUDA ops on CPU

def cpu_three_nn(b, n, m, unknown, known, dist2, idx):
    """three_nn_kernel_fast (interpolate_gpu.cu) per query: known points in index order, d = (ux - x)^2 + (uy - y)^2 +
    (uz - z)^2 in fp32, strict-< insertion into best1..3 (initialised to 1e40, index 0); vectorised over the queries"""
    u, k = unknown.float(), known.float()
    best = torch.full((b, n, 3), 1e40, dtype=torch.float64)
    besti = torch.zeros(b, n, 3, dtype=torch.int32)
    for j in range(m):
        x, y, z = k[:, j, 0:1], k[:, j, 1:2], k[:, j, 2:3]
        d = ((u[..., 0] - x) * (u[..., 0] - x) + (u[..., 1] - y) * (u[..., 1] - y) + (u[..., 2] - z) * (u[..., 2] - z)).double()
        c1, c2, c3 = d < best[..., 0], d < best[..., 1], d < best[..., 2]
        nb, ni = best.clone(), besti.clone()
        # if d < best1: shift 1 -> 2 -> 3; elif d < best2: shift 2 -> 3; elif d < best3: replace 3
        nb[..., 2] = torch.where(c2, best[..., 1], torch.where(c3, d, best[..., 2]))
        ni[..., 2] = torch.where(c2, besti[..., 1], torch.where(c3, torch.full_like(besti[..., 2], j), besti[..., 2]))
        nb[..., 1] = torch.where(c1, best[..., 0], torch.where(c2, d, best[..., 1]))
        ni[..., 1] = torch.where(c1, besti[..., 0], torch.where(c2, torch.full_like(besti[..., 1], j), besti[..., 1]))
        nb[..., 0] = torch.where(c1, d, best[..., 0])
        ni[..., 0] = torch.where(c1, torch.full_like(besti[..., 0], j), besti[..., 0])
        best, besti = nb, ni
    dist2.copy_(best.float())
    idx.copy_(besti)
    NN_LOG.append(besti.clone())


def cpu_three_interpolate(b, c, m, n, points, idx, weight, out):
    """three_interpolate_kernel_fast: out[b, c, q] = w0 f[b, c, i0] + w1 f[b, c, i1] + w2 f[b, c, i2] (fp32)"""
    i = idx.long()
    g = [torch.gather(points, 2, i[..., j].unsqueeze(1).expand(b, c, n)) for j in range(3)]
    w = [weight[..., j].unsqueeze(1) for j in range(3)]
    out.copy_(w[0] * g[0] + w[1] * g[1] + w[2] * g[2])


NN_LOG = []


# ----------------------------------------------------------------------------------------------------- loading the reference

def load_reference():
    """(pointvit module, base_seg module, upsampling module), loaded unmodified under oracle.ref_loader's package mirror"""
    from oracle import ref_loader
    ref_loader.reference_pointcloud_modules()
    root = os.path.join(ref_loader.REF_ROOT, "PointCloud", "openpoints")
    L = "_ref_op.models.layers"
    layers = sys.modules[L]

    def pkg(name, path=None, **attrs):
        m = sys.modules.get(name)
        if m is None:
            m = types.ModuleType(name)
            m.__path__ = [path] if path else []
            sys.modules[name] = m
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    def load(full, rel):
        if full in sys.modules and getattr(sys.modules[full], "__file__", None):
            return sys.modules[full]
        spec = importlib.util.spec_from_file_location(full, os.path.join(root, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
        return mod

    conv, norm, act = sys.modules[L + ".conv"], sys.modules[L + ".norm"], sys.modules[L + ".activation"]
    sub, grp, la = sys.modules[L + ".subsample"], sys.modules[L + ".group"], sys.modules[L + ".local_aggregation"]
    ext = sys.modules["openpoints.cpp.pointnet2_batch"].pointnet2_cuda
    ext.three_nn_wrapper, ext.three_interpolate_wrapper = cpu_three_nn, cpu_three_interpolate
    pkg("openpoints.models"); pkg("openpoints.models.layers", create_convblock1d=conv.create_convblock1d)
    up = load(L + ".upsampling", "models/layers/upsampling.py")

    class _Block:                     # layers.attention.Block: the encoder's, which the decoders never construct
        def __init__(self, *a, **k):
            raise RuntimeError("stub")
    pkg(L + ".attention", Block=_Block)
    for k, v in dict(create_convblock1d=conv.create_convblock1d, create_convblock2d=conv.create_convblock2d,
                     create_linearblock=conv.create_linearblock, create_norm=norm.create_norm, create_act=act.create_act,
                     CHANNEL_MAP=la.CHANNEL_MAP, create_grouper=grp.create_grouper, get_aggregation_feautres=grp.get_aggregation_feautres,
                     furthest_point_sample=sub.furthest_point_sample, random_sample=sub.random_sample,
                     three_interpolation=up.three_interpolation).items():
        setattr(layers, k, v)
    pkg("_ref_op.models.backbone", os.path.join(root, "models", "backbone"))
    pkg("_ref_op.models.segmentation", os.path.join(root, "models", "segmentation"))
    load("_ref_op.models.backbone.pointnext", "models/backbone/pointnext.py")
    pv = load("_ref_op.models.backbone.pointvit", "models/backbone/pointvit.py")
    bs = load("_ref_op.models.segmentation.base_seg", "models/segmentation/base_seg.py")
    return pv, bs, up


class _CpuCudaTensors:
    """torch.cuda.FloatTensor / IntTensor as CPU allocations while the fixture is generated"""

    def __enter__(self):
        self.saved = torch.cuda.FloatTensor, torch.cuda.IntTensor
        torch.cuda.FloatTensor = lambda *s: torch.empty(*s, dtype=torch.float32)
        torch.cuda.IntTensor = lambda *s: torch.empty(*s, dtype=torch.int32)

    def __exit__(self, *a):
        torch.cuda.FloatTensor, torch.cuda.IntTensor = self.saved


# ----------------------------------------------------------------------------------------------------- cases

def _h(t: torch.Tensor) -> torch.Tensor:
    """rounded to fp16-representable values (stored as float16, exact in fp32)"""
    return t.half().float()


def _randomize(mod, g):
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(_h(0.1 * torch.randn(m.running_mean.shape, generator=g)))
            m.running_var.copy_(_h(0.5 + torch.rand(m.running_var.shape, generator=g)))
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)):
            m.weight.data.copy_(_h(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g)))
            m.bias.data.copy_(_h(0.05 * torch.randn(m.bias.shape, generator=g)))
        elif isinstance(m, torch.nn.Conv1d):
            m.weight.data.copy_(_h(torch.randn(m.weight.shape, generator=g) * (m.weight[0].numel() ** -0.5)))
            if m.bias is not None:
                m.bias.data.copy_(_h(0.05 * torch.randn(m.bias.shape, generator=g)))


def nn_margin(unknown: torch.Tensor, known: torch.Tensor, dedup: bool = False) -> float:
    """smallest relative gap between consecutive float64 distances among every query's 4 nearest known positions"""
    k = known.double()
    if dedup:
        k = k[:, : k.shape[1] // 2]
    d = torch.cdist(unknown.double(), k, compute_mode="donot_use_mm_for_euclid_dist").pow(2)
    t = min(4, d.shape[2])
    if t < 2:
        return float("inf")
    v = d.topk(t, dim=2, largest=False).values
    return float(((v[..., 1:] - v[..., :-1]) / v[..., 1:].clamp_min(1e-30)).min())


def generate() -> dict:
    pv, bs, up = load_reference()
    fps = sys.modules["_ref_op.models.layers.subsample"].furthest_point_sample
    out = {}
    with _CpuCudaTensors():
        for name, r in RECIPES.items():
            dec = getattr(pv, r["decoder"])(**r["dec"])
            head = bs.SegHead(in_channels=dec.out_channels, **r["head"])
            out[f"recipe/{name}/config"] = json.dumps(r)
            out[f"recipe/{name}/keys"] = json.dumps([["decoder." + k, list(v.shape)] for k, v in dec.state_dict().items()]
                                                    + [["head." + k, list(v.shape)] for k, v in head.state_dict().items()])
            out[f"recipe/{name}/out_channels"] = np.int64(dec.out_channels)
        for ci, (name, c) in enumerate(CASES.items()):
            g = torch.Generator().manual_seed(7300 + ci)
            dec = getattr(pv, c["decoder"])(**c["dec"]).eval()
            head = bs.SegHead(in_channels=dec.out_channels, **c["head"]).eval()
            _randomize(dec, g)
            _randomize(head, g)
            B, N, ch = c["B"], c["N"], c["dec"]["encoder_channel_list"]
            for attempt in range(100):
                p0 = _h(torch.rand(B, N, 3, generator=g) * 2 - 1)
                p1 = torch.gather(p0, 1, fps(p0, N // 4).long().unsqueeze(-1).expand(-1, -1, 3))
                p2 = torch.gather(p1, 1, fps(p1, N // 16).long().unsqueeze(-1).expand(-1, -1, 3))
                if min(nn_margin(p1, p2), nn_margin(p0, p1)) > 1e-5:
                    break
            else:
                raise RuntimeError(f"{name}: no cloud with separated nearest neighbours")
            f0 = _h(torch.randn(B, ch[0], N, generator=g))
            if c["resample"]:                    # p = [p0, centres]: the decoder inserts FPS(p0, N // 4) itself
                p = [p0, p2]
                f = [f0, _h(torch.randn(B, ch[-1], N // 16 + 1, generator=g))]
            else:
                p = [p0, p1, p2]
                f = [f0, _h(torch.randn(B, ch[1], N // 4, generator=g)), _h(torch.randn(B, ch[-1], N // 16 + 1, generator=g))]
            inputs = {f"{name}/p{i}": t.half().numpy() for i, t in enumerate(p)}
            inputs.update({f"{name}/f{i}": t.half().numpy() for i, t in enumerate(f)})
            args = [list(p), list(f)]
            if c["decoder"] == "PointViTPartDecoder":
                cls_label = torch.randint(0, 16, (B, 1), generator=g)
                inputs[f"{name}/cls_label"] = cls_label.numpy()
                args.append(cls_label)
            NN_LOG.clear()
            with torch.no_grad():
                f_out = dec(*args)
                logits = head(f_out)
            out.update(inputs)
            out.update({f"{name}/config": json.dumps(c), f"{name}/logits": logits.numpy(),
                        f"{name}/nn_stages": np.int64(len(NN_LOG)),
                        f"{name}/f_out_head": f_out[:, :, :32].contiguous().numpy()})
            for s, i in enumerate(NN_LOG):
                out[f"{name}/nn{s}"] = i.numpy().astype(np.int16)
            for prefix, mod in (("decoder", dec), ("head", head)):
                for k, v in mod.state_dict().items():
                    out[f"{name}/w/{prefix}.{k}"] = v.numpy() if v.dtype == torch.int64 else v.half().numpy()
            print(f"  {name}: attempt {attempt}, f_out {tuple(f_out.shape)}, logits {tuple(logits.shape)}")
        for ci, (name, (B, n, m, C, dup)) in enumerate(INTERP.items()):
            g = torch.Generator().manual_seed(7400 + ci)
            for attempt in range(100):
                unknown = _h(torch.rand(B, n, 3, generator=g) * 2 - 1)
                known = _h(torch.rand(B, m, 3, generator=g) * 2 - 1)
                if dup:
                    known[:, m // 2:] = known[:, : m - m // 2].clone()
                if nn_margin(unknown, known, dedup=dup) > 1e-5:
                    break
            else:
                raise RuntimeError(f"interp/{name}: no cloud with separated nearest neighbours")
            feat = _h(torch.randn(B, C, m, generator=g))
            NN_LOG.clear()
            res = up.three_interpolation(unknown.contiguous(), known.contiguous(), feat.contiguous())
            out.update({f"interp/{name}/unknown": unknown.half().numpy(), f"interp/{name}/known": known.half().numpy(),
                        f"interp/{name}/feat": feat.half().numpy(), f"interp/{name}/out": res.numpy(),
                        f"interp/{name}/idx": NN_LOG[0].numpy().astype(np.int16)})
            print(f"  interp/{name}: attempt {attempt}, out {tuple(res.shape)}")
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
