"""Write tests/golden/msda.npz from the reference's own multi-scale deformable attention and ViT-Adapter interaction code:
Image/detection/ops/functions/ms_deform_attn_func.py, ops/modules/ms_deform_attn.py and
mmdet_custom/models/backbones/adapter_modules.py, all three loaded unmodified.

    python tools/make_msda_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_msda_golden.py --check    # regenerate and compare with the stored fixture, write nothing

The files are loaded by path under synthetic package names (`_ref_msda.functions`, `_ref_msda.modules`; `ops.modules` is an
alias of the loaded module file, which is what adapter_modules.py imports).  Stand-ins, and only these: the compiled extension
`MultiScaleDeformableAttention` (an empty module; the reference's CPU entry point raises), with `MSDeformAttnFunction.apply`
routed to the reference's own `ms_deform_attn_core_pytorch`, and timm's DropPath (the in-tree twin oracle.ref_loader mirrors).
The `Block`s of the block case are those of base/vit.py through oracle.ref_loader.reference_detection_vit_module.

Inputs and parameters are not stored: tests/msda_cases.py synthesises them from a counter hash on both sides (the fixture is
kept below 1 MB; the value tensors of these cases alone would take 2 MB and more).  Stored per output / gradient `t` of a case:
  * `<case>/<t>`      the reference evaluated in float64 at the flat positions msda_cases.subset_index(numel) (everything for
                      tensors up to 2048 elements, an even stride beyond), followed by the element of largest magnitude;
  * `<case>/<t>/argmax`  the flat position of that element (so the stored values carry the whole tensor's scale);
  * `<case>/<t>/ref_err`  max |reference in float32 - reference in float64| / max |float64| over the whole tensor: the
                      reference's own distance from exact arithmetic, which the tests' bounds are multiples of.
Cases: core/* (the bare function: injector- and extractor-like, D = 64, D = 20, locations outside the levels, a pile-up of all
samples onto one 2 x 2 neighbourhood per level), module/* (MSDeformAttn with both reference_points widths, with and without
padding mask, ratio 1.0 and 0.5, random non-zero sampling_offsets / attention_weights weights), block/* (one InteractionBlock
around two reference Blocks), keys/* (state-dict keys and shapes of `interactions` at the Base detection / segmentation width),
init/* (the result of _reset_parameters under torch.manual_seed(0)) and points/* (deform_inputs for a 128 x 192 image).
Every sampling location used lies at least 1e-3 pixel from a pixel boundary, in float64 and in float32 arithmetic (the gradient
with respect to a location jumps there); the generator asserts it on the locations the reference actually samples.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import msda_cases as mc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "msda.npz")
# the Base recipes (configs/mask_rcnn/mask_rcnn_meta_transformer_adapter_base_fpn_3x_coco.py:14-24,
# configs/ade20k/upernet_meta_transformer_base_512_160k_ade20k.py:14-24): four interactions, the last with extra extractors
RECIPES = {"det_base": dict(dim=768, num_heads=12, n_points=4, cffn_ratio=0.25, deform_ratio=0.5, drop_path=0.3, n=4),
           "seg_base": dict(dim=768, num_heads=12, n_points=4, cffn_ratio=0.25, deform_ratio=0.5, drop_path=0.3, n=4)}
SAMPLED = []          # (locations, shapes) of every call of the sampling function, for the pixel-boundary check


def load_reference():
    """(function module, MSDeformAttn module file, adapter_modules, base/vit.py module)"""
    from oracle import ref_loader
    vit = ref_loader.reference_detection_vit_module()           # also installs the timm stand-in with the in-tree DropPath
    ops_dir = os.path.join("Image", "detection", "ops")
    sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
    for name in ("_ref_msda", "_ref_msda.functions", "_ref_msda.modules"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    fn = ref_loader._load_file("_ref_msda.functions.ms_deform_attn_func", os.path.join(ops_dir, "functions", "ms_deform_attn_func.py"))

    class Routed:
        """MSDeformAttnFunction.apply -> ms_deform_attn_core_pytorch (same file)"""
        @staticmethod
        def apply(value, shapes, level_start, loc, attn, im2col_step=None):
            hw = [(int(h), int(w)) for h, w in shapes]
            SAMPLED.append((loc.detach().numpy().copy(), hw))
            return fn.ms_deform_attn_core_pytorch(value, hw, loc, attn)
    sys.modules["_ref_msda.functions"].MSDeformAttnFunction = Routed
    mod = ref_loader._load_file("_ref_msda.modules.ms_deform_attn", os.path.join(ops_dir, "modules", "ms_deform_attn.py"))
    sys.modules["ops"] = types.ModuleType("ops")
    sys.modules["ops.modules"] = mod
    am = ref_loader._load_file("_ref_adapter_modules",
                               os.path.join("Image", "detection", "mmdet_custom", "models", "backbones", "adapter_modules.py"))
    return fn, mod, am, vit


def T(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def put(out: dict, key: str, t64: torch.Tensor, t32: torch.Tensor):
    a64, a32 = t64.detach().double().numpy().reshape(-1), t32.detach().double().numpy().reshape(-1)
    mx = float(np.abs(a64).max())
    am = int(np.abs(a64).argmax())
    out[key] = a64[np.append(mc.subset_index(a64.size), am)]
    out[key + "/argmax"] = np.int64(am)
    out[key + "/ref_err"] = np.float64(np.abs(a32 - a64).max() / max(mx, 1e-30))


def load_params(module, tag: str, dtype):
    sd = mc.state_dict_arrays([(k, tuple(v.shape)) for k, v in module.state_dict().items()], tag)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return module.to(dtype)


def run_core(fn, name: str, dtype):
    i = mc.core_inputs(name)
    v, lo, aw = (T(i[k], dtype).requires_grad_() for k in ("value", "loc", "attn"))
    out = fn.ms_deform_attn_core_pytorch(v, i["shapes"], lo, aw)
    out.backward(T(i["dout"], dtype))
    return dict(out=out, dvalue=v.grad, dloc=lo.grad, dattn=aw.grad)


def run_module(mod, name: str, dtype):
    c, i = mc.MODULE[name], mc.module_inputs(name)
    m = load_params(mod.MSDeformAttn(d_model=c["d_model"], n_levels=len(c["shapes"]), n_heads=c["M"], n_points=c["P"], ratio=c["ratio"]),
                    "module/" + name, dtype)
    q, f = T(i["query"], dtype).requires_grad_(), T(i["feat"], dtype).requires_grad_()
    mask = None if i["mask"] is None else torch.from_numpy(i["mask"])
    y = m(q, T(i["ref"], dtype), f, torch.tensor(i["shapes"]), torch.tensor(i["starts"]), mask)
    y.backward(T(i["dout"], dtype))
    res = dict(out=y, dquery=q.grad, dinput=f.grad)
    res.update({"dparam/" + k: p.grad for k, p in m.named_parameters()})
    return res


def run_block(am, vit, dtype):
    b, i = mc.BLOCK, mc.block_inputs()
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    ib = load_params(am.InteractionBlock(dim=b["dim"], num_heads=b["num_heads"], n_points=b["n_points"], norm_layer=norm,
                                         with_cffn=b["with_cffn"], cffn_ratio=b["cffn_ratio"], init_values=b["init_values"],
                                         deform_ratio=b["deform_ratio"], extra_extractor=b["extra_extractor"]), "block/interaction", dtype)
    blocks = load_params(torch.nn.Sequential(*[vit.Block(dim=b["dim"], num_heads=b["vit_heads"], qkv_bias=True, norm_layer=norm,
                                                          layer_scale=True) for _ in range(b["depth"])]), "block/vit", dtype)
    ib.eval(); blocks.eval()
    h, w = i["image_hw"]
    d1, d2 = am.deform_inputs(torch.zeros(1, 3, h, w))
    d1[0], d2[0] = d1[0].to(dtype), d2[0].to(dtype)
    x, c = T(i["x"], dtype).requires_grad_(), T(i["c"], dtype).requires_grad_()
    xo, co = ib(x, c, blocks, d1, d2, b["H"], b["W"])
    torch.autograd.backward([xo, co], [T(i["dx"], dtype), T(i["dc"], dtype)])
    res = dict(x_out=xo, c_out=co, dx=x.grad, dc=c.grad)
    for k in ("injector.gamma", "injector.attn.sampling_offsets.weight", "extractor.attn.value_proj.weight",
              "extra_extractors.1.ffn.fc1.weight"):
        res["dparam/" + k] = dict(ib.named_parameters())[k].grad
    return res


def generate() -> dict:
    fn, mod, am, vit = load_reference()
    out = {}
    for name in mc.CORE:
        r64, r32 = run_core(fn, name, torch.float64), run_core(fn, name, torch.float32)
        for k in r64:
            put(out, f"core/{name}/{k}", r64[k], r32[k])
        print(f"  core/{name}: ref_err out {out[f'core/{name}/out/ref_err']:.2e} dvalue {out[f'core/{name}/dvalue/ref_err']:.2e} "
              f"dloc {out[f'core/{name}/dloc/ref_err']:.2e} dattn {out[f'core/{name}/dattn/ref_err']:.2e}")
    for name in mc.MODULE:
        SAMPLED.clear()
        r64, r32 = run_module(mod, name, torch.float64), run_module(mod, name, torch.float32)
        margin = min(mc.check_clear(lo, hw, f"module/{name}") for lo, hw in SAMPLED)
        for k in r64:
            put(out, f"module/{name}/{k}", r64[k], r32[k])
        print(f"  module/{name}: boundary margin {margin:.3f}, ref_err out {out[f'module/{name}/out/ref_err']:.2e}")
    SAMPLED.clear()
    r64, r32 = run_block(am, vit, torch.float64), run_block(am, vit, torch.float32)
    margin = min(mc.check_clear(lo, hw, "block") for lo, hw in SAMPLED)
    for k in r64:
        put(out, f"block/{k}", r64[k], r32[k])
    print(f"  block: {len(SAMPLED)} sampling calls, boundary margin {margin:.3f}, ref_err x {out['block/x_out/ref_err']:.2e} "
          f"c {out['block/c_out/ref_err']:.2e}")
    norm = partial(torch.nn.LayerNorm, eps=1e-6)
    for name, r in RECIPES.items():
        inter = torch.nn.Sequential(*[am.InteractionBlock(dim=r["dim"], num_heads=r["num_heads"], n_points=r["n_points"], init_values=0.,
                                                           drop_path=r["drop_path"], norm_layer=norm, with_cffn=True,
                                                           cffn_ratio=r["cffn_ratio"], deform_ratio=r["deform_ratio"],
                                                           extra_extractor=(i == r["n"] - 1)) for i in range(r["n"])])
        out[f"keys/{name}/config"] = json.dumps(r)
        out[f"keys/{name}/keys"] = json.dumps([[k, list(v.shape)] for k, v in inter.state_dict().items()])
    torch.manual_seed(0)
    m = mod.MSDeformAttn(d_model=96, n_levels=3, n_heads=6, n_points=4, ratio=0.5)
    out["init/config"] = json.dumps(dict(d_model=96, n_levels=3, n_heads=6, n_points=4, ratio=0.5, seed=0))
    for k, v in m.state_dict().items():
        out["init/" + k] = v.numpy()
    d1, d2 = am.deform_inputs(torch.zeros(1, 3, 128, 192))
    for tag, d in (("points/1", d1), ("points/2", d2)):
        out[tag + "/reference_points"], out[tag + "/spatial_shapes"], out[tag + "/level_start_index"] = (t.numpy() for t in d)
    out["points/image_hw"] = np.array([128, 192])
    return {k: np.asarray(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the stored fixture instead of writing it")
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = generate()
    if args.check:
        z = np.load(GOLDEN, allow_pickle=False)
        assert sorted(z.files) == sorted(out), sorted(set(z.files) ^ set(out))
        bad = [k for k in out if out[k].dtype != z[k].dtype or out[k].tobytes() != z[k].tobytes()]
        assert not bad, f"differs from {GOLDEN}: {bad[:8]}"
        print(f"[check] {GOLDEN}: {len(out)} arrays identical")
        return
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN) / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
