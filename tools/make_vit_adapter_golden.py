"""Write tests/golden/vit_adapter.npz from the reference's own ViT-Adapter backbone: SpatialPriorModule
(Image/detection/mmdet_custom/models/backbones/adapter_modules.py:194-246) and ViTAdapter (vit_adapter.py:19-132), loaded
unmodified by path, with base/vit.py through oracle.ref_loader.reference_detection_vit_module.

    python tools/make_vit_adapter_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_vit_adapter_golden.py --check    # regenerate and compare with the stored fixture, write nothing

Stand-ins: those of tools/make_msda_golden.py (the compiled sampling extension routed to the reference's own
ms_deform_attn_core_pytorch, timm's DropPath) plus only
  * `mmdet.models.builder.BACKBONES`, whose register_module() returns the class;
  * `timm.models.layers.trunc_normal_` = the one of the reference's in-tree weight_init.py.
nn.SyncBatchNorm is NOT replaced: this PyTorch runs it on CPU tensors in training mode too when no process group exists (it
then is F.batch_norm, the function nn.BatchNorm2d calls), so the training cases run the reference's own modules.

Inputs and parameters are synthesised on both sides by tests/vit_adapter_cases.py (the counter hash of tests/msda_cases.py).
Stored per tensor, exactly as msda.npz does: the float64 result at msda_cases.subset_index positions plus the element of
largest magnitude, its position (`/argmax`), and `/ref_err` = max |float32 run - float64 run| / max |float64|.  The eval cases
also store `/ref_err_bf16`: the same distance for the reference modules converted to bfloat16 and run on the CPU.
Cases: spm/eval/{odd,even}, spm/train, backbone/eval, backbone/train, keys/det_base, init/*.

The gradients of the training cases jump where a ReLU pre-activation crosses zero or two values of a pool window swap rank.
For spm/train and backbone/train the generator therefore takes the first tag of vit_adapter_cases.tags() for which, in the
float64 and in the float32 run of the reference, every ReLU pre-activation has |v| >= RELU_MARGIN max |v| of its tensor and
every pool window's winner leads the runner-up by POOL_MARGIN max |input| -- or is exactly zero: such a window holds only dead
ReLU outputs, and whichever tap wins, its gradient stops at that ReLU.  The tag is stored (`<case>/tag`).  The sampling
locations of the training backbone are checked against pixel boundaries as make_msda_golden.py does.  The two gradients of
vit_adapter_cases.BACKBONE_TRAIN_ZERO_GRADS are exactly zero and are asserted to be, not stored.

bfloat16 on the CPU: the spatial prior module is converted with .to(bfloat16); the whole backbone cannot be (the reference's
deform_inputs builds float32 reference points whatever the model's dtype, and its sampling core refuses the mixed dtypes), so
backbone/eval keeps float32 parameters and runs under torch.autocast("cpu", bfloat16).  A case for which neither works is
listed in `bf16_missing` and carries no ref_err_bf16.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import msda_cases as mc  # noqa: E402
import vit_adapter_cases as vc  # noqa: E402
import make_msda_golden as mg  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "vit_adapter.npz")
BACKBONES_DIR = os.path.join("Image", "detection", "mmdet_custom", "models", "backbones")


def load_reference():
    """(adapter_modules, vit_adapter) of the detection copy"""
    from oracle import ref_loader
    _, _, am, vit = mg.load_reference()

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls
    sys.modules["mmdet.models"] = types.ModuleType("mmdet.models")
    builder = types.ModuleType("mmdet.models.builder")
    builder.BACKBONES = _Registry()
    sys.modules["mmdet.models.builder"] = builder
    sys.modules["timm.models.layers"].trunc_normal_ = sys.modules[ref_loader._PKG + ".weight_init"].trunc_normal_
    for name in ("_ref_backbones", "_ref_backbones.base"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    sys.modules["_ref_backbones.base.vit"] = vit
    sys.modules["_ref_backbones.adapter_modules"] = am
    va = ref_loader._load_file("_ref_backbones.vit_adapter", os.path.join(BACKBONES_DIR, "vit_adapter.py"))
    return am, va


def T(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def put(out: dict, key: str, t64, t32, t16=None):
    mg.put(out, key, t64, t32)
    if t16 is not None:
        a64, a16 = t64.detach().double().numpy().reshape(-1), t16.detach().double().numpy().reshape(-1)
        out[key + "/ref_err_bf16"] = np.float64(np.abs(a16 - a64).max() / max(float(np.abs(a64).max()), 1e-30))


def load_params(module, tag: str, dtype):
    sd = vc.state_dict_arrays([(k, tuple(v.shape)) for k, v in module.state_dict().items()], tag)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return module.to(dtype)


class Margins:
    """hooks on every ReLU and MaxPool2d of a module: the smallest relative clearance seen (see the module docstring)"""

    def __init__(self, module):
        self.relu, self.pool = np.inf, np.inf
        self.handles = []
        for m in module.modules():
            if isinstance(m, nn.ReLU):
                self.handles.append(m.register_forward_pre_hook(self._relu))
            elif isinstance(m, nn.MaxPool2d):
                self.handles.append(m.register_forward_pre_hook(self._pool))

    def _relu(self, _m, args):
        v = args[0].detach().double().abs()
        self.relu = min(self.relu, float(v.min() / v.max()))

    def _pool(self, _m, args):
        x = args[0].detach().double()
        win = F.pad(x, (1, 1, 1, 1), value=-np.inf).unfold(2, 3, 2).unfold(3, 3, 2).flatten(-2)
        top = win.topk(2, dim=-1).values
        lead = (top[..., 0] - top[..., 1])[top[..., 0] != 0]
        if lead.numel():
            self.pool = min(self.pool, float(lead.min() / x.abs().max()))

    def ok(self) -> bool:
        return self.relu >= vc.RELU_MARGIN and self.pool >= vc.POOL_MARGIN

    def remove(self):
        for h in self.handles:
            h.remove()


def build_spm(am, c, tag, dtype):
    return load_params(am.SpatialPriorModule(inplanes=c["inplanes"], embed_dim=c["embed_dim"]), tag, dtype)


def build_backbone(va, tag, dtype):
    cfg = dict(vc.BACKBONE)
    return load_params(va.ViTAdapter(img_size=cfg["pretrain_size"], **cfg), tag, dtype)


def find_tag(case: str, c: dict, build, spm_of):
    """the first tag whose spatial prior module run clears both margins in float64 and float32"""
    for tag in vc.tags():
        good = True
        for dtype in (torch.float64, torch.float32):
            model = build(f"{case}/{tag}", dtype).train()
            mar = Margins(spm_of(model))
            with torch.no_grad():
                spm_of(model)(T(vc.image(case, tag, c["B"], c["H"], c["W"]), dtype))
            mar.remove()
            print(f"  {case} tag {tag} {str(dtype)[6:]}: relu margin {mar.relu:.2e} pool margin {mar.pool:.2e}")
            good = good and mar.ok()
            if not good:
                break
        if good:
            return tag
    raise AssertionError(f"{case}: none of the first {vc.MAX_TAGS} tags clears the margins: shrink the case")


def run_spm_eval(am, name, dtype):
    c = vc.SPM_EVAL[name]
    m = build_spm(am, c, f"spm/eval/{name}", torch.float32).to(dtype).eval()
    x = T(vc.image(f"spm/eval/{name}", "", c["B"], c["H"], c["W"]), dtype)
    with torch.no_grad():
        return dict(zip(("c1", "c2", "c3", "c4"), m(x)))


def run_spm_train(am, tag, dtype):
    c = vc.SPM_TRAIN
    m = build_spm(am, c, f"spm/train/{tag}", dtype).train()
    mar = Margins(m)
    x = T(vc.image("spm/train", tag, c["B"], c["H"], c["W"]), dtype).requires_grad_()
    outs = m(x)
    mar.remove()
    assert mar.ok(), (mar.relu, mar.pool)
    names = ("c1", "c2", "c3", "c4")
    torch.autograd.backward(list(outs), [T(vc.cotangent("spm/train", tag, n, o.shape), dtype) for n, o in zip(names, outs)])
    res = dict(zip(names, outs))
    res["dx"] = x.grad
    res.update({"dparam/" + k: p.grad for k, p in m.named_parameters()})
    res.update({"buffer/" + k: b for k, b in m.named_buffers() if not k.endswith("num_batches_tracked")})
    return res


def run_backbone_eval(va, dtype):
    """dtype bfloat16: float32 parameters and image under torch.autocast("cpu", bfloat16) -- converting the module instead
    fails in the reference's sampling core ("expected scalar type BFloat16 but found Float": deform_inputs builds float32
    reference points whatever the model's dtype)"""
    c = vc.BACKBONE_EVAL
    auto = dtype == torch.bfloat16
    m = build_backbone(va, "backbone/eval", torch.float32).to(torch.float32 if auto else dtype).eval()
    x = T(vc.image("backbone/eval", "", c["B"], c["H"], c["W"]), torch.float32 if auto else dtype)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=auto):
        return dict(zip(("f1", "f2", "f3", "f4"), m(x)))


def run_backbone_train(va, tag, dtype):
    c = vc.BACKBONE_TRAIN
    m = build_backbone(va, f"backbone/train/{tag}", dtype).train()
    mar = Margins(m.spm)
    x = T(vc.image("backbone/train", tag, c["B"], c["H"], c["W"]), dtype).requires_grad_()
    mg.SAMPLED.clear()
    outs = m(x)
    mar.remove()
    assert mar.ok(), (mar.relu, mar.pool)
    margin = min(mc.check_clear(lo, hw, "backbone/train") for lo, hw in mg.SAMPLED)
    names = ("f1", "f2", "f3", "f4")
    torch.autograd.backward(list(outs), [T(vc.cotangent("backbone/train", tag, n, o.shape), dtype) for n, o in zip(names, outs)])
    res = dict(zip(names, outs))
    res["dx"] = x.grad
    for k, p in m.named_parameters():
        if k in vc.BACKBONE_TRAIN_ZERO_GRADS:
            assert float(p.grad.abs().max()) <= (1e-12 if dtype == torch.float64 else 1e-4) * float(m.up.weight.grad.abs().max()), k
        elif k.startswith(vc.BACKBONE_TRAIN_GRADS):
            res["dparam/" + k] = p.grad
    return res, margin


def moments(t):
    t = t.detach().double()
    return np.array([float(t.mean()), float(t.std(unbiased=False))])


def generate() -> dict:
    am, va = load_reference()
    out = {}
    bf16_missing = []
    for name in vc.SPM_EVAL:
        r64, r32 = run_spm_eval(am, name, torch.float64), run_spm_eval(am, name, torch.float32)
        try:
            r16 = run_spm_eval(am, name, torch.bfloat16)
        except RuntimeError as e:           # an op of the reference without a CPU bfloat16 kernel: no bf16 figure for this case
            r16, _ = None, bf16_missing.append(f"spm/eval/{name}: {e}")
        for k in r64:
            put(out, f"spm/eval/{name}/{k}", r64[k], r32[k], None if r16 is None else r16[k])
        print(f"  spm/eval/{name}: ref_err c1 {out[f'spm/eval/{name}/c1/ref_err']:.2e} c4 {out[f'spm/eval/{name}/c4/ref_err']:.2e}"
              + ("" if r16 is None else f" bf16 c1 {out[f'spm/eval/{name}/c1/ref_err_bf16']:.2e}"))
    tag = find_tag("spm/train", vc.SPM_TRAIN, lambda t, dt: build_spm(am, vc.SPM_TRAIN, t, dt), lambda m: m)
    out["spm/train/tag"] = np.array(tag)
    r64, r32 = run_spm_train(am, tag, torch.float64), run_spm_train(am, tag, torch.float32)
    for k in r64:
        put(out, f"spm/train/{k}", r64[k], r32[k])
    print(f"  spm/train ({tag}): ref_err c1 {out['spm/train/c1/ref_err']:.2e} dx {out['spm/train/dx/ref_err']:.2e}")
    r64, r32 = run_backbone_eval(va, torch.float64), run_backbone_eval(va, torch.float32)
    try:
        r16 = run_backbone_eval(va, torch.bfloat16)
    except RuntimeError as e:
        r16, _ = None, bf16_missing.append(f"backbone/eval: {e}")
    for k in r64:
        put(out, f"backbone/eval/{k}", r64[k], r32[k], None if r16 is None else r16[k])
    print("  backbone/eval: ref_err " + " ".join(f"{k} {out[f'backbone/eval/{k}/ref_err']:.2e}" for k in r64)
          + ("" if r16 is None else " bf16 " + " ".join(f"{out[f'backbone/eval/{k}/ref_err_bf16']:.2e}" for k in r64)))
    tag = find_tag("backbone/train", vc.BACKBONE_TRAIN, lambda t, dt: build_backbone(va, t, dt), lambda m: m.spm)
    out["backbone/train/tag"] = np.array(tag)
    (r64, m64), (r32, m32) = run_backbone_train(va, tag, torch.float64), run_backbone_train(va, tag, torch.float32)
    for k in r64:
        put(out, f"backbone/train/{k}", r64[k], r32[k])
    print(f"  backbone/train ({tag}): boundary margin {min(m64, m32):.3f}, ref_err f1 {out['backbone/train/f1/ref_err']:.2e} "
          f"dx {out['backbone/train/dx/ref_err']:.2e}")
    for line in bf16_missing:
        print("  no CPU bfloat16 run:", line[:200])
    out["bf16_missing"] = np.array(json.dumps([s.split(":")[0] for s in bf16_missing]))
    base = va.ViTAdapter(**vc.DET_BASE)
    out["keys/det_base/config"] = np.array(json.dumps(vc.DET_BASE))
    out["keys/det_base/keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in base.state_dict().items()]))
    del base
    torch.manual_seed(0)
    cfg = dict(vc.BACKBONE)
    m = va.ViTAdapter(img_size=cfg["pretrain_size"], **cfg)
    out["init/config"] = np.array(json.dumps(dict(cfg, seed=0)))
    init = [(k, v) for k, v in m.state_dict().items() if k.startswith(("spm.", "up.")) or k == "level_embed"]
    out["init/keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in init]))
    out["init/moments"] = np.stack([moments(v) for _, v in init])
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
