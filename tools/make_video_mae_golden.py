"""Write tests/golden/video_mae.npz from the reference's own VideoMAE pre-training model.

    python tools/make_video_mae_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_video_mae_golden.py --check    # regenerate and compare with the stored fixture, write nothing

What runs is the reference's Video/models/modeling_pretrain.py, unmodified (``PretrainVisionTransformer`` and, for the encoder alone,
its ``encoder.forward_features``).  The file imports ``.modeling_finetune`` relatively and timm helpers: it is loaded under a
synthetic parent package whose ``__path__`` is Video/models, with the timm stand-in of oracle.ref_loader (decorators and initialisers,
no arithmetic).  The loss is the formula of Video/engine_for_pretraining.py:75-105 written with einops (that file is a training
script that cannot be imported here); tests/test_video_mae_cpu.py ties tests/video_mae_cases.py to the same formulation.

Cases, variants and synthetic inputs: tests/video_mae_cases.py.  Weights are the reference's initialisation, then every parameter is
redrawn or rounded onto a 1/1024 grid (biases, norms and tokens are made non-trivial), so that the stored float32 arrays -- in full --
compress.  Stored, for case `<c>` in (p16, p8) and variant `<v>` (`<c>`, `<c>_dm` with a decoder mask, `p8_ls_dm` with layer scale too):
  `<c>/clip` float32, `<c>/mask`, `<c>/decode_mask` bool, `<c>/sd/<key>` float32 for every reference state-dict key, `<c>/keys`
  (JSON list of [key, shape]), `<c>/sd_ls/<key>` the layer-scale vectors of the `_ls` variants (the other weights are shared);
  `<v>/out` the model output and `<v>/enc` the encoder's forward_features, evaluated in float64 and stored as float32;
  `<v>/out_ref_err` the reference's own float32-vs-float64 distance; `<v>/loss` float64; `<v>/grad/<key>` float32 (float64
  autograd of that loss) for the keys of video_mae_cases.grad_keys(v); without a decoder mask `<v>/grad_rows/encoder.patch_embed.proj.weight`,
  the output channels video_mae_cases.PROJ_GRAD_ROWS of that gradient.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import video_mae_cases as vc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "video_mae.npz")
GRID = 1024.0


def load_reference():
    """the reference's modeling_pretrain module"""
    from oracle import ref_loader
    for k, v in ref_loader._timm_stub().items():
        sys.modules.setdefault(k, v)
    pkg = types.ModuleType("_ref_video_models")
    pkg.__path__ = [os.path.join(ref_loader.REF_ROOT, "Video", "models")]
    sys.modules["_ref_video_models"] = pkg
    return importlib.import_module("_ref_video_models.modeling_pretrain")


def on_grid(t: torch.Tensor) -> torch.Tensor:
    return torch.round(t * GRID) / GRID


def build(mp, case: str, init_values: float, base_sd=None):
    torch.manual_seed(vc._seed(f"model/{case}/{init_values}"))
    model = mp.PretrainVisionTransformer(norm_layer=partial(nn.LayerNorm, eps=vc.MODEL["eps"]), **vc.model_kwargs(case, init_values))
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith(("gamma_1", "gamma_2")):
                prm.copy_(on_grid(init_values + 0.05 * torch.randn_like(prm)))
            elif prm.dim() == 1 and name.endswith("norm1.weight") or name.endswith("norm2.weight") or name.endswith("norm.weight"):
                prm.copy_(on_grid(1.0 + 0.1 * torch.randn_like(prm)))
            elif prm.dim() == 1 or name == "mask_token":
                prm.copy_(on_grid(0.1 * torch.randn_like(prm)))
            else:
                prm.copy_(on_grid(prm))
    if base_sd is not None:
        missing, unexpected = model.load_state_dict(base_sd, strict=False)
        assert not unexpected and all(k.endswith(("gamma_1", "gamma_2")) for k in missing), (missing, unexpected)
    return model.eval()


def reference_loss(out, clip, mask, decode_mask, patch):
    """engine_for_pretraining.py:66-105 with normlize_target=True; decode_masked_pos = ~bool_masked_pos when no decoder mask is used (:55-57)"""
    from einops import rearrange
    dmp = ~mask if decode_mask is None else decode_mask
    mean = torch.as_tensor(vc.MEAN, dtype=clip.dtype)[None, :, None, None, None]
    std = torch.as_tensor(vc.STD, dtype=clip.dtype)[None, :, None, None, None]
    unnorm = clip * std + mean
    sq = rearrange(unnorm, "b c (t p0) (h p1) (w p2) -> b (t h w) (p0 p1 p2) c", p0=vc.MODEL["tubelet"], p1=patch, p2=patch)
    norm = (sq - sq.mean(dim=-2, keepdim=True)) / (sq.var(dim=-2, unbiased=True, keepdim=True).sqrt() + 1e-6)
    patches = rearrange(norm, "b n p c -> b n (p c)")
    B, N, C = patches.shape
    labels = patches[~dmp].reshape(B, -1, C)
    loss = ((out - labels) ** 2).mean(dim=-1)
    cal = mask[~dmp].reshape(B, -1)
    return (loss * cal).sum() / cal.sum()


def generate() -> dict:
    mp = load_reference()
    out = {}
    models = {}
    for case in vc.CASES:
        clip, (mask, dmask) = vc.make_clip(case), vc.make_masks(case)
        base = build(mp, case, 0.)
        sd = {k: v.detach().clone() for k, v in base.state_dict().items()}
        ls = build(mp, case, 0.1, base_sd=sd) if any(v[0] == case and v[2] > 0 for v in vc.VARIANTS.values()) else None
        models[case] = (base, ls)
        out[f"{case}/clip"], out[f"{case}/mask"], out[f"{case}/decode_mask"] = clip, mask, dmask
        out[f"{case}/keys"] = json.dumps([[k, list(v.shape)] for k, v in sd.items()])
        for k, v in sd.items():
            out[f"{case}/sd/{k}"] = v.float().numpy()
        if ls is not None:
            for k, v in ls.state_dict().items():
                if k.endswith(("gamma_1", "gamma_2")):
                    out[f"{case}/sd_ls/{k}"] = v.detach().float().numpy()
    for variant, (case, with_dm, init_values) in vc.VARIANTS.items():
        model = models[case][1 if init_values > 0 else 0]
        clip = torch.from_numpy(out[f"{case}/clip"])
        mask = torch.from_numpy(out[f"{case}/mask"])
        dmask = torch.from_numpy(out[f"{case}/decode_mask"]) if with_dm else None
        with torch.no_grad():
            y32 = model.float()(clip, mask, dmask).double()
        model.double().zero_grad()
        y = model(clip.double(), mask, dmask)
        loss = reference_loss(y, clip.double(), mask, dmask, vc.CASES[case]["patch"])
        loss.backward()
        with torch.no_grad():
            enc = model.encoder.forward_features(clip.double(), mask)
        params = dict(model.named_parameters())
        out[f"{variant}/out"], out[f"{variant}/enc"] = y.detach().float().numpy(), enc.float().numpy()
        out[f"{variant}/out_ref_err"] = np.float64((y32 - y.detach()).abs().max() / y.detach().abs().max())
        out[f"{variant}/loss"] = np.float64(loss.item())
        for k in vc.grad_keys(variant):
            out[f"{variant}/grad/{k}"] = params[k].grad.float().numpy()
        if not with_dm:
            k = "encoder.patch_embed.proj.weight"
            out[f"{variant}/grad_rows/{k}"] = params[k].grad.float().numpy()[list(vc.PROJ_GRAD_ROWS)]
        print(f"  {variant}: out {tuple(y.shape)}, enc {tuple(enc.shape)}, loss {loss.item():.6f}, ref_err {out[f'{variant}/out_ref_err']:.1e}")
        model.float()
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
    size = os.path.getsize(GOLDEN)
    assert size <= 1000 * 1000, f"{GOLDEN} is {size} bytes (at most 1 MB)"
    print(f"wrote {GOLDEN} ({size / 1e6:.2f} MB)")


if __name__ == "__main__":
    main()
