"""Write tests/golden/hyperspectral.npz from the reference's own hyperspectral code.

    python tools/make_hyperspectral_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_hyperspectral_golden.py --check    # regenerate and compare with the stored fixture, write nothing

What runs is the reference's, unmodified:
  * `mirror_hsi`, `gain_neighborhood_pixel`, `gain_neighborhood_band` of Hyper-spectrum/train.py.  That file is a script (it parses
    arguments and loads a dataset at import), so it is parsed and only those three function nodes are compiled, at run time;
  * `MetaTransformer.forward` of Hyper-spectrum/metatransformer.py (imported as it is; it needs only einops).  Its `__init__` loads a
    checkpoint file and timm, so the object is assembled attribute by attribute -- the same attributes, in the same order -- with
    seeded weights, and the transformer is the reference's in-tree Block (oracle.ref_loader.reference_encoder).

Stored (cases and synthetic inputs: tests/hyperspectral_cases.py), per small case `<c>`:
  `<c>/cube` float32, `<c>/points` int64, `<c>/gathered` float32 (the reference's float64 tensor of float32 data: exact),
  `<c>/param/<name>` float32, `<c>/out` float64 (the tokenizer half of forward, evaluated in float64) and `<c>/out_ref_err`, the
  reference's own float32-vs-float64 distance.  For the classifier case: `cls/sd/<key>` float32 for every state-dict key,
  `cls/keys` (JSON list of [key, shape]), `cls/logits` float64, `cls/config` (JSON).
"""
from __future__ import annotations

import argparse
import ast
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import hyperspectral_cases as hc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "hyperspectral.npz")
FUNCS = ("mirror_hsi", "gain_neighborhood_pixel", "gain_neighborhood_band")


def load_reference():
    """(namespace holding the three train.py functions, the metatransformer module)"""
    from oracle import ref_loader
    path = os.path.join(ref_loader.REF_ROOT, "Hyper-spectrum", "train.py")
    tree = ast.parse(open(path).read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(n.name for n in nodes) == sorted(FUNCS), [n.name for n in nodes]
    ns = {"np": np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    mt = ref_loader._load_file("_ref_hyper_mt", os.path.join("Hyper-spectrum", "metatransformer.py"))
    return ns, mt


def reference_gather(ns, cube: np.ndarray, points: np.ndarray, patch: int, band_patch: int) -> np.ndarray:
    """train.py:320-325 for the given pixels: [B, bands, patch^2 band_patch] float64"""
    H, W, bands = cube.shape
    with contextlib.redirect_stdout(io.StringIO()):
        mirror = ns["mirror_hsi"](H, W, bands, cube, patch=patch)
    x = np.zeros((points.shape[0], patch, patch, bands), dtype=float)
    for i in range(points.shape[0]):
        x[i] = ns["gain_neighborhood_pixel"](mirror, points, i, patch)
    return ns["gain_neighborhood_band"](x, bands, band_patch, patch).transpose(0, 2, 1)


def assemble(mt, name: str, params: dict, C: int, transformer: nn.Module, num_classes: int):
    """a MetaTransformer with the attributes its __init__ sets, without the checkpoint load"""
    _, _, bands, p, bp = hc.geometry(name)
    m = mt.MetaTransformer.__new__(mt.MetaTransformer)
    nn.Module.__init__(m)
    m.pos_embedding = nn.Parameter(torch.from_numpy(params["pos_embedding"]).clone())
    m.patch_to_embedding = nn.Linear(p * p * bp, C)
    m.patch_to_embedding.weight.data.copy_(torch.from_numpy(params["patch_to_embedding.weight"]))
    m.patch_to_embedding.bias.data.copy_(torch.from_numpy(params["patch_to_embedding.bias"]))
    m.cls_token = nn.Parameter(torch.from_numpy(params["cls_token"]).clone())
    m.dropout = nn.Dropout(0.)
    m.transformer = transformer
    m.pool = "cls"
    m.to_latent = nn.Identity()
    m.mlp_head = nn.Sequential(nn.LayerNorm(C), nn.Linear(C, num_classes))
    return m.eval()


class _Tokens(nn.Module):
    """stands where the transformer does and keeps what reaches it: the tokenizer half of the reference's forward"""

    def forward(self, x):
        self.seen = x.detach().clone()
        return x


def generate() -> dict:
    from oracle import ref_loader
    ns, mt = load_reference()
    out = {}
    for name, (H, W, bands, p, bp) in hc.SMALL.items():
        cube, pts = hc.make_cube(name), hc.make_points(name)
        g = reference_gather(ns, cube, pts, p, bp)
        assert g.dtype == np.float64 and np.array_equal(g, g.astype(np.float32)), name
        params = hc.make_params(name, hc.SMALL_C)
        res = {}
        for dt in (torch.float64, torch.float32):
            spy = _Tokens()
            m = assemble(mt, name, params, hc.SMALL_C, spy, 3).to(dt)
            with torch.no_grad():
                m(torch.from_numpy(g).to(dt))
            res[dt] = spy.seen.double().numpy()
        out[f"{name}/cube"], out[f"{name}/points"], out[f"{name}/gathered"] = cube, pts, g.astype(np.float32)
        for k, v in params.items():
            out[f"{name}/param/{k}"] = v
        out[f"{name}/out"] = res[torch.float64]
        out[f"{name}/out_ref_err"] = np.float64(np.abs(res[torch.float32] - res[torch.float64]).max() / np.abs(res[torch.float64]).max())
        print(f"  {name}: gathered {g.shape}, out {res[torch.float64].shape}, ref_err {out[f'{name}/out_ref_err']:.1e}")
    c = hc.CLASSIFIER
    name, C = c["case"], c["dim"]
    torch.manual_seed(hc._seed("classifier"))
    enc = ref_loader.reference_encoder(c["depth"], C, c["heads"], mlp_ratio=c["mlp_dim"] / C)
    m = assemble(mt, name, hc.make_params(name, C), C, enc, c["num_classes"])
    with torch.no_grad():
        for prm in m.mlp_head.parameters():
            prm.normal_(0.0, 0.5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.from_numpy(out[f"{name}/gathered"])
    with torch.no_grad():
        logits64 = m.double()(g.double()).numpy()
    out["cls/config"] = json.dumps(c)
    out["cls/keys"] = json.dumps([[k, list(v.shape)] for k, v in sd.items()])
    for k, v in sd.items():
        out["cls/sd/" + k] = v.float().numpy()
    out["cls/logits"] = logits64
    print(f"  classifier: {len(sd)} keys, logits {logits64.shape}")
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
