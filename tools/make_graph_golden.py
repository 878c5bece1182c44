"""Write tests/golden/graph_tokenizer.npz from the reference's own GraphFeatureTokenizer (Data2Seq/Graph.py, loaded unmodified
through oracle.ref_loader._load_file).

    python tools/make_graph_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_graph_golden.py --check    # regenerate and compare with the stored fixture, write nothing

Stand-ins, and only these, are the two random sources, so that the float32 and the float64 evaluation of a case draw the same
numbers: `torch.rand` as the module sees it and the module's `gaussian_orthogonal_random_matrix_batched` return the stored draws
of tests/graph_cases.py.  The identifiers the reference actually used are recorded by forward pre-hooks on rand_encoder /
orf_encoder / lap_encoder (the [Sn, D] rows of their [B, T, 2D] inputs at the node tokens) and stored as `<case>/ids/<kind>` from
the float32 evaluation: the tests hand them to the product as `node_ids`.

Inputs and parameters are not stored (tests/graph_cases.py synthesises them on both sides).  Stored per case:
  * `<case>/padded_index`, `<case>/padding_mask`   whole;
  * `<case>/<t>`, `<case>/<t>/argmax`, `<case>/<t>/ref_err` for t = out, dparam/<key>, dperturb: the float64 result at
    graph_cases.subset_index positions followed by the element of largest magnitude, its position, and the reference's own
    float32-vs-float64 distance max |f32 - f64| / max |f64| (the unit of the tests' bounds).  ref_err is asserted positive except
    where the reference only copies (dperturb; the token-row gradients of a one-graph batch): the tests ask for equality there.
Also keys/<recipe|default>/{config,keys} (state-dict keys and shapes) and init/* (parameters after construction under
torch.manual_seed(0), for the small configuration).  The case properties the fixture must have are asserted in check_cases().
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import graph_cases as gc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_tokenizer.npz")
COPIES = ("dperturb",)


def load_reference():
    from oracle import ref_loader
    return ref_loader._load_file("_ref_d2s_graph", os.path.join("Data2Seq", "Graph.py"))


class _TorchWithStoredRand:
    """the torch module as Graph.py sees it, `rand` answering with the stored draw"""

    def __init__(self, stored):
        self._stored = stored

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand(self, *size, device=None, dtype=torch.float32):
        assert tuple(size) == tuple(self._stored.shape), (size, self._stored.shape)
        return self._stored.to(dtype)


def run(ref, name: str, dtype):
    c, b, dr = gc.CASES[name], gc.batch(name), gc.draws(name)
    tok = ref.GraphFeatureTokenizer(**c["cfg"])
    sd = gc.params(name, [(k, tuple(v.shape)) for k, v in tok.state_dict().items()])
    tok.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    tok = tok.to(dtype).eval()
    seen = {}
    for kind in ("rand", "orf", "lap"):
        enc = getattr(tok, kind + "_encoder", None)
        if enc is not None:
            enc.register_forward_pre_hook(lambda m, inp, kind=kind: seen.__setitem__(kind, inp[0].detach().clone()))
    bd = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in b.items() if k not in ("perturb", "dout")}
    bd["lap_eigvec"] = bd["lap_eigvec"].to(dtype)
    perturb = None if b["perturb"] is None else torch.from_numpy(b["perturb"]).to(dtype).requires_grad_()
    keep = ref.torch, ref.gaussian_orthogonal_random_matrix_batched
    ref.torch = _TorchWithStoredRand(torch.from_numpy(dr["rand"]))
    ref.gaussian_orthogonal_random_matrix_batched = lambda nb, r, cc, device=None, dtype=torch.float32: torch.from_numpy(dr["orf"]).to(dtype)
    try:
        out, mask, idx = tok(bd, perturb)
    finally:
        ref.torch, ref.gaussian_orthogonal_random_matrix_batched = keep
    out.backward(torch.from_numpy(b["dout"]).to(dtype))
    res = {"out": out.detach()}
    res.update({"dparam/" + k: p.grad for k, p in tok.named_parameters()})
    if perturb is not None:
        res["dperturb"] = perturb.grad
    bs, ts = gc.node_rows(name)
    ids = {kind: t[bs, ts, :t.shape[-1] // 2] for kind, t in seen.items()}
    return res, idx, mask, ids


def put(out: dict, key: str, t64: torch.Tensor, t32: torch.Tensor):
    a64, a32 = t64.detach().double().numpy().reshape(-1), t32.detach().double().numpy().reshape(-1)
    mx = float(np.abs(a64).max())
    am = int(np.abs(a64).argmax())
    out[key] = a64[np.append(gc.subset_index(a64.size), am)]
    out[key + "/argmax"] = np.int64(am)
    out[key + "/ref_err"] = np.float64(np.abs(a32 - a64).max() / max(mx, 1e-30))


def check_cases():
    """the properties the fixture's cases must have (the issue's list), asserted on the synthesised inputs"""
    r, a, s, p = (gc.CASES[k] for k in ("recipe", "all_ids", "single", "pile"))
    assert r["cfg"]["num_atoms"] == 512 * 9 and r["cfg"]["num_edges"] == 512 * 3 and r["Fn"] == 9 and r["Fe"] == 3
    assert r["cfg"]["lap_node_id_k"] == 16 and r["cfg"]["type_id"] and r["cfg"]["hidden_dim"] == 768
    assert a["cfg"]["rand_node_id"] and a["cfg"]["orf_node_id"] and a["cfg"]["lap_node_id"]
    assert a["cfg"]["orf_node_id_dim"] < max(a["node_num"]) and s["cfg"]["orf_node_id_dim"] > max(s["node_num"])
    assert a["cfg"]["lap_node_id_k"] < a["lap"] and s["cfg"]["lap_node_id_k"] > s["lap"]
    assert 0 in a["edge_num"] and len(s["node_num"]) == 1 and a["perturb"]
    for name, c in gc.CASES.items():
        b = gc.batch(name)
        T = max(n + e for n, e in zip(c["node_num"], c["edge_num"]))
        assert b["dout"].shape[1] == T + 2 and any(n + e == T for n, e in zip(c["node_num"], c["edge_num"]))
        ei = b["edge_index"]
        at = 0
        for n, e in zip(c["node_num"], c["edge_num"]):
            assert e == 0 or (ei[:, at:at + e].min() >= 0 and ei[:, at:at + e].max() < n), name
            at += e
    b = gc.batch("recipe")
    ei = b["edge_index"]
    assert (ei[0] == ei[1]).any() and (ei[0] != ei[1]).any(), "self-loops and ordinary edges"
    assert (ei[:, 1] == ei[:, 2]).all(), "a duplicate edge"
    assert (b["node_data"] == 0).any() and (b["edge_data"] == 0).any(), "feature value 0"
    pb = gc.batch("pile")
    assert (pb["node_data"] == p["pile"][0]).all() and (pb["edge_data"] == p["pile"][1]).all() and pb["node_data"].size > 1024


def generate() -> dict:
    ref = load_reference()
    check_cases()
    out = {}
    for name, c in gc.CASES.items():
        (r64, i64, m64, _), (r32, i32, m32, ids) = run(ref, name, torch.float64), run(ref, name, torch.float32)
        assert torch.equal(i64, i32) and torch.equal(m64, m32)
        out[f"{name}/padded_index"], out[f"{name}/padding_mask"] = i32.numpy(), m32.numpy()
        for k in r64:
            put(out, f"{name}/{k}", r64[k], r32[k])
            copy = k in COPIES or (len(c["node_num"]) == 1 and k in ("dparam/graph_token.weight", "dparam/null_token.weight"))
            assert copy or out[f"{name}/{k}/ref_err"] > 0, (name, k)
        for kind, t in ids.items():
            if kind != "lap":
                out[f"{name}/ids/{kind}"] = t.float().numpy()
        print(f"  {name}: ref_err " + " ".join(f"{k.split('/')[-1]} {out[f'{name}/{k}/ref_err']:.1e}" for k in r64))
    for tag, cfg in (("recipe", gc.RECIPE), ("default", dict(rand_node_id_dim=768, orf_node_id_dim=768))):
        tok = ref.GraphFeatureTokenizer(**cfg)
        out[f"keys/{tag}/config"] = json.dumps(cfg)
        out[f"keys/{tag}/keys"] = json.dumps([[k, list(v.shape)] for k, v in tok.state_dict().items()])
    torch.manual_seed(0)
    tok = ref.GraphFeatureTokenizer(**gc.SMALL)
    out["init/config"] = json.dumps(dict(gc.SMALL, seed=0))
    for k, v in tok.state_dict().items():
        out["init/" + k] = v.numpy()
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
