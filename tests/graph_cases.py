"""Inputs and parameters of the graph tokenizer fixture (tests/golden/graph_tokenizer.npz), synthesised rather than stored:
tools/make_graph_golden.py (which runs the reference's GraphFeatureTokenizer on them) and the tests build the same arrays from
the counter hash of msda_cases.py, so nothing depends on a library's random stream.  Parameters, output gradients and
eigenvectors carry full float32 mantissas (a 24-bit grid times a non-dyadic scale), so that sums of them round and the
reference's float32-vs-float64 distance is not zero.
"""
from __future__ import annotations

import numpy as np

from msda_cases import seed_of, subset_index, uniform  # noqa: F401  (subset_index: re-exported for the generator and the tests)

RECIPE = dict(num_atoms=512 * 9, num_edges=512 * 3, rand_node_id=False, rand_node_id_dim=64, orf_node_id=False, orf_node_id_dim=64,
              lap_node_id=True, lap_node_id_k=16, lap_node_id_sign_flip=True, lap_node_id_eig_dropout=0.2, type_id=True,
              hidden_dim=768, n_layers=12)
SMALL = dict(num_atoms=40, num_edges=12, rand_node_id=True, rand_node_id_dim=16, orf_node_id=True, orf_node_id_dim=8,
             lap_node_id=True, lap_node_id_k=4, lap_node_id_sign_flip=True, lap_node_id_eig_dropout=0.2, type_id=True,
             hidden_dim=64, n_layers=12)

# cfg: constructor arguments; node_num / edge_num; Fn / Fe feature columns; lap: width of lap_eigvec; perturb; pile: every entry of
# node_data (edge_data) holds one value
CASES = {
    # the PCQM4Mv2 recipe (Graph/scripts/pcqv2-metatransformer_fixed.sh + type id), eval mode; graph 4 fills T exactly
    "recipe": dict(cfg=RECIPE, node_num=[12, 9, 17, 5, 20, 14], edge_num=[24, 16, 36, 8, 44, 28], Fn=9, Fe=3, lap=16, perturb=False),
    # all three identifier kinds; orf width 8 < max_n = 11, lap k = 4 < eigenvector width 6; a graph without edges; perturb
    "all_ids": dict(cfg=SMALL, node_num=[7, 11, 4, 6], edge_num=[10, 14, 0, 13], Fn=3, Fe=2, lap=6, perturb=True),
    # B = 1; orf width 24 > max_n = 9, lap k = 8 > eigenvector width 5; no type id, no rand identifiers
    "single": dict(cfg=dict(SMALL, rand_node_id=False, orf_node_id_dim=24, lap_node_id_k=8, type_id=False, hidden_dim=128),
                   node_num=[9], edge_num=[15], Fn=3, Fe=2, lap=5, perturb=False),
    # pile-up: every node shares one atom value in all 9 columns (1440 entries on one table row), every edge one edge value
    "pile": dict(cfg=dict(RECIPE, hidden_dim=128), node_num=[20] * 8, edge_num=[40] * 8, Fn=9, Fe=3, lap=16, perturb=False,
                 pile=(7, 3)),
}
SELF_LOOPS = (0, 5)      # local edge numbers made self-loops (u == v) in every graph that has them
DUPLICATE = (2, 1)       # local edge 2 repeats edge 1


def _ints(shape, seed, hi):
    return np.minimum((uniform(shape, seed, 0.0, 1.0, bits=24).astype(np.float64) * hi).astype(np.int64), hi - 1)


def full(shape, seed, scale):
    """float32 values with full mantissas in (-scale, scale)"""
    return (uniform(shape, seed, -1.0, 1.0, bits=24) * np.float32(scale * 0.973)).astype(np.float32)


def batch(name: str) -> dict:
    """the collator's dict as numpy arrays (node_num / edge_num lists), plus perturb [B, max_n, C] or None and dout [B, 2+T, C]"""
    c = CASES[name]
    cfg, nn_, en = c["cfg"], c["node_num"], c["edge_num"]
    Sn, Se, C = sum(nn_), sum(en), cfg["hidden_dim"]
    node_data = _ints((Sn, c["Fn"]), seed_of("graph", name, "node_data"), cfg["num_atoms"])
    edge_data = _ints((Se, c["Fe"]), seed_of("graph", name, "edge_data"), cfg["num_edges"])
    node_data[1::5, 0] = 0                        # the padding row is read like any other
    edge_data[2::7, -1] = 0
    if c.get("pile"):
        node_data[:], edge_data[:] = c["pile"]
    h = uniform((2, Se), seed_of("graph", name, "edge_index"), 0.0, 1.0, bits=24).astype(np.float64)
    edge_index = np.zeros((2, Se), dtype=np.int64)
    at = 0
    for n, e in zip(nn_, en):
        ei = np.minimum((h[:, at:at + e] * n).astype(np.int64), n - 1)
        for k in SELF_LOOPS:
            if k < e:
                ei[1, k] = ei[0, k]
        if e > max(DUPLICATE):
            ei[:, DUPLICATE[0]] = ei[:, DUPLICATE[1]]
        edge_index[:, at:at + e] = ei
        at += e
    T = max(n + e for n, e in zip(nn_, en))
    out = dict(node_data=node_data, edge_data=edge_data, edge_index=edge_index, node_num=list(nn_), edge_num=list(en),
               lap_eigvec=full((Sn, c["lap"]), seed_of("graph", name, "lap_eigvec"), 0.5),
               lap_eigval=np.zeros((Sn, c["lap"]), dtype=np.float32), in_degree=np.zeros(Sn, dtype=np.int64),
               out_degree=np.zeros(Sn, dtype=np.int64),
               perturb=full((len(nn_), max(nn_), C), seed_of("graph", name, "perturb"), 0.01) if c["perturb"] else None,
               dout=full((len(nn_), T + 2, C), seed_of("graph", name, "dout"), 1.0))
    return out


def draws(name: str) -> dict:
    """stand-ins of the reference's two random sources: the uniform draw behind the rand identifiers [Sn, D] and the batched
    orthogonal matrices [B, max_n, max_n] (rows of unit norm: the Q factor of a hashed matrix, in float64, rounded to float32)"""
    c = CASES[name]
    Sn, B, max_n = sum(c["node_num"]), len(c["node_num"]), max(c["node_num"])
    rand = uniform((Sn, c["cfg"]["rand_node_id_dim"]), seed_of("graph", name, "rand"), 0.0, 1.0, bits=24)
    g = uniform((B, max_n, max_n), seed_of("graph", name, "orf"), -1.0, 1.0, bits=24).astype(np.float64)
    q = np.stack([np.linalg.qr(m)[0].T for m in g])
    return dict(rand=rand, orf=q.astype(np.float32))


def params(name_or_cfg, keys_shapes) -> dict:
    """parameters for a [(key, shape)] list: tables and token rows of scale 0.02 (the reference's init), Linears fan-in scaled"""
    tag = name_or_cfg
    out = {}
    for key, shape in keys_shapes:
        shape = tuple(shape)
        scale = 0.02 if "encoder.weight" not in key or key.startswith(("atom", "edge", "order")) else 1.0 / np.sqrt(shape[1])
        out[key] = full(shape, seed_of("graph", tag, key), scale)
    return out


def node_rows(name: str):
    """(b, t) of every node token, in node order: where the recorded [B, T, 2D] encoder inputs hold the [Sn, D] identifiers"""
    bs, ts = [], []
    for b, n in enumerate(CASES[name]["node_num"]):
        bs.extend([b] * n)
        ts.extend(range(n))
    return np.array(bs), np.array(ts)
