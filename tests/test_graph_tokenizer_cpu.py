"""CPU: the host side of the graph tokenizer -- constructor / state-dict / initialisation parity with the reference
(tests/golden/graph_tokenizer.npz, tools/make_graph_golden.py), argument errors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import metatransformer_amd as M
import graph_cases as gc


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "graph_tokenizer.npz"), allow_pickle=False)


def _build(tag, cfg):
    return M.Data2Seq("graph", 768).embed if tag == "default" else M.GraphFeatureTokenizer(**cfg)


@pytest.mark.parametrize("tag", ["recipe", "default"])
def test_state_dict_matches_the_reference(gold, tag):
    cfg = json.loads(str(gold[f"keys/{tag}/config"]))
    want = [(k, tuple(s)) for k, s in json.loads(str(gold[f"keys/{tag}/keys"]))]
    tok = _build(tag, cfg)
    assert [(k, tuple(v.shape)) for k, v in tok.state_dict().items()] == want
    tok.load_state_dict({k: torch.zeros(s) for k, s in want}, strict=True)      # a checkpoint with exactly the reference's keys


def test_constructor_signature_is_the_reference_one():
    import inspect
    names = list(inspect.signature(M.GraphFeatureTokenizer.__init__).parameters)[1:]
    assert names == ["num_atoms", "num_edges", "rand_node_id", "rand_node_id_dim", "orf_node_id", "orf_node_id_dim", "lap_node_id",
                     "lap_node_id_k", "lap_node_id_sign_flip", "lap_node_id_eig_dropout", "type_id", "hidden_dim", "n_layers"]
    d = M.GraphFeatureTokenizer()
    assert d.rand_encoder.weight.shape == (1, 1536) and d.lap_encoder.weight.shape == (1, 2) and d.lap_eig_dropout.p == 1
    assert "orf_encoder.weight" not in M.GraphFeatureTokenizer(orf_node_id=0).state_dict()
    assert M.GraphFeatureTokenizer(lap_node_id_eig_dropout=0).lap_eig_dropout is None


def test_seeded_construction_equals_the_reference(gold):
    c = json.loads(str(gold["init/config"]))
    torch.manual_seed(c.pop("seed"))
    sd = M.GraphFeatureTokenizer(**c).state_dict()
    keys = [k[len("init/"):] for k in gold.files if k.startswith("init/") and k != "init/config"]
    assert sorted(keys) == sorted(sd)
    for k in keys:
        assert sd[k].dtype == torch.float32 and np.array_equal(sd[k].numpy(), gold["init/" + k]), k
    assert float(np.abs(gold["init/atom_encoder.weight"][0]).max()) > 0          # row 0 is overwritten with noise, as in the reference


def test_data2seq_dispatch():
    tok = M.Data2Seq("graph", 768)
    assert isinstance(tok.embed, M.GraphFeatureTokenizer)
    assert tok.embed.rand_node_id_dim == 768 and tok.embed.orf_node_id_dim == 768
    with pytest.raises(M.MetaEncError, match=r"text.*in scope: image, audio, video, time-series, graph"):
        M.Data2Seq("text", 768)


def _fake_cuda(t):
    """stands for a CUDA tensor in the host-side checks (which read is_cuda, dtype, device and shape only)"""
    class T(torch.Tensor):
        @property
        def is_cuda(self):
            return True
    return t.as_subclass(T)


def _batch(name="all_ids", cuda=True):
    b = gc.batch(name)
    wrap = _fake_cuda if cuda else (lambda t: t)
    bd = {k: wrap(torch.from_numpy(v)) if isinstance(v, np.ndarray) else v for k, v in b.items() if k not in ("perturb", "dout")}
    return bd, gc.CASES[name]


def test_cpu_tensors_raise():
    bd, c = _batch(cuda=False)
    tok = M.GraphFeatureTokenizer(**c["cfg"])
    with pytest.raises(M.MetaEncError, match=r"node_data.*CUDA.*no CPU fallback"):
        tok(bd)
    bd2, _ = _batch()
    bd2["lap_eigvec"] = bd["lap_eigvec"]
    with pytest.raises(M.MetaEncError, match=r"lap_eigvec.*CUDA.*no CPU fallback"):
        tok(bd2)
    with pytest.raises(M.MetaEncError, match=r"perturb.*CUDA.*no CPU fallback"):
        tok(_batch()[0], torch.zeros(4, 11, 64))


def test_bad_arguments_name_the_argument():
    bd, c = _batch()
    tok = M.GraphFeatureTokenizer(**c["cfg"])

    def bad(match, perturb=None, node_ids=None, **change):
        d = dict(bd, **change)
        with pytest.raises(M.MetaEncError, match=match):
            tok(d, perturb, node_ids=node_ids)
    bad(r"node_data must be int64", node_data=_fake_cuda(bd["node_data"].int()))
    bad(r"edge_index must be int64", edge_index=_fake_cuda(bd["edge_index"].float()))
    bad(r"edge_data must be int64", edge_data=_fake_cuda(bd["edge_data"].short()))
    bad(r"lap_eigvec must be a floating-point", lap_eigvec=_fake_cuda(bd["lap_eigvec"].long()))
    bad(r"node_data \(28, 3\).*sum\(node_num\) = 29", node_num=[7, 11, 4, 7])
    bad(r"edge_index \(2, 37\).*sum\(edge_num\) = 38", edge_num=[10, 14, 1, 13])
    bad(r"edge_data \(36, 2\).*sum\(edge_num\) = 37", edge_data=_fake_cuda(bd["edge_data"][:-1]))
    bad(r"lap_eigvec \(27, 6\).*one row per node \(28\)", lap_eigvec=_fake_cuda(bd["lap_eigvec"][:-1]))
    bad(r"node_num / edge_num", edge_num=[10, 14, 0])
    bad(r"perturb \(4, 10, 64\).*\(4, 11, 64\)", perturb=_fake_cuda(torch.zeros(4, 10, 64)))
    bad(r"node_ids\['rand'\].*\[28, 16\]", node_ids={"rand": _fake_cuda(torch.zeros(28, 8))})
    bad(r"node_ids has unknown kinds \['lap'\]", node_ids={"lap": _fake_cuda(torch.zeros(28, 4))})
    d = dict(bd)
    del d["edge_num"]
    with pytest.raises(M.MetaEncError, match="edge_num"):
        tok(d)


def test_cases_have_the_properties_the_fixture_needs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_graph_golden as mg
    mg.check_cases()


def test_fixture_is_what_the_reference_gives():
    from oracle import ref_loader
    if not os.path.isfile(os.path.join(ref_loader.REF_ROOT, "Data2Seq", "Graph.py")):
        pytest.skip("reference tree not present")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_graph_golden.py"), "--check"], check=True, cwd=ROOT)
