"""CPU: the Time-Series decoder's boundary -- key and shape lists against the fixture the reference's own classes wrote
(tests/golden/ts_decoder.npz), constructor defaults, the new entry points in the ctypes table, the case
coverage, and the host restatement of the attention dropout mask."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import stoch_cases as sc
import ts_decoder_cases as tc
import metatransformer_amd as M
from metatransformer_amd import _capi, timeseries as ts
from oracle import ref_loader


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ts_decoder.npz"), allow_pickle=False)


def shapes(module):
    return [[k, list(v.shape)] for k, v in module.state_dict().items()]


def make_decoder(d, H, ff, nl, co, dropout=0.1):
    return M.Decoder([M.DecoderLayer(M.AttentionLayer(M.FullAttention(True, 1, attention_dropout=dropout, output_attention=False), d, H),
                                     M.AttentionLayer(M.FullAttention(False, 1, attention_dropout=dropout, output_attention=False), d, H),
                                     d, ff, dropout=dropout, activation="gelu") for _ in range(nl)],
                     norm_layer=torch.nn.LayerNorm(d), projection=torch.nn.Linear(d, co, bias=True))


def test_key_and_shape_lists_equal_the_fixture(golden):
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES["recipe"]
    assert shapes(make_decoder(d, H, ff, nl, co)) == json.loads(str(golden["keys/decoder"]))
    assert shapes(make_decoder(d, H, ff, nl, co)) == [[k, list(s)] for k, s in tc.decoder_keys(d, H, ff, nl, co)]
    assert shapes(M.DataEmbedding(7, d, "timeF", "h", 0.1)) == json.loads(str(golden["keys/embed_timeF"]))
    fc = json.loads(str(golden["keys/forecaster"]))
    cfg = fc["config"]
    f = M.Forecaster(cfg["enc_in"], cfg["dec_in"], cfg["c_out"], 96, d_model=cfg["d_model"], n_heads=cfg["n_heads"], d_ff=cfg["d_ff"],
                     d_layers=cfg["d_layers"], embed=cfg["embed"], freq=cfg["freq"], depth=cfg["depth"], num_heads=cfg["num_heads"])
    assert shapes(f) == fc["keys"]
    assert [n for n, _ in f.named_children()] == ["enc_embedding", "encoder", "dec_embedding", "decoder"]
    assert all(not p.requires_grad for p in f.encoder.parameters())
    assert all(p.requires_grad for n, p in f.named_parameters() if n.startswith(("decoder.", "dec_embedding.value", "enc_embedding.value")))
    for freq, d_inp in tc.D_INP.items():
        assert tuple(M.DataEmbedding(3, 16, "timeF", freq).temporal_embedding.embed.weight.shape) == (16, d_inp)


def defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}


def test_constructor_defaults_are_the_references():
    assert defaults(M.FullAttention.__init__) == dict(mask_flag=True, factor=5, scale=None, attention_dropout=0.1, output_attention=False)
    assert defaults(M.AttentionLayer.__init__) == dict(d_keys=None, d_values=None)
    assert list(inspect.signature(M.AttentionLayer.__init__).parameters)[1:] == ["attention", "d_model", "n_heads", "d_keys", "d_values"]
    assert defaults(M.DecoderLayer.__init__) == dict(d_ff=None, dropout=0.1, activation="relu")
    assert list(inspect.signature(M.DecoderLayer.__init__).parameters)[1:4] == ["self_attention", "cross_attention", "d_model"]
    assert defaults(M.Decoder.__init__) == dict(norm_layer=None, projection=None)
    assert defaults(M.Forecaster.__init__) == dict(d_model=768, n_heads=8, d_ff=2048, d_layers=1, embed="timeF", freq="h", dropout=0.1,
                                                   activation="gelu", depth=12, num_heads=12)
    with pytest.raises(M.MetaEncError, match="relu"):
        M.DecoderLayer(None, None, 64)
    with pytest.raises(M.MetaEncError, match="relu"):
        M.DecoderLayer(None, None, 64, activation="relu")
    lay = M.DecoderLayer(None, None, 64, activation="gelu")
    assert lay.conv1.weight.shape == (256, 64, 1) and lay.dropout.p == 0.1            # d_ff defaults to 4 * d_model
    with pytest.raises(M.MetaEncError):
        M.DataEmbedding(7, 64, "learned")
    sites = [ts.SEED_SELF_ATTN_DROP, ts.SEED_SELF_BRANCH, ts.SEED_CROSS_ATTN_DROP, ts.SEED_CROSS_BRANCH, ts.SEED_MLP_HIDDEN, ts.SEED_MLP_BRANCH]
    assert len(set(sites)) == 6 and 0 < min(sites) and max(sites) < ts.SEED_LAYER_STRIDE


def test_entry_points_are_in_the_signature_table():
    for name in ("me_attention_qkv_fwd", "me_attention_qkv_bwd"):
        res, args = _capi.SIGNATURES[name]
        assert res is ctypes.c_int and args == [ctypes.POINTER(_capi.AttnQkvDesc), ctypes.c_void_p]
    assert len(_capi.AttnQkvDesc._fields_) == 28
    from metatransformer_amd import ops
    assert callable(ops.attention_qkv_fwd) and callable(ops.attention_qkv_bwd)


def test_case_coverage():
    tc.assert_coverage()
    for dt in (torch.float32, torch.bfloat16):
        cases = tc.qkv_cases(dt)
        assert {(a, b) for a, b, c, _, _ in cases if not c} == set(tc.QKV_NONCAUSAL) and {a for a, _, c, _, _ in cases if c} == set(tc.QKV_CAUSAL)
        assert {hd for *_, hd, _ in cases} == set(tc.QKV_HEAD_DIMS[dt]) and {lay for *_, lay in cases} == set(tc.QKV_LAYOUTS)
        for causal in (False, True):      # every head_dim in every layout, for both variants
            assert {(hd, lay) for _, _, c, hd, lay in cases if c == causal} >= {(hd, lay) for hd in tc.QKV_HEAD_DIMS[dt] for lay in tc.QKV_LAYOUTS}
    want = {(2, 144, 96, 768, 8, 2048, 1, 7), (2, 33, 65, 192, 2, 256, 2, 7), (1, 1, 1, 96, 1, 128, 1, 3), (2, 70, 17, 64, 2, 128, 1, 5)}
    assert set(tc.DECODER_CASES.values()) >= want
    assert 768 // 8 == 96 and 96 in tc.QKV_HEAD_DIMS[torch.float32]                      # the recipe's head width


def test_attention_mask_restatement_equals_attn_keep_when_nq_equals_nk():
    for seed, B, H, N, p in ((5, 2, 3, 17, 0.1), (-7, 1, 2, 65, 0.25), (0x5DEECE66D, 2, 3, 33, 0.1)):
        assert np.array_equal(tc.qkv_keep(seed, B, H, N, N, p), sc.attn_keep(seed, B, H, N, p))
    k = tc.qkv_keep(3, 2, 3, 33, 65, 0.1)
    assert k.shape == (2, 3, 33, 65) and 0.85 < k.mean() < 0.95
    flat = sc.u01(3, np.arange(2 * 3 * 33 * 65, dtype=np.uint64)) >= np.float32(0.1)
    assert np.array_equal(k.reshape(-1), flat) and k[1, 2, 32, 64] == flat[-1]


def test_fixture_holds_every_case(golden):
    for name, (B, L, S, d, H, ff, nl, co) in tc.DECODER_CASES.items():
        for t in ["out", "dx", "dcross"] + ["dparam/" + k for k, _ in tc.decoder_keys(d, H, ff, nl, co)]:
            key = f"decoder/{name}/{t}"
            assert key in golden.files and key + "/argmax" in golden.files and float(golden[key + "/ref_err"]) >= 0, key
    for name, (B, L, c_in, d, freq) in tc.EMBED_CASES.items():
        for t in ["out"] + ["dparam/" + k for k, _ in tc.embed_keys(c_in, d, freq)]:
            assert f"embed/{name}/{t}" in golden.files
    assert os.path.getsize(os.path.join(GOLDEN, "ts_decoder.npz")) < 1_000_000


def test_decoder_torch_restatement_reproduces_the_fixture(golden):
    """the plain-torch restatement (the bf16 yardstick and the exact-mask reference of the GPU tests) is the reference's function: in
    float64 it reproduces the stored output and gradients to rounding"""
    name = "two_layers"
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES[name]
    sd = {k: torch.from_numpy(v).double().requires_grad_() for k, v in tc.synth_params(name, tc.decoder_keys(d, H, ff, nl, co)).items()}
    x, cross, dout = (torch.from_numpy(a).double() for a in tc.decoder_inputs(name))
    x.requires_grad_()
    cross.requires_grad_()
    tc.decoder_torch(x, cross, sd, H, nl).backward(dout)
    got = {"dx": x.grad, "dcross": cross.grad}
    got.update({"dparam/" + k: v.grad for k, v in sd.items()})
    for t, g in got.items():
        want = golden[f"decoder/{name}/{t}"]
        have = tc.picked(g, int(golden[f"decoder/{name}/{t}/argmax"]))
        scale = max(float(np.abs(want).max()), 1e-12) if "key_projection.bias" not in t else 1.0
        assert float(np.abs(have - want).max()) <= 1e-11 * scale, t


def test_generator_check_passes():
    if not ref_loader.reference_available():
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_ts_decoder_golden.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
