"""GPU: the Time-Series decoder (metatransformer_amd/timeseries.py) and DataEmbedding(embed_type='timeF') against the fixture the
reference's own classes wrote (tests/golden/ts_decoder.npz: float64 values at subset positions + the reference's float32-vs-float64
distance ref_err), the bf16 path against a plain-torch restatement under autocast on the same GPU, training mode against float64 with
the exact masks, and the Forecaster against the composition of its parts.

Error of a tensor: max |got - want| over the stored positions / scale, scale = max |want| -- except the two kinds the issue names,
which are zero in exact arithmetic and so have no scale of their own:
  * `*.key_projection.bias` gradients (softmax is shift-invariant per row): scale = max |d query_projection.bias| of the same layer;
  * with L = S = 1, the query and key projection gradients: scale = max |d value_projection.weight| of the same layer.
Every comparison prints a `TS_PARITY` line with err, ref_err and their ratio."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TOL_F32, check_close

import stoch_cases as sc
import ts_decoder_cases as tc
import metatransformer_amd as M
from metatransformer_amd import data2seq, timeseries as ts

pytestmark = pytest.mark.gpu

OFFSETS = dict(stride=ts.SEED_LAYER_STRIDE, self_attn=ts.SEED_SELF_ATTN_DROP, self_branch=ts.SEED_SELF_BRANCH, cross_attn=ts.SEED_CROSS_ATTN_DROP,
               cross_branch=ts.SEED_CROSS_BRANCH, mlp_hidden=ts.SEED_MLP_HIDDEN, mlp_branch=ts.SEED_MLP_BRANCH)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ts_decoder.npz"), allow_pickle=False)


def make_decoder(d, H, ff, nl, co, dropout=0.1, final=True):
    return M.Decoder([M.DecoderLayer(M.AttentionLayer(M.FullAttention(True, 1, attention_dropout=dropout, output_attention=False), d, H),
                                     M.AttentionLayer(M.FullAttention(False, 1, attention_dropout=dropout, output_attention=False), d, H),
                                     d, ff, dropout=dropout, activation="gelu") for _ in range(nl)],
                     norm_layer=torch.nn.LayerNorm(d) if final else None, projection=torch.nn.Linear(d, co, bias=True) if final else None)


def zero_scale_key(t: str, one_token: bool):
    """the tensor whose scale bounds t, for the tensors that are zero in exact arithmetic; None for an ordinary tensor"""
    if one_token and ("query_projection" in t or "key_projection" in t):      # (the query bias gradient is zero too: no scale for the key bias there)
        return t.rsplit(".", 2)[0] + ".value_projection.weight"
    if t.endswith("key_projection.bias"):
        return t.replace("key_projection.bias", "query_projection.bias")
    return None


def tensor_errors(golden, group: str, got: dict, one_token: bool = False) -> dict:
    """{t: (err, ref_err, got at the stored positions, want, scale)}"""
    res = {}
    for t, g in got.items():
        want = golden[f"{group}/{t}"]
        have = tc.picked(g, int(golden[f"{group}/{t}/argmax"]))
        zk = zero_scale_key(t, one_token)
        scale = float(np.abs(golden[f"{group}/{zk}"]).max()) if zk else float(np.abs(want).max())
        res[t] = (float(np.abs(have - want).max()) / max(scale, 1e-30), float(golden[f"{group}/{t}/ref_err"]), have, want, scale, zk is not None)
    return res


def run_product_decoder(dev, name, autocast=False):
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES[name]
    m = make_decoder(d, H, ff, nl, co)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in tc.synth_params(name, tc.decoder_keys(d, H, ff, nl, co)).items()}, strict=True)
    m = m.to(dev).eval()
    x, cross, dout = (torch.from_numpy(a).to(dev) for a in tc.decoder_inputs(name))
    x.requires_grad_()
    cross.requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = m(x, cross)
    assert y.shape == (B, L, co) and y.dtype == torch.float32
    y.backward(dout)
    got = {"out": y.detach(), "dx": x.grad, "dcross": cross.grad}
    got.update({"dparam/" + k: p.grad for k, p in m.named_parameters()})
    assert all(g is not None for g in got.values())
    return got


def run_torch_decoder(dev, name, autocast):
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES[name]
    sd = {k: torch.from_numpy(v).to(dev).requires_grad_() for k, v in tc.synth_params(name, tc.decoder_keys(d, H, ff, nl, co)).items()}
    x, cross, dout = (torch.from_numpy(a).to(dev) for a in tc.decoder_inputs(name))
    x.requires_grad_()
    cross.requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = tc.decoder_torch(x, cross, sd, H, nl)
    y.float().backward(dout)
    got = {"out": y.detach().float(), "dx": x.grad, "dcross": cross.grad}
    got.update({"dparam/" + k: v.grad for k, v in sd.items()})
    return got


@pytest.mark.parametrize("name", list(tc.DECODER_CASES))
def test_decoder_fp32_parity(dev, golden, name):
    """output and every gradient within TOL_F32 of the reference's float64 (per element on the stored positions for ordinary tensors)"""
    errs = tensor_errors(golden, f"decoder/{name}", run_product_decoder(dev, name), one_token=name == "one_token")
    fails = []
    for t, (err, ref_err, have, want, scale, zero) in errs.items():
        print(f"TS_PARITY fp32 decoder/{name}/{t} err {err:.3e} ref_err {ref_err:.3e} ratio {err / max(ref_err, 1e-30):.2f}"
              + (" (zero in exact arithmetic: absolute, against the layer's scale)" if zero else ""))
        if err > TOL_F32:
            fails.append((t, err))
        elif not zero:
            check_close(torch.from_numpy(have), torch.from_numpy(want), TOL_F32, f"decoder/{name}/{t}")
    assert not fails, fails


@pytest.mark.parametrize("name", list(tc.EMBED_CASES))
def test_timef_embedding_fp32_parity(dev, golden, name):
    B, L, c_in, d, freq = tc.EMBED_CASES[name]
    m = M.DataEmbedding(c_in, d, "timeF", freq, 0.1)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in tc.synth_params(name, tc.embed_keys(c_in, d, freq)).items()})
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    x, mark, dout = (torch.from_numpy(a).to(dev) for a in tc.embed_inputs(name))
    y = m(x, mark)
    y.backward(dout)
    got = {"out": y.detach()}
    got.update({"dparam/" + k: p.grad for k, p in m.named_parameters() if p.requires_grad})
    for t, (err, ref_err, have, want, scale, _) in tensor_errors(golden, f"embed/{name}", got).items():
        print(f"TS_PARITY fp32 embed/{name}/{t} err {err:.3e} ref_err {ref_err:.3e} ratio {err / max(ref_err, 1e-30):.2f}")
        check_close(torch.from_numpy(have), torch.from_numpy(want), TOL_F32, f"embed/{name}/{t}")
    # without marks: value + positional only, and eval mode is deterministic
    assert torch.equal(m(x, mark), y.detach()) and not torch.equal(m(x, None), y.detach())


@pytest.mark.parametrize("name", list(tc.DECODER_CASES))
def test_decoder_bf16_autocast_within_3x_of_torch_autocast(dev, golden, name):
    """The yardstick is measured, not fixed in advance: the plain-torch restatement of the decoder (ts_decoder_cases.decoder_torch) under
    bf16 autocast on the same GPU against the float64 fixture.  The product must be within 3x that distance per tensor (the "about 3x
    measured" rule of tests/conftest.py).  Measured on an MI355X (profiles/ts_decoder_parity.txt, the TS_PARITY bf16 lines), output of
    recipe / two_layers / one_token / short_cross: product 3.1e-3 / 3.5e-3 / 7.3e-3 / 4.2e-3, torch autocast 4.9e-3 / 4.3e-3 / 7.0e-3 /
    4.6e-3; over every tensor the product's largest distance is 1.1e-2, torch's 1.2e-2, the largest ratio 2.2 (a key-bias gradient)."""
    one = name == "one_token"
    mine = tensor_errors(golden, f"decoder/{name}", run_product_decoder(dev, name, autocast=True), one_token=one)
    yard = tensor_errors(golden, f"decoder/{name}", run_torch_decoder(dev, name, autocast=True), one_token=one)
    fails = []
    for t in mine:
        err, yerr = mine[t][0], yard[t][0]
        print(f"TS_PARITY bf16 decoder/{name}/{t} err {err:.3e} torch_autocast_err {yerr:.3e} ratio {err / max(yerr, 1e-30):.2f}")
        if err > 3.0 * yerr:
            fails.append((t, err, yerr))
    assert not fails, fails


def test_training_mode_without_dropout_equals_eval(dev):
    name = "short_cross"
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES[name]
    m = make_decoder(d, H, ff, nl, co, dropout=0.0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in tc.synth_params(name, tc.decoder_keys(d, H, ff, nl, co)).items()}, strict=True)
    m = m.to(dev)
    x, cross, _ = (torch.from_numpy(a).to(dev) for a in tc.decoder_inputs(name))
    state = torch.random.get_rng_state()
    y_train = m.train()(x, cross)
    assert torch.equal(torch.random.get_rng_state(), state), "dropout = 0 draws no seed"
    assert torch.equal(y_train, m.eval()(x, cross))
    m2 = make_decoder(d, H, ff, nl, co, dropout=0.1).to(dev)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.eval()(x, cross), y_train) and torch.equal(m2.eval()(x, cross), y_train)
    assert not torch.equal(m2.train()(x, cross), y_train)


def test_decoder_layer_dropout_against_exact_masks(dev):
    """one DecoderLayer (L = 33, S = 17, d = 64) in train() with dropout 0.1 at every site -- the two attention-probability dropouts, the
    two attention branches, the hidden activation and the MLP branch -- against float64 with the masks restated on the host
    (the precedent of stoch_cases.block_forward_masked)"""
    B, L, S, d, H, ff, p = 2, 33, 17, 64, 2, 128, 0.1
    keys = [(k, s) for k, s in tc.decoder_keys(d, H, ff, 1, 5) if k.startswith("layers.")]
    params = tc.synth_params("dropout_layer", keys)
    m = make_decoder(d, H, ff, 1, 5, dropout=p, final=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.to(dev).train()
    u = lambda what, shape: torch.from_numpy(tc.mc.uniform(shape, tc.mc.seed_of("dropout_layer", what), -1.0, 1.0, bits=16) * np.float32(1.7))      # noqa: E731
    x, cross, dout = u("x", (B, L, d)), u("cross", (B, S, d)), u("dout", (B, L, d))
    seed = sc.block_seed(1234)                       # the first draw after torch.manual_seed(1234) ...
    torch.manual_seed(1234)                          # ... which Decoder.forward makes
    xd, cd = x.to(dev).requires_grad_(), cross.to(dev).requires_grad_()
    y = m(xd, cd)
    y.backward(dout.to(dev))
    sd = {k: torch.from_numpy(v).double().requires_grad_() for k, v in params.items()}
    xr, cr = x.double().requires_grad_(), cross.double().requires_grad_()
    ref = tc.decoder_torch(xr, cr, sd, H, 1, p=p, p_attn=p, seed=seed, offsets=OFFSETS, project=False)
    ref.backward(dout.double())
    check_close(y, ref.detach(), TOL_F32, "masked layer out")
    check_close(xd.grad, xr.grad, TOL_F32, "masked layer dx")
    check_close(cd.grad, cr.grad, TOL_F32, "masked layer dcross")
    grads = dict(m.named_parameters())
    for k, v in sd.items():
        g = grads[k].grad
        if k.endswith("key_projection.bias"):        # zero in exact arithmetic: against the query bias gradient's scale
            scale = float(sd[k.replace("key_projection", "query_projection")].grad.abs().max())
            assert float((g.double().cpu() - v.grad).abs().max()) <= TOL_F32 * scale, k
        else:
            check_close(g, v.grad, TOL_F32, "masked layer d " + k)
    torch.manual_seed(1234)
    assert torch.equal(m(xd, cd), y), "same seed, same masks"


def test_forecaster_composition_shape_and_gradients(dev):
    B, seq, label, pred, c = 2, 24, 12, 9, 7
    torch.manual_seed(0)
    f = M.Forecaster(c, c, c, pred, d_model=192, n_heads=2, d_ff=256, d_layers=1, embed="timeF", freq="h", dropout=0.1, depth=2, num_heads=3)
    f = f.to(dev).eval()
    u = lambda what, shape, s=1.0: torch.from_numpy(tc.mc.uniform(shape, tc.mc.seed_of("forecaster", what), -1.0, 1.0, bits=16) * np.float32(s)).to(dev)      # noqa: E731
    x_enc, m_enc, x_dec, m_dec = u("xe", (B, seq, c)), u("me", (B, seq, 4), 0.5), u("xd", (B, label + pred, c)), u("md", (B, label + pred, 4), 0.5)
    y = f(x_enc, m_enc, x_dec, m_dec)
    assert y.shape == (B, pred, c) and y.dtype == torch.float32
    manual = f.decoder(f.dec_embedding(x_dec, m_dec), f.encoder(f.enc_embedding(x_enc, m_enc)))[:, -pred:, :]
    assert torch.equal(y, manual)
    y.square().sum().backward()
    assert all(p.grad is None for p in f.encoder.parameters())
    for emb in (f.enc_embedding, f.dec_embedding):
        for p in (emb.value_embedding.tokenConv.weight, emb.temporal_embedding.embed.weight):
            assert p.grad is not None and float(p.grad.abs().max()) > 0 and bool(torch.isfinite(p.grad).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in f.decoder.parameters())


def test_fixed_embedding_keeps_its_code_path(dev):
    """embed='fixed': DataEmbedding's result is, bit for bit, the one fused kernel call it made before 'timeF' existed (_TSEmbedFn with the
    marks and tables), inside a Forecaster too"""
    B, L, c, d = 2, 24, 7, 192
    f = M.Forecaster(c, c, c, 8, d_model=d, n_heads=2, d_ff=256, embed="fixed", freq="h", depth=1, num_heads=3).to(dev).eval()
    emb = f.enc_embedding
    assert isinstance(emb.temporal_embedding, data2seq._Temporal) and emb.embed_type == "fixed"
    x = torch.from_numpy(tc.mc.uniform((B, L, c), 5, -1.0, 1.0, bits=16)).to(dev)
    marks = torch.stack([torch.arange(B * L) % 13, torch.arange(B * L) % 32, torch.arange(B * L) % 7, torch.arange(B * L) % 24], -1)
    marks = marks.reshape(B, L, 4).float().to(dev)
    tabs = [t.detach().float().contiguous() for t in emb.temporal_embedding.tables()]
    want = data2seq._TSEmbedFn.apply(x, emb.value_embedding.tokenConv.weight, marks.long().to(torch.int32).contiguous(), tabs,
                                     emb.position_embedding.pe[0].contiguous(), torch.float32, 0.0, 0)
    assert torch.equal(emb(x, marks), want)
    alone = M.DataEmbedding(c, d).to(dev).eval()
    alone.load_state_dict(emb.state_dict())
    assert torch.equal(alone(x, marks), want) and json.dumps(list(alone.state_dict())) == json.dumps(list(emb.state_dict()))


def test_attention_layer_and_full_attention_forward_on_their_own(dev):
    """the reference's call forms outside a DecoderLayer: AttentionLayer.forward(queries, keys, values, None) with keys and values the
    same tensor (one key | value GEMM) and different tensors (three GEMMs), and FullAttention.forward on [B, L, H, E] operands --
    output and input gradients against float64"""
    B, L, S, d, H = 2, 33, 17, 64, 2
    hd = d // H
    keys = [(k.replace("layers.0.cross_attention.", ""), s) for k, s in tc.decoder_keys(d, H, 128, 1, 5) if "layers.0.cross_attention." in k]
    params = tc.synth_params("attention_layer", keys)
    layer = M.AttentionLayer(M.FullAttention(False, attention_dropout=0.1), d, H)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    layer = layer.to(dev).eval()
    u = lambda what, shape: torch.from_numpy(tc.mc.uniform(shape, tc.mc.seed_of("attention_layer", what), -1.0, 1.0, bits=16) * np.float32(1.7))      # noqa: E731
    x, kin, vin, dout = u("x", (B, L, d)), u("k", (B, S, d)), u("v", (B, S, d)), u("dout", (B, L, d))
    w = {k: torch.from_numpy(v).double() for k, v in params.items()}

    def ref(xq, xk, xv):
        lin = lambda t, n: torch.nn.functional.linear(t, w[n + "_projection.weight"], w[n + "_projection.bias"])      # noqa: E731
        o, _ = tc.qkv_ref(lin(xq, "query").reshape(B * L, d), lin(xk, "key").reshape(B * S, d), lin(xv, "value").reshape(B * S, d), B, L, S, H, hd,
                          hd ** -0.5, False)
        return lin(o.reshape(B, L, d), "out")

    for same in (True, False):
        ins = [t.to(dev).requires_grad_() for t in ((x, kin) if same else (x, kin, vin))]
        out, attn = layer(ins[0], ins[1], ins[1] if same else ins[2], None)
        assert attn is None and out.shape == (B, L, d)
        out.backward(dout.to(dev))
        rin = [t.double().requires_grad_() for t in ((x, kin) if same else (x, kin, vin))]
        r = ref(rin[0], rin[1], rin[1] if same else rin[2])
        r.backward(dout.double())
        check_close(out, r.detach(), TOL_F32, f"AttentionLayer out (same={same})")
        for a, b_ in zip(ins, rin):
            check_close(a.grad, b_.grad, TOL_F32, f"AttentionLayer input gradient (same={same})")
    full = M.FullAttention(True, attention_dropout=0.1).to(dev).eval()
    q4, k4, v4 = u("q4", (B, L, H, hd)), u("k4", (B, L, H, hd)), u("v4", (B, L, H, hd))
    o4, attn = full(q4.to(dev), k4.to(dev), v4.to(dev), None)
    want, _ = tc.qkv_ref(q4.reshape(B * L, d), k4.reshape(B * L, d), v4.reshape(B * L, d), B, L, L, H, hd, hd ** -0.5, True)
    assert attn is None and o4.shape == (B, L, H, hd)
    check_close(o4, want.reshape(B, L, H, hd), TOL_F32, "FullAttention forward")
    with pytest.raises(M.MetaEncError):
        full(q4.to(dev), k4[:, :5].to(dev), v4[:, :5].to(dev), None)             # causal with L != S
