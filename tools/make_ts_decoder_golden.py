"""Write tests/golden/ts_decoder.npz from the reference's own Time-Series classes (Time-Series/layers/Transformer_EncDec.py,
SelfAttention_Family.py, Embed.py, utils/masking.py, loaded unmodified through oracle.ref_loader._load_file).

    python tools/make_ts_decoder_golden.py            # (re)write the fixture        (needs the reference tree; CPU only)
    python tools/make_ts_decoder_golden.py --check    # regenerate and compare with the stored fixture, write nothing

Stand-ins, and only these: a `reformer_pytorch` module with an `LSHSelfAttention` attribute and an empty `utils` package (imports of
SelfAttention_Family.py that the classes used here never touch).

Inputs and parameters are not stored (tests/ts_decoder_cases.py synthesises them on both sides).  Stored per case, for the output and
every gradient t (dx, dcross, dparam/<key>; for the timeF embedding out and dparam/<key>):
  * `<case>/<t>`: the float64 result at msda_cases.subset_index(numel, KEEP) positions followed by the element of largest magnitude,
  * `<case>/<t>/argmax`: that element's flat position,
  * `<case>/<t>/ref_err`: the reference's own float32-vs-float64 distance max |f32 - f64| / max |f64|.
Also keys/decoder, keys/embed_timeF and keys/forecaster: state-dict keys and shapes as the reference's classes register them (the
forecaster's assembled from DataEmbedding x 2, the decoder and the encoder Blocks' key set, as Model.__init__ does for the forecast tasks).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import ts_decoder_cases as tc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "ts_decoder.npz")
TS = "Time-Series"


def load_reference():
    from oracle import ref_loader
    rp = types.ModuleType("reformer_pytorch")
    rp.LSHSelfAttention = object
    ut = types.ModuleType("utils")
    ut.__path__ = []
    stubs = {"reformer_pytorch": rp, "utils": ut}
    ref_loader._load_file("utils.masking", os.path.join(TS, "utils", "masking.py"), stubs)
    saf = ref_loader._load_file("_ref_ts_saf", os.path.join(TS, "layers", "SelfAttention_Family.py"), stubs)
    ed = ref_loader._load_file("_ref_ts_encdec", os.path.join(TS, "layers", "Transformer_EncDec.py"))
    emb = ref_loader._load_file("_ref_ts_embed", os.path.join(TS, "layers", "Embed.py"))
    return saf, ed, emb


def make_decoder(saf, ed, d_model, H, d_ff, layers, c_out):
    """as Time-Series/models/MetaTransformer.py:46-70 builds it"""
    return ed.Decoder(
        [ed.DecoderLayer(saf.AttentionLayer(saf.FullAttention(True, 1, attention_dropout=0.1, output_attention=False), d_model, H),
                         saf.AttentionLayer(saf.FullAttention(False, 1, attention_dropout=0.1, output_attention=False), d_model, H),
                         d_model, d_ff, dropout=0.1, activation="gelu") for _ in range(layers)],
        norm_layer=torch.nn.LayerNorm(d_model), projection=torch.nn.Linear(d_model, c_out, bias=True))


def run_decoder(saf, ed, name, dtype):
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES[name]
    m = make_decoder(saf, ed, d, H, ff, nl, co)
    keys = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert keys == tc.decoder_keys(d, H, ff, nl, co), name
    m.load_state_dict({k: torch.from_numpy(v) for k, v in tc.synth_params(name, keys).items()}, strict=True)
    m = m.to(dtype).eval()
    x, cross, dout = (torch.from_numpy(a).to(dtype) for a in tc.decoder_inputs(name))
    x.requires_grad_()
    cross.requires_grad_()
    y = m(x, cross, x_mask=None, cross_mask=None)
    y.backward(dout)
    res = {"out": y.detach(), "dx": x.grad, "dcross": cross.grad}
    res.update({"dparam/" + k: p.grad for k, p in m.named_parameters()})
    return res


def run_embed(emb, name, dtype):
    B, L, c_in, d, freq = tc.EMBED_CASES[name]
    m = emb.DataEmbedding(c_in, d, "timeF", freq, 0.1)
    want = tc.embed_keys(c_in, d, freq)
    trainable = [(k, tuple(p.shape)) for k, p in m.named_parameters() if p.requires_grad]
    assert trainable == want, (trainable, want)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in tc.synth_params(name, want).items()})
    m.load_state_dict(sd, strict=True)
    m = m.to(dtype).eval()
    x, mark, dout = (torch.from_numpy(a).to(dtype) for a in tc.embed_inputs(name))
    y = m(x, mark)
    y.backward(dout)
    res = {"out": y.detach()}
    res.update({"dparam/" + k: p.grad for k, p in m.named_parameters() if p.requires_grad})
    return res


def put(out: dict, key: str, t64: torch.Tensor, t32: torch.Tensor):
    a64, a32 = t64.detach().double().numpy().reshape(-1), t32.detach().double().numpy().reshape(-1)
    mx = float(np.abs(a64).max())
    out[key] = tc.stored(a64)
    out[key + "/argmax"] = np.int64(int(np.abs(a64).argmax()))
    out[key + "/ref_err"] = np.float64(np.abs(a32 - a64).max() / max(mx, 1e-30))


def key_list(module) -> str:
    return json.dumps([[k, list(v.shape)] for k, v in module.state_dict().items()])


def generate() -> dict:
    saf, ed, emb = load_reference()
    tc.assert_coverage()
    out = {}
    for name in tc.DECODER_CASES:
        r64, r32 = run_decoder(saf, ed, name, torch.float64), run_decoder(saf, ed, name, torch.float32)
        for k in r64:
            put(out, f"decoder/{name}/{k}", r64[k], r32[k])
        worst = max(float(out[f"decoder/{name}/{k}/ref_err"]) for k in r64 if "key_projection.bias" not in k)
        print(f"  decoder/{name}: out ref_err {float(out[f'decoder/{name}/out/ref_err']):.1e}, worst {worst:.1e}")
    for name in tc.EMBED_CASES:
        r64, r32 = run_embed(emb, name, torch.float64), run_embed(emb, name, torch.float32)
        for k in r64:
            put(out, f"embed/{name}/{k}", r64[k], r32[k])
        print(f"  embed/{name}: ref_err " + " ".join(f"{k.split('/')[-1]} {float(out[f'embed/{name}/{k}/ref_err']):.1e}" for k in r64))
    B, L, S, d, H, ff, nl, co = tc.DECODER_CASES["recipe"]
    dec = make_decoder(saf, ed, d, H, ff, nl, co)
    e_tf = emb.DataEmbedding(7, d, "timeF", "h", 0.1)
    out["keys/decoder"] = key_list(dec)
    out["keys/embed_timeF"] = key_list(e_tf)
    # the forecast Model's key set: enc_embedding, encoder (timm Blocks of the reference encoder: the names of oracle.ref_loader's
    # reference_encoder, qkv_bias=True), dec_embedding, decoder -- in registration order
    from oracle import ref_loader
    blocks = ref_loader.reference_encoder(2, d, 12)
    fk = [["enc_embedding." + k, s] for k, s in json.loads(key_list(e_tf))]
    fk += [["encoder." + k, list(v.shape)] for k, v in blocks.state_dict().items()]
    fk += [["dec_embedding." + k, s] for k, s in json.loads(key_list(e_tf))]
    fk += [["decoder." + k, s] for k, s in json.loads(key_list(dec))]
    out["keys/forecaster"] = json.dumps(dict(config=dict(enc_in=7, dec_in=7, c_out=co, d_model=d, n_heads=H, d_ff=ff, d_layers=nl,
                                                         embed="timeF", freq="h", depth=2, num_heads=12), keys=fk))
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
