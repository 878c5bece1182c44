"""GPU: the hyperspectral tokenizer (me_hsi_gather / me_hsi_embed_fwd / me_hsi_embed_wgrad, HyperSpectralEmbed, HyperSpectralClassifier)
against the reference-made fixture on the small cases and against the float64 restatement (tests/hyperspectral_cases.py, tied to the
reference by tests/test_hyperspectral_cpu.py) on the wide ones.  Bounds are conftest's: fp32 TOL_F32; bf16 forward of the single
op TOL_BF16_OP, bf16 gradients TOL_BF16_GRAD, the classifier's bf16 logits TOL_BF16_FWD."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, TOL_BF16_FWD, TOL_BF16_GRAD, TOL_BF16_OP, TOL_F32, check_close

import hyperspectral_cases as hc
import metatransformer_amd as M
from guarded import Guarded
from metatransformer_amd import _capi
from metatransformer_amd import hyperspectral as hs

pytestmark = pytest.mark.gpu

ALL = list(hc.SMALL) + list(hc.WIDE)
_cache = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "hyperspectral.npz"), allow_pickle=False)


def case_channels(name):
    return (hc.SMALL_C,) if name in hc.SMALL else hc.WIDE_C


def reference(name, C):
    """computed once per (case, C), shared and left unchanged: inputs, the restated tokens, the float64 output and the float64
    autograd gradients for the case's dy"""
    key = (name, C)
    if key not in _cache:
        _, _, bands, p, bp = hc.geometry(name)
        cube, pts = torch.from_numpy(hc.make_cube(name)), torch.from_numpy(hc.make_points(name))
        tokens = hc.restate(cube, pts, p, bp)
        params = {k: torch.from_numpy(v) for k, v in hc.make_params(name, C).items()}
        p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
        out = hc.embed_reference(tokens.double(), p64)
        dy = hc.make_dy(name, C, pts.shape[0])
        (out * dy.double()).sum().backward()
        _cache[key] = dict(cube=cube, pts=pts, tokens=tokens, params=params, out=out.detach(), dy=dy, grads={k: v.grad for k, v in p64.items()},
                           geom=(bands, p, bp))
    return _cache[key]


def make_embed(name, C, dev, route="auto"):
    r = reference(name, C)
    bands, p, bp = r["geom"]
    emb = M.HyperSpectralEmbed(bands=bands, patch=p, near_band=bp, embed_dim=C).to(dev)
    emb.load_state_dict(r["params"], strict=True)
    emb.route = route
    return emb, r


@pytest.mark.parametrize("name", ALL)
def test_gather_is_bit_exact(gold, dev, name):
    r = reference(name, case_channels(name)[0])
    bands, p, bp = r["geom"]
    want = torch.from_numpy(gold[f"{name}/gathered"]) if name in hc.SMALL else r["tokens"]
    got = M.neighborhood_tokens(r["cube"].to(dev), r["pts"].to(dev), p, bp)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    # a bf16 cube is copied as it is; int32 points are taken as they are
    cb = r["cube"].bfloat16()
    got = M.neighborhood_tokens(cb.to(dev), r["pts"].to(dev).int(), p, bp)
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), hc.restate(cb, r["pts"], p, bp))
    # the K-padded form the unfused route feeds to the GEMM: zero columns behind K
    got = M.neighborhood_tokens(r["cube"].to(dev), r["pts"].to(dev), p, bp, pad_to=8).cpu()
    K = p * p * bp
    assert got.shape[2] % 8 == 0 and torch.equal(got[:, :, :K], want) and not bool(got[:, :, K:].any())


@pytest.mark.parametrize("route", ["auto", "fused", "gathered"])
@pytest.mark.parametrize("name,C", [(n, C) for n in ALL for C in case_channels(n)])
def test_forward_fp32(gold, dev, name, C, route):
    emb, r = make_embed(name, C, dev, route)
    want = torch.from_numpy(gold[f"{name}/out"]) if name in hc.SMALL else r["out"]
    with torch.no_grad():
        y = emb(r["cube"].to(dev), r["pts"].to(dev))
        y_x = emb(r["tokens"].to(dev))                         # the reference's call form, on the gathered tensor
    assert y.dtype == torch.float32 and y_x.dtype == torch.float32
    check_close(y, want, TOL_F32, f"{name} C={C} {route} fp32 vs float64")
    check_close(y_x, want, TOL_F32, f"{name} C={C} forward(x) vs float64")
    check_close(y, y_x, TOL_F32, f"{name} C={C} {route} vs forward(x)")


@pytest.mark.parametrize("route", ["auto", "fused", "gathered"])
@pytest.mark.parametrize("name,C", [(n, C) for n in ALL for C in case_channels(n)])
def test_forward_bf16_autocast(gold, dev, name, C, route):
    emb, r = make_embed(name, C, dev, route)
    want = torch.from_numpy(gold[f"{name}/out"]) if name in hc.SMALL else r["out"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = emb(r["cube"].to(dev), r["pts"].to(dev))
    assert y.dtype == torch.bfloat16
    check_close(y, want, TOL_BF16_OP, f"{name} C={C} {route} bf16 vs float64")


def test_forward_takes_fewer_bands_in_the_reference_call_form(dev):
    emb, r = make_embed("p3b3", hc.SMALL_C, dev)
    n = 5
    with torch.no_grad():
        y = emb(r["tokens"][:, :n].to(dev))
    check_close(y, r["out"][:, :n + 1], TOL_F32, "forward(x[:, :5])")


@pytest.mark.parametrize("route", ["auto", "fused", "gathered"])
@pytest.mark.parametrize("mode,tol", [("fp32", TOL_F32), ("bf16", TOL_BF16_GRAD)])
@pytest.mark.parametrize("name,C", [(n, C) for n in ALL for C in case_channels(n)])
def test_parameter_gradients(dev, name, C, mode, tol, route):
    emb, r = make_embed(name, C, dev, route)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
        y = emb(r["cube"].to(dev), r["pts"].to(dev))
    (y.float() * r["dy"].to(dev)).sum().backward()
    for k, p in emb.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype, k
        check_close(p.grad, r["grads"][k].reshape(p.shape), tol, f"{name} C={C} {route} {mode} d{k}")


@pytest.mark.parametrize("dyt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,C", [("p7b5", hc.SMALL_C), ("p1b1", hc.SMALL_C), ("indian", 64), ("pavia", 768)])
def test_wgrad_is_deterministic_skips_null_outputs_and_accumulates(dev, name, C, dyt):
    r = reference(name, C)
    bands, p, bp = r["geom"]
    cube, pts, dy = r["cube"].to(dev), r["pts"].to(dev), r["dy"].to(dev).to(dyt)
    names = {"dw": "patch_to_embedding.weight", "dbias": "patch_to_embedding.bias", "dcls": "cls_token", "dpos": "pos_embedding"}
    tol = TOL_F32 if dyt == torch.float32 else TOL_BF16_GRAD
    a = hs.hsi_embed_wgrad(cube, pts, p, bp, dy)
    b = hs.hsi_embed_wgrad(cube, pts, p, bp, dy)
    for n, key in names.items():
        assert torch.equal(a[n], b[n]), f"{name} {n}: two runs differ"
        check_close(a[n], r["grads"][key].reshape(a[n].shape), tol, f"{name} C={C} {n}")
    # any subset: what is not asked for is not computed into anything, what is asked for does not depend on the others
    for want in (("dw",), ("dbias",), ("dcls", "dpos"), ("dpos",)):
        g = hs.hsi_embed_wgrad(cube, pts, p, bp, dy, want=want)
        assert sorted(g) == sorted(want)
        for n in want:
            assert torch.equal(g[n], a[n]), f"{name} {n} alone"
    # beta = 1 adds to what is there
    old = {n: torch.full_like(t, 0.25) for n, t in a.items()}
    g = hs.hsi_embed_wgrad(cube, pts, p, bp, dy, into={n: t.clone() for n, t in old.items()}, beta=1.0)
    for n in names:
        assert torch.equal(g[n], old[n] + a[n]), f"{name} {n}: beta = 1"


def _desc(cube_g, H, W, bands, pix, pts, p, bp, dt):
    d = _capi.HsiDesc()
    d.cube, d.cube_dtype, d.row_stride, d.pix_stride = cube_g.ptr(), dt, W * pix, pix
    d.H, d.W, d.bands, d.points, d.B, d.patch, d.band_patch = H, W, bands, pts.data_ptr(), pts.shape[0], p, bp
    return d


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,C", [("p7b3", hc.SMALL_C), ("p5b7", hc.SMALL_C), ("indian", 64), ("pavia", 64)])
def test_contract_guards_and_padded_strides(dev, name, C, cdt):
    """the cube between NaN guards with NaN pad columns behind every pixel's bands, every output between sentinel guards with pad columns
    (padded ld_out / ld_w / ld_pos / ld_dw / ld_dpos): nothing outside the described extents is read into a result or written"""
    lib = _capi.load()
    r = reference(name, C)
    bands, p, bp = r["geom"]
    H, W, _ = r["cube"].shape
    K, B = p * p * bp, r["pts"].shape[0]
    pix = bands + 3
    code = _capi.dtype_code(cdt)
    cube_g = Guarded.input(r["cube"].reshape(H * W, bands).to(dev).to(cdt), ld=pix)
    pts = r["pts"].to(dev).int().contiguous()
    d = _desc(cube_g, H, W, bands, pix, pts, p, bp, code)
    stream = _capi.stream_ptr()
    cube_used = r["cube"].to(cdt)
    tokens = hc.restate(cube_used, r["pts"], p, bp)
    # gather
    out_g = Guarded.output(B * bands, K, K + 5, cdt, dev)
    _capi.check(lib.me_hsi_gather(ctypes.byref(d), out_g.ptr(), code, K + 5, stream), "me_hsi_gather")
    out_g.check(f"{name} gather")
    assert out_g.untouched_interior() == 0 and torch.equal(out_g.t.cpu().reshape(B, bands, K), tokens)
    # fused forward
    P = r["params"]
    w_g = Guarded.input(P["patch_to_embedding.weight"].to(dev).to(cdt), ld=K + 3)
    b_g = Guarded.input(P["patch_to_embedding.bias"].to(dev))
    c_g = Guarded.input(P["cls_token"].reshape(C).to(dev))
    p_g = Guarded.input(P["pos_embedding"].reshape(bands + 1, C).to(dev), ld=C + 4)
    y_g = Guarded.output(B * (bands + 1), C, C + 8, cdt, dev)
    _capi.check(lib.me_hsi_embed_fwd(ctypes.byref(d), w_g.ptr(), code, K + 3, b_g.ptr(), c_g.ptr(), p_g.ptr(), C + 4, y_g.ptr(), code, C + 8, C,
                                     stream), "me_hsi_embed_fwd")
    y_g.check(f"{name} embed_fwd")
    assert y_g.untouched_interior() == 0
    check_close(y_g.t.reshape(B, bands + 1, C), r["out"], TOL_F32 if cdt == torch.float32 else TOL_BF16_OP, f"{name} {cdt} guarded forward")
    # weight gradient
    dy_g = Guarded.input(r["dy"].reshape(B * (bands + 1), C).to(dev).to(cdt), ld=C + 12)
    nbytes = lib.me_hsi_embed_wgrad_workspace(ctypes.byref(d), C)
    ws_g = Guarded.output_bytes(nbytes, dev)
    dw_g = Guarded.output(C, K, K + 3, torch.float32, dev)
    dp_g = Guarded.output(bands + 1, C, C + 4, torch.float32, dev)
    db_g, dc_g = Guarded.output_vec(C, torch.float32, dev), Guarded.output_vec(C, torch.float32, dev)
    _capi.check(lib.me_hsi_embed_wgrad(ctypes.byref(d), dy_g.ptr(), code, C + 12, C, dw_g.ptr(), K + 3, db_g.ptr(), dc_g.ptr(), dp_g.ptr(), C + 4,
                                       0.0, ws_g.ptr(), nbytes, stream), "me_hsi_embed_wgrad")
    tol = TOL_F32 if cdt == torch.float32 else TOL_BF16_GRAD
    for g, key, what in ((dw_g, "patch_to_embedding.weight", "dw"), (db_g, "patch_to_embedding.bias", "dbias"), (dc_g, "cls_token", "dcls"),
                         (dp_g, "pos_embedding", "dpos"), (ws_g, None, "workspace")):
        g.check(f"{name} wgrad {what}")
        if key is not None:
            assert g.untouched_interior() == 0, what
            check_close(g.t, r["grads"][key].reshape(g.t.shape), tol, f"{name} {cdt} guarded {what}")


def test_data2seq_hyper_and_dropout(dev):
    r = reference("p3b3", hc.SMALL_C)
    bands, p, bp = r["geom"]
    tok = M.Data2Seq("hyper", hc.SMALL_C, bands=bands, patch=p, near_band=bp, emb_dropout=0.5).to(dev)
    tok.embed.load_state_dict(r["params"], strict=True)
    cube, pts = r["cube"].to(dev), r["pts"].to(dev)
    y_eval = tok.eval()(cube, pts)
    check_close(y_eval, r["out"], TOL_F32, "Data2Seq('hyper') eval")
    y = tok.train()(cube, pts)
    kept = y != 0
    assert 0.3 < float(kept.float().mean()) < 0.7
    assert torch.equal(y[kept], 2.0 * y_eval[kept])                                # inverted dropout: survivors scaled by 1 / (1 - p) = 2, exactly
    y.sum().backward()
    g = tok.embed.cls_token.grad.reshape(-1)
    assert torch.equal(g, 2.0 * kept[:, 0].float().sum(0))


@pytest.mark.parametrize("mode,tol", [("fp32", TOL_F32), ("bf16", TOL_BF16_FWD)])
def test_classifier_logits(gold, dev, mode, tol):
    c = json.loads(str(gold["cls/config"]))
    name = c["case"]
    _, _, bands, p, bp = hc.geometry(name)
    sd = {k: torch.from_numpy(gold["cls/sd/" + k]) for k, _ in json.loads(str(gold["cls/keys"]))}
    m = M.HyperSpectralClassifier(image_size=p, near_band=bp, num_patches=bands, num_classes=c["num_classes"], dim=c["dim"], depth=c["depth"],
                                  heads=c["heads"], mlp_dim=c["mlp_dim"]).to(dev).eval()
    m.load_state_dict(sd, strict=True)
    cube, pts = torch.from_numpy(gold[f"{name}/cube"]).to(dev), torch.from_numpy(gold[f"{name}/points"]).to(dev)
    want = torch.from_numpy(gold["cls/logits"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
        logits = m(cube, pts)
        logits_x = m(torch.from_numpy(gold[f"{name}/gathered"]).to(dev))
    print(f"classifier {mode}: max-abs error / max|ref| = {float((logits.double().cpu() - want).abs().max() / want.abs().max()):.3e}")
    check_close(logits, want, tol, f"classifier {mode} forward(cube, points)")
    check_close(logits_x, want, tol, f"classifier {mode} forward(x)")
