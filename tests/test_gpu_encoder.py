"""GPU: the drop-in modules (Block stack, tokenizers) against the golden vectors produced by the reference's own code,
against the CPU oracle on seeded inputs, and -- at BASELINE sizes -- through size-independent properties."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import (GOLDEN, TOL_BF16, TOL_BF16_FWD, TOL_BF16_OP, TOL_BF16_GRAD, TOL_BF16_STREAM1, TOL_BF16_STREAM12, TOL_F32, check_close,
                      rel_err)
import metatransformer_amd as M
from oracle import block_oracle as bo
from oracle import tokenizer_oracle as to
from oracle.make_golden import ENCODER_CASES, _inputs

pytestmark = pytest.mark.gpu


def golden(name):
    z = np.load(os.path.join(GOLDEN, f"encoder_{name}.npz"), allow_pickle=False)
    return z, json.loads(str(z["config"]))


def make_encoder(c, dev, dtype=torch.float32):
    from functools import partial
    enc = M.build_encoder(c["depth"], c["dim"], c["heads"], norm_layer=partial(nn.LayerNorm, eps=c["eps"]))
    enc.load_state_dict(bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"]), strict=True)
    return enc.to(dev).to(dtype).eval()


@pytest.mark.parametrize("name", list(ENCODER_CASES))
def test_forward_fp32_matches_reference_golden(dev, name):
    z, c = golden(name)
    enc = make_encoder(c, dev)
    x, _ = _inputs(c)
    with torch.no_grad():
        y = enc(x.to(dev))
    assert y.shape == x.shape and y.dtype == torch.float32
    assert rel_err(y[:, ::c["tok_stride"]], torch.from_numpy(z["y"])) < TOL_F32


@pytest.mark.parametrize("name", ["small_hd64", "base_1blk", "base_12blk", "large_2blk", "graph_hd24"])
@pytest.mark.parametrize("mode", ["autocast", "bf16_params"])
def test_forward_bf16_matches_reference_golden(dev, name, mode):
    """bf16 MFMA path vs the fp32 reference output: TOL_BF16_FWD of max-abs plus the per-element bound of check_close."""
    z, c = golden(name)
    x, _ = _inputs(c)
    with torch.no_grad():
        if mode == "autocast":
            enc = make_encoder(c, dev)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = enc(x.to(dev))
            assert y.dtype == torch.float32            # fp32 residual stream under autocast
        else:
            enc = make_encoder(c, dev, torch.bfloat16)
            y = enc(x.to(dev).bfloat16())
            assert y.dtype == torch.bfloat16
    if mode == "autocast":          # fp32 residual stream
        tol = TOL_BF16_FWD * (2.0 if c["depth"] > 2 else 1.0)
    else:                           # bf16 parameters AND a bf16 residual stream
        tol = TOL_BF16_STREAM12 if c["depth"] > 2 else TOL_BF16_STREAM1
    check_close(y[:, ::c["tok_stride"]].float(), torch.from_numpy(z["y"]), tol, name)


@pytest.mark.parametrize("name", [n for n, c in ENCODER_CASES.items() if c["backward"]])
def test_backward_fp32_matches_reference_golden(dev, name):
    z, c = golden(name)
    enc = make_encoder(c, dev).train()
    x, go = _inputs(c)
    xr = x.to(dev).requires_grad_(True)
    y = enc(xr)
    (y * go.to(dev)).sum().backward()
    s = c["tok_stride"]
    assert rel_err(xr.grad[:, ::s], torch.from_numpy(z["dx"])) < TOL_F32
    for k, p in enc.named_parameters():
        stats = z["dparam_stats/" + k]
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert abs(p.grad.double().abs().sum().item() - stats[1]) < 1e-3 * max(stats[1], 1e-6), k
        head = p.grad.flatten()[:16].cpu().numpy()
        assert np.allclose(head, z["dparam_head/" + k], rtol=5e-3, atol=1e-3 * stats[1] / p.numel() + 1e-6), k
        if c.get("grad_stride"):      # the reference's OWN gradient values, element for element (whole, or every 5th of the Base block)
            check_close(p.grad.flatten()[::c["grad_stride"]], torch.from_numpy(z["dparam_s/" + k]), TOL_F32, f"{name} d{k} vs reference values")
    # EVERY element of every gradient (the fixture keeps sums and heads only: a wrong tail column of a 3072-wide weight
    # gradient would pass those): against the CPU restatement on the fixture's inputs, which tests/test_oracle.py pins to the
    # same reference-generated statistics
    sd = bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"])
    _, dx_o, dp_o = bo.encoder_forward_backward(x, sd, c["heads"], go, eps=c["eps"])
    check_close(xr.grad, dx_o, TOL_F32, name + " dx (all elements)")
    for k, p in enc.named_parameters():
        check_close(p.grad, dp_o[k], TOL_F32, f"{name} d{k} (all elements)")


def test_backward_full_parity_vs_oracle(dev):
    """every gradient element, fp32 and bf16, on a Base-width block with ragged token count"""
    c = dict(depth=2, dim=256, heads=4, eps=1e-5, seed=5)
    sd = bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"])
    g = torch.Generator().manual_seed(42)
    x, go = torch.randn(3, 70, 256, generator=g), torch.randn(3, 70, 256, generator=g)
    y_ref, dx_ref, dp_ref = bo.encoder_forward_backward(x, sd, c["heads"], go)
    for dt, t in ((torch.float32, TOL_F32), (torch.bfloat16, TOL_BF16_GRAD)):
        enc = make_encoder(c, dev).train()
        xr = x.to(dev).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            y = enc(xr)
        (y * go.to(dev)).sum().backward()
        assert rel_err(y, y_ref) < t and rel_err(xr.grad, dx_ref) < t
        for k, p in enc.named_parameters():
            check_close(p.grad, dp_ref[k], t, f"d{k} {dt}")      # (max-abs AND per element)


def test_block_backward_side_stream_equals_serial_order(dev):
    """me_block_bwd issues the weight-gradient GEMMs on its side stream (forked from / joined to the caller's stream inside the call):
    every gradient is BIT-identical to the serial order (no kernel's arithmetic depends on what shares the chip with it), over
    several backward passes with unrelated traffic on a third stream, at a shape whose resident kernels claim their tiles, and the
    caller's stream really is joined (the gradients are read on it right after the call returns)."""
    from metatransformer_amd import ops, parallel
    c = dict(depth=3, dim=768, heads=12, eps=1e-6, seed=11)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(96, 197, 768, generator=g).to(dev)
    go = (torch.randn(96, 197, 768, generator=g) / 1000).to(dev)
    noise = torch.empty(32 << 20, device=dev)
    side = torch.cuda.Stream()
    got = {}
    prev = ops.block_bwd_overlap(True)
    try:
        for overlap in (False, True, True):
            ops.block_bwd_overlap(overlap)
            enc = make_encoder(c, dev).train()
            flat = parallel.FlatParams(enc.parameters())
            flat.zero_grad()
            xr = x.clone().requires_grad_(True)
            for rep in range(2):                              # (accumulating passes: beta = 1 into the flat buffer)
                with torch.cuda.stream(side):
                    noise.add_(1.0)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = enc(xr)
                y.backward(go)
            snap = (flat.flat_grad.clone(), xr.grad.clone())  # read on the caller's stream, no synchronisation in between
            key = "overlap" if overlap else "serial"
            if key in got:
                assert torch.equal(got[key][0], snap[0]) and torch.equal(got[key][1], snap[1])      # run to run
            got[key] = snap
    finally:
        ops.block_bwd_overlap(prev)
    assert torch.equal(got["serial"][0], got["overlap"][0])
    assert torch.equal(got["serial"][1], got["overlap"][1])
    assert float(got["serial"][0].abs().max()) > 0


def test_flat_params_fused_gradient_accumulation(dev):
    """parallel.FlatParams: weight gradients accumulated in place by the wgrad epilogue == autograd's own accumulation,
    over two backward passes (gradient accumulation), and the direct-write listeners fire once per weight per pass"""
    from metatransformer_amd import parallel
    c = dict(depth=2, dim=256, heads=4, eps=1e-5, seed=7)
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(2, 300, 256, generator=g).to(dev) for _ in range(2)]
    grads = {}
    for fused in (False, True):
        enc = make_encoder(c, dev).train()
        flat = parallel.FlatParams(enc.parameters(), fused_accumulate=fused)
        fired = []
        flat._listeners.append(fired.append)
        flat.zero_grad()
        for x in xs:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                enc(x).float().square().mean().backward()
        grads[fused] = flat.flat_grad.clone()
        assert len(fired) == (2 * 12 * c["depth"] if fused else 0)      # all 12 parameters of a block, each pass
        for p in enc.parameters():
            assert flat.direct_grad(p) is not None or not fused       # .grad views were not replaced
    assert rel_err(grads[True], grads[False]) < 1e-6


@pytest.mark.parametrize("mode", ["autocast_fp16", "half_params"])
def test_fp16_call_sites_run_on_bf16_kernels(dev, mode):
    """fp16 autocast (Audio/src/traintest.py:145, mmcv fp16) and `.half()` models: fp16 tensors are converted at the
    boundary (me_cast), compute is bf16, outputs / gradients come back in the caller's dtype"""
    c = dict(depth=2, dim=256, heads=4, eps=1e-5, seed=9)
    sd = bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"])
    g = torch.Generator().manual_seed(4)
    x, go = torch.randn(2, 150, 256, generator=g), torch.randn(2, 150, 256, generator=g)
    y_ref, dx_ref, dp_ref = bo.encoder_forward_backward(x, sd, c["heads"], go)
    enc = make_encoder(c, dev).train()
    if mode == "half_params":
        enc = enc.half()
        xr = x.to(dev).half().requires_grad_(True)
        y = enc(xr)
        assert y.dtype == torch.float16
    else:
        xr = x.to(dev).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = enc(xr)
    (y.float() * go.to(dev)).sum().backward()
    assert xr.grad.dtype == xr.dtype
    assert rel_err(y.float(), y_ref) < 2 * TOL_BF16_FWD and rel_err(xr.grad.float(), dx_ref) < TOL_BF16_GRAD
    for k, p in enc.named_parameters():
        assert p.grad.dtype == p.dtype and rel_err(p.grad.float(), dp_ref[k]) < 6e-2, k


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_c_side_block_equals_op_by_op_composition(dev, dt):
    """me_block_fwd / me_block_bwd (one call per block and direction) launch the same kernels in the same order as the
    Python op-by-op composition: results must be bit-identical"""
    c = dict(depth=2, dim=256, heads=4, eps=1e-6, seed=12)
    g = torch.Generator().manual_seed(8)
    x, go = torch.randn(3, 197, 256, generator=g).to(dev), torch.randn(3, 197, 256, generator=g).to(dev)
    res = {}
    for c_side in (True, False):
        enc = make_encoder(c, dev).train()
        for b in enc:
            b.c_side = c_side
            b.fp32_mode = "exact"           # (the op-by-op composition has no three-product form: compare like with like)
        xr = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            y = enc(xr)
        (y * go).sum().backward()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            y_inf = enc.eval()(x)
        res[c_side] = [y.detach(), y_inf, xr.grad] + [p.grad for p in enc.parameters()]
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_optimizer_mirror_and_batched_transposes(dev):
    """FusedAdamW's bf16 mirror feeds the forward weight copies, stale transposed copies of ALL blocks are rebuilt in one
    batched launch; results equal the per-weight refresh (mirror off), also after load_state_dict and on a deepcopy"""
    import copy
    from metatransformer_amd import parallel, ops
    c = dict(depth=3, dim=128, heads=2, eps=1e-5, seed=13)
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(2, 100, 128, generator=g).to(dev) for _ in range(3)]
    outs = {}
    for mirror in (True, False):
        enc = make_encoder(c, dev).train()
        flat = parallel.FlatParams(enc.parameters())
        opt = parallel.FusedAdamW(flat, lr=1e-2, bf16_mirror=mirror)
        ys = []
        for x in xs:
            flat.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = enc(x)
            y.float().square().mean().backward()
            opt.step()
            ys.append(y.detach().clone())
        if mirror:
            w = enc[0].attn.qkv.weight
            assert flat.bf16_view(w) is not None and torch.equal(flat.bf16_view(w), w.detach().bfloat16())
            tr = enc[1]._wcache.transposed("fc1", enc[1].mlp.fc1.weight, torch.bfloat16)      # refreshes every block at once
            assert torch.equal(tr, enc[1].mlp.fc1.weight.detach().bfloat16().t())
            assert all(b._wcache.has("t", n, tr.device) for b in enc for n in ("qkv", "proj", "fc1", "fc2"))
            with torch.no_grad():
                w.mul_(2.0)                                   # a write the optimizer did not make: the mirror is stale
            assert flat.bf16_view(w) is None
            enc2 = copy.deepcopy(enc).eval()                 # caches are not shared with the copy
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                assert torch.equal(enc2(xs[0]), enc.eval()(xs[0]))
        outs[mirror] = ys
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("depth", [1, 2, 5])
def test_encoder_forward_single_call(dev, dt, depth):
    """me_encoder_fwd (the whole stack in one C call, for serving hosts) == encoder(x), bit for bit"""
    c = dict(depth=depth, dim=256, heads=4, eps=1e-5, seed=31)
    enc = make_encoder(c, dev, dt)
    x = torch.randn(3, 77, 256, generator=torch.Generator().manual_seed(1)).to(dev).to(dt)
    with torch.no_grad():
        ref = enc(x)
    assert torch.equal(M.encoder_forward_inference(enc, x), ref)


def test_training_steps_match_torch_adamw_on_the_oracle(dev):
    """row f1 end to end: three optimizer steps of the fused training path (C-side block calls, gradients accumulated in
    place into FlatParams, one-kernel AdamW) against torch.optim.AdamW driving autograd through the CPU oracle"""
    from metatransformer_amd import parallel
    c = dict(depth=2, dim=128, heads=2, eps=1e-5, seed=17)
    sd = bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"])
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(2, 80, 128, generator=g) for _ in range(3)]
    tgt = [torch.randn(2, 80, 128, generator=g) for _ in range(3)]
    ref = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
    opt_ref = torch.optim.AdamW(list(ref.values()), lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    enc = make_encoder(c, dev).train()
    flat = parallel.FlatParams(enc.parameters())
    opt = parallel.FusedAdamW(flat, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    for x, t in zip(xs, tgt):
        opt_ref.zero_grad()
        ((bo.encoder_forward(x.double(), ref, c["heads"]) - t.double()) ** 2).mean().backward()
        opt_ref.step()
        flat.zero_grad()
        ((enc(x.to(dev)) - t.to(dev)) ** 2).mean().backward()
        opt.step()
    for k, p in enc.named_parameters():
        assert rel_err(p.detach(), ref[k].detach()) < 2e-4, k


def test_frozen_encoder_passes_input_grad_only(dev):
    """most reference pipelines freeze the encoder but train the tokenizer in front of it."""
    c = dict(depth=1, dim=128, heads=2, eps=1e-5, seed=6)
    enc = make_encoder(c, dev)
    for p in enc.parameters():
        p.requires_grad = False
    x = torch.randn(2, 33, 128, generator=torch.Generator().manual_seed(1))
    xr = x.to(dev).requires_grad_(True)
    enc(xr).square().sum().backward()
    sd = bo.make_encoder_state_dict(1, 128, seed=6)
    xo = x.clone().requires_grad_(True)
    bo.encoder_forward(xo, sd, 2).square().sum().backward()
    assert rel_err(xr.grad, xo.grad) < TOL_F32
    assert all(p.grad is None for p in enc.parameters())


def test_block_api_behaviours(dev):
    enc = make_encoder(dict(depth=3, dim=64, heads=4, eps=1e-5, seed=2), dev)
    x = torch.randn(2, 10, 64, device=dev)
    with torch.no_grad():
        y = enc(x)
        z = x
        for blk in enc:                      # iteration form (Audio/src/models/ast_models.py:161-162)
            z = blk(z)
        assert torch.equal(y, z)
        assert torch.equal(enc[1:](enc[0:1](x)), y)           # slicing form (vit_adapter.py:107)
        pos = torch.randn(1, 10, 64, device=dev)
        w = x
        for blk in enc:                      # per-block pos re-injection (PointCloud metatransformer.py:161-163)
            w = blk(w + pos)
        sd = {k: v.cpu() for k, v in enc.state_dict().items()}
        ref = bo.encoder_forward(x.cpu(), sd, 4, pos_embed=pos.cpu())
        assert rel_err(w, ref) < TOL_F32
        # [T,B,C] fed as batch-first, as the Graph pipeline does (tokengt_graph_encoder.py:321,331-334)
        assert rel_err(enc(x.transpose(0, 1)), bo.encoder_forward(x.cpu().transpose(0, 1), sd, 4)) < TOL_F32
    # activation checkpointing (Video/models/modeling_finetune.py:440-441)
    import torch.utils.checkpoint as cp
    xr = x.clone().requires_grad_(True)
    out = xr
    for blk in enc.train():
        out = cp.checkpoint(blk, out, use_reentrant=False)
    out.sum().backward()
    xr2 = x.clone().requires_grad_(True)
    enc(xr2).sum().backward()
    assert rel_err(xr.grad, xr2.grad) < 1e-6


def test_stochastic_training_ops(dev):
    """Dropout(drop) on proj / MLP and DropPath in training mode (attention.py:37,49,56-57; mlp.py:32,35; drop.py:135-152):
    the RNG stream is our own, so check (i) eval is unaffected, (ii) distribution and 1/keep scaling, (iii) backward uses
    exactly the forward masks (finite-difference free: linearity of the masked branch in its input gradient)."""
    from metatransformer_amd import ops
    # (ii) kernel-level statistics
    v = torch.ones(64 * 50, 256, device=dev)
    torch.manual_seed(0)
    out = ops.dropout_add(v, None, 50, 0.25, 0.0, seed=1234)
    kept = (out != 0).float().mean().item()
    assert abs(kept - 0.75) < 0.01 and torch.allclose(out[out != 0], torch.tensor(1 / 0.75, device=dev))
    out = ops.dropout_add(v, None, 50, 0.0, 0.3, seed=99)
    per_sample = out.reshape(64, 50, 256)
    assert all(bool((s == 0).all() or torch.allclose(s, torch.tensor(1 / 0.7, device=dev))) for s in per_sample), "drop-path is per sample"
    assert 0 < int(sum(bool((s == 0).all()) for s in per_sample)) < 64
    assert torch.equal(ops.dropout_add(v, None, 50, 0.25, 0.3, seed=7), ops.dropout_add(v, None, 50, 0.25, 0.3, seed=7))
    res = torch.randn_like(v)
    assert torch.allclose(ops.dropout_add(v, res, 50, 0.25, 0.0, seed=1234), ops.dropout_add(v, None, 50, 0.25, 0.0, seed=1234) + res)
    # (i) + (iii) module level
    blk = M.Block(128, 2, qkv_bias=True, drop=0.2, drop_path=0.25).to(dev)
    x = torch.randn(16, 20, 128, device=dev)
    blk.eval()
    with torch.no_grad():
        sd = {k: v.cpu() for k, v in blk.state_dict().items()}
        assert rel_err(blk(x), bo.block_forward(x.cpu(), sd, 2)) < TOL_F32
    blk.train()
    torch.manual_seed(5); y1 = blk(x)
    torch.manual_seed(5); y2 = blk(x)
    torch.manual_seed(6); y3 = blk(x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    dropped = [(y1[b] - x[b]).abs().max().item() == 0 for b in range(16)]     # both branches dropped for a sample: y == x
    torch.manual_seed(5)
    xr = x.clone().requires_grad_(True)
    y = blk(xr)
    g1, g2 = torch.randn_like(y), torch.randn_like(y)
    (ga,) = torch.autograd.grad(y, xr, g1, retain_graph=True)
    (gb,) = torch.autograd.grad(y, xr, g2, retain_graph=True)
    (gab,) = torch.autograd.grad(y, xr, g1 + 2 * g2)
    assert rel_err(gab, ga + 2 * gb) < 1e-4, "backward must be linear in the incoming gradient (same masks every time)"
    for b, d in enumerate(dropped):
        if d:
            assert torch.equal(ga[b], g1[b]), "a sample whose branches are dropped passes its gradient through unchanged"
    # attn_drop (the Graph call site trains with 0.1, tokengt_graph_encoder.py:191-205): runs, is seeded, is off in eval
    ga_blk = M.Block(128, 2, qkv_bias=True, attn_drop=0.1).to(dev)
    torch.manual_seed(3); y1 = ga_blk.train()(x)
    torch.manual_seed(3); y2 = ga_blk(x)
    torch.manual_seed(4); y3 = ga_blk(x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y3)
    ref_blk = M.Block(128, 2, qkv_bias=True).to(dev)
    ref_blk.load_state_dict(ga_blk.state_dict())
    assert torch.equal(ga_blk.eval()(x), ref_blk.eval()(x))


def test_layer_scale_variant(dev):
    blk = M.Block(128, 2, qkv_bias=True, layer_scale=True).to(dev).eval()
    with torch.no_grad():
        blk.gamma1.uniform_(0.1, 1.0); blk.gamma2.uniform_(0.1, 1.0)
        x = torch.randn(2, 20, 128, device=dev)
        sd = {k: v.cpu() for k, v in blk.state_dict().items()}
        ref = bo.block_forward(x.cpu(), sd, 2, gamma1=sd["gamma1"], gamma2=sd["gamma2"])
        assert rel_err(blk(x), ref) < TOL_F32


@pytest.mark.parametrize("dt,tol", [(torch.float32, TOL_F32), (torch.bfloat16, TOL_BF16_GRAD)])
def test_layer_scale_backward_vs_oracle(dev, dt, tol):
    """gamma1/gamma2 of the Image pipelines (vit.py:313-316): every gradient incl. d gamma against autograd through the
    oracle's restatement"""
    torch.manual_seed(11)
    blk = M.Block(256, 4, qkv_bias=True, layer_scale=True).to(dev).train()
    with torch.no_grad():
        blk.gamma1.uniform_(0.2, 1.5); blk.gamma2.uniform_(0.2, 1.5)
    x = torch.randn(2, 70, 256)
    go = torch.randn(2, 70, 256)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr = x.double().requires_grad_(True)
    y_ref = bo.block_forward(xr, sd, 4, gamma1=sd["gamma1"], gamma2=sd["gamma2"])
    (y_ref * go.double()).sum().backward()
    xd = x.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        y = blk(xd)
    (y * go.to(dev)).sum().backward()
    assert rel_err(y, y_ref) < tol and rel_err(xd.grad, xr.grad) < tol
    for k, p in blk.named_parameters():
        assert rel_err(p.grad, sd[k].grad) < tol, k


@pytest.mark.parametrize("B,H,W,ws,C", [(2, 5, 9, 4, 64), (1, 28, 28, 14, 128), (3, 20, 31, 14, 32)])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_window_rows_bit_exact(dev, B, H, W, ws, C, dt):
    from metatransformer_amd import ops
    x = torch.randn(B * H * W, C).to(dt)
    gh, gw = -(-H // ws), -(-W // ws)
    grid = torch.zeros(B, gh * ws, gw * ws, C, dtype=dt)
    grid[:, :H, :W] = x.reshape(B, H, W, C)
    ref = grid.reshape(B, gh, ws, gw, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
    win = ops.window_rows(x.to(dev), B, H, W, ws, merge=False)
    assert torch.equal(win.cpu(), ref)
    back = ops.window_rows(win, B, H, W, ws, merge=True)
    assert torch.equal(back.cpu(), x)


@pytest.mark.parametrize("dt,tol", [(torch.float32, TOL_F32), (torch.bfloat16, TOL_BF16_GRAD)])
@pytest.mark.parametrize("H,W,ws", [(20, 31, 14), (28, 28, 14), (9, 5, 4)])
def test_windowed_block_vs_oracle(dev, dt, tol, H, W, ws):
    """row f3: WindowedAttention blocks of the detection backbone (vit.py:148-192, 284-287) -- forward, dL/dx and every
    parameter gradient against autograd through the oracle restatement; grids that are not multiples of the window
    exercise the zero-padded keys"""
    torch.manual_seed(5)
    blk = M.Block(128, 4, qkv_bias=True, windowed=True, window_size=ws).to(dev).train()
    x, go = torch.randn(2, H * W, 128), torch.randn(2, H * W, 128)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in blk.state_dict().items()}
    xr = x.double().requires_grad_(True)
    y_ref = bo.block_forward(xr, sd, 4, window=(H, W, ws))
    (y_ref * go.double()).sum().backward()
    xd = x.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        y = blk(xd, H, W)
    (y * go.to(dev)).sum().backward()
    assert rel_err(y, y_ref) < tol and rel_err(xd.grad, xr.grad) < tol
    for k, p in blk.named_parameters():
        assert rel_err(p.grad, sd[k].grad) < tol, k
    with pytest.raises(M.MetaEncError):
        blk(xd)                                    # the token grid is mandatory for a windowed block


# ----------------------------------------------------------------------------- BASELINE-size properties

def test_base_config2_shape_properties(dev):
    """[256,197,768] bf16 (BASELINE config 2): too big for the CPU oracle in seconds, so check properties that do not
    depend on size: batch independence (sample b of the big batch == the same sample run alone: no kernel reduces
    across samples; equal up to the fp32 summation order of the split-K schedules the GEMM planner picks per problem
    size, i.e. a few bf16 ulps) and agreement of the first samples with the CPU oracle."""
    c = dict(depth=12, dim=768, heads=12, eps=1e-5, seed=14)
    enc = make_encoder(c, dev, torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(256, 197, 768, generator=g).bfloat16()
    with torch.no_grad():
        y = enc(x.to(dev))
        y_sub = enc(x[37:39].to(dev))
    assert torch.isfinite(y.float()).all()
    assert rel_err(y_sub.float(), y[37:39].float()) < TOL_BF16_STREAM12, "batch independence (ulp flips of the bf16 stream only)"
    with torch.no_grad():      # same problem size -> same schedule -> bit-exact run to run
        assert torch.equal(enc(x[37:39].to(dev)), y_sub)
    sd = bo.make_encoder_state_dict(12, 768, seed=14)
    ref = bo.encoder_forward(x[:2].float(), sd, 12)
    check_close(y[:2].float(), ref, TOL_BF16_STREAM12, 'config 2, 12 bf16 layers, bf16 stream')


def test_large_config3_slice_vs_oracle(dev):
    """Large (24L/1024d/16h), N=512 (BASELINE config 3 shape, batch cut to 2 for the CPU oracle)."""
    c = dict(depth=24, dim=1024, heads=16, eps=1e-5, seed=21)
    enc = make_encoder(c, dev)
    x = torch.randn(2, 512, 1024, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        y32 = enc(x.to(dev))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y16 = enc(x.to(dev))
    ref = bo.encoder_forward(x, bo.make_encoder_state_dict(24, 1024, seed=21), 16)
    assert rel_err(y32, ref) < TOL_F32
    assert rel_err(y16, ref) < 1.5e-2       # 24 bf16 layers


def test_large_config5_video_tokens_vs_oracle(dev):
    """BASELINE config 5 shape: VideoMAE tubelet tokens, N = 1568, Large width (4 of the 24 blocks, batch 1 for the CPU
    oracle): forward and input gradient through the tiled (N > 256) attention path"""
    c = dict(depth=4, dim=1024, heads=16, eps=1e-6, seed=23)
    sd = bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"])
    g = torch.Generator().manual_seed(6)
    x, go = torch.randn(1, 1568, 1024, generator=g), torch.randn(1, 1568, 1024, generator=g)
    xr = x.clone().requires_grad_(True)
    y_ref = bo.encoder_forward(xr, sd, 16, eps=1e-6)
    (y_ref * go).sum().backward()
    enc = make_encoder(c, dev)
    for dt, tol in ((torch.float32, TOL_F32), (torch.bfloat16, TOL_BF16_GRAD)):
        xd = x.to(dev).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            y = enc(xd)
        (y * go.to(dev)).sum().backward()
        assert rel_err(y, y_ref) < tol and rel_err(xd.grad, xr.grad) < tol


# ----------------------------------------------------------------------------- tokenizers

def _tok():
    return np.load(os.path.join(GOLDEN, "tokenizers.npz"), allow_pickle=False)


def test_image_tokenizer_matches_reference_golden(dev):
    z = _tok()
    g = torch.Generator().manual_seed(2001)
    pe = M.PatchEmbed(img_size=224, patch_size=16, in_c=3, embed_dim=768)
    pe.proj.weight.data.copy_(0.02 * torch.randn(768, 3, 16, 16, generator=g))
    pe.proj.bias.data.copy_(0.05 * torch.randn(768, generator=g))
    x = torch.randn(2, 3, 224, 224, generator=g)
    pe = pe.to(dev)
    with torch.no_grad():
        y = pe(x.to(dev))
    assert y.shape == (2, 196, 768)
    assert rel_err(y[:, ::7, ::3], torch.from_numpy(z["image/y"])) < TOL_F32
    # BASELINE config 1 plumbing: Data2Seq.Image 224x224 patch16 -> 12-layer/768-d encoder, batch 8, + cls/pos fused
    with torch.no_grad():
        pos = torch.randn(196, 768, device=dev)
        y2 = pe(x.to(dev), pos_embed=pos, prefix_rows=1)
        assert y2.shape == (2, 197, 768) and torch.all(y2[:, 0] == 0)
        assert rel_err(y2[:, 1:], y + pos) < 1e-5
    # gradients of the projection
    pe.train()
    xg = x.to(dev).requires_grad_(True)
    out = pe(xg)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    (out * go.to(dev)).sum().backward()
    conv = nn.Conv2d(3, 768, 16, 16)
    conv.load_state_dict({k.replace("proj.", ""): v.cpu() for k, v in pe.state_dict().items()})
    xc = x.clone().requires_grad_(True)
    (conv(xc).flatten(2).transpose(1, 2) * go).sum().backward()
    assert rel_err(pe.proj.weight.grad, conv.weight.grad) < TOL_F32
    assert rel_err(pe.proj.bias.grad, conv.bias.grad) < TOL_F32
    assert rel_err(xg.grad, xc.grad) < TOL_F32


def test_acoustic_and_video_tokenizers_match_reference_golden(dev):
    z = _tok()
    g = torch.Generator().manual_seed(2002)
    ac = M.AcousticPatchEmbed(embed_dim=768)
    ac.proj.weight.data.copy_(0.02 * torch.randn(768, 1, 16, 16, generator=g))
    ac.proj.bias.data.copy_(0.05 * torch.randn(768, generator=g))
    x = torch.randn(2, 1, 128, 100, generator=g)
    with torch.no_grad():
        y = ac.to(dev)(x.to(dev))
    assert y.shape[1] == int(z["acoustic/tokens"])
    assert rel_err(y[:, ::3, ::3], torch.from_numpy(z["acoustic/y"])) < TOL_F32
    g = torch.Generator().manual_seed(2003)
    vp = M.VideoPatchEmbed(img_size=64, patch_size=16, in_chans=3, embed_dim=768, num_frames=4, tubelet_size=2)
    vp.proj.weight.data.copy_(0.02 * torch.randn(768, 3, 2, 16, 16, generator=g))
    vp.proj.bias.data.copy_(0.05 * torch.randn(768, generator=g))
    x = torch.randn(2, 3, 4, 64, 64, generator=g)
    with torch.no_grad():
        y = vp.to(dev)(x.to(dev))
    assert rel_err(y[:, :, ::3], torch.from_numpy(z["video/y"])) < TOL_F32
    assert np.allclose(M.video_sinusoid_table(32, 768)[0, :, :16].numpy(), z["video/sinusoid_head"], atol=1e-6)


def test_time_series_tokenizer_matches_reference_golden(dev):
    z = _tok()
    ts = M.DataEmbedding(c_in=7, d_model=768).eval()
    ts.value_embedding.tokenConv.weight.data.copy_(torch.from_numpy(z["ts/conv_weight"]))
    ts.value_embedding.tokenConv.weight.requires_grad = False
    ts = ts.to(dev)
    x, mark = torch.from_numpy(z["ts/x"]), torch.from_numpy(z["ts/mark"])
    y = ts(x.to(dev), mark.to(dev))
    assert rel_err(y[:, ::4, ::3], torch.from_numpy(z["ts/y"])) < 1e-5
    assert rel_err(ts(x.to(dev))[:, ::4, ::3], torch.from_numpy(z["ts/y_nomark"])) < 1e-5
    # the temporal gather alone is integer-indexed: with a zero conv weight and no PE term it must be bit-exact
    tabs = [to.sinusoid_table_ts(n, 768) for n in (13, 32, 7, 24)]
    ts.value_embedding.tokenConv.weight.data.zero_()
    ts.position_embedding.pe.zero_()
    m = mark.long()
    exact = ((tabs[3][m[..., 3]] + tabs[2][m[..., 2]]) + tabs[1][m[..., 1]]) + tabs[0][m[..., 0]]
    assert torch.equal(ts(x.to(dev), mark.to(dev)).cpu(), exact)
    bad = mark.clone(); bad[0, 0, 3] = 24
    with pytest.raises(IndexError):
        ts(x.to(dev), bad.to(dev))


@pytest.mark.parametrize("cin,L", [(7, 96), (1, 36), (21, 50)])
def test_time_series_tokenizer_backward_and_dropout(dev, cin, L):
    """the Time-Series pipelines train this tokenizer in front of the frozen encoder (Time-Series/run.py): Conv1d weight
    gradient against autograd through the oracle restatement; training-mode Dropout(0.1) is seeded and unbiased"""
    torch.manual_seed(1)
    B, C = 4, 256
    ts = M.DataEmbedding(c_in=cin, d_model=C).to(dev).eval()
    x = torch.randn(B, L, cin)
    mark = torch.stack([torch.randint(0, n, (B, L)) for n in (13, 32, 7, 24)], dim=-1).float()
    go = torch.randn(B, L, C)
    w = ts.value_embedding.tokenConv.weight.detach().cpu().double().requires_grad_(True)
    tabs = [to.sinusoid_table_ts(n, C).double() for n in (13, 32, 7, 24)]
    ref = to.time_series_embedding(x.double(), w, mark, tabs, to.sinusoid_table_ts(5000, C).double())
    (ref * go.double()).sum().backward()
    y = ts(x.to(dev), mark.to(dev))
    (y * go.to(dev)).sum().backward()
    assert rel_err(y, ref) < 1e-5
    assert rel_err(ts.value_embedding.tokenConv.weight.grad, w.grad) < 1e-5
    # dropout in training mode
    ts.train()
    torch.manual_seed(7); y1 = ts(x.to(dev), mark.to(dev))
    torch.manual_seed(7); y2 = ts(x.to(dev), mark.to(dev))
    assert torch.equal(y1, y2)
    kept = (y1 != 0)
    assert 0.85 < kept.float().mean().item() < 0.95
    assert torch.allclose(y1[kept], (y.detach() / 0.9)[kept], rtol=1e-5, atol=1e-6)
    ts.value_embedding.tokenConv.weight.grad = None
    torch.manual_seed(7); (ts(x.to(dev), mark.to(dev)) * go.to(dev)).sum().backward()
    g_drop = ts.value_embedding.tokenConv.weight.grad
    # same masks in backward: dW equals the oracle's gradient for the masked, rescaled upstream gradient
    w2 = w.detach().clone().requires_grad_(True)
    ref2 = to.time_series_embedding(x.double(), w2, mark, tabs, to.sinusoid_table_ts(5000, C).double())
    (ref2 * (go.double() * kept.cpu().double() / 0.9)).sum().backward()
    assert rel_err(g_drop, w2.grad) < 1e-5


def test_tokenizers_fp16_boundary_and_mark_device(dev):
    """fp16 at the tokenizer boundary follows Block's rule (Audio/src/traintest.py trains under autocast(float16)): fp16 in /
    out, bf16 compute; a time-mark tensor on the wrong device is rejected before its pointer reaches a kernel."""
    torch.manual_seed(3)
    pe = M.PatchEmbed(img_size=64, patch_size=16, in_c=3, embed_dim=256).to(dev)
    x = torch.randn(2, 3, 64, 64, device=dev)
    with torch.no_grad():
        ref = pe(x)
        with torch.autocast("cuda", dtype=torch.float16):
            y = pe(x)
    assert y.dtype == torch.float16 and rel_err(y.float(), ref) < 1e-2
    # a .half() module with fp16 input, forward and backward
    ph = M.PatchEmbed(img_size=64, patch_size=16, in_c=3, embed_dim=256).to(dev)
    ph.load_state_dict(pe.state_dict())
    ph = ph.half()
    xh = x.half().requires_grad_(True)
    yh = ph(xh)
    assert yh.dtype == torch.float16 and rel_err(yh.float(), ref) < 1e-2
    go = torch.randn_like(ref)
    (yh.float() * go).sum().backward()
    xr = x.clone().requires_grad_(True)
    (pe(xr) * go).sum().backward()
    assert xh.grad.dtype == torch.float16 and ph.proj.weight.grad.dtype == torch.float16
    assert rel_err(xh.grad.float(), xr.grad) < 2e-2 and rel_err(ph.proj.weight.grad.float(), pe.proj.weight.grad) < 2e-2
    ts = M.DataEmbedding(c_in=7, d_model=256).to(dev).eval()
    xs = torch.randn(2, 48, 7, device=dev)
    mark = torch.stack([torch.randint(0, n, (2, 48)) for n in (13, 32, 7, 24)], dim=-1).float()
    with torch.no_grad():
        r32 = ts(xs, mark.to(dev))
        with torch.autocast("cuda", dtype=torch.float16):
            r16 = ts(xs, mark.to(dev))
    assert r16.dtype == torch.float16 and rel_err(r16.float(), r32) < 1e-2
    with pytest.raises(M.MetaEncError, match="x_mark is on"):
        ts(xs, mark)                                      # CPU marks


def test_multimodal_concat_through_encoder(dev):
    """README.md:118-149 demo: tokens of several modalities concatenated along N, one shared encoder."""
    torch.manual_seed(0)
    img_tok = M.Data2Seq("image", 768).to(dev).eval()
    ts_tok = M.Data2Seq("time-series", 768, c_in=7).to(dev).eval()
    au_tok = M.Data2Seq("audio", 768).to(dev).eval()
    ts_tok.embed.value_embedding.tokenConv.weight.requires_grad = False
    enc = make_encoder(dict(depth=2, dim=768, heads=12, eps=1e-5, seed=4), dev)
    img, ts, spec = torch.randn(2, 3, 224, 224), torch.randn(2, 96, 7), torch.randn(2, 1, 128, 100)
    with torch.no_grad():
        feats = torch.concat([img_tok(img.to(dev)), ts_tok(ts.to(dev)), au_tok(spec.to(dev))], dim=1)
        assert feats.shape == (2, 196 + 96 + 108, 768)
        y = enc(feats)
        ref = bo.encoder_forward(feats.cpu(), bo.make_encoder_state_dict(2, 768, seed=4), 12)
    assert rel_err(y, ref) < TOL_F32


# ---------------------------------------------------------------- Block variants pinned to the reference's own classes
# (tests/golden/variants.npz: outputs of Video/models/modeling_finetune.py Block and Image/detection/.../base/vit.py Block,
#  generated by oracle/make_golden.py in the build container)
def _variants():
    return np.load(os.path.join(GOLDEN, "variants.npz"))


def _variant_sd(z, tag):
    pre = f"{tag}/w/"
    return {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}


def _check_param_grads(z, tag, grads, tol_rel):
    for k, g in grads.items():
        st = z[f"{tag}/dw_stats/{k}"]
        gd = g.detach().double().cpu()
        assert abs(gd.abs().sum().item() - st[1]) <= tol_rel * st[1], (k, gd.abs().sum().item(), st[1])
        head = torch.from_numpy(z[f"{tag}/dw_head/{k}"])
        assert rel_err(g.detach().flatten()[:head.numel()].reshape(head.shape).float(), head) < 10 * tol_rel, k


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_video_block_matches_reference_golden(dev, dt):
    """VideoMAE-style block: q/v-only bias, q pre-scaled, gamma_1 / gamma_2 -- through the state-dict adapter."""
    from functools import partial
    z = _variants()
    ref_sd = _variant_sd(z, "video")
    blk = M.Block(128, 2, qkv_bias=True, layer_scale=True, norm_layer=partial(nn.LayerNorm, eps=1e-6))
    blk.load_state_dict(M.convert_video_state_dict(ref_sd), strict=True)
    assert set(M.to_video_state_dict(blk.state_dict())) == set(ref_sd)          # the adapter round-trips the key set
    blk = blk.to(dev).train()
    x = torch.from_numpy(z["video/x"]).to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        y = blk(x)
    (y * torch.from_numpy(z["video/go"]).to(dev)).sum().backward()
    tf, tg = (TOL_F32, TOL_F32) if dt == torch.float32 else (TOL_BF16_FWD, TOL_BF16_GRAD)
    check_close(y.float(), torch.from_numpy(z["video/y"]), tf, "video block y")
    check_close(x.grad.float(), torch.from_numpy(z["video/dx"]), tg, "video block dx")
    grads = M.to_video_state_dict({k: p.grad for k, p in blk.named_parameters()})
    _check_param_grads(z, "video", grads, 2e-3 if dt == torch.float32 else 2e-2)
    kb = blk.attn.qkv.bias.grad[128:256]                                       # no K bias in the reference: its gradient is ~0
    assert kb.abs().max() < 1e-3 * blk.attn.qkv.bias.grad.abs().max()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tag", ["det_win", "det_full"])
def test_detection_blocks_match_reference_golden(dev, tag, dt):
    """layer-scale block with WindowedAttention (4 x 4 windows on a ragged 9 x 11 grid) / global attention, loaded
    strict=True from the reference's own key set and called the reference's way: blk(x, H, W)."""
    from functools import partial
    z = _variants()
    H, W, ws = (int(v) for v in z[f"{tag}/hw"])
    blk = M.Block(128, 2, qkv_bias=True, layer_scale=True, windowed=ws > 0, window_size=ws or 14,
                  norm_layer=partial(nn.LayerNorm, eps=1e-6))
    blk.load_state_dict(_variant_sd(z, tag), strict=True)
    blk = blk.to(dev).train()
    x = torch.from_numpy(z[f"{tag}/x"]).to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        y = blk(x, H, W)
    (y * torch.from_numpy(z[f"{tag}/go"]).to(dev)).sum().backward()
    tf, tg = (TOL_F32, TOL_F32) if dt == torch.float32 else (TOL_BF16_FWD, TOL_BF16_GRAD)
    check_close(y.float(), torch.from_numpy(z[f"{tag}/y"]), tf, tag + " y")
    check_close(x.grad.float(), torch.from_numpy(z[f"{tag}/dx"]), tg, tag + " dx")
    _check_param_grads(z, tag, {k: p.grad for k, p in blk.named_parameters()}, 2e-3 if dt == torch.float32 else 2e-2)


def test_windowed_base_block_matches_reference_golden(dev):
    """Base width, 14 x 14 windows on a 20 x 30 grid (the detection backbone's shape class), fp32 and bf16 forward."""
    from functools import partial
    z = _variants()
    sd = bo.make_encoder_state_dict(1, 768, seed=3004)
    assert abs(bo.state_dict_checksum(sd) - float(z["det_win_base/weights_checksum"])) < 1e-6
    blk = M.Block(768, 12, qkv_bias=True, layer_scale=True, windowed=True, window_size=14, norm_layer=partial(nn.LayerNorm, eps=1e-6))
    blk.load_state_dict({**{k[2:]: v for k, v in sd.items()}, "gamma1": torch.from_numpy(z["det_win_base/gamma1"]),
                         "gamma2": torch.from_numpy(z["det_win_base/gamma2"])}, strict=True)
    blk = blk.to(dev).eval()
    g = torch.Generator().manual_seed(3004)
    torch.rand(768, generator=g); torch.rand(768, generator=g)                 # (the two gamma draws of the generator script)
    x = torch.randn(1, 600, 768, generator=g).to(dev)
    ref = torch.from_numpy(z["det_win_base/y"])
    with torch.no_grad():
        y = blk(x, 20, 30)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y16 = blk(x, 20, 30)
    check_close(y[:, ::5, ::3], ref, TOL_F32, "windowed base fp32")
    check_close(y16[:, ::5, ::3].float(), ref, TOL_BF16_FWD, "windowed base bf16")


def test_resize_pos_embed_matches_reference_golden(dev):
    """a16: TIMMVisionTransformer.resize_pos_embed (vit.py:459-486) -- cls row kept bit-exactly, grid resampled."""
    z = _variants()
    pos = torch.from_numpy(z["resize/pos"]).to(dev)
    for tag, shp, mode in (("up", (20, 24), "bicubic"), ("down", (10, 7), "bicubic"), ("bilinear_up", (20, 24), "bilinear")):
        out = M.resize_pos_embed(pos, shp, (14, 14), mode)
        ref = torch.from_numpy(z[f"resize/{tag}"])
        assert out.shape == ref.shape and torch.equal(out[:, 0].cpu(), ref[:, 0])
        assert rel_err(out, ref) < 1e-5, tag
    # identity resize returns the table itself (up to fp32 rounding of weights that are exactly 0 / 1)
    same = M.resize_pos_embed(pos, (14, 14), (14, 14), "bicubic")
    assert rel_err(same, pos) < 1e-6
    with pytest.raises(M.MetaEncError):
        M.resize_pos_embed(pos.cpu(), (20, 24), (14, 14))


# ---------------------------------------------------------------- full-size backward parity
@pytest.mark.slow
def test_base_config2_full_batch_backward_vs_oracle(dev):
    """BASELINE config 2 at FULL size: B = 256, N = 197, 12 x 768 -- dL/dx of every sample and all 144 parameter gradients
    (weight gradients reduce over 50 432 rows: split-K inside the Block path, bias-colsum fusion, in-place flat accumulation)
    against the CPU oracle's autograd.  The oracle runs the batch in chunks of 32 samples and sums the parameter gradients
    (the loss is a sum over samples, so that is exact)."""
    from metatransformer_amd import parallel
    L, C, Hh, B, N = 12, 768, 12, 256, 197
    sd = bo.make_encoder_state_dict(L, C, seed=77)
    g = torch.Generator().manual_seed(78)
    x = torch.randn(B, N, C, generator=g)
    go = torch.randn(B, N, C, generator=g) / (B * N) ** 0.5
    enc = M.build_encoder(L, C, Hh)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).train()
    for blk in enc:
        blk.compute_dtype = torch.bfloat16
    flat = parallel.FlatParams(enc.named_parameters(), no_decay=parallel.no_decay_rule)       # the bench's configuration
    xd = x.to(dev).bfloat16().requires_grad_(True)
    flat.zero_grad()
    y = enc(xd)
    y.backward(go.to(dev).bfloat16())
    torch.cuda.synchronize()
    # oracle on the SAME bf16-rounded inputs, fp32 arithmetic
    xr, gor = x.bfloat16().float(), go.bfloat16().float()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    dx_ref = torch.empty_like(xr)
    y_ref = torch.empty_like(xr)
    torch.set_num_threads(max(1, min(64, len(os.sched_getaffinity(0)))))
    for i in range(0, B, 32):
        xs = xr[i:i + 32].clone().requires_grad_(True)
        ys = bo.encoder_forward(xs, params, Hh)
        (ys * gor[i:i + 32]).sum().backward()
        dx_ref[i:i + 32] = xs.grad
        y_ref[i:i + 32] = ys.detach()
    check_close(y.float(), y_ref, TOL_BF16_STREAM12, "config 2 y (12 bf16 layers, bf16 stream)")
    assert rel_err(xd.grad.float(), dx_ref) < TOL_BF16_STREAM12         # dL/dx through 12 layers of bf16 stream (measured 1.7e-2)
    worst = {}
    for k, p in enc.named_parameters():
        e = rel_err(p.grad, params[k].grad)
        worst[k.split(".", 1)[1]] = max(worst.get(k.split(".", 1)[1], 0.0), e)
        # per element too: an error confined to a few columns of a weight gradient -- a wrong tail tile
        # of the split-K fold, a dropped slab -- sits far below the tensor's max-abs scale
        check_close(p.grad, params[k].grad, TOL_BF16_STREAM12, f"config 2 d{k}")
    print("config-2 full-batch gradient errors (worst over layers):", {k: f"{v:.1e}" for k, v in worst.items()})
    for k, e in worst.items():
        assert e < TOL_BF16_STREAM12, (k, e)


def test_large_config3_backward_vs_oracle(dev):
    """config 3 shape class (Large, N = 512): dL/dx and every parameter gradient of a 2-block slice, batch 3."""
    sd = bo.make_encoder_state_dict(2, 1024, seed=31)
    g = torch.Generator().manual_seed(32)
    x, go = torch.randn(3, 512, 1024, generator=g), torch.randn(3, 512, 1024, generator=g)
    y_ref, dx_ref, dp_ref = bo.encoder_forward_backward(x, sd, 16, go)
    for dt, tf, tg in ((torch.float32, TOL_F32, TOL_F32), (torch.bfloat16, TOL_BF16_FWD, TOL_BF16_GRAD)):
        enc = M.build_encoder(2, 1024, 16)
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(dev).train()
        xr = x.to(dev).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            y = enc(xr)
        (y * go.to(dev)).sum().backward()
        check_close(y.float(), y_ref, tf, f"config 3 y {dt}")
        check_close(xr.grad.float(), dx_ref, tg, f"config 3 dx {dt}")
        for k, p in enc.named_parameters():
            check_close(p.grad, dp_ref[k], tg, f"config 3 d{k} {dt}")


@pytest.mark.slow
@pytest.mark.parametrize("L,C,Hh,B,N", [(2, 1024, 16, 32, 1568), (2, 1024, 16, 128, 512), (2, 768, 12, 64, 592)], ids=["config5", "config3", "config4"])
def test_configs_3_4_5_full_batch_backward_vs_oracle(dev, L, C, Hh, B, N):
    """BASELINE config 5 (and 3, 4) at the batch bench.py runs it at -- tokens [32, 1568, 1024], Large width, 16 heads ([128, 512, 1024];
    [64, 592, 768] Base: the sequence-concat reading of config 4) -- through a 2-block slice in bf16
    (bf16 token stream, the bench's configuration): y, dL/dx of every sample and all 24 parameter gradients against the CPU oracle in fp32
    on the same bf16-rounded inputs (batch in chunks of 4 samples, parameter gradients summed: the loss is a sum over samples).  This is the
    size at which the resident GEMMs run K = 1024 / 4096, the weight gradients reduce over 50 176 rows and the streaming attention kernels
    walk 14 items per workgroup (the 32-key dK / dV kernel)."""
    from metatransformer_amd import parallel
    sd = bo.make_encoder_state_dict(L, C, seed=91)
    g = torch.Generator().manual_seed(92)
    x = torch.randn(B, N, C, generator=g)
    go = torch.randn(B, N, C, generator=g) / (B * N) ** 0.5
    enc = M.build_encoder(L, C, Hh)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).train()
    for blk in enc:
        blk.compute_dtype = torch.bfloat16
    flat = parallel.FlatParams(enc.named_parameters(), no_decay=parallel.no_decay_rule)
    xd = x.to(dev).bfloat16().requires_grad_(True)
    flat.zero_grad()
    y = enc(xd)
    y.backward(go.to(dev).bfloat16())
    torch.cuda.synchronize()
    xr, gor = x.bfloat16().float(), go.bfloat16().float()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    dx_ref, y_ref = torch.empty_like(xr), torch.empty_like(xr)
    torch.set_num_threads(max(1, min(64, len(os.sched_getaffinity(0)))))
    ch = max(1, 8192 // N)                              # ~8 k tokens per oracle chunk
    for i in range(0, B, ch):
        xs = xr[i:i + ch].clone().requires_grad_(True)
        ys = bo.encoder_forward(xs, params, Hh)
        (ys * gor[i:i + ch]).sum().backward()
        dx_ref[i:i + ch] = xs.grad
        y_ref[i:i + ch] = ys.detach()
    check_close(y.float(), y_ref, TOL_BF16_STREAM1, f"[{B},{N},{C}] y (2 bf16 layers, bf16 stream)")
    check_close(xd.grad.float(), dx_ref, TOL_BF16_GRAD, f"[{B},{N},{C}] dx")
    worst = {}
    for k, p in enc.named_parameters():
        worst[k.split(".", 1)[1]] = max(worst.get(k.split(".", 1)[1], 0.0), rel_err(p.grad, params[k].grad))
        check_close(p.grad, params[k].grad, TOL_BF16_GRAD, f"[{B},{N},{C}] d{k}")
    print(f"[{B},{N},{C}] full-batch gradient errors (worst over the 2 layers):", {k: f"{v:.1e}" for k, v in worst.items()})


def test_block_with_fp8_attention_config5_shape(dev):
    """BASELINE config 5's block (Large: 1024-d, 16 heads) on video-length sequences with attn_fp8: forward against the fp32
    oracle, backward (bf16 kernels on the saved bf16 qkv with the fp8 forward's LSE) against the oracle's gradients."""
    sd = bo.make_encoder_state_dict(1, 1024, seed=55)
    g = torch.Generator().manual_seed(56)
    x, go = torch.randn(2, 1568, 1024, generator=g), torch.randn(2, 1568, 1024, generator=g)
    y_ref, dx_ref, dp_ref = bo.encoder_forward_backward(x, sd, 16, go)
    enc = M.build_encoder(1, 1024, 16)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).train()
    enc[0].attn_fp8 = True
    xr = x.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = enc(xr)
    (y * go.to(dev)).sum().backward()
    assert rel_err(y, y_ref) < 1e-2 and rel_err(xr.grad, dx_ref) < 3e-2
    for k, p in enc.named_parameters():
        check_close(p.grad, dp_ref[k], 3e-2, f"config 5 block d{k} (fp8 attention forward)")
    enc[0].attn_fp8 = False
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y16 = enc(x.to(dev))
    assert rel_err(y16, y_ref) < TOL_BF16_FWD          # the bf16 attention on the same block, for scale


# ---------------------------------------------------------------- LayerNorm folded into the Linear behind it (inference)
@pytest.mark.parametrize("M_rows,N_out,act", [(8192, 2304, False), (8192, 3072, True), (333, 64, False), (64 * 197, 3072, True)])
def test_gemm_with_folded_layernorm_matches_layernorm_then_linear(dev, M_rows, N_out, act):
    """me_row_stats + me_gemm(row_affine, col_shift) == Linear(LayerNorm(x)) [+ GELU] (attention.py:56 / mlp.py:29-31), resident
    and generic kernel families, token stream with a mean offset well above its spread (the rank-1 correction must cancel it)"""
    from metatransformer_amd import ops
    from metatransformer_amd._capi import ME_ACT_GELU, ME_ACT_NONE
    g = torch.Generator().manual_seed(M_rows + N_out)
    K = 768
    x = (torch.randn(M_rows, K, generator=g) * torch.rand(M_rows, 1, generator=g) * 2 + 3.0 * torch.randn(M_rows, 1, generator=g)).bfloat16()
    w, b = torch.randn(N_out, K, generator=g) * 0.03, torch.randn(N_out, generator=g) * 0.1
    ln_w, ln_b = 1.0 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x.double(), (K,), ln_w.double(), ln_b.double(), 1e-6), w.double(), b.double())
    if act:
        ref = torch.nn.functional.gelu(ref)
    wf = (w * ln_w[None, :]).bfloat16()
    s_vec, c_vec = wf.float().sum(1), w @ ln_b + b
    xd = x.to(dev)
    st = ops.row_stats(xd, 1e-6)
    mean, var = x.double().mean(1), x.double().var(1, unbiased=False)
    rstd = (var + 1e-6).rsqrt()
    assert rel_err(st[:, 0], rstd) < 1e-5 and float((st[:, 1].double().cpu() + rstd * mean).abs().max()) < 1e-4 * float((rstd * mean).abs().max() + 1)
    y = ops.gemm(xd, wf.to(dev), bias=c_vec.to(dev), act=ME_ACT_GELU if act else ME_ACT_NONE, row_affine=st, col_shift=s_vec.to(dev))
    assert y.dtype == torch.bfloat16
    check_close(y.float(), ref, TOL_BF16, f"folded LN GEMM M={M_rows} N={N_out}")


@pytest.mark.parametrize("name", ["base_1blk", "base_12blk", "large_2blk"])
def test_inference_with_folded_layernorm_matches_reference_golden(dev, name):
    """bf16 parameters + bf16 token stream + no_grad: norm1 / norm2 are folded into qkv / fc1 (Block.fold_norm).  Same bound
    as the unfolded bf16 stream, the folded and unfolded outputs agree to bf16 noise, and the one-call serving entry point
    (me_encoder_fwd) takes the same path."""
    z, c = golden(name)
    x, _ = _inputs(c)
    enc = make_encoder(c, dev, torch.bfloat16)
    xd = x.to(dev).bfloat16()
    tol = TOL_BF16_STREAM12 if c["depth"] > 2 else TOL_BF16_STREAM1
    for b in enc:
        b.fold_norm = "always"                         # (the default folds only where the resident GEMM takes the shape)
    with torch.no_grad():
        y_fold = enc(xd)
        y_one = M.encoder_forward_inference(enc, xd)
        for b in enc:
            b.fold_norm = False
        y_plain = enc(xd)
    ref = torch.from_numpy(z["y"])
    s = c["tok_stride"]
    check_close(y_fold[:, ::s].float(), ref, tol, name + " folded")
    check_close(y_plain[:, ::s].float(), ref, tol, name + " unfolded")
    assert torch.equal(y_one, y_fold)
    # folded against unfolded: two bf16 evaluations of the same arithmetic.  One or two blocks: bf16 rounding noise (measured
    # 6.0e-3 / 6.1e-3 of max-abs: the output is rounded once per block) -> bound 8e-3, where a fold-specific error of 1e-2 would
    # show.  Through 12 blocks the two bf16 streams drift apart as any two bf16 evaluations do (measured 1.7e-2, either is
    # 1.3 - 2.1e-2 from the fp32 reference) -> bound 2.5e-2 (was the 3e-2 of the reference comparison)
    ff = rel_err(y_fold.float(), y_plain.float())
    print(f"folded vs unfolded ({name}): {ff:.2e}")
    assert ff < (TOL_BF16_OP if c["depth"] <= 2 else 2.5e-2)
    assert not torch.equal(y_fold, y_plain)            # (they are different kernels: identical bits would mean the fold is off)
    # a weight update invalidates the folded copies
    with torch.no_grad():
        enc[0].norm1.weight.mul_(1.5)
        for b in enc:
            b.fold_norm = "always"
        y2 = enc(xd)
    assert rel_err(y2.float(), y_fold.float()) > 1e-3


@pytest.mark.parametrize("K,offset", [(768, 0.0), (3072, 0.0), (768, 40.0)])
def test_residual_gemm_emits_row_statistics(dev, K, offset):
    """me_gemm_desc.row_stats: the proj / fc2 launches leave per-row (mean, M2) partials of their OUTPUT over 256-column groups;
    me_row_stats_combine folds them into the pairs me_row_stats computes from the stored tensor.  `offset`: rows whose mean is
    hundreds of times their spread (the shifted sums must not cancel, and the statistics must be those of the bf16 values as
    stored).  The output itself is bit-identical to the same launch without statistics."""
    from metatransformer_amd import ops
    M_rows, N = 22016 + 37, 768                    # 87 x 3 tiles: every CU gets one (the resident kernel), ragged last row tile
    g = torch.Generator().manual_seed(K + int(offset))
    a = torch.randn(M_rows, K, generator=g).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().to(dev)
    b = (0.1 * torch.randn(N, generator=g)).to(dev)
    res = (torch.randn(M_rows, N, generator=g) * torch.rand(M_rows, 1, generator=g) + offset * torch.randn(M_rows, 1, generator=g)).bfloat16().to(dev)
    y0 = ops.gemm(a, w, bias=b, residual=res)
    y, part = ops.gemm(a, w, bias=b, residual=res, want_row_stats=True)
    assert part is not None and part.shape == (N // 256, M_rows, 2)
    assert torch.equal(y, y0)
    yd = y.double()
    for i in range(N // 256):                      # every partial against the stored values of its 256 columns (one output tile)
        blk = yd[:, 256 * i:256 * i + 256]
        mean, m2 = blk.mean(1), ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1)
        assert float((part[i, :, 0].double() - mean).abs().max()) <= 2e-6 * float(blk.abs().max()), i
        assert float((part[i, :, 1].double() - m2).abs().max()) <= 2e-5 * float(m2.max()) + 1e-9, i
    st = ops.row_stats_combine(part, 1e-6)
    ref = ops.row_stats(y, 1e-6)
    rstd = (yd.var(1, unbiased=False) + 1e-6).rsqrt()
    assert rel_err(st[:, 0], rstd) < 2e-5 and rel_err(ref[:, 0], rstd) < 2e-5
    assert float((st[:, 1].double() + rstd * yd.mean(1)).abs().max()) <= 1e-4 * float((rstd * yd.mean(1)).abs().max() + 1)
    # shapes the resident kernel does not take report "no statistics" instead of failing
    ys, none = ops.gemm(a[:4096], w, bias=b, residual=res[:4096], want_row_stats=True)
    assert none is None and torch.equal(ys, ops.gemm(a[:4096], w, bias=b, residual=res[:4096]))


def test_inference_chains_layernorm_statistics_between_blocks(dev):
    """Folded inference at a batch the resident GEMMs take: norm2's statistics come out of the proj epilogue, the next block's
    norm1 statistics ride on the output tensor (Block.forward tags it), me_encoder_fwd chains them on the C side -- same bits --
    and everything agrees with the un-chained folded route (me_row_stats passes) to bf16 noise and with the fp32 oracle."""
    from metatransformer_amd import ops
    c = dict(depth=3, dim=768, heads=12, eps=1e-6, seed=41)
    enc = make_encoder(c, dev, torch.bfloat16)
    B, N = 112, 197                                # 22 064 rows: 87 x 3 tiles of proj / fc2
    x = torch.randn(B, N, 768, generator=torch.Generator().manual_seed(9)).bfloat16().to(dev)
    with torch.no_grad():
        attrs = [set(vars(blk)) for blk in enc]
        y = enc(x)
        # the hand-over between Block.forward and the autograd Function is per call: a forward leaves nothing on the module
        assert [set(vars(blk)) for blk in enc] == attrs and not any(a in s for s in attrs for a in ("_stats_in", "_stats_out"))
        tag = getattr(y, "_me_ln_stats", None)
        assert tag is not None and tag[1] == 1e-6                       # the last block left the statistics of its output
        want = ops.row_stats(y.reshape(B * N, 768), 1e-6)
        got = ops.row_stats_combine(tag[0], 1e-6)                       # (round 6: the fc2 partials themselves travel; the next qkv GEMM folds them)
        assert rel_err(got[:, 0], want[:, 0]) < 2e-5 and float((got[:, 1] - want[:, 1]).abs().max()) < 1e-4 * float(want[:, 1].abs().max() + 1)
        y_one = M.encoder_forward_inference(enc, x)
        assert torch.equal(y_one, y)
        # un-chained: a fresh tensor object between the blocks carries no statistics -> every block reads its input (me_row_stats)
        h = x
        for blk in enc:
            h = blk(h.clone())
        ff = rel_err(h.float(), y.float())
        print(f"chained vs un-chained statistics: {ff:.2e}")
        assert ff < TOL_BF16_OP
        # an in-place edit of a tagged tensor invalidates the tag (the version moves)
        h1 = enc[0](x)
        h1.mul_(2.0)
        h2 = enc[1](h1)
        assert rel_err(h2.float(), enc[1](h1.clone()).float()) < 1e-6
    sd = bo.make_encoder_state_dict(c["depth"], c["dim"], seed=c["seed"])
    y_ref = bo.encoder_forward(x[:4].float().cpu(), {k: v.bfloat16().float() for k, v in sd.items()}, c["heads"], c["eps"])
    check_close(y[:4].float(), y_ref, TOL_BF16_STREAM12, "chained folded inference vs the oracle")


def test_graph_capture_replays_on_other_streams(dev):
    """a captured forward at a batch the resident GEMM takes must not share claimed-tile counters between replays.
    Captured launches run the static schedule; replays on two other streams, back to back with eager work, reproduce eager."""
    enc = make_encoder(dict(depth=2, dim=768, heads=12, eps=1e-5, seed=21), dev, torch.bfloat16)
    x = torch.randn(128, 197, 768, generator=torch.Generator().manual_seed(3)).to(dev).bfloat16()
    with torch.no_grad():
        y = enc(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            enc(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            yg = enc(x)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for st in (s1, s2, s1):
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                g.replay()
                outs.append(yg.clone())
            y_eager = enc(x)                                   # eager work on the default stream next to the replay
            torch.cuda.current_stream().wait_stream(st)
            assert torch.equal(y_eager, y)
        torch.cuda.synchronize()
    assert all(torch.equal(o, y) for o in outs)


@pytest.mark.parametrize("mode", ["fp32", "autocast"])
def test_data_parallel_replicas_share_the_weight_cache(dev, mode):
    """nn.DataParallel call site (Audio/src/traintest.py:45-46): replicas are shallow copies of the Blocks that share one
    weight-copy cache and run in threads.  Two replicas on the one visible GPU exercise exactly that; outputs and gradients
    must equal the plain module's."""
    c = dict(depth=2, dim=128, heads=4, eps=1e-5, seed=31)
    enc = make_encoder(c, dev).train()
    dp = torch.nn.DataParallel(enc, device_ids=[0, 0])
    g = torch.Generator().manual_seed(8)
    x, go = torch.randn(6, 40, 128, generator=g).to(dev), torch.randn(6, 40, 128, generator=g).to(dev)
    ac = mode == "autocast"
    xr = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
        y_ref = enc(xr)
    (y_ref * go).sum().backward()
    want = {k: p.grad.clone() for k, p in enc.named_parameters()}
    dx_want = xr.grad.clone()
    for p in enc.parameters():
        p.grad = None
    for it in range(2):                                    # twice: the second pass hits the warm shared cache
        xd = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
            y = dp(xd)
        (y * go).sum().backward()
        tol = 2e-2 if ac else 1e-4                         # (two half batches: wgrad sums in a different order)
        assert rel_err(y, y_ref) < (5e-3 if ac else 1e-5) and rel_err(xd.grad, dx_want) < tol
        for k, p in enc.named_parameters():
            assert rel_err(p.grad, want[k]) < tol, (it, k)
            p.grad = None
