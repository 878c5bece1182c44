"""GPU: the row kernels of csrc/conv_rows.hip, SpatialPriorModule and ViTAdapter.

Ops: against a float64 restatement with torch.nn.functional on the CPU.  Bound per tensor (rule of tests/test_gpu_msda.py):
max |got - f64| / max |f64| <= min(max(4 x ref_err, OP_FLOOR), TOL_F32), ref_err being the distance of the same restatement
evaluated in float32 on the CPU.  OP_FLOOR = 2^-22 = four float32 roundings (2^-24 each, relative to the tensor's largest
magnitude): a pure selection or permutation has ref_err 0 and must then be exact up to the few additions the backward makes.
Index outputs are compared with torch.equal.
conv3x3_rows contracts fp32 operands 128 columns at a time (linear._gemm_nt_chunked): as one me_gemm call the K = 576 forward
measured 4.07 x ref_err, outside this bound.

Fixture cases (tests/golden/vit_adapter.npz, tools/make_vit_adapter_golden.py): max |got - f64| / max |f64| <=
min(4 x ref_err, TOL_F32), with a floor of BLOCK_FP32_FLOOR where encoder Blocks are inside; under bf16 autocast
4 x ref_err_bf16.  Every comparison prints a `VITADAPTER_PARITY` line first (pytest -s; profiles/vit_adapter_parity.txt).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, TOL_BF16_OP, TOL_F32, check_close

import metatransformer_amd as M
from metatransformer_amd import adapter
import msda_cases as mc
import vit_adapter_cases as vc

pytestmark = pytest.mark.gpu

BLOCK_FP32_FLOOR = 1e-6        # what the exact-fp32 Block path measures against its own fixtures (tests/test_gpu_msda.py)
OP_FLOOR = 2.0 ** -22


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "vit_adapter.npz"), allow_pickle=False)


def _report(case, err, ref_err):
    print(f"VITADAPTER_PARITY {case}: err {err:.3e} ref_err {ref_err:.3e} ratio {err / max(ref_err, 1e-30):.2f}")


def compare(gold, key, got, floor=0.0, which="ref_err"):
    a = got.detach().double().cpu().reshape(-1)
    idx = np.append(mc.subset_index(a.numel()), int(gold[key + "/argmax"]))
    ref = torch.from_numpy(gold[key])
    assert ref.numel() == idx.size, key
    ref_err = float(gold[key + "/" + which])
    sub = a[torch.from_numpy(idx)]
    _report(key + ("" if which == "ref_err" else " (bf16 autocast)"), float((sub - ref).abs().max() / ref.abs().max()), ref_err)
    check_close(sub, ref, 4.0 * ref_err if which != "ref_err" else min(max(4.0 * ref_err, floor), TOL_F32), key)


def compare_op(case, got, exact, ref32, tol=None):
    scale = float(exact.abs().max())
    ref_err = float((ref32.double() - exact).abs().max()) / scale
    _report(case, float((got.detach().double().cpu() - exact).abs().max()) / scale, ref_err)
    check_close(got, exact, tol if tol is not None else min(max(4.0 * ref_err, OP_FLOOR), TOL_F32), case)


def rows_of(img):
    """[B, C, H, W] -> [B*H*W, C]"""
    return img.permute(0, 2, 3, 1).reshape(-1, img.shape[1]).contiguous()


def image_of(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def distinct(shape, seed):
    """distinct values in (-1, 1), exact in fp32, in a shuffled order"""
    n = int(np.prod(shape))
    perm = np.argsort(mc.uniform((n,), seed, bits=30), kind="stable")
    return torch.from_numpy(((perm.astype(np.float64) - n / 2) / n).astype(np.float32).reshape(shape))


def U(shape, *names):
    return torch.from_numpy(mc.uniform(tuple(shape), mc.seed_of("vit_adapter_ops", *names)))


def grads_of(fn, inputs, dout):
    leaves = [t.detach().clone().requires_grad_() for t in inputs]
    out = fn(*leaves)
    out.backward(dout.to(out.dtype).to(out.device))
    return [out.detach()] + [t.grad for t in leaves]


# ----------------------------------------------------------------------------- ops
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin,cout,B,H,W", [(3, 16, 2, 13, 18), (3, 64, 1, 32, 20), (64, 64, 2, 9, 12), (128, 72, 1, 7, 10), (256, 256, 1, 8, 5)])
def test_conv3x3_rows_matches_conv2d(dev, stride, cin, cout, B, H, W):
    x, w = U((B, cin, H, W), "conv", cin, stride, "x"), U((cout, cin, 3, 3), "conv", cin, stride, "w") * (cin * 9) ** -0.5
    Ho, Wo = adapter.conv_out_size(H, stride), adapter.conv_out_size(W, stride)
    dy = U((B, cout, Ho, Wo), "conv", cin, stride, "dy")
    ref = lambda dt: grads_of(lambda a, b: F.conv2d(a, b, stride=stride, padding=1), (x.to(dt), w.to(dt)), dy)      # noqa: E731
    e, r = ref(torch.float64), ref(torch.float32)
    assert e[0].shape == (B, cout, Ho, Wo)
    got = grads_of(lambda a, b: M.conv3x3_rows(a, b, B, H, W, stride), (rows_of(x).to(dev), w.to(dev)), rows_of(dy))
    assert got[0].dtype == torch.float32 and got[0].shape == (B * Ho * Wo, cout)
    compare_op(f"conv3x3 s{stride} cin{cin} y", image_of(got[0].cpu(), B, Ho, Wo), e[0], r[0])
    compare_op(f"conv3x3 s{stride} cin{cin} dx", image_of(got[1].cpu(), B, H, W), e[1], r[1])
    compare_op(f"conv3x3 s{stride} cin{cin} dw", got[2], e[2], r[2])


@pytest.mark.parametrize("stride,cin", [(1, 64), (2, 3)])
def test_conv3x3_rows_bf16(dev, stride, cin):
    B, H, W, cout = 2, 11, 14, 32
    x = U((B, cin, H, W), "convbf", cin, "x").bfloat16()
    w = (U((cout, cin, 3, 3), "convbf", cin, "w") * (cin * 9) ** -0.5).bfloat16()
    exact = F.conv2d(x.double(), w.double(), stride=stride, padding=1)
    got = M.conv3x3_rows(rows_of(x).to(dev), w.to(dev), B, H, W, stride)
    Ho, Wo = exact.shape[-2:]
    assert got.dtype == torch.float32
    compare_op(f"conv3x3 bf16 s{stride} cin{cin} y", image_of(got.cpu(), B, Ho, Wo), exact, exact.float(), tol=TOL_BF16_OP)


def test_conv3x3_unfold_is_exact_and_its_adjoint_deterministic(dev):
    B, H, W, cin = 2, 7, 9, 12
    x = U((B, cin, H, W), "unfold", "x")
    for stride in (1, 2):
        for dt in (torch.float32, torch.bfloat16):
            xr = rows_of(x).to(dev, dt)
            cols = adapter._Conv3x3UnfoldFn.apply(xr, B, H, W, stride)
            Ho, Wo = adapter.conv_out_size(H, stride), adapter.conv_out_size(W, stride)
            want = F.unfold(x.to(dt).float(), 3, padding=1, stride=stride).view(B, cin, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 9 * cin)
            assert cols.shape == (B * Ho * Wo, adapter.conv3x3_kpad(cin)) and cols.dtype == dt
            assert torch.equal(cols[:, :9 * cin].float().cpu(), want) and not cols[:, 9 * cin:].any()
            g = U(tuple(cols.shape), "unfold", "g", stride).to(dev, dt)
            runs = []
            for _ in range(2):
                leaf = xr.clone().requires_grad_()
                adapter._Conv3x3UnfoldFn.apply(leaf, B, H, W, stride).backward(g)
                runs.append(leaf.grad.clone())
            assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("B,C,H,W", [(2, 16, 9, 12), (1, 64, 16, 7), (2, 8, 1, 5)])
def test_max_pool_rows(dev, B, C, H, W):
    x = distinct((B, C, H, W), mc.seed_of("pool", H, W))
    Ho, Wo = adapter.conv_out_size(H, 2), adapter.conv_out_size(W, 2)
    dy = U((B, C, Ho, Wo), "pool", H, W, "dy")
    ref = lambda dt: grads_of(lambda a: F.max_pool2d(a, 3, 2, 1), (x.to(dt),), dy)      # noqa: E731
    e, r = ref(torch.float64), ref(torch.float32)
    assert e[0].shape == (B, C, Ho, Wo)
    leaf = rows_of(x).to(dev).requires_grad_()
    y, idx = M.max_pool3x3s2_rows(leaf, B, H, W, return_indices=True)
    y.backward(rows_of(dy).to(dev))
    assert torch.equal(image_of(y.detach().cpu(), B, Ho, Wo).double(), e[0])
    compare_op(f"maxpool {H}x{W} dx", image_of(leaf.grad.cpu(), B, H, W), e[1], r[1])
    # the winner as ATen reports it: flat position in the input plane -> tap dy * 3 + dx of the window
    _, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    tap = (torch.div(flat, W, rounding_mode="floor") - (2 * oy - 1)) * 3 + (flat % W - (2 * ox - 1))
    assert idx.dtype == torch.int8 and torch.equal(image_of(idx.cpu(), B, Ho, Wo).long(), tap)


def test_max_pool_rows_tie_order(dev):
    B, C, H, W = 2, 8, 8, 10
    x = torch.from_numpy(np.floor(mc.uniform((B, C, H, W), mc.seed_of("pool", "ties"), 0.0, 3.0))).float()      # values 0, 1, 2: ties everywhere
    Ho, Wo = adapter.conv_out_size(H, 2), adapter.conv_out_size(W, 2)
    y, idx = M.max_pool3x3s2_rows(rows_of(x).to(dev), B, H, W, return_indices=True)
    want, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    tap = (torch.div(flat, W, rounding_mode="floor") - (2 * oy - 1)) * 3 + (flat % W - (2 * ox - 1))
    assert torch.equal(image_of(y.cpu(), B, Ho, Wo), want)
    assert torch.equal(image_of(idx.cpu(), B, Ho, Wo).long(), tap)
    # the gradient goes to that one tap
    dy = U((B, C, Ho, Wo), "pool", "ties", "dy")
    leaf = x.clone().double().requires_grad_()
    F.max_pool2d(leaf, 3, 2, 1).backward(dy.double())
    mine = rows_of(x).to(dev).requires_grad_()
    M.max_pool3x3s2_rows(mine, B, H, W).backward(rows_of(dy).to(dev))
    compare_op("maxpool ties dx", image_of(mine.grad.cpu(), B, H, W), leaf.grad, leaf.grad.float())


@pytest.mark.parametrize("h,w,f", [(6, 9, 4), (7, 5, 2), (8, 10, 0.5), (7, 9, 0.5), (5, 3, 0.5), (1, 4, 2)])
def test_resize_rows_batched_scale_factor(dev, h, w, f):
    B, C = 2, 24
    x = U((B, C, h, w), "resize", h, w, f, "x")
    H, W = adapter.interpolate_geometry(h, f)[0], adapter.interpolate_geometry(w, f)[0]
    dy = U((B, C, H, W), "resize", h, w, f, "dy")
    ref = lambda dt: grads_of(lambda a: F.interpolate(a, scale_factor=f, mode="bilinear", align_corners=False), (x.to(dt),), dy)      # noqa: E731
    e, r = ref(torch.float64), ref(torch.float32)
    assert e[0].shape == (B, C, H, W)
    got = grads_of(lambda a: M.resize_rows_batched(a, B, h, w, scale_factor=f), (rows_of(x).to(dev),), rows_of(dy))
    compare_op(f"resize {h}x{w} x{f} y", image_of(got[0].cpu(), B, H, W), e[0], r[0])
    compare_op(f"resize {h}x{w} x{f} dx", image_of(got[1].cpu(), B, h, w), e[1], r[1])


@pytest.mark.parametrize("h,w,H,W", [(7, 9, 10, 20), (9, 8, 4, 5)])
def test_resize_rows_batched_size(dev, h, w, H, W):
    B, C = 1, 16
    x, dy = U((B, C, h, w), "resize", h, w, H, "x"), U((B, C, H, W), "resize", h, w, H, "dy")
    ref = lambda dt: grads_of(lambda a: F.interpolate(a, size=(H, W), mode="bilinear", align_corners=False), (x.to(dt),), dy)      # noqa: E731
    e, r = ref(torch.float64), ref(torch.float32)
    got = grads_of(lambda a: M.resize_rows_batched(a, B, h, w, size=(H, W)), (rows_of(x).to(dev),), rows_of(dy))
    compare_op(f"resize {h}x{w} -> {H}x{W} y", image_of(got[0].cpu(), B, H, W), e[0], r[0])
    compare_op(f"resize {h}x{w} -> {H}x{W} dx", image_of(got[1].cpu(), B, h, w), e[1], r[1])


@pytest.mark.parametrize("with_add", [True, False])
def test_conv_transpose2x2_rows(dev, with_add):
    B, C, h, w = 2, 48, 5, 7
    x, wt, b = U((B, C, h, w), "up", "x"), U((C, C, 2, 2), "up", "w") * C ** -0.5, U((C,), "up", "b")
    add, dy = U((B, C, 2 * h, 2 * w), "up", "add"), U((B, C, 2 * h, 2 * w), "up", "dy")

    def ref(dt):
        return grads_of(lambda a, ww, bb, ad: F.conv_transpose2d(a, ww, bb, stride=2) + (ad if with_add else 0 * ad),
                        (x.to(dt), wt.to(dt), b.to(dt), add.to(dt)), dy)
    e, r = ref(torch.float64), ref(torch.float32)

    def mine(a, ww, bb, ad):
        return M.conv_transpose2x2_rows(a, ww, bb, B, h, w, add=ad if with_add else None)
    leaves = [t.to(dev).requires_grad_() for t in (rows_of(x), wt, b, rows_of(add))]
    out = mine(*leaves)
    out.backward(rows_of(dy).to(dev))
    assert out.dtype == torch.float32 and out.shape == (B * 4 * h * w, C)
    compare_op("up y", image_of(out.detach().cpu(), B, 2 * h, 2 * w), e[0], r[0])
    compare_op("up dx", image_of(leaves[0].grad.cpu(), B, h, w), e[1], r[1])
    compare_op("up dw", leaves[1].grad, e[2], r[2])
    compare_op("up db", leaves[2].grad, e[3], r[3])
    if with_add:
        compare_op("up dadd", image_of(leaves[3].grad.cpu(), B, 2 * h, 2 * w), e[4], r[4])
    else:
        assert leaves[3].grad is None


def test_backward_kernels_are_bit_reproducible(dev):
    B, C, H, W = 2, 32, 12, 10
    x = U((B * H * W, C), "repro", "x").to(dev)

    def twice(fn, dshape):
        g = U(dshape, "repro", "g", len(dshape), dshape[0]).to(dev)
        runs = []
        for poison in (float("nan"), 7.0):
            torch.full((1 << 20,), poison, device=dev)          # (whatever the allocator hands out next has been written over)
            leaf = x.clone().requires_grad_()
            fn(leaf).backward(g)
            runs.append(leaf.grad.clone())
        assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    w = (U((16, C, 3, 3), "repro", "w") * 0.05).to(dev)
    for s in (1, 2):
        Ho, Wo = adapter.conv_out_size(H, s), adapter.conv_out_size(W, s)
        twice(lambda t: M.conv3x3_rows(t, w, B, H, W, s), (B * Ho * Wo, 16))
    twice(lambda t: M.max_pool3x3s2_rows(t, B, H, W), (B * 6 * 5, C))
    twice(lambda t: M.resize_rows_batched(t, B, H, W, scale_factor=4), (B * 16 * H * W, C))
    twice(lambda t: M.resize_rows_batched(t, B, H, W, scale_factor=0.5), (B * 6 * 5, C))
    wt = (U((C, C, 2, 2), "repro", "wt") * 0.1).to(dev)
    twice(lambda t: M.conv_transpose2x2_rows(t, wt, None, B, H, W), (B * 4 * H * W, C))


# ----------------------------------------------------------------------------- the bf16 branches of the kernels
# inputs are rounded to bf16 first, the exact result is the float64 function of those; bound TOL_BF16_OP (tests/conftest.py)
def test_conv3x3_rows_bf16_gradients(dev):
    B, H, W, cin, cout, stride = 2, 9, 10, 16, 24, 2
    x = U((B, cin, H, W), "convbfg", "x").bfloat16()
    w = (U((cout, cin, 3, 3), "convbfg", "w") * (cin * 9) ** -0.5).bfloat16()
    Ho, Wo = adapter.conv_out_size(H, stride), adapter.conv_out_size(W, stride)
    dy = U((B, cout, Ho, Wo), "convbfg", "dy").bfloat16()
    e = grads_of(lambda a, b: F.conv2d(a, b, stride=stride, padding=1), (x.double(), w.double()), dy.double())
    got = grads_of(lambda a, b: M.conv3x3_rows(a, b, B, H, W, stride), (rows_of(x).to(dev), w.to(dev)), rows_of(dy).float())
    assert got[1].dtype == torch.bfloat16 and got[2].dtype == torch.bfloat16
    compare_op("conv3x3 bf16 dx", image_of(got[1].float().cpu(), B, H, W), e[1], e[1].float(), tol=TOL_BF16_OP)
    compare_op("conv3x3 bf16 dw", got[2].float(), e[2], e[2].float(), tol=TOL_BF16_OP)


def test_max_pool_rows_bf16(dev):
    B, C, H, W = 2, 16, 9, 11
    x = U((B, C, H, W), "poolbf", "x").bfloat16()
    Ho, Wo = adapter.conv_out_size(H, 2), adapter.conv_out_size(W, 2)
    dy = U((B, C, Ho, Wo), "poolbf", "dy").bfloat16()
    leaf64 = x.double().requires_grad_()
    want, flat = F.max_pool2d(leaf64, 3, 2, 1, return_indices=True)
    want.backward(dy.double())
    leaf = rows_of(x).to(dev).requires_grad_()
    y, idx = M.max_pool3x3s2_rows(leaf, B, H, W, return_indices=True)
    y.backward(rows_of(dy).to(dev))
    assert y.dtype == torch.bfloat16 and leaf.grad.dtype == torch.bfloat16
    assert torch.equal(image_of(y.detach().float().cpu(), B, Ho, Wo).double(), want.detach())
    oy, ox = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    tap = (torch.div(flat, W, rounding_mode="floor") - (2 * oy - 1)) * 3 + (flat % W - (2 * ox - 1))
    assert torch.equal(image_of(idx.cpu(), B, Ho, Wo).long(), tap)
    compare_op("maxpool bf16 dx", image_of(leaf.grad.float().cpu(), B, H, W), leaf64.grad, leaf64.grad.float(), tol=TOL_BF16_OP)


@pytest.mark.parametrize("f", [2, 0.5])
def test_resize_rows_batched_bf16(dev, f):
    B, C, h, w = 2, 16, 7, 6
    x = U((B, C, h, w), "resizebf", f, "x").bfloat16()
    H, W = adapter.interpolate_geometry(h, f)[0], adapter.interpolate_geometry(w, f)[0]
    dy = U((B, C, H, W), "resizebf", f, "dy").bfloat16()
    e = grads_of(lambda a: F.interpolate(a, scale_factor=f, mode="bilinear", align_corners=False), (x.double(),), dy.double())
    got = grads_of(lambda a: M.resize_rows_batched(a, B, h, w, scale_factor=f), (rows_of(x).to(dev),), rows_of(dy))
    assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.bfloat16
    compare_op(f"resize bf16 x{f} y", image_of(got[0].float().cpu(), B, H, W), e[0], e[0].float(), tol=TOL_BF16_OP)
    compare_op(f"resize bf16 x{f} dx", image_of(got[1].float().cpu(), B, h, w), e[1], e[1].float(), tol=TOL_BF16_OP)


def test_conv_transpose2x2_rows_bf16(dev):
    B, C, h, w = 2, 32, 4, 5
    x, wt, b = U((B, C, h, w), "upbf", "x").bfloat16(), (U((C, C, 2, 2), "upbf", "w") * C ** -0.5).bfloat16(), U((C,), "upbf", "b")
    add, dy = U((B, C, 2 * h, 2 * w), "upbf", "add").bfloat16(), U((B, C, 2 * h, 2 * w), "upbf", "dy")
    e = grads_of(lambda a, ww, bb, ad: F.conv_transpose2d(a, ww, bb, stride=2) + ad, (x.double(), wt.double(), b.double(), add.double()), dy)
    leaves = [t.to(dev).requires_grad_() for t in (rows_of(x), wt, b, rows_of(add))]
    out = M.conv_transpose2x2_rows(leaves[0], leaves[1], leaves[2], B, h, w, add=leaves[3])
    out.backward(rows_of(dy).to(dev))
    assert out.dtype == torch.float32 and leaves[0].grad.dtype == torch.bfloat16 and leaves[3].grad.dtype == torch.bfloat16
    compare_op("up bf16 y", image_of(out.detach().cpu(), B, 2 * h, 2 * w), e[0], e[0].float(), tol=TOL_BF16_OP)
    compare_op("up bf16 dx", image_of(leaves[0].grad.float().cpu(), B, h, w), e[1], e[1].float(), tol=TOL_BF16_OP)
    compare_op("up bf16 dw", leaves[1].grad.float(), e[2], e[2].float(), tol=TOL_BF16_OP)
    compare_op("up bf16 db", leaves[2].grad, e[3], e[3].float(), tol=TOL_BF16_OP)
    compare_op("up bf16 dadd", image_of(leaves[3].grad.float().cpu(), B, 2 * h, 2 * w), e[4], e[4].float(), tol=TOL_BF16_OP)


# ----------------------------------------------------------------------------- fixture cases
def load_params(module, tag, dev):
    sd = vc.state_dict_arrays([(k, tuple(v.shape)) for k, v in module.state_dict().items()], tag)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return module.to(dev)


def T(a, dev):
    return torch.from_numpy(np.asarray(a)).to(dev)


@pytest.mark.parametrize("name", list(vc.SPM_EVAL))
def test_spm_eval_matches_the_reference(gold, dev, name):
    c = vc.SPM_EVAL[name]
    m = load_params(M.SpatialPriorModule(inplanes=c["inplanes"], embed_dim=c["embed_dim"]), f"spm/eval/{name}", dev).eval()
    x = T(vc.image(f"spm/eval/{name}", "", c["B"], c["H"], c["W"]), dev)
    with torch.no_grad():
        outs = m(x)
    assert outs[0].shape == (c["B"], c["embed_dim"], c["H"] // 4, c["W"] // 4) and outs[1].shape == (c["B"], (c["H"] // 8) * (c["W"] // 8), c["embed_dim"])
    for k, o in zip(("c1", "c2", "c3", "c4"), outs):
        compare(gold, f"spm/eval/{name}/{k}", o)
    if f"spm/eval/{name}" in json.loads(str(gold["bf16_missing"])):
        return
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        outs = m(x)
    for k, o in zip(("c1", "c2", "c3", "c4"), outs):
        compare(gold, f"spm/eval/{name}/{k}", o, which="ref_err_bf16")


def test_spm_train_matches_the_reference(gold, dev):
    c, tag = vc.SPM_TRAIN, str(gold["spm/train/tag"])
    m = load_params(M.SpatialPriorModule(inplanes=c["inplanes"], embed_dim=c["embed_dim"]), f"spm/train/{tag}", dev).train()
    x = T(vc.image("spm/train", tag, c["B"], c["H"], c["W"]), dev).requires_grad_()
    outs = m(x)
    names = ("c1", "c2", "c3", "c4")
    torch.autograd.backward(list(outs), [T(vc.cotangent("spm/train", tag, n, o.shape), dev) for n, o in zip(names, outs)])
    for k, o in zip(names, outs):
        compare(gold, f"spm/train/{k}", o)
    compare(gold, "spm/train/dx", x.grad)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        compare(gold, f"spm/train/dparam/{k}", p.grad)
    for k, b in m.named_buffers():
        if not k.endswith("num_batches_tracked"):
            compare(gold, f"spm/train/buffer/{k}", b)


def build_backbone(tag, dev):
    cfg = dict(vc.BACKBONE)
    return load_params(M.ViTAdapter(img_size=cfg["pretrain_size"], **cfg), tag, dev)


def test_backbone_eval_matches_the_reference(gold, dev):
    c = vc.BACKBONE_EVAL
    m = build_backbone("backbone/eval", dev).eval()
    x = T(vc.image("backbone/eval", "", c["B"], c["H"], c["W"]), dev)
    with torch.no_grad():
        outs = m(x)
    D = vc.BACKBONE["embed_dim"]
    assert [tuple(o.shape) for o in outs] == [(c["B"], D, c["H"] // s, c["W"] // s) for s in (4, 8, 16, 32)]
    for k, o in zip(("f1", "f2", "f3", "f4"), outs):
        assert o.dtype == torch.float32 and o.is_contiguous()
        compare(gold, f"backbone/eval/{k}", o, floor=BLOCK_FP32_FLOOR)
    if "backbone/eval" in json.loads(str(gold["bf16_missing"])):
        return
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        outs = m(x)
    for k, o in zip(("f1", "f2", "f3", "f4"), outs):
        compare(gold, f"backbone/eval/{k}", o, which="ref_err_bf16")


def test_backbone_train_matches_the_reference(gold, dev):
    c, tag = vc.BACKBONE_TRAIN, str(gold["backbone/train/tag"])
    m = build_backbone(f"backbone/train/{tag}", dev).train()
    x = T(vc.image("backbone/train", tag, c["B"], c["H"], c["W"]), dev).requires_grad_()
    outs = m(x)
    names = ("f1", "f2", "f3", "f4")
    torch.autograd.backward(list(outs), [T(vc.cotangent("backbone/train", tag, n, o.shape), dev) for n, o in zip(names, outs)])
    for k, o in zip(names, outs):
        compare(gold, f"backbone/train/{k}", o, floor=BLOCK_FP32_FLOOR)
    compare(gold, "backbone/train/dx", x.grad, floor=BLOCK_FP32_FLOOR)
    seen = 0
    for k, p in m.named_parameters():
        if k in vc.BACKBONE_TRAIN_ZERO_GRADS:         # exactly zero by construction: float32 rounding noise at most
            assert float(p.grad.abs().max()) <= 1e-4 * float(m.up.weight.grad.abs().max()), k
        elif k.startswith(vc.BACKBONE_TRAIN_GRADS):
            assert p.grad is not None, k
            compare(gold, f"backbone/train/dparam/{k}", p.grad, floor=BLOCK_FP32_FLOOR)
            seen += 1
    assert seen == sum(1 for k in gold.files if k.startswith("backbone/train/dparam/") and k.endswith("/argmax"))


def test_base_detection_backbone_runs_forward_and_backward(dev):
    m = M.ViTAdapter(**vc.DET_BASE).to(dev)
    B, H, W = 1, 256, 320
    x = T(vc.image("base", "", B, H, W), dev)
    m.eval()
    with torch.no_grad():
        a, b = m(x), m(x)
    for s, fa, fb in zip((4, 8, 16, 32), a, b):
        assert fa.shape == (B, 768, H // s, W // s) and fa.dtype == torch.float32 and torch.isfinite(fa).all()
        assert torch.equal(fa, fb), f"eval forward differs between two calls at stride {s}"
    m.train()
    torch.manual_seed(0)
    outs = m(x.clone().requires_grad_())
    sum((o * o).mean() for o in outs).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
