"""GPU: the P3Embed tokenizer (group_embed.py:176-286) and the kernels under it.

  * me_knn beyond the LDS-resident form (n > 10 240, me_knn_stream) against the (distance, index) ranking computed on the GPU
    in float64 from the kernel's own distance expression, with ties (duplicated points); the two KNN forms agree at n <= 10 240;
  * me_group_features against the torch gather-and-subtract (bit for bit) and me_group_features_bwd against float64 autograd
    of the same gather (deterministic: two runs bit-identical);
  * P3Embed against tests/golden/p3embed.npz (tools/make_p3embed_golden.py, the reference's own class);
  * full size (S3DIS [8, 24000, 7] ln2d, ScanObjectNN [32, 1024, 3] bn in training mode) forward and backward against a float64
    restatement on the GPU with the same sampled, neighbour and pooled indices;
  * P3Embed tokens through a frozen 2-block encoder, forward and backward.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, TOL_F32, check_close, rel_err
import metatransformer_amd as M
from metatransformer_amd import _capi, heads
from metatransformer_amd._capi import ptr, stream_ptr

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------- KNN

def _cloud(B, n, seed, dup=False):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, n, 3, generator=g) * 2 - 1
    if dup:
        p[:, n // 2:] = p[:, : n - n // 2].clone()
    return p


def _kernel_dist(p, q):
    """[B, m, n] squared distances as knn_kernel rounds them: fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32.  Each fmaf is taken
    exactly in float64 (the product of two floats is exact there) and rounded once to fp32."""
    d = p.unsqueeze(1) - q.unsqueeze(2)                                   # fp32 differences, as the kernel forms them
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    acc = dx * dx
    acc = (dy.double() * dy.double() + acc.double()).float()
    return (dz.double() * dz.double() + acc.double()).float()


def _rank(p, q, k):
    """the lexicographic (distance, index) order of the first k, computed in float64 on the GPU (a stable sort keeps equal
    distances in index order)"""
    return torch.sort(_kernel_dist(p, q).double(), dim=2, stable=True).indices[..., :k].to(torch.int32)


def _knn_stream(p, q, k):
    B, n, _ = p.shape
    m = q.shape[1]
    idx = torch.empty(B, m, k, dtype=torch.int32, device=p.device)
    rc = _capi.load().me_knn_stream(ptr(p), ptr(q), ptr(idx), B, n, m, k, stream_ptr())
    return rc, idx


@pytest.mark.parametrize("n", [10241, 24000, 64000])
@pytest.mark.parametrize("k", [16, 32, 64])
@pytest.mark.parametrize("dup", [False, True])
def test_knn_beyond_lds_resident_form(dev, n, k, dup):
    B = 2
    p = _cloud(B, n, 700 + n + k, dup).to(dev)
    g = torch.Generator().manual_seed(n + k)
    on = torch.randperm(n if not dup else n // 2, generator=g)[:300].to(dev)        # queries drawn from the cloud
    off = (torch.rand(B, 200, 3, generator=g) * 2.4 - 1.2).to(dev)                  # and off-cloud points
    q = torch.cat([p[:, on], off], dim=1).contiguous()
    got = heads.knn_indices(p, q, k)
    want = _rank(p, q, k)
    assert torch.equal(got, want), f"n={n} k={k} dup={dup}: {int((got != want).sum())} indices differ"
    # a centre's first neighbour is itself (with duplicates: the lowest index among its copies, which is the centre here)
    assert torch.equal(got[:, :300, 0].long(), on.unsqueeze(0).expand(B, -1))
    # and the exact float64 distances are ascending
    d64 = (p.double().unsqueeze(1) - q.double().unsqueeze(2)).pow(2).sum(-1).gather(2, got.long())
    assert bool((d64[..., 1:] >= d64[..., :-1] - 1e-6).all())


def test_knn_stream_limits(dev):
    p = _cloud(1, 12000, 3).to(dev)
    rc, _ = _knn_stream(p, p[:, :10].contiguous(), 65)
    assert rc == -2                                                      # ME_ERR_UNSUPPORTED: k > 64
    with pytest.raises(M.MetaEncError):
        heads.knn_indices(p, p[:, :10].contiguous(), 65)


@pytest.mark.parametrize("n,m,k", [(64, 64, 64), (1000, 250, 16), (1024, 256, 32), (4096, 1024, 32), (10240, 640, 64)])
@pytest.mark.parametrize("dup", [False, True])
def test_knn_forms_agree(dev, n, m, k, dup):
    p = _cloud(3, n, 900 + n, dup).to(dev)
    q = torch.cat([p[:, : m // 2], _cloud(3, m - m // 2, 5).to(dev)], dim=1).contiguous()
    rc, got = _knn_stream(p, q, k)
    assert rc == 0
    assert torch.equal(got, heads.knn_indices(p, q, k))


# ----------------------------------------------------------------------------------------------------- grouping

def _indices(B, n, m, k, seed, dev):
    g = torch.Generator().manual_seed(seed)
    ctr = torch.stack([torch.randperm(n, generator=g)[:m] for _ in range(B)]).to(torch.int32)
    nbr = torch.randint(0, n, (B, m, k), generator=g, dtype=torch.int32)
    nbr[:, :, 0] = ctr                                                       # the centre is its own first neighbour
    return ctr.to(dev), nbr.to(dev)


def _torch_rows(p, f, ctr, nbr, ft):
    B, m, k = nbr.shape
    gat = lambda x, i: torch.gather(x, 1, i.long().reshape(B, -1, 1).expand(-1, -1, x.shape[2])).reshape(B, *i.shape[1:], x.shape[2])
    dp = gat(p, nbr) - gat(p, ctr).unsqueeze(2)
    parts = [dp]
    if ft in ("dp_fj", "dp_fj_df"):
        parts.append(gat(f, nbr))
    if ft in ("dp_df", "dp_fj_df"):
        parts.append(gat(f, nbr) - gat(f, ctr).unsqueeze(2))
    return torch.cat(parts, dim=3).reshape(B * m * k, -1)


@pytest.mark.parametrize("ft", ["dp", "dp_fj", "dp_df", "dp_fj_df"])
@pytest.mark.parametrize("C", [7, 64])
def test_group_features_equals_torch_gather(dev, ft, C):
    B, n, m, k = 2, 3000, 750, 32
    g = torch.Generator().manual_seed(C)
    p, f = torch.randn(B, n, 3, generator=g).to(dev), torch.randn(B, n, C, generator=g).to(dev)
    ctr, nbr = _indices(B, n, m, k, 11, dev)
    rows = heads.group_features(p, f, ctr, nbr, ft)
    want = _torch_rows(p, f, ctr, nbr, ft)
    w = want.shape[1]
    assert rows.shape == (B * m * k, (w + 7) // 8 * 8) and rows.dtype == torch.float32
    assert torch.equal(rows[:, :w], want)
    assert bool((rows[:, w:] == 0).all())
    # bf16 features: the same gather of the bf16 values, subtracted in fp32
    fb = f.to(torch.bfloat16)
    assert torch.equal(heads.group_features(p, fb, ctr, nbr, ft)[:, :w], _torch_rows(p, fb.float(), ctr, nbr, ft))
    # a wider padded operand
    assert torch.equal(heads.group_features(p, f, ctr, nbr, ft, cols=(w + 7) // 8 * 8 + 16)[:, :w], want)


@pytest.mark.parametrize("ft", ["dp_fj", "dp_df", "dp_fj_df"])
@pytest.mark.parametrize("B,n,m,k,C,dupctr", [(2, 3000, 750, 32, 7, False), (3, 1024, 256, 16, 64, False),
                                                (1, 24000, 6000, 32, 8, False), (2, 500, 200, 8, 16, True)])
def test_group_features_backward(dev, ft, B, n, m, k, C, dupctr):
    g = torch.Generator().manual_seed(n + C)
    p, f = torch.randn(B, n, 3, generator=g).to(dev), torch.randn(B, n, C, generator=g).to(dev)
    ctr, nbr = _indices(B, n, m, k, 12, dev)
    if dupctr:                                                                # FPS can repeat a centre on a degenerate cloud
        ctr[:, 1::2] = ctr[:, ::2][:, : ctr[:, 1::2].shape[1]]
        nbr[:, :, 0] = ctr
    fr = f.clone().requires_grad_(True)
    rows = heads.group_features(p, fr, ctr, nbr, ft)
    go = torch.randn(rows.shape, generator=g).to(dev)
    (rows * go).sum().backward()
    f64 = f.double().requires_grad_(True)
    want = _torch_rows(p.double(), f64, ctr, nbr, ft)
    (want * go[:, : want.shape[1]].double()).sum().backward()
    assert rel_err(fr.grad, f64.grad) < 1e-6
    fr2 = f.clone().requires_grad_(True)
    (heads.group_features(p, fr2, ctr, nbr, ft) * go).sum().backward()
    assert torch.equal(fr.grad, fr2.grad), "me_group_features_bwd is not deterministic"


# ----------------------------------------------------------------------------------------------------- the reference class

@pytest.mark.parametrize("name", ["bn1", "ln2"])
def test_p3embed_equals_the_reference_class(dev, name):
    z = np.load(os.path.join(GOLDEN, "p3embed.npz"))
    kw = json.loads(str(z[f"{name}/config"]))
    mod = M.P3Embed(**kw)
    prefix = f"{name}/w/"
    mod.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)}, strict=True)
    mod = mod.to(dev).eval()
    p, f = torch.from_numpy(z[f"{name}/p"]).to(dev), torch.from_numpy(z[f"{name}/f"]).to(dev)
    with torch.no_grad():
        out_p, out_f = mod(p, f)
    stages = int(z[f"{name}/stages"])
    assert len(out_p) == len(out_f) == stages + 1 and out_p[0] is p and out_f[0] is f
    for s in range(1, stages + 1):
        assert torch.equal(out_p[s].cpu(), torch.from_numpy(z[f"{name}/center{s}"])), f"{name} stage {s}: centres differ"
        check_close(out_f[s], torch.from_numpy(z[f"{name}/out_f{s}"]), TOL_F32, f"{name} stage {s} out_f")


# ----------------------------------------------------------------------------------------------------- full size vs float64

class _Recorder:
    """records the sampled centres, neighbour lists, max-pool arg-maxes and ReLU masks P3Embed uses, in call order.  The
    float64 restatement takes every discrete choice from here, so it compares arithmetic only: a pre-activation within
    rounding of zero, or two group members within rounding of each other, would otherwise route a gradient differently
    (at S3DIS size a few thousand such elements move the first layer's weight gradient by ~1e-3)."""

    def __init__(self, monkeypatch):
        self.fps, self.knn, self.arg, self.relu = [], [], [], []
        fps, knn, pool, relu = heads.furthest_point_sample, heads.knn_indices, heads.pool_tokens, torch.relu

        def r_relu(x):
            y = relu(x)
            self.relu.append(y.detach() > 0)
            return y
        monkeypatch.setattr(torch, "relu", r_relu)

        def r_fps(p, m):
            i = fps(p, m)
            self.fps.append(i.long())
            return i

        def r_knn(s, q, k):
            i = knn(s, q, k)
            self.knn.append(i.long())
            return i

        def r_pool(x, mode="mean"):
            self.arg.append(x.detach().argmax(dim=1) if mode == "max" else None)
            return pool(x, mode)
        monkeypatch.setattr(heads, "furthest_point_sample", r_fps)
        monkeypatch.setattr(heads, "knn_indices", r_knn)
        monkeypatch.setattr(heads, "pool_tokens", r_pool)


def _restate(mod, params, p, f, rec):
    """P3Embed.forward (group_embed.py:266-286) in float64 torch, token-major, on the recorded indices"""
    B, N, _ = p.shape
    cur_p, cur_f = p.double(), f.double().transpose(1, 2)
    outs, pools, masks = [], iter(rec.arg), iter(rec.relu)
    for si, (conv1, conv2) in enumerate(mod.convs):
        N = N // 4
        idx, nbr = rec.fps[si], rec.knn[si]
        k = nbr.shape[2]
        gat = lambda x, i: torch.gather(x, 1, i.reshape(B, -1, 1).expand(-1, -1, x.shape[2])).reshape(B, *i.shape[1:], x.shape[2])
        cp, cf = gat(cur_p, idx), gat(cur_f, idx)
        x = torch.cat([gat(cur_p, nbr) - cp.unsqueeze(2), gat(cur_f, nbr) - cf.unsqueeze(2)], dim=3)        # dp_df [B, S, k, 3 + C]

        def block(blk, pre, x):
            conv = blk[0]
            x = x @ params[pre + "0.weight"].reshape(conv.out_channels, -1).t()
            if conv.bias is not None:
                x = x + params[pre + "0.bias"]
            if len(blk) > 1:
                if isinstance(blk[1], nn_BN):
                    sh = x.shape
                    x = F.batch_norm(x.reshape(-1, sh[-1]), None, None, params[pre + "1.weight"], params[pre + "1.bias"], True, 0.0,
                                     blk[1].eps).reshape(sh) if blk[1].training else \
                        F.batch_norm(x.reshape(-1, sh[-1]), blk[1].running_mean.double(), blk[1].running_var.double(),
                                     params[pre + "1.weight"], params[pre + "1.bias"], False, 0.0, blk[1].eps).reshape(sh)
                else:
                    x = F.layer_norm(x, (x.shape[-1],), params[pre + "1.weight"], params[pre + "1.bias"], 1e-5)
                x = x * next(masks).reshape(x.shape)                        # ReLU, on the module's own mask
            return x

        def pool(x):
            arg = next(pools).reshape(B, N, 1, -1)
            return torch.gather(x, 2, arg).squeeze(2)
        for i, blk in enumerate(conv1):
            x = block(blk, f"convs.{si}.0.{i}.", x)
        x = torch.cat([pool(x).unsqueeze(2).expand(-1, -1, k, -1), x], dim=3)
        for i, blk in enumerate(conv2):
            x = block(blk, f"convs.{si}.1.{i}.", x)
        cur_p, cur_f = cp, pool(x)
        outs.append(cur_f)                                                   # [B, S, C]
    return outs


nn_BN = torch.nn.BatchNorm2d


def _full_size(dev, monkeypatch, kw, B, N, train):
    torch.manual_seed(21)
    mod = M.P3Embed(**kw)
    for m in mod.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.LayerNorm)):
            m.weight.data.normal_(1.0, 0.1)
            m.bias.data.normal_(0.0, 0.05)
    mod = mod.to(dev).train(train)
    g = torch.Generator().manual_seed(22)
    p = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    f = torch.randn(B, kw["in_channels"], N, generator=g).to(dev)
    rec = _Recorder(monkeypatch)
    fr = f.clone().requires_grad_(True)
    out_p, out_f = mod(p, fr)
    gos = [torch.randn(o.shape, generator=g).to(dev) for o in out_f[1:]]
    sum((o * go).sum() for o, go in zip(out_f[1:], gos)).backward()
    monkeypatch.undo()
    assert len(rec.relu) == sum(len(blk) > 2 for c in mod.convs for seq in c for blk in seq)
    params = {k: v.detach().double().requires_grad_(True) for k, v in mod.named_parameters()}
    f64 = f.double().requires_grad_(True)
    ref = _restate(mod, params, p, f64, rec)
    for s, (o, r) in enumerate(zip(out_f[1:], ref)):
        check_close(o, r.transpose(1, 2), TOL_F32, f"stage {s + 1} out_f")
    sum((r.transpose(1, 2) * go.double()).sum() for r, go in zip(ref, gos)).backward()
    top = max(float(params[k].grad.abs().max()) for k in params)
    for k, v in mod.named_parameters():
        if float(params[k].grad.abs().max()) < 1e-6 * top:
            # exactly zero: a conv bias whose constant shift the training-mode BatchNorm behind conv2's first layer removes;
            # what is left is rounding, held to the scale of the other gradients
            assert float(v.grad.abs().max()) <= TOL_F32 * top, f"d{k}"
        else:
            check_close(v.grad, params[k].grad, TOL_F32, f"d{k}")
    check_close(fr.grad, f64.grad, TOL_F32, "df")


@pytest.mark.slow
def test_full_size_s3dis_vs_float64(dev, monkeypatch):
    kw = dict(sample_ratio=0.0625, group_size=32, in_channels=7, layers=4, embed_dim=768, subsample="fps", group="knn",
              feature_type="dp_df", norm_args={"norm": "ln2d"}, reduction="max")
    _full_size(dev, monkeypatch, kw, 8, 24000, True)


@pytest.mark.slow
def test_full_size_scanobjectnn_train_vs_float64(dev, monkeypatch):
    kw = dict(sample_ratio=0.25, group_size=32, in_channels=3, layers=4, embed_dim=768, subsample="fps", group="knn",
              feature_type="dp_df", norm_args="bn", reduction="max")
    _full_size(dev, monkeypatch, kw, 32, 1024, True)


def test_small_bn_eval_vs_float64(dev, monkeypatch):
    kw = dict(sample_ratio=0.0625, group_size=16, in_channels=7, layers=4, embed_dim=64, subsample="fps", group="knn",
              feature_type="dp_df", norm_args="bn", reduction="max")
    _full_size(dev, monkeypatch, kw, 2, 2048, False)


# ----------------------------------------------------------------------------------------------------- into the encoder

def test_p3embed_feeds_the_encoder(dev):
    torch.manual_seed(31)
    emb = M.P3Embed(sample_ratio=0.25, group_size=32, in_channels=3, embed_dim=192, group="knn", norm_args="bn").to(dev).train()
    enc = M.build_encoder(2, 192, 3).to(dev)
    for q in enc.parameters():
        q.requires_grad_(False)
    p = (torch.rand(4, 1024, 3) * 2 - 1).to(dev)
    f = p.transpose(1, 2).contiguous().requires_grad_(True)
    _, out_f = emb(p, f)
    y = enc(out_f[-1].transpose(1, 2).contiguous())
    assert y.shape == (4, 256, 192)
    y.square().mean().backward()
    assert torch.isfinite(f.grad).all() and f.grad.abs().sum() > 0
    for k, q in emb.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), k
