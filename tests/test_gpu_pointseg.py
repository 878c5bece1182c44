"""GPU: the point segmentation decoder (pointvit.py:177-393, pointnext.py:173-226, upsampling.py, base_seg.py:92-149) and the
kernels under it.

  * me_three_nn against the (distance, index) ranking computed on the GPU in float64 from the kernel's own distance
    expression (ties, queries on known points, m < 3), against me_knn(k = 3), and its weights against float64;
  * me_three_interpolate (write / accumulate, column offset, leading dimensions) against float64, and
    me_three_interpolate_bwd against float64 autograd of the gather (deterministic: two runs bit-identical; heavy fan-in);
  * the modules against tests/golden/pointseg.npz (tools/make_pointseg_golden.py, the reference's own classes);
  * full size (S3DIS [8, 24000], ShapeNetPart [8, 2048], width 768, training mode) forward and every gradient against a
    float64 restatement on the GPU with the same neighbour indices, ReLU masks and max arg-maxes;
  * P3Embed -> a frozen 2-block encoder -> PointViTDecoder -> SegHead -> cross-entropy, backward.
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


# ----------------------------------------------------------------------------------------------------- three_nn

def _cloud(B, n, seed, dup=False):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, n, 3, generator=g) * 2 - 1
    if dup:
        p[:, n // 2:] = p[:, : n - n // 2].clone()
    return p


def _kernel_dist(known, q):
    """[B, n, m] squared distances as the kernels round them: fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32 (each fmaf exact in
    float64, rounded once)"""
    d = known.unsqueeze(1) - q.unsqueeze(2)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    acc = dx * dx
    acc = (dy.double() * dy.double() + acc.double()).float()
    return (dz.double() * dz.double() + acc.double()).float()


def _rank3(known, q, chunk):
    """the first 3 of the lexicographic (distance, index) order (stable sort), in query chunks; with m < 3 the slots past m are
    index 0 / distance +inf as in the reference"""
    B, n, _ = q.shape
    m = known.shape[1]
    idx = torch.zeros(B, n, 3, dtype=torch.int32, device=q.device)
    d2 = torch.full((B, n, 3), float("inf"), dtype=torch.float32, device=q.device)
    t = min(3, m)
    for a in range(0, n, chunk):
        d = _kernel_dist(known, q[:, a:a + chunk])
        s = torch.sort(d.double(), dim=2, stable=True)
        idx[:, a:a + chunk, :t] = s.indices[..., :t].to(torch.int32)
        d2[:, a:a + chunk, :t] = s.values[..., :t].float()
    return idx, d2


def _three_nn_raw(unknown, known):
    B, n, _ = unknown.shape
    m = known.shape[1]
    idx = torch.empty(B, n, 3, dtype=torch.int32, device=unknown.device)
    w = torch.empty(B, n, 3, dtype=torch.float32, device=unknown.device)
    dist = torch.empty(B, n, 3, dtype=torch.float32, device=unknown.device)
    rc = _capi.load().me_three_nn(ptr(unknown), ptr(known), ptr(idx), ptr(w), ptr(dist), B, n, m, stream_ptr())
    return rc, idx, w, dist


@pytest.mark.parametrize("B,n,m", [(2, 100, 1), (2, 100, 2), (3, 1000, 3), (2, 4097, 1031), (8, 24000, 6000), (2, 64000, 16000)])
@pytest.mark.parametrize("dup", [False, True])
def test_three_nn_ranking(dev, B, n, m, dup):
    known = _cloud(B, m, 100 + m, dup and m >= 2).to(dev)
    q = _cloud(B, n, 200 + n).to(dev)
    on = min(m, 50)
    q[:, :on] = known[:, :on]                                             # queries on known points
    q = q.contiguous()
    rc, idx, w, dist = _three_nn_raw(q, known)
    assert rc == 0
    want, d2 = _rank3(known, q, max(1, (1 << 26) // (B * m)))
    assert torch.equal(idx, want), f"{int((idx != want).sum())} indices differ"
    if m >= 3:
        assert torch.equal(idx, heads.knn_indices(known, q, 3))
    # a query on a known point: that point (the lowest index among its copies) first, at distance 0, weight ~1
    dupd = dup and m >= 2
    # (known[m // 2 + t] = the original known[t] for t < m - m // 2, so a copy sits lower only where that original survived)
    first = torch.tensor([j - m // 2 if dupd and m // 2 <= j < 2 * (m // 2) else j for j in range(on)])
    assert torch.equal(idx[:, :on, 0].long().cpu(), first.expand(B, -1))
    assert bool((dist[:, :on, 0] == 0).all())
    if m >= 2 and not dupd:
        assert bool((w[:, :on, 0] > 1 - 1e-4).all())
    # distances: sqrt of the ranked squared distances; unused slots +inf with index 0 and weight exactly 0
    assert rel_err(dist[torch.isfinite(d2)], d2[torch.isfinite(d2)].double().sqrt()) < 1e-6
    if m < 3:
        assert bool((idx[..., m:] == 0).all()) and bool((w[..., m:] == 0).all()) and bool(torch.isinf(dist[..., m:]).all())
    r = 1.0 / (dist.double() + float(np.float32(1e-8)))
    w64 = r / r.sum(dim=2, keepdim=True)
    assert bool(((w.double() - w64).abs() <= 2e-6 * w64.abs()).all())
    # the public forms
    d_pub, i_pub = heads.three_nn(q, known)
    assert torch.equal(i_pub, idx) and torch.equal(d_pub, dist)
    i_w, w_w = heads.three_nn_weights(q, known)
    assert torch.equal(i_w, idx) and torch.equal(w_w, w)


def test_three_nn_rejects_empty_known(dev):
    q = _cloud(1, 10, 1).to(dev)
    rc, *_ = _three_nn_raw(q, q[:, :0].contiguous())
    assert rc == -1                                                          # ME_ERR_ARG: m = 0
    with pytest.raises(M.MetaEncError):
        heads.three_nn(q, q[:, :0].contiguous())


# ----------------------------------------------------------------------------------------------------- interpolation

def _interp64(feats, idx, w):
    """[B, m, C], [B, n, 3], [B, n, 3] -> [B, n, C] float64"""
    B, m, C = feats.shape
    g = torch.gather(feats.double(), 1, idx.long().reshape(B, -1, 1).expand(-1, -1, C)).reshape(B, idx.shape[1], 3, C)
    return (w.double().unsqueeze(-1) * g).sum(2)


def _idx_w(B, n, m, seed, dev, fan_in=False):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, m, (B, n, 3), generator=g, dtype=torch.int32)
    if fan_in:
        idx[:] = 0
    w = torch.rand(B, n, 3, generator=g)
    return idx.to(dev), (w / w.sum(2, keepdim=True)).to(dev)


@pytest.mark.parametrize("C", [1, 7, 64, 384, 768, 1000])
def test_three_interpolate_write_and_accumulate(dev, C):
    B, n, m = 2, 3000, 750
    g = torch.Generator().manual_seed(C)
    idx, w = _idx_w(B, n, m, C, dev)
    ldf, col0, ldo = C + 4, 8, C + 8 + 5
    fbuf = torch.randn(B * m, ldf, generator=g).to(dev)
    feats = fbuf[:, :C]
    want = _interp64(feats.reshape(B, m, C), idx, w).reshape(B * n, C)
    lib = _capi.load()
    out = torch.full((B * n, ldo), 7.0, device=dev)
    assert lib.me_three_interpolate(ptr(fbuf), ldf, ptr(idx), ptr(w), ptr(out), ldo, col0, B, n, m, C, 0, stream_ptr()) == 0
    check_close(out[:, col0:col0 + C], want, TOL_F32, f"C={C} write")
    assert rel_err(out[:, col0:col0 + C], want) < 1e-6
    assert bool((out[:, :col0] == 7).all()) and bool((out[:, col0 + C:] == 7).all())           # nothing outside the columns
    base = torch.randn(B * n, ldo, generator=g).to(dev)
    acc = base.clone()
    assert lib.me_three_interpolate(ptr(fbuf), ldf, ptr(idx), ptr(w), ptr(acc), ldo, col0, B, n, m, C, 1, stream_ptr()) == 0
    assert rel_err(acc[:, col0:col0 + C], want + base[:, col0:col0 + C].double()) < 1e-6
    assert torch.equal(acc[:, :col0], base[:, :col0]) and torch.equal(acc[:, col0 + C:], base[:, col0 + C:])
    # dense operands (the vectorised path where C allows it)
    fd = feats.contiguous()
    od = torch.empty(B * n, C, device=dev)
    assert lib.me_three_interpolate(ptr(fd), C, ptr(idx), ptr(w), ptr(od), C, 0, B, n, m, C, 0, stream_ptr()) == 0
    assert torch.equal(od, out[:, col0:col0 + C])


def _bwd(dout, idx, w, B, n, m, C, ldo=None, col0=0):
    lib = _capi.load()
    ldo = ldo or C
    df = torch.full((B * m, C), float("nan"), device=dout.device)
    ws = torch.empty(max(1, int(lib.me_three_interpolate_bwd_workspace(B, n, m))), dtype=torch.uint8, device=dout.device)
    rc = lib.me_three_interpolate_bwd(ptr(dout), ldo, col0, ptr(idx), ptr(w), ptr(df), C, B, n, m, C, ptr(ws), ws.numel(), stream_ptr())
    assert rc == 0
    return df


@pytest.mark.parametrize("B,n,m,C,fan_in", [(2, 3000, 750, 7, False), (2, 3000, 750, 768, False), (3, 1024, 256, 64, False),
                                            (8, 24000, 6000, 8, False), (2, 2000, 500, 64, True), (2, 1500, 1, 12, False),
                                            (2, 4000, 4000, 16, False)])
def test_three_interpolate_backward(dev, B, n, m, C, fan_in):
    idx, w = _idx_w(B, n, m, n + C, dev, fan_in)
    g = torch.Generator().manual_seed(C)
    f = torch.randn(B, m, C, generator=g).to(dev)
    dout = torch.randn(B * n, C + 3, generator=g).to(dev)
    f64 = f.double().requires_grad_(True)
    (_interp64(f64, idx, w).reshape(B * n, C) * dout[:, 1:C + 1].double()).sum().backward()
    df = _bwd(dout, idx, w, B, n, m, C, ldo=C + 3, col0=1)
    check_close(df, f64.grad.reshape(B * m, C), TOL_F32, "dfeats")
    assert rel_err(df, f64.grad.reshape(B * m, C)) < 1e-5                  # (fp32 sums of up to 3 n terms at heavy fan-in)
    assert bool(torch.isfinite(df).all())
    unused = torch.ones(B * m, dtype=torch.bool, device=dev)
    unused[(idx.long() + torch.arange(B, device=dev).reshape(B, 1, 1) * m).reshape(-1)] = False
    assert bool((df[unused] == 0).all())                                                       # rows nobody references
    assert torch.equal(df, _bwd(dout, idx, w, B, n, m, C, ldo=C + 3, col0=1)), "me_three_interpolate_bwd is not deterministic"
    # through autograd (the module route)
    fr = f.clone().requires_grad_(True)
    out = heads._interpolate_rows(fr, idx, w)
    (out * dout[:, 1:C + 1]).sum().backward()
    assert torch.equal(fr.grad.reshape(B * m, C), df)


def test_three_interpolation_drop_in(dev):
    B, n, m, C = 2, 2048, 512, 32
    unknown, known = _cloud(B, n, 1).to(dev), _cloud(B, m, 2).to(dev)
    f = torch.randn(B, C, m).to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = M.three_interpolation(unknown, known, f)
    assert out.dtype == torch.float32 and out.shape == (B, C, n)
    dist, idx = M.three_nn(unknown, known)
    r = 1.0 / (dist.double() + 1e-8)
    f64 = f.detach().double().requires_grad_(True)
    want = _interp64(f64.transpose(1, 2), idx, r / r.sum(2, keepdim=True)).transpose(1, 2)
    check_close(out, want, TOL_F32, "three_interpolation")
    go = torch.randn(out.shape).to(dev)
    (out * go).sum().backward()
    (want * go.double()).sum().backward()
    check_close(f.grad, f64.grad, TOL_F32, "three_interpolation df")


# ----------------------------------------------------------------------------------------------------- the reference classes

def _load_case(z, name, dev):
    c = json.loads(str(z[f"{name}/config"]))
    dec = getattr(M, c["decoder"])(**c["dec"])
    head = M.SegHead(in_channels=dec.out_channels, **c["head"])
    for prefix, mod in (("decoder.", dec), ("head.", head)):
        pre = f"{name}/w/{prefix}"
        mod.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}, strict=True)
    t = lambda k: torch.from_numpy(z[k]).float().to(dev)          # noqa: E731
    p = [t(f"{name}/p{i}") for i in range(3) if f"{name}/p{i}" in z.files]
    f = [t(f"{name}/f{i}") for i in range(3) if f"{name}/f{i}" in z.files]
    extra = [torch.from_numpy(z[f"{name}/cls_label"]).to(dev)] if f"{name}/cls_label" in z.files else []
    return c, dec.to(dev).eval(), head.to(dev).eval(), p, f, extra


@pytest.mark.parametrize("name", ["s3dis", "part", "resample"])
def test_modules_equal_the_reference_classes(dev, name):
    z = np.load(os.path.join(GOLDEN, "pointseg.npz"))
    c, dec, head, p, f, extra = _load_case(z, name, dev)
    p_in, f_in = list(p), list(f)
    with torch.no_grad():
        f_out = dec(p, f, *extra)
        logits = head(f_out)
    check_close(f_out[:, :, :32], torch.from_numpy(z[f"{name}/f_out_head"]), TOL_F32, f"{name} decoder output")
    check_close(logits, torch.from_numpy(z[f"{name}/logits"]), TOL_F32, f"{name} logits")
    # the caller's lists are mutated as the reference mutates them
    assert len(p) == len(f) == dec.n_decoder_stages + 1 and p[0] is p_in[0] and p[-1] is p_in[-1]
    assert f[-1].shape[2] == f_in[-1].shape[2] - 1 and torch.equal(f[-1], f_in[-1][:, :, 1:])
    # the three_nn indices of every stage, in the reference's call order (coarsest stage first)
    stages = int(z[f"{name}/nn_stages"])
    for s in range(stages):
        i = -1 - s
        _, idx = heads.three_nn(p[i - 1], p[i])
        assert torch.equal(idx.cpu(), torch.from_numpy(z[f"{name}/nn{s}"].astype(np.int32))), f"{name} stage {s}: three_nn differs"
    # the split route computes the same
    p2, f2 = list(p_in), list(f_in)
    with torch.no_grad():
        g, tok = dec.forward_split(p2, f2, *extra)
        check_close(head.forward_split(g, tok), logits, 1e-5, f"{name} forward_split")


@pytest.mark.parametrize("name", ["dup", "m1", "m2"])
def test_three_interpolation_equals_the_reference(dev, name):
    z = np.load(os.path.join(GOLDEN, "pointseg.npz"))
    t = lambda k: torch.from_numpy(z[f"interp/{name}/{k}"]).float().to(dev)      # noqa: E731
    out = M.three_interpolation(t("unknown"), t("known"), t("feat"))
    check_close(out, torch.from_numpy(z[f"interp/{name}/out"]), TOL_F32, f"interp/{name}")
    _, idx = M.three_nn(t("unknown"), t("known"))
    assert torch.equal(idx.cpu(), torch.from_numpy(z[f"interp/{name}/idx"].astype(np.int32)))


# ----------------------------------------------------------------------------------------------------- full size vs float64

class _Recorder:
    """records the three_nn indices, max-pool arg-maxes and ReLU masks the modules use, in call order; the float64 restatement
    takes every discrete choice from here and so compares arithmetic only"""

    def __init__(self, monkeypatch):
        self.nn, self.arg, self.relu = [], [], []
        nnw, pool, relu = heads.three_nn_weights, heads.pool_tokens, torch.relu

        def r_relu(x):
            y = relu(x)
            self.relu.append(y.detach() > 0)
            return y

        def r_nn(u, k):
            i, w = nnw(u, k)
            self.nn.append(i.long())
            return i, w

        def r_pool(x, mode="mean"):
            self.arg.append(x.detach().argmax(dim=1) if mode == "max" else None)
            return pool(x, mode)
        monkeypatch.setattr(torch, "relu", r_relu)
        monkeypatch.setattr(heads, "three_nn_weights", r_nn)
        monkeypatch.setattr(heads, "pool_tokens", r_pool)


def _restate(dec, head, P, p, f, rec, cls_label=None):
    """decoder + head forward in float64 torch, token-major, on the recorded choices -> (logits [B, N, K], f_out [B, N, C])"""
    masks, nns, args = iter(rec.relu), iter(rec.nn), iter(rec.arg)

    def block(pre, blk, x):
        x = x @ P[pre + "0.weight"].reshape(blk[0].out_channels, -1).t()
        if blk[0].bias is not None:
            x = x + P[pre + "0.bias"]
        for j, mod in enumerate(list(blk)[1:], start=1):
            if isinstance(mod, torch.nn.BatchNorm1d):
                sh = x.shape
                if mod.training:
                    x = F.batch_norm(x.reshape(-1, sh[-1]), None, None, P[f"{pre}{j}.weight"], P[f"{pre}{j}.bias"], True, 0.0, mod.eps)
                else:
                    x = F.batch_norm(x.reshape(-1, sh[-1]), mod.running_mean.double(), mod.running_var.double(), P[f"{pre}{j}.weight"],
                                     P[f"{pre}{j}.bias"], False, 0.0, mod.eps)
                x = x.reshape(sh)
            elif isinstance(mod, torch.nn.LayerNorm):
                x = F.layer_norm(x, (x.shape[-1],), P[f"{pre}{j}.weight"], P[f"{pre}{j}.bias"], 1e-5)
            elif isinstance(mod, torch.nn.ReLU):
                x = x * next(masks).reshape(x.shape)
            elif isinstance(mod, torch.nn.GELU):
                x = F.gelu(x)
        return x

    def gmax(x):
        return torch.gather(x, 1, next(args).unsqueeze(1)).squeeze(1)

    B, N = p[0].shape[:2]
    cloud = None
    if cls_label is not None:
        oh = torch.zeros(B, 16, dtype=torch.float64, device=p[0].device).scatter_(1, cls_label.long(), 1)
        cloud = block("decoder.convc.0.", dec.convc[0], oh)
    cur = f[-1].transpose(1, 2)
    cls_tok, cur = cur[:, 0], cur[:, 1:]
    L = len(dec.decoder)
    for s, i in enumerate(range(-1, -L - 1, -1)):
        idx = next(nns)
        p1, p2 = p[i - 1].double(), p[i].double()
        nb = torch.gather(p2, 1, idx.reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, -1, 3, 3)
        r = 1.0 / ((nb - p1.unsqueeze(2)).pow(2).sum(-1).sqrt() + 1e-8)
        w = r / r.sum(2, keepdim=True)
        C = cur.shape[2]
        gat = torch.gather(cur, 1, idx.reshape(B, -1, 1).expand(-1, -1, C)).reshape(B, -1, 3, C)
        x = (w.unsqueeze(-1) * gat).sum(2)
        n = x.shape[1]
        parts = [f[i - 1].transpose(1, 2)] if f[i - 1] is not None else []
        if cloud is not None and i == -L:
            parts = [cloud.unsqueeze(1).expand(-1, n, -1)] + parts
        x = torch.cat(parts + [x], dim=2)
        si = L + i                                          # decoder[i] == decoder[L + i]
        for j, blk in enumerate(dec.decoder[si][0].convs):
            x = block(f"decoder.decoder.{si}.0.convs.{j}.", blk, x)
        cur = x
    gs = []
    for t in dec.global_feat or []:
        gs.append(cls_tok if "cls" in t else gmax(cur) if "max" in t else (next(args), cur.mean(1))[1])
    x = torch.cat([torch.cat(gs, 1).unsqueeze(1).expand(-1, N, -1), cur], dim=2) if gs else cur
    for mod in head.head:
        if isinstance(mod, torch.nn.Dropout):
            continue                                        # (kept in eval mode by the test)
        idx_in_head = list(head.head).index(mod)
        x = block(f"head.head.{idx_in_head}.", mod, x)
    return x, cur


def _full_size(dev, monkeypatch, part, B, N):
    torch.manual_seed(41)
    C = 768
    if part:
        dec = M.PointViTPartDecoder([7, 384, C], global_feat="cls,max,avg", progressive_input=True, act_args={"act": "gelu"})
        head = M.SegHead(50, dec.out_channels, mlps=[256], norm_args={"norm": "bn"})
    else:
        dec = M.PointViTDecoder([7, 384, C], global_feat="cls,max", progressive_input=True)
        head = M.SegHead(13, dec.out_channels, mlps=[256], norm_args={"norm": "ln1d"})
    for m in list(dec.modules()) + list(head.modules()):
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)):
            m.weight.data.normal_(1.0, 0.1)
            m.bias.data.normal_(0.0, 0.05)
    dec, head = dec.to(dev).train(), head.to(dev).train()
    head.head[1].eval()                                     # Dropout: the restatement has no mask to share
    g = torch.Generator().manual_seed(42)
    p0 = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dev)
    p1 = torch.gather(p0, 1, heads.furthest_point_sample(p0, N // 4).long().unsqueeze(-1).expand(-1, -1, 3))
    p2 = torch.gather(p1, 1, heads.furthest_point_sample(p1, N // 16).long().unsqueeze(-1).expand(-1, -1, 3))
    fs = [torch.randn(B, 7, N, generator=g).to(dev), torch.randn(B, 384, N // 4, generator=g).to(dev),
          torch.randn(B, C, N // 16 + 1, generator=g).to(dev)]
    cls_label = torch.randint(0, 16, (B, 1), generator=g).to(dev) if part else None
    extra = [cls_label] if part else []
    rec = _Recorder(monkeypatch)
    fr = [t.clone().requires_grad_(True) for t in fs]
    gl, tok = dec.forward_split([p0, p1, p2], list(fr), *extra)
    logits = head.forward_split(gl, tok)
    go = torch.randn(logits.shape, generator=g).to(dev)
    (logits * go).sum().backward()
    monkeypatch.undo()
    params = {**{"decoder." + k: v for k, v in dec.named_parameters()}, **{"head." + k: v for k, v in head.named_parameters()}}
    P = {k: v.detach().double().requires_grad_(True) for k, v in params.items()}
    f64 = [t.double().requires_grad_(True) for t in fs]
    ref, ref_tok = _restate(dec, head, P, [p0, p1, p2], list(f64), rec, cls_label)
    check_close(tok, ref_tok, TOL_F32, "decoder f_out")
    check_close(logits, ref.transpose(1, 2), TOL_F32, "logits")
    (ref.transpose(1, 2) * go.double()).sum().backward()
    top = max(float(P[k].grad.abs().max()) for k in P)
    for k, v in params.items():
        if float(P[k].grad.abs().max()) < 1e-6 * top:
            assert float(v.grad.abs().max()) <= TOL_F32 * top, f"d{k}"
        else:
            check_close(v.grad, P[k].grad, TOL_F32, f"d{k}")
    for i, (a, b) in enumerate(zip(fr, f64)):
        check_close(a.grad, b.grad, TOL_F32, f"df{i}")
    # the reference interfaces compute the same
    with torch.no_grad():
        dec.eval(), head.eval()
        g2, t2 = dec.forward_split([p0, p1, p2], list(fs), *extra)
        full = head(dec([p0, p1, p2], list(fs), *extra))
        check_close(head.forward_split(g2, t2), full, 1e-5, "forward_split vs forward")


@pytest.mark.slow
def test_full_size_s3dis_vs_float64(dev, monkeypatch):
    _full_size(dev, monkeypatch, False, 8, 24000)


@pytest.mark.slow
def test_full_size_shapenetpart_vs_float64(dev, monkeypatch):
    _full_size(dev, monkeypatch, True, 8, 2048)


# ----------------------------------------------------------------------------------------------------- end to end

def test_p3embed_encoder_decoder_head_end_to_end(dev):
    torch.manual_seed(51)
    B, N, D = 2, 2048, 192
    emb = M.P3Embed(sample_ratio=0.0625, group_size=32, in_channels=7, embed_dim=D, group="knn",
                    norm_args={"norm": "ln2d"}).to(dev).train()
    enc = M.build_encoder(2, D, 3).to(dev)
    for q in enc.parameters():
        q.requires_grad_(False)
    cls = torch.nn.Parameter(torch.randn(1, 1, D, device=dev) * 0.02)
    ch = list(emb.channel_list)
    ch[-1] = D
    dec = M.PointViTDecoder(ch, global_feat="cls,max", progressive_input=True).to(dev).train()
    head = M.SegHead(13, dec.out_channels, mlps=[64], norm_args={"norm": "ln1d"}).to(dev).train()
    p = (torch.rand(B, N, 3) * 2 - 1).to(dev)
    x = torch.cat([p.transpose(1, 2), torch.rand(B, 4, N).to(dev)], dim=1).contiguous()
    out_p, out_f = emb(p, x)
    tokens = torch.cat([cls.expand(B, -1, -1), out_f[-1].transpose(1, 2)], dim=1).contiguous()
    y = enc(tokens).float()
    f = list(out_f)
    f[-1] = y.transpose(1, 2)
    logits = head(dec(list(out_p), f))
    assert logits.shape == (B, 13, N) and logits.dtype == torch.float32
    labels = torch.randint(0, 13, (B, N)).to(dev)
    F.cross_entropy(logits, labels).backward()
    for name, mod in (("p3embed", emb), ("decoder", dec), ("head", head)):
        for k, q in mod.named_parameters():
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), f"{name}.{k}"
        assert sum(float(q.grad.abs().sum()) for q in mod.parameters()) > 0, name
    assert cls.grad is not None and bool(torch.isfinite(cls.grad).all()) and float(cls.grad.abs().sum()) > 0
