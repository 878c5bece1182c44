"""CPU: keeps tests/ew_cases.py honest without a GPU -- every reference there that is more than one torch call is tied to torch
itself, and the case tables are checked for the properties the GPU tests rely on."""
import math

import pytest
import torch
import torch.nn.functional as F

import ew_cases as ew
import metatransformer_amd as M
from ew_cases import BF16, F16, F32


def test_cast_specials_hold_what_they_claim():
    sp = ew.cast_specials()
    b = ew.bits(sp).to(torch.int64) & 0xFFFFFFFF
    assert int(((b & 0xFFFF) == 0x8000).sum()) >= 6, "exact bf16 ties"
    assert int(((b & 0x1FFF) == 0x1000).sum()) >= 6, "exact fp16 ties"
    for lo_even, lo_odd, dt in ((0x3F808000, 0x3F818000, BF16), (0x3F801000, 0x3F803000, F16)):
        e, o = ew._f32_from_bits([lo_even, lo_odd])
        assert float(e.to(dt)) < float(e) and float(o.to(dt)) > float(o), "ties go to the even neighbour: down, then up"
    assert bool(torch.isinf(sp).any()) and bool((sp == 0).sum() >= 2) and bool(torch.signbit(sp[sp == 0]).any())
    assert bool(((sp != 0) & (sp.abs() < 1.17e-38)).any()), "fp32 denormals"
    big = torch.tensor([3.4028234663852886e38, 65520.0, 65504.0])
    assert torch.isinf(big.to(BF16))[0] and torch.isinf(big.to(F16))[1] and float(big.to(F16)[2]) == 65504.0


@pytest.mark.parametrize("n", ew.CAST_SIZES[:-1])
def test_cast_input_places_the_specials(n):
    x = ew.cast_input(n, F32)
    sp = ew.cast_specials()
    assert x.shape == (n,)
    if n >= 2 * sp.numel():
        tail = x[n - 3:]
        assert torch.equal(ew.bits(tail), ew.bits(sp.flip(0)[-3:])), "the n % 4 tail holds specials"
    if n >= 3 * sp.numel():
        assert int(torch.isnan(x).sum()) == 2
    else:
        assert not bool(torch.isnan(x).any())
    again = ew.cast_input(n, F32)
    ew.assert_bits_equal(again, x, "deterministic", nan_by_isnan=True)


def test_assert_bits_equal_sees_a_signed_zero():
    a, b = torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])
    ew.assert_bits_equal(a, a.clone(), "same")
    with pytest.raises(AssertionError, match="flat index 0"):
        ew.assert_bits_equal(a, b, "zero sign")


def test_split3_planes_reassemble():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(257, 260, generator=g) * torch.logspace(-3, 3, 260)
    hi, lo = ew.split3_planes(x)
    assert torch.equal(hi, x.bfloat16())
    err = (hi.double() + lo.double() - x.double()).abs() / x.double().abs()
    assert float(err.max()) <= 2.0 ** -16
    left, right = ew.split3_ref(x, False), ew.split3_ref(x, True)
    assert torch.equal(left[:, :260], hi) and torch.equal(left[:, 260:520], lo) and torch.equal(left[:, 520:], hi)
    assert torch.equal(right[:, :260], hi) and torch.equal(right[:, 260:520], hi) and torch.equal(right[:, 520:], lo)


def test_adamw_reference_is_torch_adamw_with_parameter_groups():
    n, ends = 1027, [1, 2, 7, 1027]
    scales, wds = [1.0, 0.5, 0.25, 2.0], [0.0, 0.05, 0.1, 0.01]
    lr, b1, b2, eps = 1e-2, 0.9, 0.95, 1e-8
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    ls, wd = ew.segment_vectors(n, ends, scales, wds)
    assert float(ls[0]) == 1.0 and float(ls[1]) == 0.5 and float(ls[6]) == 0.25 and float(ls[7]) == 2.0
    params, b = [], 0
    for e in ends:
        params.append(p0[b:e].clone().requires_grad_(True))
        b = e
    opt = torch.optim.AdamW([{"params": [q], "lr": lr * s, "weight_decay": w} for q, s, w in zip(params, scales, wds)],
                            lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=g, dtype=torch.float64)
        b = 0
        for q, e in zip(params, ends):
            q.grad = 0.5 * grad[b:e].clone()
            b = e
        opt.step()
        p, m, v = ew.adamw_ref_step(p, grad, m, v, lr * ls, wd, b1, b2, eps, step, grad_scale=0.5)
        got = torch.cat([q.detach() for q in params])
        assert float((got - p).abs().max() / p.abs().max()) < 1e-13, step
    assert float((p - p0).abs().max()) > 1e-3, "the steps moved the parameters"


def test_adamw_ctl_reference():
    c = ew.adamw_ctl_ref(0, None, None, 0.5, 0.0, 0.9, 0.95)
    assert c["step"] == 1 and c["grad_mul"] == 0.5 and c["skip"] == 0.0 and c["total_norm"] == 0.0
    assert abs(c["bc1"] - (1 - ew.f32(0.9))) < 1e-15
    c = ew.adamw_ctl_ref(1, (8.0, 0.0), 4.0, 1.0, 1.0, 0.9, 0.95)          # norm 2 -> clipped to 1
    assert abs(c["total_norm"] - 2.0) < 1e-12 and abs(c["grad_mul"] - 0.25 / (2.0 + 1e-6)) < 1e-9 and c["step"] == 2
    c = ew.adamw_ctl_ref(1, (8.0, 0.0), 4.0, 1.0, 10.0, 0.9, 0.95)         # not clipped
    assert c["grad_mul"] == 0.25
    c = ew.adamw_ctl_ref(3, (8.0, 1.0), None, 1.0, 1.0, 0.9, 0.95)
    assert c["skip"] == 1.0 and c["found_inf"] == 1.0 and c["step"] == 3
    assert ew.bias_correction_tol(0.999, 1) > 1e-4 and ew.bias_correction_tol(0.9, 3) < 2e-6


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("freq,n_mark", [("h", 4), ("t", 5)])
def test_ts_embed_reference_is_dataembedding(L, freq, n_mark):
    """against the modules M.DataEmbedding is made of, run by torch on the CPU: its circular Conv1d, its embedding tables, its pe"""
    torch.manual_seed(7)
    cin, C, B = 7, 100, 2
    emb = M.DataEmbedding(cin, C, "fixed", freq).eval()
    x = torch.randn(B, L, cin)
    sizes = [13, 32, 7, 24, 4][:n_mark]
    marks = torch.stack([torch.randint(0, s, (B, L)) for s in sizes], dim=-1)
    tabs = [t.detach() for t in emb.temporal_embedding.tables()]
    assert len(tabs) == n_mark
    pe = emb.position_embedding.pe[0]
    with torch.no_grad():
        want = emb.value_embedding.tokenConv(x.permute(0, 2, 1)).transpose(1, 2)
        t = emb.temporal_embedding
        temporal = t.hour_embed.emb(marks[..., 3]) + t.weekday_embed.emb(marks[..., 2]) + t.day_embed.emb(marks[..., 1]) + t.month_embed.emb(marks[..., 0])
        if n_mark == 5:
            temporal = temporal + t.minute_embed.emb(marks[..., 4])
        want = want + temporal + pe[None, :L]
    got = ew.ts_embed_ref(x, emb.value_embedding.tokenConv.weight.detach(), marks, tabs, pe)
    assert float((got - want.double()).abs().max()) < 2e-5 * float(want.abs().max())
    bare = ew.ts_embed_ref(x, emb.value_embedding.tokenConv.weight.detach(), None, [], None)
    with torch.no_grad():
        assert float((bare - emb.value_embedding.tokenConv(x.permute(0, 2, 1)).transpose(1, 2).double()).abs().max()) < 1e-5


@pytest.mark.parametrize("L", [1, 2, 5])
def test_ts_unfold_reference_gives_the_conv_weight_gradient(L):
    torch.manual_seed(8)
    B, cin, C = 2, 7, 4
    x = torch.randn(B, L, cin, dtype=torch.float64)
    w = torch.randn(C, cin, 3, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, L, C, dtype=torch.float64)
    ew.ts_embed_ref(x, w, None, [], None).backward(dy)
    u = ew.ts_unfold_ref(x, 3 * cin + 5)
    assert bool((u[:, 3 * cin:] == 0).all()) and not bool(torch.signbit(u[:, 3 * cin:]).any())
    dw = dy.reshape(B * L, C).t() @ u[:, :3 * cin]
    assert float((dw.reshape(C, cin, 3) - w.grad).abs().max()) < 1e-12


def test_argmax_first_takes_the_first_of_equal_maxima():
    x = torch.tensor([[[1.0, -math.inf, 2.0], [3.0, -math.inf, 2.0], [3.0, -math.inf, 0.0]]])       # [1, 3, 3]
    assert ew.argmax_first(x).tolist() == [[1, 0, 0]]
    g = torch.Generator().manual_seed(2)
    y = torch.randn(3, 37, 8, generator=g)
    assert torch.equal(ew.argmax_first(y).long(), y.argmax(dim=1)), "no ties: torch's arg-max"


@pytest.mark.parametrize("B,H,W,ws", [(2, 3, 5, 7), (1, 4, 4, 1), (2, 5, 6, 4)])
def test_window_references_invert_each_other(B, H, W, ws):
    x = torch.arange(B * H * W * 4, dtype=torch.float32).reshape(B * H * W, 4) + 1
    win = ew.window_partition_ref(x, B, H, W, ws)
    gh, gw = -(-H // ws), -(-W // ws)
    assert win.shape == (B * gh * gw * ws * ws, 4)
    assert int((win == 0).all(dim=1).sum()) == B * (gh * gw * ws * ws - H * W), "padded positions are zero rows"
    assert torch.equal(ew.window_merge_ref(win, B, H, W, ws), x)
    # element (b, y, x) sits at window (y // ws, x // ws), inside position (y % ws, x % ws)
    b, yy, xx = B - 1, H - 1, W - 1
    r = (((b * gh + yy // ws) * gw + xx // ws) * ws + yy % ws) * ws + xx % ws
    assert torch.equal(win[r], x[(b * H + yy) * W + xx])


@pytest.mark.parametrize("shape,k,s", [((3, 2, 30, 27), (6, 6), (5, 7)), ((2, 1, 36, 46), (16, 16), (10, 10)),
                                       ((1, 2, 4, 16, 16), (2, 8, 8), (2, 8, 8))])
def test_patch_references_agree_with_the_convolution(shape, k, s):
    geom = ew.geom6(k, s)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    cols = ew.patches_ref(x, geom)
    K = cols.shape[1]
    w = torch.randn(12, K, generator=g, dtype=torch.float64)
    bias = torch.randn(12, generator=g, dtype=torch.float64)
    y = ew.patch_embed_ref(x, w, bias, None, geom)
    assert float(((cols @ w.t() + bias).reshape(y.shape) - y).abs().max()) < 1e-11
    # one explicit element: token 1 of sample 0 (px = 1), feature (c = last, dt = 0, dy = 1, dx = 2)
    kt, kh, kw, st, sh, sw = geom
    c = shape[1] - 1
    f = ((c * kt + 0) * kh + 1) * kw + 2
    src = x[0, c, 1, sw + 2] if x.dim() == 4 else x[0, c, 0, 1, sw + 2]
    assert float(cols[1, f]) == float(src)
    dy = torch.randn(cols.shape[0], 12, generator=g, dtype=torch.float64)
    dw, db = ew.patch_embed_grads_ref(x, dy, geom, 12)
    assert float((dw - dy.t() @ cols).abs().max()) < 1e-10 and float((db - dy.sum(0)).abs().max()) < 1e-11


def test_resize_reference_identity_and_layout():
    g = torch.Generator().manual_seed(6)
    t = torch.randn(16, 4, generator=g, dtype=torch.float64)
    for mode in ("bilinear", "bicubic"):
        assert torch.equal(ew.resize_ref(t, 4, 4, 4, 4, mode), t)
        up = ew.resize_ref(t, 4, 4, 5, 7, mode)
        want = F.interpolate(t.t().reshape(1, 4, 4, 4), size=(5, 7), mode=mode, align_corners=False).reshape(4, 35).t()
        assert torch.equal(up, want)


def test_yardstick_bound_has_a_floor():
    assert ew.yardstick_bound(0.0) == 4 * 2.0 ** -24 and ew.yardstick_bound(1e-3) == 4e-3


def test_close_tol_is_the_threshold_of_check_close():
    from conftest import check_close
    g = torch.Generator().manual_seed(9)
    ref = torch.randn(50, 8, generator=g, dtype=torch.float64)
    a = ref + 1e-4 * torch.randn(50, 8, generator=g, dtype=torch.float64)
    a[3, 3] = ref[3, 3] + 1e-3 * float(ref.abs().max())           # one large error at an arbitrary element
    t = ew.close_tol(a, ref)
    check_close(a, ref, t * (1 + 1e-9), "at the threshold")
    with pytest.raises(AssertionError):
        check_close(a, ref, t * 0.99, "below it")
    assert ew.close_tol(ref, ref) == 0.0
