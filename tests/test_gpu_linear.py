"""GPU: metatransformer_amd.linear -- the differentiable Linear on me_gemm (heads.linear) and the weight-gradient call its neighbours
share.  The reference is torch.nn.functional.linear in fp64 on the operands as the kernel sees them (bf16 cases: x, W and the incoming
gradient rounded to bf16; the bias stays fp32); bounds are conftest's: fp32 TOL_F32, bf16 TOL_BF16_OP forward / TOL_BF16_GRAD gradients."""
import pytest
import torch
import torch.nn.functional as F

from conftest import TOL_BF16_GRAD, TOL_BF16_OP, TOL_F32, check_close
from metatransformer_amd import MetaEncError, heads
from metatransformer_amd import linear as L

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
TOLS = {torch.float32: (TOL_F32, TOL_F32), torch.bfloat16: (TOL_BF16_OP, TOL_BF16_GRAD)}      # (forward, gradients)


def _rand(shape, dt, seed):
    """fp32 values that ``dt`` holds exactly"""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dt).float()


def _run(dev, x, w, b, go, x_dtype, x_grad=True, **kw):
    """linear() on the device -> (y, dx or None, dW, db or None); x goes in as ``x_dtype``, the parameters as fp32"""
    xd = x.to(dev, x_dtype).requires_grad_(x_grad)
    wd = w.to(dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True) if b is not None else None
    y = L.linear(xd, wd, bd, **kw)
    assert y.dtype == torch.float32 and y.shape == (*x.shape[:-1], w.shape[0]) and y.is_contiguous()
    (y * go.to(dev)).sum().backward()
    return y, xd.grad, wd.grad, bd.grad if bd is not None else None


def _ref(x, w, b, go, cdt):
    """the same in fp64, W rounded to the compute dtype as the kernel reads it"""
    x64 = x.double().requires_grad_(True)
    w64 = w.to(cdt).double().requires_grad_(True)
    b64 = b.double().requires_grad_(True) if b is not None else None
    y = F.linear(x64, w64, b64)
    (y * go.double()).sum().backward()
    return y, x64.grad, w64.grad, b64.grad if b64 is not None else None


def _compare(got, want, dt, what):
    f_tol, g_tol = TOLS[dt]
    for name, g, r, tol in zip(("y", "dx", "dW", "db"), got, want, (f_tol, g_tol, g_tol, g_tol)):
        if r is None or (name == "dx" and g is None):
            assert g is None, f"{what}: {name} should be None"
            continue
        check_close(g.float(), r, tol, f"{what} {name}")


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("xshape,N", [((5, 8), 7), ((16, 24), 8), ((13, 40), 174), ((2, 5, 8), 16)],
                         ids=["every_pad", "no_pad", "video174", "3d"])
def test_linear_matches_fp64(dev, xshape, N, dt, with_bias):
    K = xshape[-1]
    x, w, go = _rand(xshape, dt, 1), _rand((N, K), torch.float32, 2), _rand((*xshape[:-1], N), dt, 3)
    b = _rand((N,), torch.float32, 4) if with_bias else None
    got = _run(dev, x, w, b, go, dt)
    assert got[1].dtype == dt and got[1].shape == xshape and got[2].shape == (N, K)
    _compare(got, _ref(x, w, b, go, dt), dt, f"linear {xshape} -> {N}")


@pytest.mark.parametrize("cdt", DTYPES, ids=["fp32", "bf16"])
def test_k_padded_inside_for_data_rows(dev, cdt):
    """hyperspectral's route: 27 band neighbours, fp32 rows that are data, the compute dtype given"""
    x, w, b, go = _rand((12, 27), cdt, 5), _rand((16, 27), torch.float32, 6), _rand((16,), torch.float32, 7), _rand((12, 16), cdt, 8)
    got = _run(dev, x, w, b, go, torch.float32, x_grad=False, compute_dtype=cdt)
    assert got[1] is None and got[2].shape == (16, 27)
    want = _ref(x, w, b, go, cdt)
    _compare(got, (want[0], None, want[2], want[3]), cdt, "x [12, 27] as data")


def test_weight_narrower_than_padded_rows(dev):
    """the point-embed route: the gather kernel wrote xyz rows 8 columns wide, the Conv2d weight has 3"""
    x = torch.zeros(10, 8)
    x[:, :3] = _rand((10, 3), torch.float32, 9)
    w, go = _rand((16, 3), torch.float32, 10), _rand((10, 16), torch.float32, 11)
    y, dx, dw, _ = _run(dev, x, w, None, go, torch.float32)
    ry, rdx, rdw, _ = _ref(x[:, :3], w, None, go, torch.float32)
    assert dw.shape == (16, 3) and dx.shape == (10, 8)
    check_close(y, ry, TOL_F32, "y")
    check_close(dw, rdw, TOL_F32, "dW")
    check_close(dx[:, :3], rdx, TOL_F32, "dx")
    assert not dx[:, 3:].any()
    with pytest.raises(MetaEncError):
        L.linear(x.to(dev), torch.zeros(16, 9, device=dev), None)      # 8 columns against 9
    with pytest.raises(MetaEncError):
        L.linear(torch.zeros(10, 16, device=dev), w.to(dev), None)     # wider than the weight's granule


@pytest.mark.parametrize("K", [288, 128], ids=["three_chunks_last_partial", "one_chunk"])
def test_k_chunk_fp32(dev, K):
    x, w, b, go = _rand((13, K), torch.float32, 12), _rand((24, K), torch.float32, 13), _rand((24,), torch.float32, 14), _rand((13, 24), torch.float32, 15)
    _compare(_run(dev, x, w, b, go, torch.float32, k_chunk=128), _ref(x, w, b, go, torch.float32), torch.float32, f"k_chunk=128, K = {K}")


def test_k_chunk_bf16_is_one_call(dev):
    x, w, b, go = _rand((13, 288), torch.bfloat16, 16), _rand((24, 288), torch.float32, 17), _rand((24,), torch.float32, 18), _rand((13, 24), torch.bfloat16, 19)
    for g, r in zip(_run(dev, x, w, b, go, torch.bfloat16, k_chunk=128), _run(dev, x, w, b, go, torch.bfloat16)):
        assert torch.equal(g, r)


def test_inplace_relu_behind_a_padded_n(dev):
    """ClsHead puts nn.ReLU(inplace=True) straight behind its Linear: the sliced result must be no view"""
    x, w, b, go = _rand((6, 16), torch.float32, 20), _rand((7, 16), torch.float32, 21), _rand((7,), torch.float32, 22), _rand((6, 7), torch.float32, 23)
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    z = torch.relu_(L.linear(xd, wd, bd))
    (z * go.to(dev)).sum().backward()
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    r = torch.relu(F.linear(x64, w64, b64))
    (r * go.double()).sum().backward()
    for name, g, want in (("y", z, r), ("dx", xd.grad, x64.grad), ("dW", wd.grad, w64.grad), ("db", bd.grad, b64.grad)):
        check_close(g, want, TOL_F32, name)


def test_fp16_rows_compute_in_bf16(dev):
    x, w, b, go = _rand((5, 8), torch.float16, 24), _rand((7, 8), torch.float32, 25), _rand((7,), torch.float32, 26), _rand((5, 7), torch.bfloat16, 27)
    got = _run(dev, x, w, b, go, torch.float16)
    assert got[1].dtype == torch.float16
    xb = x.bfloat16().float()                                             # what the bf16 kernel reads
    _compare(got, _ref(xb, w, b, go, torch.bfloat16), torch.bfloat16, "fp16 rows")
    assert torch.equal(got[0], _run(dev, xb, w, b, go, torch.bfloat16)[0])


def test_refusals_and_the_heads_name(dev):
    assert heads.linear is L.linear
    with pytest.raises(MetaEncError, match="CUDA tensors only"):
        L.linear(torch.zeros(8, 8), torch.zeros(8, 8), None)


@pytest.mark.parametrize("dt", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("M", [8, 13])
def test_wgrad(dev, M, dt):
    N, K = 16, 24
    d, x = _rand((M, N), dt, 28), _rand((M, K), dt, 29)
    dd, xd = d.to(dev, dt), x.to(dev, dt)
    tol = TOLS[dt][1]
    rdw, rdb = d.double().t() @ x.double(), d.double().sum(0)
    dw, none = L.wgrad(dd, xd)
    assert none is None and dw.dtype == torch.float32
    check_close(dw, rdw, tol, "dW")
    for fused in (False, True):
        dw_b, db = L.wgrad(dd, xd, bias=True, fused_bias=fused)
        assert torch.equal(dw_b, dw) and db.dtype == torch.float32
        check_close(db, rdb, tol, f"db (fused_bias={fused})")
    # the row pad is zero rows and nothing else: the same data with the rows appended here gives the same bits
    rows = -M % 8
    by_hand = L.wgrad(torch.cat([dd, torch.zeros(rows, N, dtype=dt, device=dev)]), torch.cat([xd, torch.zeros(rows, K, dtype=dt, device=dev)]))[0]
    assert torch.equal(dw, by_hand)
