"""GPU: the LayerNorm entry points (me_layernorm_fwd / _bwd, me_row_stats, me_row_stats_combine) over every kernel the dispatcher has,
with guard bands: every input sits between NaN guards, every output, statistics vector and the backward workspace between sentinel
guards (tests/guarded.py).  The reference is torch's LayerNorm in float64 on the device and its autograd, from the stored operands.

Widths: cols = 256 V for every V in 1..16 (the register-resident kernels; V <= 4 takes two rows per wave = 8 per block, above that 4)
plus the generic widths 4, 57, 100 and 4100.  Rows 1, 13 (ragged against both rows-per-block values; in backward most blocks of the
persistent grid then own no row and their partials must fold as zeros) and 4101 (more than one wave of blocks).
Bounds: those of test_layernorm_fwd / _bwd in test_gpu_ops.py -- 1e-5 (fp32 out) / 8e-3 (bf16 out) forward, 1e-4 / 1e-2 backward,
statistics 1e-5."""
import pytest
import torch
import torch.nn.functional as F

from conftest import check_close
from guarded import Guarded
from metatransformer_amd import _capi

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
ROWS = [1, 13, 4101]
VEC_WIDTHS = [256 * v for v in range(1, 17)]
GENERIC_WIDTHS = [4, 57, 100, 4100]
X3 = "x3"      # ME_BF16X3 output: [hi | lo | hi] bf16 planes of the fp32 result


def _code(dt):
    return _capi.ME_BF16X3 if dt == X3 else (_capi.ME_F32 if dt == F32 else _capi.ME_BF16)


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _affine(dev, cols, g):
    return 1 + 0.1 * torch.randn(cols, device=dev, generator=g), 0.1 * torch.randn(cols, device=dev, generator=g)


def _stats64(x):
    xd = x.double()
    mean = xd.mean(-1)
    return mean, 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + EPS)


def ln_fwd(lib, dev, x, gamma, beta, ydt, what, eps=EPS):
    """me_layernorm_fwd on guarded buffers -> (y as float64 [rows, cols], mean, rstd, y Guarded); the guards are checked here"""
    rows, cols = x.shape
    X, G, B = Guarded.input(x), Guarded.input(gamma), Guarded.input(beta)
    Y = Guarded.output(rows, 3 * cols if ydt == X3 else cols, None, BF16 if ydt == X3 else ydt, dev)
    Mn, Rs = Guarded.output_vec(rows, F32, dev), Guarded.output_vec(rows, F32, dev)
    _capi.check(lib.me_layernorm_fwd(X.ptr(), _code(x.dtype), G.ptr(), B.ptr(), Y.ptr(), _code(ydt), Mn.ptr(), Rs.ptr(), rows, cols, eps,
                                     _capi.stream_ptr()), "me_layernorm_fwd")
    torch.cuda.synchronize()
    for o, nm in ((Y, "y"), (Mn, "mean"), (Rs, "rstd")):
        o.check(f"{what}: {nm}")
        assert not bool(torch.isnan(o.t).any()), f"{what}: NaN in {nm}"
    y = Y.t.double()
    if ydt == X3:
        assert torch.equal(Y.t[:, 2 * cols:], Y.t[:, :cols]), f"{what}: the third plane repeats hi"
        y = y[:, :cols] + y[:, cols:2 * cols]
    return y, Mn.vec(), Rs.vec(), Y


FWD_FORMS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16), (F32, X3)]


@pytest.mark.parametrize("cols", VEC_WIDTHS + GENERIC_WIDTHS)
def test_layernorm_fwd_contract(dev, cols):
    lib = _capi.load()
    for rows in ROWS:
        g = _gen(dev, cols + rows)
        x32 = torch.randn(rows, cols, device=dev, generator=g) * 2 + 0.5
        gamma, beta = _affine(dev, cols, g)
        for xdt, ydt in FWD_FORMS:
            if ydt == X3 and not (cols % 256 == 0 and cols // 256 <= 16):
                continue
            what = f"layernorm fwd {rows} x {cols} {xdt} -> {ydt}"
            x = x32.to(xdt)
            ref = F.layer_norm(x.double(), (cols,), gamma.double(), beta.double(), EPS)
            mean, rstd = _stats64(x)
            y, mn, rs, _ = ln_fwd(lib, dev, x, gamma, beta, ydt, what)
            check_close(y, ref, 8e-3 if ydt == BF16 else 1e-5, what)
            check_close(mn, mean, 1e-5, what + " mean")
            check_close(rs, rstd, 1e-5, what + " rstd")


@pytest.mark.parametrize("cols", [256 * v for v in range(1, 9)] + [57, 100, 2304])
def test_row_stats_contract(dev, cols):
    """me_row_stats: the pairs (rstd, -rstd * mean) of the same LayerNorm, V in 1..8 plus the generic kernel (by width, and 2304 = V 9)"""
    lib = _capi.load()
    for rows in ROWS:
        g = _gen(dev, 3 * cols + rows)
        x32 = torch.randn(rows, cols, device=dev, generator=g) * 2 + 0.5
        for xdt in (F32, BF16):
            what = f"row_stats {rows} x {cols} {xdt}"
            x = x32.to(xdt)
            mean, rstd = _stats64(x)
            X, out = Guarded.input(x), Guarded.output(rows, 2, None, F32, dev)
            _capi.check(lib.me_row_stats(X.ptr(), _code(xdt), out.ptr(), rows, cols, EPS, _capi.stream_ptr()), "me_row_stats")
            torch.cuda.synchronize()
            out.check(what)
            assert not bool(torch.isnan(out.t).any()), what
            check_close(out.t[:, 0], rstd, 1e-5, what + " rstd")
            check_close(out.t[:, 1], -rstd * mean, 1e-5, what + " -rstd * mean")


@pytest.mark.parametrize("nparts", [1, 2, 3, 4])
def test_row_stats_combine_contract(dev, nparts):
    """me_row_stats_combine: (mean, M2) partials over 256-column groups, laid out [nparts][rows], fold to the pairs of the whole row"""
    lib = _capi.load()
    cols = 256 * nparts
    for rows in ROWS:
        what = f"row_stats_combine {rows} x {cols}"
        g = _gen(dev, 7 * nparts + rows)
        # groups with different means: the between-group term of the combination carries weight
        x = (torch.randn(rows, nparts, 256, device=dev, generator=g) * 2 + 3 * torch.randn(rows, nparts, 1, device=dev, generator=g)).double()
        gm = x.mean(-1)
        m2 = ((x - gm[..., None]) ** 2).sum(-1)
        parts = torch.stack((gm, m2), -1).permute(1, 0, 2).contiguous().float()       # [nparts][rows][2]
        assert parts.numel() * 4 == lib.me_row_stats_partial_bytes(rows, cols)
        P, out = Guarded.input(parts.reshape(-1)), Guarded.output(rows, 2, None, F32, dev)
        _capi.check(lib.me_row_stats_combine(P.ptr(), rows, cols, EPS, out.ptr(), _capi.stream_ptr()), "me_row_stats_combine")
        torch.cuda.synchronize()
        out.check(what)
        mean, rstd = _stats64(x.reshape(rows, cols))
        assert not bool(torch.isnan(out.t).any()), what
        check_close(out.t[:, 0], rstd, 1e-5, what + " rstd")
        check_close(out.t[:, 1], -rstd * mean, 1e-5, what + " -rstd * mean")


# ------------------------------------------------------------------------------------------------ backward
def ln_bwd_case(lib, dev, rows, cols, xdt, dydt, dxdt, dresdt, seed):
    """one (shape, dtype form): dx / dgamma / dbeta against float64 autograd with the affine gradients overwritten, then accumulated
    a second time (-> twice the reference), then without them (need_affine off)"""
    what = f"layernorm bwd {rows} x {cols} x {xdt} dy {dydt} dx {dxdt} dres {dresdt}"
    g = _gen(dev, seed)
    x = (torch.randn(rows, cols, device=dev, generator=g) * 2 + 0.5).to(xdt)
    dy = torch.randn(rows, cols, device=dev, generator=g).to(dydt)
    dres = torch.randn(rows, cols, device=dev, generator=g).to(dresdt) if dresdt is not None else None
    gamma, beta = _affine(dev, cols, g)
    xr, gr, br = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.layer_norm(xr, (cols,), gr, br, EPS).backward(dy.double())
    dx_ref = xr.grad + (dres.double() if dres is not None else 0.0)
    mean, rstd = _stats64(x)
    X, DY, Mn, Rs, G = Guarded.input(x), Guarded.input(dy), Guarded.input(mean.float()), Guarded.input(rstd.float()), Guarded.input(gamma)
    DR = Guarded.input(dres) if dres is not None else None
    DG, DB = Guarded.output_vec(cols, F32, dev), Guarded.output_vec(cols, F32, dev)
    t_dx = 1e-4 if (xdt, dydt, dxdt, dresdt or F32) == (F32, F32, F32, F32) else 1e-2
    first = None
    for step, (affine, acc) in enumerate(((True, 0), (True, 1), (False, 0))):
        DX = Guarded.output(rows, cols, None, dxdt, dev)
        W = Guarded.output_bytes(lib.me_layernorm_bwd_workspace(cols), dev)
        _capi.check(lib.me_layernorm_bwd(DY.ptr(), _code(dydt), X.ptr(), _code(xdt), Mn.ptr(), Rs.ptr(), G.ptr(),
                                         DR.ptr() if DR else None, _code(dresdt) if DR else 0, DX.ptr(), _code(dxdt),
                                         DG.ptr() if affine else None, DB.ptr() if affine else None, acc, rows, cols, W.ptr(),
                                         _capi.stream_ptr()), "me_layernorm_bwd")
        torch.cuda.synchronize()
        w = f"{what} (affine {affine}, accumulate {acc})"
        for o, nm in ((DX, "dx"), (DG, "dgamma"), (DB, "dbeta"), (W, "workspace")):
            o.check(f"{w}: {nm}")
        assert not bool(torch.isnan(DX.t).any()), f"{w}: NaN in dx"
        if first is None or not torch.equal(DX.t, first):
            check_close(DX.t, dx_ref, t_dx, w + " dx")
        first = DX.t if first is None else first
        if affine:
            assert not bool(torch.isnan(DG.t).any()) and not bool(torch.isnan(DB.t).any()), f"{w}: NaN in dgamma / dbeta"
            check_close(DG.vec(), (1 + acc) * gr.grad, t_dx, w + " dgamma")
            check_close(DB.vec(), (1 + acc) * br.grad, t_dx, w + " dbeta")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cols", [256 * v for v in range(1, 9)] + [57, 2304])
def test_layernorm_bwd_contract(dev, cols, rows):
    """V in 1..8 (the persistent kernels) and the generic path by width: every (x, dy) dtype pair, with and without dres"""
    lib = _capi.load()
    for i, (xdt, dydt) in enumerate(((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16))):
        for dresdt in (None, xdt):
            ln_bwd_case(lib, dev, rows, cols, xdt, dydt, xdt, dresdt, seed=cols + rows + i)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("xdt,dxdt,dresdt", [(F32, BF16, None), (BF16, F32, None), (F32, F32, BF16), (BF16, BF16, F32), (BF16, F32, F32)])
def test_layernorm_bwd_stream_dtype_mismatch(dev, rows, xdt, dxdt, dresdt):
    """a dx or dres dtype that differs from x's sends a vector width to the generic kernels"""
    ln_bwd_case(_capi.load(), dev, rows, 768, xdt, xdt, dxdt, dresdt, seed=rows + 99)


# ------------------------------------------------------------------------------------------------ two numeric edges
@pytest.mark.parametrize("cols", [768, 100])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_layernorm_constant_rows(dev, cols, dt):
    """rows of one repeated value (dyadic, so that sum and mean are exact in fp32): the deviations are exactly zero -- y == beta
    bit for bit, rstd = eps^-1/2 to 1e-6, and the backward through these rows is finite and meets float64"""
    lib = _capi.load()
    consts = torch.tensor([0.0, 1.0, -2.5, 3.25, 1000.0, -0.015625, 7.0, 96.0, -512.0, 0.5, 2.0, -1.0, 24.0], device=dev)
    rows = consts.numel()
    x = consts[:, None].expand(rows, cols).contiguous().to(dt)
    g = _gen(dev, cols)
    gamma, beta = _affine(dev, cols, g)
    what = f"constant rows {cols} {dt}"
    y, mn, rs, Y = ln_fwd(lib, dev, x, gamma, beta, dt, what)
    assert torch.equal(Y.t, beta.to(dt)[None, :].expand(rows, cols)), f"{what}: y != beta"
    assert torch.equal(mn, consts), f"{what}: mean"
    assert float((rs.double() - EPS ** -0.5).abs().max()) <= 1e-6 * EPS ** -0.5, f"{what}: rstd {rs.tolist()}"
    dy = torch.randn(rows, cols, device=dev, generator=g).to(dt)
    X, DY, Mn, Rs, G = Guarded.input(x), Guarded.input(dy), Guarded.input(mn), Guarded.input(rs), Guarded.input(gamma)
    DX, DG, DB = Guarded.output(rows, cols, None, dt, dev), Guarded.output_vec(cols, F32, dev), Guarded.output_vec(cols, F32, dev)
    W = Guarded.output_bytes(lib.me_layernorm_bwd_workspace(cols), dev)
    _capi.check(lib.me_layernorm_bwd(DY.ptr(), _code(dt), X.ptr(), _code(dt), Mn.ptr(), Rs.ptr(), G.ptr(), None, 0, DX.ptr(), _code(dt),
                                     DG.ptr(), DB.ptr(), 0, rows, cols, W.ptr(), _capi.stream_ptr()), "me_layernorm_bwd")
    torch.cuda.synchronize()
    for o in (DX, DG, DB, W):
        o.check(what + " backward")
    assert bool(torch.isfinite(DX.t).all()) and bool(torch.isfinite(DG.t).all()) and bool(torch.isfinite(DB.t).all()), f"{what}: backward not finite"
    xr = x.double().requires_grad_(True)
    F.layer_norm(xr, (cols,), gamma.double(), beta.double(), EPS).backward(dy.double())
    check_close(DX.t, xr.grad, 1e-4 if dt == F32 else 1e-2, what + " dx")


# Rows whose mean is 1e3 times their spread.  No bound is known a priori, so the yardstick is measured where the test runs: torch's own
# fp32 LayerNorm (torch.native_layer_norm on the device) against the float64 reference on the same stored inputs, and the kernel may
# err 4 x as much (the margin is for a different but equally sound summation order), never less than 4 units of fp32 roundoff (2^-24)
# so that an exact yardstick does not ask for exact results.  Metric: max-abs error over max-abs reference, per output (y, mean, rstd).
# Measured on MI355X (yardstick = torch fp32 -> bound = 4 x; the kernel's own error behind it, fp32 output):
#   cols  x dtype   y                                mean                             rstd
#   768   fp32      4.64e-05 -> 1.86e-04 (3.7e-05)   1.30e-07 -> 5.19e-07 (1.2e-07)   4.12e-06 -> 1.65e-05 (5.4e-08)
#   100   fp32      9.99e-05 -> 4.00e-04 (3.2e-05)   2.45e-07 -> 9.79e-07 (8.6e-08)   9.78e-06 -> 3.91e-05 (6.6e-08)
#   768   bf16      1.58e-03 -> 6.32e-03 (5.8e-06)   8.20e-08 -> 3.28e-07 (2.7e-08)   4.22e-08 -> 2.38e-07 (4.2e-08)
#   100   bf16      1.23e-02 -> 4.92e-02 (5.9e-06)   2.64e-07 -> 1.06e-06 (3.9e-08)   3.33e-04 -> 1.33e-03 (4.2e-08)
# (bf16 rows near 1000 are stored in steps of 4: most elements of a row are equal, the variance is small and torch's fp32
#  statistics lose part of it; the two-pass kernel, which subtracts an exact mean, does not.)  bf16 -> bf16 output: 1.7e-03 / 2.8e-03 against the bound + 2^-9.


@pytest.mark.parametrize("cols", [768, 100])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_layernorm_rows_far_off_centre(dev, cols, dt):
    lib = _capi.load()
    rows = 64
    g = _gen(dev, cols + 5)
    spread = 0.5 + torch.rand(rows, 1, device=dev, generator=g)
    sign = torch.where(torch.rand(rows, 1, device=dev, generator=g) < 0.5, -1.0, 1.0)
    x = (spread * (1000.0 * sign + torch.randn(rows, cols, device=dev, generator=g))).to(dt)      # (bf16: the stored values, steps of 4)
    gamma, beta = _affine(dev, cols, g)
    ref = F.layer_norm(x.double(), (cols,), gamma.double(), beta.double(), EPS)
    mean, rstd = _stats64(x)

    def err(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())
    ty, tm, tr = torch.native_layer_norm(x.float(), (cols,), gamma, beta, EPS)
    yard = {"y": err(ty, ref), "mean": err(tm.reshape(rows), mean), "rstd": err(tr.reshape(rows), rstd)}
    what = f"far-off-centre rows {cols} {dt}"
    y, mn, rs, _ = ln_fwd(lib, dev, x, gamma, beta, F32, what)
    got = {"y": err(y, ref), "mean": err(mn, mean), "rstd": err(rs, rstd)}
    bound = {k: 4.0 * max(v, 2.0 ** -24) for k, v in yard.items()}
    print(f"{what}: " + ", ".join(f"{k} torch fp32 {yard[k]:.3e} -> bound {bound[k]:.3e}, kernel {got[k]:.3e}" for k in yard))
    for k in yard:
        assert got[k] <= bound[k], f"{what}: {k} error {got[k]:.3e} exceeds 4 x torch's fp32 error {yard[k]:.3e}"
    if dt == BF16:      # the bf16 -> bf16 form: the same plus the rounding of the output, half a bf16 ulp = 2^-9 of the element
        yb, _, _, _ = ln_fwd(lib, dev, x, gamma, beta, BF16, what + " -> bf16")
        eb = err(yb, ref)
        print(f"{what} -> bf16: kernel {eb:.3e}, bound {bound['y'] + 2.0 ** -9:.3e}")
        assert eb <= bound["y"] + 2.0 ** -9, f"{what} -> bf16: {eb:.3e}"
