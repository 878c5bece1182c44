"""CPU: tests/epilogue_cases.py against float64 and against torch -- the emulations of the GELU forms of csrc/common.h stay inside the
error bounds that header states, the integer form of the bf16 store is torch's conversion bit for bit, the constructed pre-activations
are exact, and every case of test_gpu_gemm_epilogue_values.py covers what it claims (points, gaps, ties, overflows)."""
import math

import pytest
import torch

import epilogue_cases as ec

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def dense_grid():
    """2.4 M points in [-12, 12] (step 1e-5) and the joints of the forms with their fp32 neighbours"""
    x = torch.arange(-1_200_000, 1_200_001, dtype=F64) * 1e-5
    sp = ec.special_biases()
    sp = sp[torch.isfinite(sp) & (sp.abs() <= 12)]
    return torch.cat((x.float(), sp))


@pytest.fixture(scope="module")
def grid():
    return dense_grid()


def test_polynomial_forms_stay_inside_the_stated_bounds(grid):
    """common.h: |gelu err| <= 1.9e-4, |gelu' err| <= 4.2e-4 for "this exact float32 formula" -- and beyond the clamp the tails are flat"""
    err = (ec.emu_gelu_bf16(grid).double() - ec.gelu64(grid)).abs()
    derr = (ec.emu_gelu_bf16_grad(grid).double() - ec.gelu_grad64(grid)).abs()
    i, k = int(err.argmax()), int(derr.argmax())
    print(f"gelu (polynomial): max error {float(err[i]):.4e} at x = {float(grid[i]):.4f}; gelu': {float(derr[k]):.4e} at x = {float(grid[k]):.4f}")
    assert float(err[i]) <= ec.GELU_BF16_ERR
    assert float(derr[k]) <= ec.GELU_BF16_GRAD_ERR
    far = torch.tensor([4.0, 5.0, 12.0, 30.0, 1e4, 3e38, math.inf], dtype=F32)
    far = torch.cat((far, -far))
    assert float((ec.emu_gelu_bf16(far).double() - ec.gelu64(far))[torch.isfinite(far)].abs().max()) <= ec.GELU_BF16_ERR
    assert float((ec.emu_gelu_bf16_grad(far).double() - ec.gelu_grad64(far)).abs().max()) <= ec.GELU_BF16_GRAD_ERR
    # the ramp: for x >= 12 the polynomial part is below half a bf16 step of x, so the stored value is x itself
    big = torch.tensor([12.0, 12.0625, 30.0, 1e4, 3e38, math.inf], dtype=F32)
    assert torch.equal(ec.bf16_bits_rne(ec.emu_gelu_bf16(big)), ec.bf16_bits_rne(big))


def test_erf_forms_stay_inside_their_measured_error(grid):
    y, dy = ec.emu_gelu_erf_pair(grid)
    err, derr = (y.double() - ec.gelu64(grid)).abs(), (dy.double() - ec.gelu_grad64(grid)).abs()
    print(f"gelu (erf): max error {float(err.max()):.3e}; gelu': {float(derr.max()):.3e}")
    assert float(err.max()) <= ec.GELU_ERF_ERR
    assert float(derr.max()) <= ec.GELU_ERF_GRAD_ERR


def test_nan_through_the_emulations():
    """what the formulas as written do with a quiet NaN: the erf forms propagate it; min / max drop it from the polynomial forms, which
    give t P(4) (about -1e-4) and 1/2 +- 4 Q(4) (0 or 1 by the NaN's sign bit)"""
    nan = torch.tensor([math.nan, -math.nan], dtype=F32)
    y, dy = ec.emu_gelu_erf_pair(nan)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(dy).all())
    p, dp = ec.emu_gelu_bf16(nan), ec.emu_gelu_bf16_grad(nan)
    assert bool((p.abs() <= ec.GELU_BF16_ERR).all()), p
    assert bool(((dp - torch.tensor([1.0, 0.0])).abs() <= ec.GELU_BF16_GRAD_ERR).all()), dp


def test_bf16_bits_rne_is_torchs_conversion():
    g = torch.Generator().manual_seed(7)
    rnd = torch.randint(0, 1 << 32, (1 << 20,), generator=g, dtype=torch.int64)
    x = torch.cat((ec.special_biases(), ec.f32_from_bits(rnd)))
    got, want = ec.bf16_bits_rne(x), ec.bf16_bits(x.to(BF16))
    nan = torch.isnan(x)
    assert torch.equal(got[~nan], want[~nan])
    assert bool(ec.bf16_bits_is_nan(got[nan]).all()) and bool(ec.bf16_bits_is_nan(want[nan]).all()) and int(nan.sum()) > 1000
    # the patterns do what their names say
    for bits, up in ((ec._TIES_DOWN, False), (ec._TIES_UP, True)):
        t = ec.f32_from_bits(bits)
        r = ec.bf16_bits_rne(t)
        assert torch.equal(r, (ec.f32_bits(t) >> 16) + (1 if up else 0))
    assert bool((ec.bf16_bits_rne(ec.f32_from_bits(ec._OVERFLOW)) == 0x7F80).all())
    assert ec.bf16_bits_rne(ec.f32_from_bits([0x7F7F7FFF])).item() == 0x7F7F


def test_bf16_half_ulp_is_the_rounding_bound_and_2_pow_minus_9_is_not():
    """The store's share of the GELU bounds.  The correctly rounded store of an EXACT value is off by up to half a unit in the last of
    bf16's 8 significant bits, 2^(floor(log2 |v|) - 8): that is 2^-9 |v| only at the top of a binade and 2^-8 |v| at its bottom, so a
    bound of 2^-9 |ref| fails the float64 reference itself (127.25 -> 127.5).  bf16_half_ulp is the exact figure: every value meets it,
    ties reach it, and it never exceeds 2^-8 |v|."""
    g = torch.Generator().manual_seed(9)
    v = torch.cat((torch.randn(1 << 18, generator=g) * 4, torch.tensor([127.25, 1.00390625, 3e38, 2.0 ** -14, 0.0])))
    stored = v.to(BF16).double()
    err, hu = (stored - v.double()).abs(), ec.bf16_half_ulp(v.double())
    assert bool((err <= hu).all())
    assert bool((hu <= 2.0 ** -8 * v.double().abs()).all()) and bool((hu > 2.0 ** -9 * v.double().abs())[v != 0].all())
    assert int((err > 2.0 ** -9 * v.double().abs()).sum()) > 1000          # the reference alone breaks 2^-9 |ref|
    ties = ec.f32_from_bits(ec._TIES_UP + ec._TIES_DOWN)
    assert torch.equal((ties.to(BF16).double() - ties.double()).abs(), ec.bf16_half_ulp(ties.double()))


def test_gg8_code():
    g = torch.tensor([-0.13, -0.129, 0.0, 0.5, 1.0, 1.129, 1.13, -1.0, 2.0], dtype=F64)
    q = ec.gg8_code(g)
    assert q.tolist() == [0, 0, 26, 128, 229, 255, 255, 0, 255]
    dec = ec.GG8_LO + ec.GG8_STEP * q[:7].double()
    assert float((dec - g[:7]).abs().max()) <= 0.5 * ec.GG8_STEP + 1e-12
    a, b = ec.gg8_decode32(torch.arange(256))
    assert float((a.double() - (ec.GG8_LO + ec.GG8_STEP * torch.arange(256).double())).abs().max()) < 2e-7
    assert float((a - b).abs().max()) <= 2.0 ** -23


SHAPES = [(130, 132, 72, 1), (200, 384, 2048, 8), (300, 776, 512, 2), (264, 328, 4133, 33)]


@pytest.mark.parametrize("M,N,K,parts", SHAPES)
def test_sum_mode_is_exact_and_covers(M, N, K, parts):
    j, scale = ec.sweep_rows(M)
    A, B, acc = ec.operands(M, N, K, j, scale, torch.ones(N), parts)
    r = j.double() * scale.double()
    assert torch.equal(acc.double(), r[:, None].expand(M, N))
    for t in (A, B):      # the stored operands are bf16-exact
        assert torch.equal(t.to(BF16).float(), t)
    # ... and the product of the stored operands in float64 IS the accumulator, with one piece in every part
    assert torch.equal(A.double() @ B.double().t(), acc.double())
    cols = ec.part_columns(K, parts)
    assert len(set(cols)) == parts and all(0 <= c < K for c in cols)
    assert int((A[:, cols] != 0).sum(1).max()) == min(parts, ec.R_J)
    bias = ec.bias_values(N)
    x = acc + bias[None, :]
    valid = ec.exact(x, acc, bias[None, :].expand(M, N))
    # float64 -> float32 -> float64 round trip of the constructed sums
    s = acc.double() + bias.double()[None, :]
    assert torch.equal(s[valid].float().double(), s[valid])
    zero = j == 0
    assert bool(valid[zero][:, ~torch.isnan(bias)].all())                     # every bias reaches the epilogue unchanged on the zero rows
    sweep = (bias.abs() <= 16) & (ec.f32_bits(bias) & 0x3FF == 0)
    assert bool(valid[:, sweep].all())
    cov = ec.coverage(x, valid)
    print(cov)
    assert cov["points"] >= 4096 and cov["gap"] <= 2.0 ** -6
    assert cov["ties_up"] >= 64 and cov["ties_down"] >= 64 and cov["overflows"] >= 16


@pytest.mark.parametrize("M,N,K,parts", SHAPES)
@pytest.mark.parametrize("tn", [False, True])
def test_prod_mode_is_exact_and_covers(M, N, K, parts, tn):
    j, scale = ec.sweep_rows(M, overflow_rows=True)
    c = ec.prod_cols(N)
    A, B, acc = ec.operands(M, N, K, j, scale, c, parts, tn=tn)
    for t in (A, B):
        assert torch.equal(t.to(BF16).float(), t)
    full = (A.double().t() @ B.double()) if tn else (A.double() @ B.double().t())
    fin = torch.isfinite(acc)
    assert torch.equal(full[fin], acc.double()[fin]) and bool((full[~fin].abs() >= 2.0 ** 128).all())
    # every partial sum over the parts, in any order, is a multiple of one quantum and no larger than the total: sum the parts in fp32
    # forwards and backwards
    cols = ec.part_columns(K, parts)
    Ap = (A[cols, :].t() if tn else A[:, cols])
    for order in (range(parts), reversed(range(parts))):
        run = torch.zeros(M, N)
        for i in order:
            run = run + Ap[:, i:i + 1] * c[None, :]
        assert torch.equal(run[fin], acc[fin])
    add = ec.small_operand(M, N, zero_rows=scale != ec.R_SCALE)
    for x, terms in ((acc, (acc,)), (acc + add, (acc, add)), (0.5 * acc + 2.0 * add, (0.5 * acc.double(), 2.0 * add.double()))):
        valid = ec.exact(x, *terms)
        cov = ec.coverage(x, valid)
        print(cov)
        assert float(valid.float().mean()) > 0.9
        assert cov["ties_up"] >= 64 and cov["ties_down"] >= 64
    # finite products that round to bf16 inf (alpha = 1/2 halves them out of that range: only the alpha = 1 forms have them)
    assert ec.coverage(acc, ec.exact(acc, acc))["overflows"] >= 16
    assert ec.coverage(acc + add, ec.exact(acc + add, acc, add))["overflows"] >= 16


def test_aux_values_cover_the_bf16_range():
    allv = ec.finite_bf16_values()
    assert allv.numel() == 65280
    for M, N in ((130, 132), (200, 384), (300, 264)):
        a = ec.aux_values(M, N)
        assert a.shape == (M, N) and a.dtype == BF16 and bool(torch.isfinite(a.float()).all())
        have = torch.unique(ec.bf16_bits(a))
        mid = ec.bf16_bits(ec.finite_bf16_values(limit=16.0, floor=2.0 ** -6))
        assert bool(torch.isin(mid, have).all())
        if M * N >= 65536:
            assert have.numel() == 65280
        assert float(a.float().abs().max()) >= 16.0          # the joint of the polynomial at |x| = 4 and both tails are inside
    jf, sf = ec.factor_rows(7)
    assert (jf.double() * sf.double()).tolist() == [1.0, -2.0, 0.5, 1.0, -2.0, 0.5, 1.0]
