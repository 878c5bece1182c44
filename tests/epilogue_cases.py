"""Known values for the me_gemm epilogues: float64 references, float32 emulations of the GELU forms of csrc/common.h, the bf16 rounding
store as integer arithmetic, the ME_GG8 code, and operand builders whose accumulators are EXACT -- so that a test of the epilogue's
values (test_gpu_gemm_epilogue_values.py) sees the epilogue's error alone and can ask for the stored bits.  A plain module (like
ew_cases.py, stoch_cases.py): everything runs on CPU tensors too, which is how tests/test_epilogue_cases_cpu.py checks it; nothing here
calls the library.

Exact accumulators.  Row m of the left operand carries ONE value r_m = j_m * s_m (an integer |j| <= 255 times a power of two: bf16-exact),
every row of the right operand one value c_n, both in the same reduction columns and zeros everywhere else, so the accumulator is
  "sum"  mode (c_n = 1):           r_m                    -- the pre-activation is x[m, n] = r_m + bias[n], one fp32 addition
  "prod" mode (c_n = odd * 2^-7):  r_m * c_n              -- a 16-bit product: many of them are ties for the bf16 store
whatever order the kernel reduces in.  For a plan that splits the reduction into P parts |j_m| is dealt out as P non-negative integers,
one per part (column (2 i + 1) K / (2 P) lies in part i of an even split): every partial sum is a multiple of one quantum, bounded by
the total, hence exact in fp32 in any order -- the fold really sums.  Row and old-C operands are s * 2^-9 with |s| <= 255.
An element is ASSERTED only where the float64 sum of the pieces equals the fp32 value (`valid`): on the rows with r_m = 0 that is every
bias, which is how values beyond |x| = 16 (+-30, +-1e4, +-3e38, the rounding patterns, +-inf) reach the epilogue.

Left out on purpose: subnormal values (whether the kernels flush them is not part of the contract -- masked where an operand or a
product is one) and -0 (the accumulator of a zero row is +0, and +0 + (-0) = +0: a -0 bias cannot reach the epilogue)."""
from __future__ import annotations

import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

# ------------------------------------------------------------------------------------------------ float64 references


def gelu64(x: torch.Tensor) -> torch.Tensor:
    """x Phi(x), by erfc on the negative side (no cancellation in the tail); the limit 0 at -inf"""
    x = x.double()
    phi = torch.where(x < 0, 0.5 * torch.erfc(-x / math.sqrt(2.0)), 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))))
    return torch.where(x == -math.inf, torch.zeros_like(x), x * phi)


def gelu_grad64(x: torch.Tensor) -> torch.Tensor:
    """Phi(x) + x phi(x); the limits 0 and 1 at -inf and +inf"""
    x = x.double()
    phi = torch.where(x < 0, 0.5 * torch.erfc(-x / math.sqrt(2.0)), 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))))
    return phi + torch.where(torch.isinf(x), torch.zeros_like(x), x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


# ------------------------------------------------------------------------------------------------ float32 emulations of csrc/common.h
# Operation for operation, every result rounded to fp32 (torch's fp32 tensor arithmetic does not fuse): the kernels may contract a
# multiply and an add into one FMA, which the tests allow 2^-18 for.  The constants are common.h's.
GELU_BF16_P = (-7.715494112e-06, 7.679707389e-04, -1.074723536e-02, 6.040871459e-02, -1.453980336e-01, 4.842520777e-02, 3.880065109e-01, -0.5)
GELU_BF16_Q = (-5.104965709e-04, 7.796528677e-03, -4.375422062e-02, 9.542723363e-02, 1.391019310e-02, -3.006181013e-01, 1.278037861e-02,
               7.978845608e-01)
GELU_BF16_ERR, GELU_BF16_GRAD_ERR = 1.9e-4, 4.2e-4          # the bounds common.h states for the two polynomial forms
GELU_ERF_ERR, GELU_ERF_GRAD_ERR = 4.65e-7, 2.98e-7          # measured for the erf forms on [-12, 12] when the forms were written down


def _c(v: float, like: torch.Tensor) -> torch.Tensor:
    return torch.tensor(v, dtype=F32, device=like.device)


def emu_gelu_clamp(x: torch.Tensor) -> torch.Tensor:
    """gelu_clamp4: v_min_f32 |x|, 4.0 -- IEEE minNum: a quiet NaN gives the OTHER operand, 4"""
    assert x.dtype == F32
    return torch.fmin(x.abs(), _c(4.0, x))


def _horner(t: torch.Tensor, coef) -> torch.Tensor:
    p = t * _c(coef[0], t) + _c(coef[1], t)
    for c in coef[2:]:
        p = p * t + _c(c, t)
    return p


def emu_gelu_bf16(x: torch.Tensor) -> torch.Tensor:
    """gelu_bf16_4: t P(t) + max(x, 0), t = min(|x|, 4)   (v_max_f32 0, x: NaN gives 0)"""
    t = emu_gelu_clamp(x)
    return t * _horner(t, GELU_BF16_P) + torch.fmax(x, _c(0.0, x))


def emu_gelu_bf16_grad(x: torch.Tensor) -> torch.Tensor:
    """gelu_bf16_grad4: 1/2 + copysign(t Q(t), x)"""
    t = emu_gelu_clamp(x)
    return _c(0.5, x) + torch.copysign(t * _horner(t, GELU_BF16_Q), x)


def emu_phi_parts(x: torch.Tensor):
    """phi_parts4: (Phi(x), exp(-x^2 / 2)) by Abramowitz-Stegun 7.1.26; the reciprocal and the exponential are correctly rounded here
    (v_rcp_f32 / v_exp_f32 are 1-ulp approximations: the tests allow for that)"""
    assert x.dtype == F32
    ax = x.abs()
    w = ax * _c(0.84932180028801907, x)
    u = w * _c(0.27273748087922245, x) + _c(1.0, x)
    nw2 = -(w * w)
    t = _c(1.0, x) / u
    e = torch.exp2(nw2.double()).float()
    poly = t * _c(0.5307027145, x) - _c(0.7265760135, x)
    poly = poly * t + _c(0.7107068705, x)
    poly = poly * t - _c(0.142248368, x)
    poly = poly * t + _c(0.127414796, x)
    q = poly * t * e
    hmq = _c(0.5, x) - q
    return _c(0.5, x) + torch.copysign(hmq, x), e


def emu_gelu_erf_pair(x: torch.Tensor):
    """gelu_erf_pair4: (gelu, gelu') from one Phi / Gaussian"""
    phi, g = emu_phi_parts(x)
    return x * phi, phi + x * g * _c(0.3989422804014327, x)


# ------------------------------------------------------------------------------------------------ the stores
def f32_bits(x: torch.Tensor) -> torch.Tensor:
    """the bit pattern of fp32 values as int64 in [0, 2^32)"""
    assert x.dtype == F32
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def f32_from_bits(bits) -> torch.Tensor:
    b = torch.as_tensor(bits, dtype=torch.int64)
    return torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32).view(F32)


def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    """the bit pattern of bf16 values as int64 in [0, 2^16)"""
    assert x.dtype == BF16
    return x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bf16_bits_rne(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 bits, round to nearest even, by integer arithmetic on the fp32 bits; a NaN stays a (quiet) NaN"""
    b = f32_bits(x)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(torch.isnan(x), (b >> 16) | 0x40, r)


def bf16_bits_is_nan(b: torch.Tensor) -> torch.Tensor:
    return (b & 0x7FFF) > 0x7F80


def same_bf16_bits(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """element-wise: the same bits, or both NaN (the payload of a NaN is not part of the contract)"""
    return (got == want) | (bf16_bits_is_nan(got) & bf16_bits_is_nan(want))


def bf16_half_ulp(a: torch.Tensor) -> torch.Tensor:
    """half a unit in the last place of a bf16 value of magnitude a (float64): 2^(floor(log2 a) - 8), 0 at 0.  bf16 keeps 8 significant
    bits, so this lies between 2^-9 a (top of a binade) and 2^-8 a (its bottom): 2^-9 |ref| alone is NOT a bound on the rounding of an
    exact value -- 127.25 stores as 127.5, 0.25 = 2^-8.99 x 127.25 away (tests/test_epilogue_cases_cpu.py)."""
    m, ex = torch.frexp(a.double().abs())
    return torch.where(a == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), ex - 9))


GG8_LO, GG8_STEP = -0.13, 1.26 / 255.0


def gg8_code(g: torch.Tensor) -> torch.Tensor:
    """ME_GG8 (include/metaenc.h): q = rne(clamp((g + 0.13) * 255 / 1.26, 0, 255)), in float64"""
    return torch.round(((g.double() - GG8_LO) / GG8_STEP).clamp(0.0, 255.0)).to(torch.int64)


def gg8_decode32(q: torch.Tensor):
    """the two fp32 values -0.13 + q * 1.26 / 255 can come out as: the multiply and the add rounded separately, or fused"""
    lo, step = torch.tensor(GG8_LO, dtype=F32), torch.tensor(GG8_STEP, dtype=F32)
    qf = q.to(F32)
    return qf * step.to(q.device) + lo.to(q.device), (qf.double() * step.double().to(q.device) + lo.double().to(q.device)).float()


# ------------------------------------------------------------------------------------------------ value sets
R_SCALE = 0.25                                  # sweep rows: r_m = j / 4, j = -36 .. 36  -> [-9, 9]
R_J = 36
SWEEP_COLS = 64                                 # sweep columns: g_n = i * 2^-8, i = 0 .. 63 -> [0, 1/4): x = r + g covers [-9, 9.25) in steps of 2^-8
OVERFLOW_J = (181, 175, 187)                    # prod mode: 181 * 181, 175 * 187 lie in [32704, 32768): r c = 0x7F7F8000 .. as fp32, which round to inf
OVERFLOW_SCALE = 2.0 ** 120

_NB4 = [0x407FFFFF, 0x40800001, 0xC07FFFFF, 0xC0800001]                      # the fp32 neighbours of +-4
# exact ties between two bf16 neighbours (low 16 bits 0x8000), lower neighbour even -> magnitude rounds DOWN, odd -> UP
_TIES_DOWN = [0x3F808000, 0x42FE8000, 0x40008000, 0x3E808000, 0x3F848000, 0x41208000, 0x3D008000, 0x447A8000]
_TIES_UP = [0x3F818000, 0x42FF8000, 0x40018000, 0x3E818000, 0x3F858000, 0x41218000, 0x3D018000, 0x447B8000]
_NEAR_TIES = [0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001]
_OVERFLOW = [0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF]                             # finite fp32 that round to bf16 inf


def special_biases() -> torch.Tensor:
    """fp32 column values at which an epilogue can go wrong: zero and the smallest step, the joint of the polynomial forms at |x| = 4 with
    both fp32 neighbours, the flat tails, the rounding patterns of the bf16 store in both signs, +-inf and NaN"""
    plain = [0.0, 2.0 ** -14, -2.0 ** -14, 4.0, -4.0, 6.0, -6.0, 12.0, -12.0, 30.0, -30.0, 1e4, -1e4, 3e38, -3e38]
    pos = _TIES_DOWN + _TIES_UP + _NEAR_TIES + _OVERFLOW
    pats = _NB4 + pos + [b | 0x80000000 for b in pos]
    return torch.cat((torch.tensor(plain, dtype=F32), f32_from_bits(pats), torch.tensor([math.inf, -math.inf, math.nan], dtype=F32)))


def bias_values(N: int) -> torch.Tensor:
    """[N] fp32: the specials, then the sweep columns, then the sweep again half a step further (as often as N allows)"""
    sp = special_biases()
    sweep = torch.arange(SWEEP_COLS, dtype=F32) * 2.0 ** -8
    assert N >= sp.numel() + SWEEP_COLS, f"N = {N} is too narrow for the specials and one sweep"
    rest = N - sp.numel()
    i = torch.arange(rest)
    return torch.cat((sp, sweep[i % SWEEP_COLS] + (i // SWEEP_COLS % 2).to(F32) * 2.0 ** -9))


def sweep_rows(M: int, overflow_rows: bool = False):
    """(j [M] int64, scale [M] fp32): r_m = j_m * scale_m.  One row in eight (m % 8 == 0) is zero; the others walk j = -36 .. 36 at scale
    1/4; with overflow_rows the rows m % 8 == 4 carry +-OVERFLOW_J at 2^120 (prod mode: products at the top of the fp32 range)"""
    m = torch.arange(M)
    rank = m - m // 8 - 1
    j = rank % (2 * R_J + 1) - R_J
    j = torch.where(m % 8 == 0, torch.zeros_like(j), j)
    scale = torch.full((M,), R_SCALE, dtype=F32)
    if overflow_rows:
        big = m % 8 == 4
        oj = torch.tensor(OVERFLOW_J)[(m // 8) % 3] * (1 - 2 * ((m // 24) % 2))
        j = torch.where(big, oj, j)
        scale = torch.where(big, torch.tensor(OVERFLOW_SCALE, dtype=F32), scale)
    return j, scale


def factor_rows(M: int):
    """r_m in {1, -2, 1/2}: powers of two, so that r_m * f(aux) is f's own error scaled"""
    j = torch.tensor([1, -2, 1])[torch.arange(M) % 3]
    scale = torch.tensor([1.0, 1.0, 0.5], dtype=F32)[torch.arange(M) % 3]
    return j, scale


def prod_cols(N: int) -> torch.Tensor:
    """[N] fp32 c_n = odd * 2^-7, odd 8-bit; every fourth column one of OVERFLOW_J"""
    n = torch.arange(N)
    odd = 2 * ((n * 37) % 128) + 1
    odd = torch.where(n % 4 == 3, torch.tensor(OVERFLOW_J)[(n // 4) % 3], odd)
    return odd.to(F32) * 2.0 ** -7


def small_operand(M: int, N: int, zero_rows: torch.Tensor | None = None) -> torch.Tensor:
    """[M, N] fp32 s * 2^-9, |s| <= 255 (bf16-exact): a row or old-C operand; zero on `zero_rows`"""
    m, n = torch.arange(M)[:, None], torch.arange(N)[None, :]
    s = ((m * 131 + n * 71) % 511 - 255).to(F32) * 2.0 ** -9
    if zero_rows is not None:
        s = torch.where(zero_rows[:, None], torch.zeros_like(s), s)
    return s


def split_parts(j: torch.Tensor, P: int) -> torch.Tensor:
    """[M, P] int64: |j_m| dealt out as P non-negative integers (the extras start at part m % P), with j's sign"""
    a = j.abs()
    base, rem = a // P, a % P
    i = torch.arange(P)[None, :]
    m = torch.arange(j.numel())[:, None]
    return (base[:, None] + (((i + m) % P) < rem[:, None]).to(torch.int64)) * torch.sign(j)[:, None]


def part_columns(K: int, P: int):
    return [(2 * i + 1) * K // (2 * P) for i in range(P)]


def operands(M: int, N: int, K: int, j: torch.Tensor, scale: torch.Tensor, c: torch.Tensor, parts: int = 1, tn: bool = False, device="cpu"):
    """the stored operands (fp32 tensors of bf16-exact values) and the exact accumulator:  NT: A [M, K], B [N, K];  TN: A [K, M], B [K, N].
    Returns (A, B, acc [M, N] fp32)."""
    cols = torch.tensor(part_columns(K, parts), device=device)
    pieces = (split_parts(j, parts).to(F32) * scale[:, None]).to(device)
    A = torch.zeros(M, K, dtype=F32, device=device)
    B = torch.zeros(N, K, dtype=F32, device=device)
    A[:, cols] = pieces
    B[:, cols] = c.to(device)[:, None].expand(N, parts)
    acc = ((j.to(F64) * scale.to(F64))[:, None] * c.to(F64)[None, :]).float().to(device)       # (the product is exact, or overflows to inf)
    if tn:
        A, B = A.t().contiguous(), B.t().contiguous()
    return A, B, acc


def exact(x32: torch.Tensor, *terms64: torch.Tensor) -> torch.Tensor:
    """where the fp32 value equals the float64 sum of its pieces (which never rounds at these magnitudes): the elements a test may assert"""
    s = terms64[0].double()
    for t in terms64[1:]:
        s = s + t.double()
    return x32.double() == s


def is_subnormal(x: torch.Tensor) -> torch.Tensor:
    a = x.float().abs()
    return (a > 0) & (a < 2.0 ** -126)


def finite_bf16_values(limit: float | None = None, floor: float | None = None) -> torch.Tensor:
    """every finite bf16 value (all 65 280 bit patterns: zeros and subnormals too), or those with floor <= |x| <= limit, as bf16"""
    bits = torch.arange(1 << 16, dtype=torch.int64)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    v = torch.where(bits >= (1 << 15), bits - (1 << 16), bits).to(torch.int16).view(BF16)
    keep = torch.ones_like(bits, dtype=torch.bool)
    if limit is not None:
        keep &= v.float().abs() <= limit
    if floor is not None:
        keep &= v.float().abs() >= floor
    return v[keep]


def aux_values(M: int, N: int) -> torch.Tensor:
    """[M, N] bf16 for the gelu'(aux) and saved-factor reads: all 65 280 finite bf16 values where they fit, else every one with |x| <= 16
    (33 794), else -- the smallest cases of the table hold fewer elements than that -- every one with 2^-6 <= |x| <= 16 (5 122: the
    whole range on which gelu' moves by more than a bf16 step) followed by every fifth of the smaller ones.  The list repeats to fill
    the matrix."""
    total = M * N
    if total >= 65536:
        vals = finite_bf16_values()
    else:
        vals = finite_bf16_values(limit=16.0)
        if total < vals.numel():
            small = finite_bf16_values(limit=2.0 ** -6)
            vals = torch.cat((finite_bf16_values(limit=16.0, floor=2.0 ** -6), small[::5]))
            assert total >= vals.numel(), (M, N)
    return vals[torch.arange(total) % vals.numel()].reshape(M, N)


# ------------------------------------------------------------------------------------------------ coverage of a value set
def coverage(x32: torch.Tensor, valid: torch.Tensor) -> dict:
    """what the asserted elements of a case cover: distinct finite points and the widest gap inside [-9, 9]; ties of the bf16 store that
    round the magnitude up / down; finite values that round to inf"""
    x = x32[valid & torch.isfinite(x32)]
    b = f32_bits(x)
    tie = (b & 0xFFFF) == 0x8000
    inside = torch.unique(x[(x >= -9.0) & (x <= 9.0)].double())
    gap = float((inside[1:] - inside[:-1]).max()) if inside.numel() > 1 else math.inf
    if inside.numel() and (float(inside[0]) > -9.0 + 2.0 ** -6 or float(inside[-1]) < 9.0 - 2.0 ** -6):
        gap = math.inf
    return dict(points=int(inside.numel()), gap=gap, ties_up=int((tie & (((b >> 16) & 1) == 1)).sum()),
                ties_down=int((tie & (((b >> 16) & 1) == 0)).sum()), overflows=int(((b & 0x7FFFFFFF) >= 0x7F7F8000).sum()))
