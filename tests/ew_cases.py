"""Case tables and float64 references for the contract tests of the tokenizer, element-wise and optimizer entry points
(test_gpu_tokenizer_contract.py, test_gpu_elementwise_contract.py, test_gpu_optim_contract.py).  A plain module (like stoch_cases.py):
everything here runs on CPU tensors too, which is how tests/test_ew_cases_cpu.py ties each reference that is more than one torch call
to torch itself.

Every reference is computed from the STORED operands (the bf16 / fp32 values the kernel reads) in float64 and never calls the library.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# ------------------------------------------------------------------------------------------------ me_cast
CAST_DTYPES = [F32, BF16, F16]
# one grid sweep of the 4-wide kernel is 2048 blocks x 256 threads x 4 elements; the last size is a sweep + a second pass + a tail of 3
CAST_SWEEP = 2048 * 256 * 4
CAST_SIZES = [1, 2, 3, 4, 5, 7, 1023, 4099, CAST_SWEEP + 1024 + 3]
assert CAST_SIZES[-1] == 2_098_179


def _f32_from_bits(bits: Sequence[int]) -> torch.Tensor:
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int64).to(torch.int32).view(F32)


def cast_specials() -> torch.Tensor:
    """fp32 values at which a conversion can go wrong: signed zeros and infinities, fp32 denormals, the largest finite fp32 (overflows
    bf16 and fp16 when rounded), the fp16 edge (65504 is the largest fp16, 65520 the first value that rounds to inf), values that
    overflow fp16 only, and exact ties between two bf16 / two fp16 neighbours with the lower neighbour even and odd (round to nearest
    EVEN goes down for the first, up for the second), in both signs."""
    ties_bf16 = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x42FE8000, 0x42FF8000]      # bit 15 set, bits 0-14 clear
    ties_f16 = [0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x477FD000, 0x477FF000]       # bit 12 set, bits 0-11 clear (the last: 65520)
    near_ties = [0x3F808001, 0x3F807FFF, 0x3F801001, 0x3F800FFF]                             # one fp32 ulp off a tie: no longer a tie
    plain = torch.tensor([0.0, -0.0, math.inf, -math.inf, 1e-45, -1e-40, 1.1e-38, 3.4028234663852886e38, -3.4028234663852886e38,
                          65504.0, 65520.0, -65520.0, 1e5, -7e4, 6e-8, 3e-8, 6.1e-5, 1.0, -2.5], dtype=F32)
    return torch.cat((plain, _f32_from_bits(ties_bf16 + ties_f16 + near_ties)))


def cast_input(n: int, src: torch.dtype, seed: int = 0) -> torch.Tensor:
    """a normal sample of n values in `src` with the specials at the head and at the tail (the tail of n % 4 elements goes through
    other code than the body), rotated by n so that small sizes see different ones, and NaNs where there is room"""
    g = torch.Generator().manual_seed(1000 + seed + n)
    x = torch.randn(n, generator=g) * 3
    sp = cast_specials()
    S = sp.numel()
    k = min(n, S)
    idx = (torch.arange(k) + n) % S
    x[:k] = sp[idx]
    if n >= 2 * S:
        x[n - S:] = sp.flip(0)
    if n >= 3 * S:
        x[n // 2] = math.nan
        x[S + 1] = math.nan
    return x.to(src)


def bits(t: torch.Tensor) -> torch.Tensor:
    """integer view for bit-exact comparison"""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_bits_equal(got: torch.Tensor, want: torch.Tensor, what: str, nan_by_isnan: bool = False) -> None:
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = bits(got), bits(want)
    if nan_by_isnan:
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
        gb, wb = gb[~nan], wb[~nan]
        got, want = got[~nan], want[~nan]
    bad = gb != wb
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bit for bit; first at flat index {i}: "
                             f"got {float(got.flatten()[i])!r} (bits {int(gb.flatten()[i]) & 0xFFFFFFFF:#x}), "
                             f"want {float(want.flatten()[i])!r} (bits {int(wb.flatten()[i]) & 0xFFFFFFFF:#x})")


# ------------------------------------------------------------------------------------------------ me_split3
def split3_planes(x: torch.Tensor):
    """hi = bf16(x), lo = bf16(x - hi): each a single rounding of an exactly representable fp32 value (x - hi is exact in fp32)"""
    hi = x.to(BF16)
    lo = (x - hi.float()).to(BF16)
    return hi, lo


def split3_ref(x: torch.Tensor, right_operand: bool) -> torch.Tensor:
    """[rows, cols] fp32 -> [rows, 3 cols] bf16: [hi | lo | hi] (left operand) or [hi | hi | lo] (right operand)"""
    hi, lo = split3_planes(x)
    return torch.cat((hi, hi, lo) if right_operand else (hi, lo, hi), dim=1)


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_ref_step(p, g, m, v, lr, wd, beta1: float, beta2: float, eps: float, step: int, grad_scale: float = 1.0):
    """one step of torch.optim.AdamW (decoupled weight decay) restated per element in float64; lr and wd are per-element vectors (or
    scalars).  Returns new (p, m, v); the inputs are left alone."""
    p, g, m, v = p.double(), g.double() * grad_scale, m.double(), v.double()
    lr = torch.as_tensor(lr, dtype=torch.float64)
    wd = torch.as_tensor(wd, dtype=torch.float64)
    p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2_sqrt + eps))
    return p, m, v


def segment_vectors(n: int, ends: Sequence[int], lr_scale: Sequence[float], weight_decay: Sequence[float]):
    """per-element (lr scale, weight decay) of a segment table: segment k covers [ends[k - 1], ends[k])"""
    assert list(ends) == sorted(ends) and ends[-1] == n and len(ends) == len(lr_scale) == len(weight_decay)
    ls, wd = torch.empty(n, dtype=torch.float64), torch.empty(n, dtype=torch.float64)
    b = 0
    for e, s, w in zip(ends, lr_scale, weight_decay):
        ls[b:e], wd[b:e] = s, w
        b = e
    return ls, wd


def f32(x: float) -> float:
    """the value an fp32 argument of the C API carries"""
    return float(torch.tensor(x, dtype=F32))


def adamw_ctl_ref(step_before: int, stats, loss_scale: Optional[float], grad_scale: float, max_norm: float, beta1: float, beta2: float):
    """the control block me_adamw_prepare writes (include/metaenc.h), in float64 from the fp32 arguments:
        grad_mul = grad_scale / loss_scale * min(1, max_norm / (norm + 1e-6)),  norm = stats[0] * |grad_scale / loss_scale|
        found_inf = skip = stats[1] > 0 or norm not finite;  the step advances only when the step is taken."""
    mul = f32(grad_scale)
    if loss_scale is not None:
        mul /= f32(loss_scale)
    norm, bad = 0.0, 0.0
    if stats is not None:
        norm = float(stats[0]) * abs(mul)
        bad = 1.0 if (float(stats[1]) > 0 or not math.isfinite(norm) or norm > 3.0e38) else 0.0
        if max_norm > 0:
            mul *= min(1.0, f32(max_norm) / (norm + 1e-6))
    step = step_before + (0 if bad else 1)
    b1, b2 = f32(beta1), f32(beta2)
    return {"grad_mul": mul, "skip": bad, "found_inf": bad, "total_norm": norm, "step": step,
            "bc1": 1.0 - b1 ** step, "bc2_sqrt": math.sqrt(1.0 - b2 ** step)}


def bias_correction_tol(beta: float, step: int) -> float:
    """relative bound on 1 - powf(beta, step) formed in fp32: powf is within 2 ulp (2^-22 relative) of beta^step, the subtraction
    carries that absolute error into a result of size 1 - beta^step, plus the roundings of the subtraction and the square root"""
    b = f32(beta) ** step
    return 2.0 ** -22 * (b / (1.0 - b) + 1.0) if step > 0 else 0.0


# ------------------------------------------------------------------------------------------------ time-series embed
def ts_embed_ref(x, conv_w, marks, tables: Sequence[torch.Tensor], pe) -> torch.Tensor:
    """DataEmbedding in float64: Conv1d(k = 3) over the circularly padded series + the sum of the table rows the marks select + pe[l].
    x [B, L, cin], conv_w [C, cin, 3], marks [B, L, n_mark] integer or None, pe [>= L, C] or None -> [B, L, C] float64"""
    B, L, cin = x.shape
    xt = x.double().transpose(1, 2)                                           # [B, cin, L]
    xp = torch.cat((xt[:, :, -1:], xt, xt[:, :, :1]), dim=2)                  # circular padding by one on either side
    out = F.conv1d(xp, conv_w.double()).transpose(1, 2)                       # [B, L, C]
    if marks is not None:
        for f, tab in enumerate(tables):
            out = out + F.embedding(marks[..., f].long(), tab.double())
    if pe is not None:
        out = out + pe[:L].double()[None]
    return out


def ts_unfold_ref(x: torch.Tensor, ncols: int) -> torch.Tensor:
    """out[(b, l), i * 3 + k] = x[b, (l + k - 1) mod L, i], pad columns +0"""
    B, L, cin = x.shape
    cols = torch.stack([torch.roll(x, shifts=1 - k, dims=1) for k in range(3)], dim=-1)      # [B, L, cin, 3]
    out = torch.zeros(B * L, ncols, dtype=x.dtype, device=x.device)
    out[:, :3 * cin] = cols.reshape(B * L, 3 * cin)
    return out


# ------------------------------------------------------------------------------------------------ pooling
def argmax_first(x: torch.Tensor) -> torch.Tensor:
    """[B, N, C] -> [B, C] int32: the FIRST token index at which the column's maximum is reached (explicit, not torch.max's choice)"""
    B, N, C = x.shape
    mx = x.max(dim=1, keepdim=True).values
    n = torch.arange(N, device=x.device).reshape(1, N, 1).expand(B, N, C)
    return torch.where(x == mx, n, torch.full_like(n, N)).min(dim=1).values.to(torch.int32)


# ------------------------------------------------------------------------------------------------ windows
def window_partition_ref(x: torch.Tensor, B: int, H: int, W: int, ws: int) -> torch.Tensor:
    """[B * H * W, cols] -> [B * gh * gw * ws * ws, cols]: zero-pad the grid to multiples of ws, reshape, permute"""
    cols = x.shape[-1]
    gh, gw = -(-H // ws), -(-W // ws)
    grid = F.pad(x.reshape(B, H, W, cols), (0, 0, 0, gw * ws - W, 0, gh * ws - H))
    return grid.reshape(B, gh, ws, gw, ws, cols).permute(0, 1, 3, 2, 4, 5).reshape(-1, cols)


def window_merge_ref(x: torch.Tensor, B: int, H: int, W: int, ws: int) -> torch.Tensor:
    cols = x.shape[-1]
    gh, gw = -(-H // ws), -(-W // ws)
    grid = x.reshape(B, gh, gw, ws, ws, cols).permute(0, 1, 3, 2, 4, 5).reshape(B, gh * ws, gw * ws, cols)
    return grid[:, :H, :W].reshape(-1, cols)


# ------------------------------------------------------------------------------------------------ patches
def geom6(k, s):
    """(kt, kh, kw, st, sh, sw) from 2-D or 3-D kernel / stride"""
    k = (1,) + tuple(k) if len(k) == 2 else tuple(k)
    s = (1,) + tuple(s) if len(s) == 2 else tuple(s)
    return k + s


def patches_ref(x: torch.Tensor, geom) -> torch.Tensor:
    """x [B, Cin, (T,) H, W] -> [B * tokens, Cin * kt * kh * kw], feature order (c, dt, dy, dx), token order (t, h, w): F.unfold in 2-D,
    chained Tensor.unfold in 3-D.  Differentiable (its autograd is the scatter)."""
    kt, kh, kw, st, sh, sw = geom
    if x.dim() == 4:
        assert kt == 1 and st == 1
        u = F.unfold(x, (kh, kw), stride=(sh, sw))                             # [B, Cin * kh * kw, tokens]
        return u.transpose(1, 2).reshape(-1, u.shape[1])
    B, Cin = x.shape[:2]
    u = x.unfold(2, kt, st).unfold(3, kh, sh).unfold(4, kw, sw)                # [B, Cin, gt, gh, gw, kt, kh, kw]
    return u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(-1, Cin * kt * kh * kw)


def patch_embed_ref(x, w, bias, pos, geom):
    """conv patch embed in float64: F.conv2d / F.conv3d(...).flatten(2).transpose(1, 2) (+ pos) -> [B, tokens, Cout]; w is the conv
    weight viewed as [Cout, Cin * kt * kh * kw]"""
    kt, kh, kw, st, sh, sw = geom
    Cout, Cin = w.shape[0], x.shape[1]
    xd, wd = x.double(), w.double()
    bd = bias.double() if bias is not None else None
    if x.dim() == 4:
        y = F.conv2d(xd, wd.reshape(Cout, Cin, kh, kw), bd, stride=(sh, sw))
    else:
        y = F.conv3d(xd, wd.reshape(Cout, Cin, kt, kh, kw), bd, stride=(st, sh, sw))
    y = y.flatten(2).transpose(1, 2)
    return y + pos.double()[None] if pos is not None else y


def patch_embed_grads_ref(x, dy, geom, Cout: int):
    """(dW [Cout, K], dbias [Cout]) by autograd through the same convolution; dy [B * tokens, Cout]"""
    kt, kh, kw, st, sh, sw = geom
    Cin = x.shape[1]
    K = Cin * kt * kh * kw
    w = torch.zeros(Cout, K, dtype=torch.float64, device=x.device, requires_grad=True)
    b = torch.zeros(Cout, dtype=torch.float64, device=x.device, requires_grad=True)
    y = patch_embed_ref(x, w, b, None, geom)
    y.backward(dy.double().reshape(y.shape))
    return w.grad, b.grad


# ------------------------------------------------------------------------------------------------ resize
def resize_ref(table: torch.Tensor, h: int, w: int, H: int, W: int, mode: str) -> torch.Tensor:
    """[h * w, C] -> [H * W, C]: F.interpolate(align_corners=False) in the table's own precision (pass a double table for the
    reference, a float one for the fp32 yardstick)"""
    C = table.shape[-1]
    g = table.reshape(1, h, w, C).permute(0, 3, 1, 2)
    o = F.interpolate(g, size=(H, W), mode=mode, align_corners=False)
    return o.permute(0, 2, 3, 1).reshape(H * W, C)


# ------------------------------------------------------------------------------------------------ yardstick
def close_tol(a: torch.Tensor, ref: torch.Tensor) -> float:
    """the smallest tol at which conftest.check_close(a, ref, tol) passes: the larger of max-abs error / max|ref| and, per element,
    error / (4 |ref| + max|ref| / 2).  Yardstick and kernel are measured with this one metric, on whatever device the tensors are."""
    a, ref = a.detach().double(), ref.detach().double()
    scale = float(ref.abs().max().clamp_min(1e-30))
    err = (a - ref).abs()
    return max(float(err.max()) / scale, float((err / (4.0 * ref.abs() + 0.5 * scale)).max()))


def yardstick_bound(yard: float) -> float:
    """4 x the error of torch's fp32 arithmetic on the same inputs, never less than 4 units of fp32 roundoff (an exact yardstick must
    not ask for exact results) -- the rule of test_layernorm_rows_far_off_centre"""
    return 4.0 * max(yard, 2.0 ** -24)
