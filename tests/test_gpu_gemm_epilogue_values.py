"""GPU: the VALUES of the me_gemm epilogues on exact accumulators, per kernel family -- the rounding store to the bit, the GELU forms over
the whole range (clamp, joint at |x| = 4, flat tails, sign), the saved-gelu' pair in bf16, fp32 and ME_GG8, the factor reads, and what a
NaN pre-activation becomes.

Shapes and expected plans are the contract table's (tests/gemm_cases.py); operands and references come from tests/epilogue_cases.py: the
accumulator of every element is exact whatever order the kernel reduces in, so what is compared is the epilogue alone.

  rounding store   bits == bf16_bits_rne(x) (NaN <-> NaN), fp32 outputs == x bit for bit
  polynomial GELU  |y - ref| <= E + h, E = the emulation's own maximum error on the case's points + 2^-18 (fused against separate rounding
                   of eight Horner steps on O(1) values), h = the bf16 half-ulp of the stored value.  gelu(x) == x to the bit for
                   x >= 12, |gelu(x)| <= E for x <= -12.  The aux form is r_m gelu'(aux) with r_m in {1, -2, 1/2}: E scales with |r_m|.
                   (h is the EXACT half-ulp 2^(floor(log2 a) - 8) at a = |ref| + E, not 2^-9 |ref|: bf16 keeps 8 significant bits, so
                   half a unit in the last place is 2^-9 a only at the top of a binade and 2^-8 a at its bottom -- the correctly
                   rounded store of the float64 reference itself misses 2^-9 |ref|, e.g. 127.25 -> 127.5; tests/test_epilogue_cases_cpu.py
                   shows both.)
  erf forms        emulation maximum + 3 * 2^-23 max(1, |x|) (v_rcp_f32 / v_exp_f32 are 1-ulp approximations) + the store's half-ulp
                   (none for fp32, h for bf16, 2^-16 |ref| for hi + lo of the planes)
  ME_GG8           the saved byte within one step of the reference code (so never wrapped); the read returns r_m (-0.13 + q 1.26 / 255)
                   rounded once; where me_gemm_takes_gg8 says no, me_gemm refuses
  NaN              pre-activation NaN: the erf forms give NaN; the polynomial forms do NOT (v_min / v_max drop a quiet NaN): gelu gives
                   4 P(4) = -9.7e-5, gelu' 1/2 +- 4 Q(4) = 1.0001 / -9.7e-5 by the NaN's sign bit -- the same in every family (pinned
                   here; include/metaenc.h says so)

Measured on MI355X (profiles/gemm_epilogue_values.txt: per family and epilogue the largest error beyond the store's rounding, where, and
the bound): every store bit-exact; polynomial gelu 1.86e-4 (bound 1.92e-4), gelu' 4.04e-4 per unit of r_m (4.16e-4); erf gelu 4.6e-7, gelu'
1.9e-7 in fp32 (1.6e-6, 6.3e-7); ME_GG8 half a step -- the same figures in every family.  (ME_EPILOGUE_VALUES_OUT=<file> makes a run
write that table.)"""
import ctypes
import os

import pytest
import torch

import epilogue_cases as ec
from gemm_cases import BF16, CASE_BY_ID, F32, FACTOR, G128, G2B, G2W, G3, NT, SAVE_GG, TN, assert_g3_form, describe, dtype_code
from guarded import Guarded
from metatransformer_amd import _capi

pytestmark = pytest.mark.gpu

U8 = torch.uint8
X3 = "bf16x3"                     # ME_BF16X3 output: [hi | lo | hi] planes in one row of 3 N bf16
FAMILY = {G128: "g128", G2B: "g2b", G2W: "g2w", G3: "g3"}

BF16_FORMS = ["plain", "bias", "res", "bias_res", "beta1", "alpha_beta", "gelu_pre", "gelu", "aux", "factor", "save_gg", "save_gg_f32"]
GG8 = ["save_gg8", "factor_gg8"]
F32_FORMS = ["plain", "bias", "bias_res32", "beta1", "alpha_beta", "gelu_pre", "gelu", "save_gg_f32"]
TN_FORMS = ["plain", "beta1", "plain_bf16", "beta1_bf16"]
PLAN = {
    "nt_f32_g128": F32_FORMS,
    "nt_g128_n4": BF16_FORMS,
    "nt_g2b_64x128": BF16_FORMS,
    "nt_g2b_split8": BF16_FORMS,
    "nt_g2b_128x256_n264": BF16_FORMS,
    "nt_g2w": BF16_FORMS + GG8,
    "nt_g2w_split2": BF16_FORMS,
    "nt_g3_one_tile": BF16_FORMS + GG8 + ["planes_gelu", "planes_factor"],
    "nt_g3_resident": BF16_FORMS + GG8,
    "nt_g3_resident_n3848": BF16_FORMS + GG8,
    "nt_g3_tail8": ["plain", "bias", "bias_res32", "gelu_pre", "gelu"],
    "tn_g2b_128": TN_FORMS,
    "tn_g2b_split4_128": TN_FORMS,
    "tn_g3_wgrad33": TN_FORMS,
}
PARAMS = [(c, e) for c, es in PLAN.items() for e in es]

TOP = 3.3e38                      # the error bounds are asked below this: beyond it (0x7F7F8000 ..) a bf16 store of gelu(x) = x rounds to inf, which the bit checks cover
RECORDS = []                      # (family, case, epilogue, output, max error, at x, bound there)


@pytest.fixture(scope="module", autouse=True)
def _write_records():
    yield
    path = os.environ.get("ME_EPILOGUE_VALUES_OUT")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write(f"{'family':8} {'case':22} {'epilogue':14} {'output':8} {'max error':>11} {'at x':>13} {'bound':>11}\n")
            for r in RECORDS:
                f.write(f"{r[0]:8} {r[1]:22} {r[2]:14} {r[3]:8} {r[4]:11.4e} {r[5]:13.6g} {r[6]:11.4e}\n")


def record(ctx, output, err, x, bound):
    """err, x, bound: same-shape tensors of the asserted elements; keeps the element with the largest error"""
    if err.numel() == 0:
        return
    i = int(torch.argmax(err))
    RECORDS.append((ctx["family"], ctx["case"], ctx["epi"], output, float(err.flatten()[i]), float(x.flatten()[i]), float(bound.flatten()[i])))
    print(f"{ctx['case']}/{ctx['epi']} {output}: max error {RECORDS[-1][4]:.4e} at x = {RECORDS[-1][5]:.6g} (bound {RECORDS[-1][6]:.4e})")


# ------------------------------------------------------------------------------------------------ one launch
def launch(lib, dev, op, abdt, M, N, K, A, B, cdt, *, c_old=None, alpha=1.0, beta=0.0, bias=None, gelu=False, flags=0, pre_dt=None, aux=None,
           res=None, refuse=False):
    """one me_gemm call; inputs between NaN guards, outputs between sentinel guards.  Returns (plan, C [M, cols] , preact or None)."""
    keep = []

    def inp(t):
        g = Guarded.input(t)
        keep.append(g)
        return g
    Ag, Bg = inp(A.to(abdt)), inp(B.to(abdt))
    planes = cdt == X3
    C = Guarded.output(M, 3 * N if planes else N, None, BF16 if planes else cdt, dev, old=c_old)
    d = _capi.GemmDesc()
    d.op, d.ab_dtype, d.M, d.N, d.K = op, dtype_code(abdt), M, N, K
    d.A, d.lda, d.B, d.ldb = Ag.ptr(), Ag.ld, Bg.ptr(), Bg.ld
    d.C, d.ldc, d.c_dtype = C.ptr(), C.ld, _capi.ME_BF16X3 if planes else dtype_code(cdt)
    d.alpha, d.beta, d.flags = alpha, beta, flags
    d.act = _capi.ME_ACT_GELU if gelu else _capi.ME_ACT_NONE
    if bias is not None:
        d.bias = inp(bias).ptr()
    P = None
    if pre_dt is not None:
        P = Guarded.output(M, N, None, pre_dt, dev)
        d.preact, d.ldpre, d.preact_dtype = P.ptr(), P.ld, _capi.ME_GG8 if pre_dt == U8 else dtype_code(pre_dt)
    if aux is not None:
        if aux.dtype == U8:
            keep.append(aux)
            d.aux, d.ldaux, d.aux_dtype = aux.data_ptr(), N, _capi.ME_GG8
        else:
            X = inp(aux)
            d.aux, d.ldaux, d.aux_dtype = X.ptr(), X.ld, dtype_code(aux.dtype)
    if res is not None:
        R = inp(res)
        d.residual, d.ldres, d.res_dtype = R.ptr(), R.ld, dtype_code(res.dtype)
    wsb = lib.me_gemm_workspace_bytes(ctypes.byref(d))
    W = Guarded.output_bytes(wsb, dev)
    d.workspace, d.workspace_bytes = (W.ptr(), wsb) if wsb else (None, 0)
    if refuse:
        assert lib.me_gemm_takes_gg8(ctypes.byref(d)) == 0
        assert lib.me_gemm(ctypes.byref(d), _capi.stream_ptr()) != 0, "me_gemm took an ME_GG8 operand that me_gemm_takes_gg8 refuses"
        torch.cuda.synchronize()
        assert C.untouched_interior() == M * C.cols, "a refused call wrote its output"
        return None, None, None
    lib.me_gemm_profile_enable(1)
    try:
        _capi.check(lib.me_gemm(ctypes.byref(d), _capi.stream_ptr()), "me_gemm")
        recs = (_capi.GemmProfileRec * 8)()
        n = lib.me_gemm_profile_read(recs, 8)
    finally:
        lib.me_gemm_profile_enable(0)
    torch.cuda.synchronize()
    plans = [r.plan for r in recs[:n] if r.op in (NT, TN)]
    assert len(plans) == 1, plans
    for g in (C, P, W):
        if g is not None:
            g.check("epilogue values")
    return plans[0], C.t, (P.t if P is not None else None)


def takes_gg8(lib, dev, M, N, K, save):
    d = _capi.GemmDesc()
    dummy = torch.empty(16, dtype=BF16, device=dev)
    d.op, d.ab_dtype, d.M, d.N, d.K = NT, _capi.ME_BF16, M, N, K
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.c_dtype = dummy.data_ptr(), K, dummy.data_ptr(), K, dummy.data_ptr(), N, _capi.ME_BF16
    d.alpha = 1.0
    if save:
        d.act, d.flags, d.preact, d.ldpre, d.preact_dtype = _capi.ME_ACT_GELU, SAVE_GG, dummy.data_ptr(), N, _capi.ME_GG8
    else:
        d.flags, d.aux, d.ldaux, d.aux_dtype = FACTOR, dummy.data_ptr(), N, _capi.ME_GG8
    return lib.me_gemm_takes_gg8(ctypes.byref(d)) == 1


# ------------------------------------------------------------------------------------------------ the checks
def first_bad(bad, x, got, want, what):
    m, n = (int(v) for v in torch.nonzero(bad)[0])
    xb = int(ec.f32_bits(x[m:m + 1, n:n + 1].contiguous()))
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements; first at (m, n) = ({m}, {n}): x = {xb:#010x} ({float(x[m, n])!r}), "
            f"got {int(got[m, n]):#x}, want {int(want[m, n]):#x}")


def check_store(ctx, out, x, valid, name="C"):
    """the rounding store: `out` holds bf16_bits_rne(x) (bf16) or x itself (fp32) wherever `valid`"""
    valid = valid & ~ec.is_subnormal(x)
    if out.dtype == BF16:
        got, want = ec.bf16_bits(out), ec.bf16_bits_rne(x)
        bad = valid & ~ec.same_bf16_bits(got, want)
    else:
        got, want = ec.f32_bits(out), ec.f32_bits(x)
        bad = valid & ~((got == want) | (torch.isnan(out) & torch.isnan(x)))
    assert not bool(bad.any()), first_bad(bad, x, got, want, f"{ctx['case']}/{ctx['epi']} {name}: stored bits")
    cov = ec.coverage(x, valid)
    print(f"{ctx['case']}/{ctx['epi']} {name}: {int(valid.sum())} elements bit-exact; {cov}")
    return cov


def check_bound(ctx, name, y, ref, own, h, mask, x):
    """|y - ref| <= own + h on `mask`: `own` bounds the form's arithmetic, h the store's rounding.  Recorded: the largest error in excess of
    h -- the part of the error that the store does not explain -- next to `own` there."""
    err = (y.double() - ref).abs()
    bound = own + h
    bad = mask & ~(err <= bound)
    if bool(bad.any()):
        m, n = (int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{ctx['case']}/{ctx['epi']} {name}: {int(bad.sum())} elements outside the bound; first at ({m}, {n}): x = {float(x[m, n])!r}, "
                             f"got {float(y[m, n])!r}, want {float(ref[m, n])!r}, error {float(err[m, n]):.4e} > {float(bound[m, n]):.4e}")
    record(ctx, name, (err - h).clamp_min(0.0)[mask], x.double()[mask], (own + torch.zeros_like(err))[mask])


def half_ulp(out_kind, ref, E=0.0):
    """the store's rounding of a computed value within E of ref: nothing for fp32, 2^-16 |ref| for hi + lo of the planes, and for bf16 half a
    unit in the last of its 8 significant bits, 2^(floor(log2 a) - 8) at a = |ref| + E  (between 2^-9 a and 2^-8 a: ec.bf16_half_ulp)"""
    if out_kind == "bf16":
        return ec.bf16_half_ulp(ref.abs() + E)
    return {"planes": 2.0 ** -16, "f32": 0.0}[out_kind] * ref.abs()


def check_poly_gelu(ctx, y, x, valid):
    """bf16-mode gelu of the pre-activation x, stored as bf16"""
    assert y.dtype == BF16
    fin = valid & (x.abs() < TOP)
    ref, emu = ec.gelu64(x), ec.emu_gelu_bf16(x)
    E = float((emu.double() - ref)[fin].abs().max()) + 2.0 ** -18
    assert E <= ec.GELU_BF16_ERR + 2.0 ** -18
    check_bound(ctx, "gelu", y, ref, E, half_ulp("bf16", ref, E), fin, x)
    ramp = valid & (x >= 12)                                    # (+inf too)
    # (the form adds its flat remainder 4 P(4), |.| <= E, to x before the store: the stored bits are x's own unless x lies within E of a
    #  tie between two bf16 neighbours -- the rounding patterns among the biases do -- where either neighbour is a correct answer)
    got, want = ec.bf16_bits(y), ec.bf16_bits_rne(x)
    lo, hi = ec.bf16_bits_rne((x.double() - E).float()), ec.bf16_bits_rne((x.double() + E).float())
    off = ramp & (got != lo) & (got != hi)
    assert int((ramp & (lo == hi)).sum()) > 0 and not bool(off.any()), first_bad(off, x, got, want, f"{ctx['case']}/{ctx['epi']}: gelu(x) != x for x >= 12")
    tail = valid & (x <= -12)                                   # (-inf too)
    assert int(tail.sum()) > 0 and bool((y.double().abs()[tail] <= E).all()), f"{ctx['case']}/{ctx['epi']}: |gelu(x)| > {E:.3e} for some x <= -12"
    # a NaN pre-activation: t = min(|NaN|, 4) = 4 and max(NaN, 0) = 0 -- the polynomial's value at the clamp, not NaN (pinned)
    nan = torch.isnan(x)
    want_nan = ec.emu_gelu_bf16(x[nan]).double()
    assert int(nan.sum()) > 0 and bool(((y.double()[nan] - want_nan).abs() <= 2.0 ** -18 + 2.0 ** -9 * want_nan.abs()).all()), \
        f"{ctx['case']}/{ctx['epi']}: gelu(NaN) = {y[nan][:4].tolist()}, the formula gives {want_nan[:4].tolist()}"


def check_erf_pair(ctx, y, dy, x, valid, y_kind, dy_kind):
    fin = valid & (x.abs() < TOP)
    ey, edy = ec.emu_gelu_erf_pair(x)
    slack = 3 * 2.0 ** -23 * x.double().abs().clamp_min(1.0)
    for name, got, emu, ref, kind in (("gelu", y, ey, ec.gelu64(x), y_kind), ("gelu'", dy, edy, ec.gelu_grad64(x), dy_kind)):
        if got is None:
            continue
        E = float((emu.double() - ref)[fin].abs().max())
        assert E <= 1e-6
        if kind == "gg8":
            q, want = got.to(torch.int64), ec.gg8_code(ref)
            bad = fin & ((q - want).abs() > 1)
            assert not bool(bad.any()), first_bad(bad, x, q, want, f"{ctx['case']}/{ctx['epi']}: ME_GG8 byte more than one step off")
            dec = ec.GG8_LO + ec.GG8_STEP * q.double()
            record(ctx, "gelu'8", (dec - ref).abs()[fin], x.double()[fin], torch.full_like(ref, 1.5 * ec.GG8_STEP)[fin])
            assert bool((q[torch.isnan(x)] == 0).all()), "ME_GG8 of a NaN: v_cvt_pk_u8_f32 gives 0"
            continue
        check_bound(ctx, name, got, ref, E + slack, half_ulp(kind, ref, E + slack), fin, x)
        nan = torch.isnan(x)
        assert int(nan.sum()) > 0 and bool(torch.isnan(got.float()[nan]).all()), f"{ctx['case']}/{ctx['epi']}: {name}(NaN) is not NaN in an erf form"


# ------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("case,epi", PARAMS, ids=[f"{c}-{e}" for c, e in PARAMS])
def test_epilogue_values(dev, case, epi):
    name, op, abdt, cdt, M, N, K, want_plan = CASE_BY_ID[case][:8]
    lib = _capi.load()
    assert_g3_form(lib, name, cdt, M, N)
    parts = max(want_plan >> 8, 1)
    tn = op == TN
    if epi.endswith("_bf16"):                  # TN into a bf16 C
        cdt, epi_kind = BF16, epi[:-5]
    else:
        epi_kind = epi
    ctx = dict(case=case, epi=epi, family=FAMILY[want_plan & 15] + ("+fold" if want_plan & 16 else ""))
    prod = epi_kind in ("plain", "res", "beta1", "alpha_beta")
    factor_r = epi_kind in ("aux", "factor_gg8", "planes_factor")
    if factor_r:
        j, scale = ec.factor_rows(M)
    else:
        j, scale = ec.sweep_rows(M, overflow_rows=prod)
    c = ec.prod_cols(N) if prod else torch.ones(N)
    A, B, acc = ec.operands(M, N, K, j, scale, c, parts, tn=tn, device=dev)
    r32 = (j.double() * scale.double()).float().to(dev)
    kw, out_c = {}, cdt
    bias = ec.bias_values(N).to(dev) if epi_kind in ("bias", "bias_res", "bias_res32", "gelu_pre", "gelu", "save_gg", "save_gg_f32", "save_gg8", "planes_gelu") else None
    if bias is not None:
        kw["bias"] = bias
    small = ec.small_operand(M, N, zero_rows=(scale != ec.R_SCALE) | (j == 0) if bias is not None else scale != ec.R_SCALE).to(dev)
    x = acc if bias is None else acc + bias[None, :]
    terms = [acc] if bias is None else [acc, bias[None, :].expand(M, N)]
    if epi_kind in ("res", "bias_res"):
        kw["res"] = small.to(BF16)
        x, terms = x + small, terms + [small]
    if epi_kind == "bias_res32":
        kw["res"] = small
        x, terms, out_c = x + small, terms + [small], F32
    if epi_kind == "beta1":
        kw.update(c_old=small.to(cdt), beta=1.0)
        x, terms = x + small, terms + [small]
    if epi_kind == "alpha_beta":
        kw.update(c_old=small.to(cdt), alpha=0.5, beta=2.0)
        x, terms = 0.5 * acc + 2.0 * small, [0.5 * acc.double(), 2.0 * small.double()]
    valid = ec.exact(x, *terms)
    if epi_kind in ("gelu_pre", "gelu", "save_gg", "save_gg_f32", "save_gg8", "planes_gelu"):
        kw["gelu"] = True
    if epi_kind == "gelu_pre":
        kw["pre_dt"] = cdt
    if epi_kind in ("save_gg", "save_gg_f32", "save_gg8", "planes_gelu"):
        kw.update(flags=SAVE_GG, pre_dt={"save_gg": BF16, "save_gg_f32": F32, "save_gg8": U8, "planes_gelu": F32}[epi_kind])
    aux = None
    if epi_kind in ("aux", "factor"):
        aux = ec.aux_values(M, N).to(dev)
        aux.view(torch.int16)[1, :8], aux.view(torch.int16)[2, :8] = 0x7FC0, 0xFFC0 - 0x10000      # +NaN, -NaN (the sign bit decides below)
    if epi_kind == "factor_gg8":
        aux = ((torch.arange(M, device=dev)[:, None] * 7 + torch.arange(N, device=dev)[None, :]) % 256).to(U8)
    if epi_kind == "planes_factor":
        aux = ec.aux_values(M, N).to(dev).float() * (1.0 + 2.0 ** -12)       # fp32 factors with more than 8 bits
    if aux is not None:
        kw["aux"] = aux
        if epi_kind != "aux":
            kw["flags"] = FACTOR
    if epi_kind.startswith("planes"):
        out_c = X3
    # ---- ME_GG8 where the resident kernel does not take the problem: the call is refused
    if epi_kind in ("save_gg8", "factor_gg8") and not takes_gg8(lib, dev, M, N, K, epi_kind == "save_gg8"):
        assert not name.startswith("nt_g3_resident"), f"{name}: the resident kernel must take ME_GG8"
        launch(lib, dev, op, abdt, M, N, K, A, B, out_c, refuse=True, **kw)
        return
    plan, C, P = launch(lib, dev, op, abdt, M, N, K, A, B, out_c, **kw)
    assert plan == want_plan, f"{case}/{epi}: the run reports {describe(plan)}, the table says {describe(want_plan)}"
    if out_c == X3:
        hi, lo = C[:, :N].float(), C[:, N:2 * N].float()
        assert torch.equal(ec.bf16_bits(C[:, 2 * N:]), ec.bf16_bits(C[:, :N])), "the third plane repeats the first"
        Csum = hi.double() + lo.double()
    # ---- what the output must hold
    if epi_kind in ("plain", "bias", "res", "bias_res", "bias_res32", "beta1", "alpha_beta"):
        cov = check_store(ctx, C, x, valid | torch.isnan(x))
        if out_c == BF16:
            assert cov["ties_up"] >= 64 and cov["ties_down"] >= 64, cov
            assert cov["overflows"] >= 16 or epi_kind == "alpha_beta", cov       # (alpha = 1/2 halves the products out of that range)
    elif epi_kind in ("gelu_pre", "gelu"):
        if P is not None:
            check_store(ctx, P, x, valid | torch.isnan(x), "preact")
        if out_c == BF16:
            check_poly_gelu(ctx, C, x, valid)
        else:
            check_erf_pair(ctx, C, None, x, valid, "f32", None)
    elif epi_kind in ("save_gg", "save_gg_f32", "save_gg8"):
        check_erf_pair(ctx, C, P, x, valid, "bf16" if out_c == BF16 else "f32", {BF16: "bf16", F32: "f32", U8: "gg8"}[P.dtype])
    elif epi_kind == "planes_gelu":
        check_erf_pair(ctx, Csum, P, x, valid, "planes", "f32")
    elif epi_kind == "aux":
        # r_m gelu'(aux), the polynomial form; r_m a power of two, so the error is the form's own, scaled
        a32 = aux.float()
        fin = torch.isfinite(a32)
        ref, emu = ec.gelu_grad64(a32), ec.emu_gelu_bf16_grad(a32)
        E = float((emu.double() - ref)[fin].abs().max()) + 2.0 ** -18
        assert E <= ec.GELU_BF16_GRAD_ERR + 2.0 ** -18
        rr = r32.double()[:, None]
        check_bound(ctx, "r gelu'", C, rr * ref, rr.abs() * E, half_ulp("bf16", rr * ref, rr.abs() * E), fin, a32)
        nan = ~fin                                              # NaN aux: 1/2 + copysign(4 Q(4), NaN) -- by the NaN's sign bit, not NaN (pinned)
        want = (rr * ec.emu_gelu_bf16_grad(a32).double())[nan]
        assert bool(((C.double()[nan] - want).abs() <= 2.0 ** -17 + 2.0 ** -9 * want.abs()).all()), \
            f"{case}/{epi}: r gelu'(NaN) = {C[nan].tolist()}, the formula gives {want.tolist()}"
    elif epi_kind == "factor":
        a32 = aux.float()
        xf = r32[:, None] * a32                                 # 8 bits x 8 bits: exact, then rounded once
        ok = ec.exact(xf, r32.double()[:, None] * a32.double()) & ~ec.is_subnormal(a32) | torch.isnan(a32)
        check_store(ctx, C, xf, ok)
    elif epi_kind == "factor_gg8":
        q = aux.to(torch.int64)
        d1, d2 = ec.gg8_decode32(q)
        got = ec.bf16_bits(C)
        w1, w2 = ec.bf16_bits_rne(r32[:, None] * d1), ec.bf16_bits_rne(r32[:, None] * d2)
        bad = (got != w1) & (got != w2)
        assert not bool(bad.any()), first_bad(bad, d1, got, w1, f"{case}/{epi}: r (-0.13 + q 1.26 / 255)")
        assert torch.unique(q).numel() == 256
    elif epi_kind == "planes_factor":
        ref = r32.double()[:, None] * aux.double()
        check_bound(ctx, "r aux", Csum, ref, 2.0 ** -23 * ref.abs(), half_ulp("planes", ref), ~ec.is_subnormal(aux) & (ref.abs() >= 2.0 ** -100) & (ref.abs() < 1e38), aux)
    else:
        raise AssertionError(epi_kind)


# ------------------------------------------------------------------------------------------------ a NaN token through a whole Block
@pytest.mark.parametrize("mode", ["autocast", "bf16_params"])
@pytest.mark.parametrize("train", [False, True], ids=["inference", "training"])
def test_block_nan_token_stays_in_its_sample(dev, mode, train):
    """The polynomial GELU of the MLP does not propagate a NaN pre-activation (above) -- the RESIDUAL STREAM does: one NaN in one token of
    sample 0 makes that token's output row non-finite, sample 1's output and dx rows are bit-identical to the run without the NaN
    (nothing leaks across samples), and after backward ops.grad_stats counts non-finite weight gradients."""
    import metatransformer_amd as M
    from metatransformer_amd import ops
    Bn, Nt, Cw, heads, tok = 2, 70, 256, 4, 5
    torch.manual_seed(11)
    blk = M.Block(Cw, heads, qkv_bias=True).to(dev)
    dt = F32
    if mode == "bf16_params":
        blk, dt = blk.to(BF16), BF16
    blk.train(train)
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(Bn, Nt, Cw, device=dev, generator=g).to(dt)
    dy = torch.randn(Bn, Nt, Cw, device=dev, generator=g).to(dt)

    def run(x):
        x = x.clone().requires_grad_(train)
        blk.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF16, enabled=mode == "autocast"), torch.set_grad_enabled(train):
            y = blk(x)
        if not train:
            return y.detach(), None, None
        y.backward(dy)
        flat = torch.cat([p.grad.float().flatten() for p in blk.parameters()])
        return y.detach(), x.grad.detach(), ops.grad_stats(flat)
    y_ok, dx_ok, st_ok = run(x0)
    assert bool(torch.isfinite(y_ok).all())
    xn = x0.clone()
    xn[0, tok, 3] = float("nan")
    y, dx, st = run(xn)
    assert not bool(torch.isfinite(y[0, tok]).any()), "the NaN token's output row must be non-finite in every column"
    assert torch.equal(y[1], y_ok[1]), "a NaN in sample 0 changed sample 1's output"
    if train:
        assert float(st_ok[1]) == 0 and bool(torch.isfinite(dx_ok).all())
        assert torch.equal(dx[1], dx_ok[1]), "a NaN in sample 0 changed sample 1's dx"
        assert float(st[1]) > 0, "grad_stats must count the non-finite weight gradients"
