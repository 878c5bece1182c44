"""GPU: the tokenizer entry points (me_patch_embed, me_patch_embed_wgrad, me_patchify, me_unpatchify_add, me_timeseries_embed,
me_timeseries_unfold) called through _capi with raw descriptors on guard-band buffers (tests/guarded.py): inputs between NaN guards
with NaN pad columns, outputs and workspaces between sentinel guards, workspaces exactly as large as their query says.

References (tests/ew_cases.py), float64 from the stored operands: F.conv2d / F.conv3d(...).flatten(2).transpose(1, 2) and its autograd
for the patch embed, F.unfold / chained Tensor.unfold and its autograd for the gathers, F.conv1d on the circularly padded series +
F.embedding + pe for the time-series embed.
Bounds: patch embed and its weight gradient 2e-5 (fp32 out) / TOL_BF16_OP (bf16 out), those of test_patch_embed_gathers_inside_the_gemm;
gathers, the non-overlapping scatter and the unfold bit for bit; the overlapping (atomic) scatter 1e-6.
me_timeseries_embed had no bound: the yardstick is the same sum formed by torch in fp32 on the device (F.conv1d, F.embedding, + pe)
against the float64 reference, metric ew_cases.close_tol; the kernel may err 4 x as much, never less than 4 x 2^-24, and a bf16 output
adds its rounding (2^-8 of the element).  Measured on MI355X, the worst over the whole family:
    fp32 out   torch fp32 1.80e-07 -> bound 7.20e-07, kernel 1.38e-07
    bf16 out   bound 7.20e-07 + 2^-8 = 3.91e-03, kernel 3.68e-03 (the output rounding)
(the test prints the figures of every case before it asserts)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ew_cases as ew
from conftest import TOL_BF16_OP, check_close
from ew_cases import BF16, F32
from guarded import Guarded
from metatransformer_amd import _capi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WORKSPACE = -1, -4


def code(dt):
    return _capi.dtype_code(dt)


def S():
    return _capi.stream_ptr()


def sync():
    torch.cuda.synchronize()


def cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def all_sentinel(G: Guarded) -> bool:
    return G.violation() is None and G.untouched_interior() == G.rows * G.cols


def old_pattern(rows, cols, dt, dev, salt=0):
    """recognisable old contents (small integers, exact in bf16) for rows a call must leave alone or accumulate into"""
    r = torch.arange(rows, device=dev).reshape(rows, 1)
    c = torch.arange(cols, device=dev).reshape(1, cols)
    return (((r * 7 + c * 3 + salt) % 251) - 125).to(dt)


def shape5(shape):
    return (shape[0], shape[1], 1, shape[2], shape[3]) if len(shape) == 4 else tuple(shape)


def n_tokens(shape, geom):
    _, _, T, H, W = shape5(shape)
    kt, kh, kw, st, sh, sw = geom
    return ((T - kt) // st + 1) * ((H - kh) // sh + 1) * ((W - kw) // sw + 1)


def make_desc(X: Guarded, xdt, shape, geom, wdt, Cout):
    d = _capi.PatchEmbedDesc()
    d.x, d.x_dtype = X.ptr(), code(xdt)
    d.B, d.Cin, d.T, d.H, d.W = shape5(shape)
    d.kt, d.kh, d.kw, d.st, d.sh, d.sw = geom
    d.w_dtype, d.Cout = code(wdt), Cout
    return d


# ------------------------------------------------------------------------------------------------ me_patch_embed
# (shape, kernel, stride, Cout, prefix_rows, fused)
PE_FUSED = [
    ((2, 3, 48, 40), (16, 16), (16, 16), 264, 1, 1),        # 12 rows; the second column tile is 8 wide
    ((2, 3, 32, 36), (16, 16), (16, 16), 8, 0, 1),          # W % 8 != 0: patch rows 8-byte aligned only
    ((1, 3, 4, 32, 32), (2, 16, 16), (2, 16, 16), 8, 0, 1),   # tubelets: six planes
    ((2, 2, 48, 16), (32, 8), (16, 8), 8, 0, 1),            # vertical overlap
    ((1, 1, 8, 128), (4, 64), (4, 64), 8, 0, 1),
    ((2, 1, 16, 64), (8, 32), (8, 32), 8, 2, 1),
    ((1, 1, 36, 46), (16, 16), (10, 10), 8, 0, 1),          # patch rows start at byte 20 px
    ((86, 1, 16, 48), (16, 16), (16, 16), 8, 2, 1),         # 258 rows: the 256-row tile edge falls inside a sample's group
    ((1, 3, 16, 16), (16, 16), (16, 16), 8, 0, 1),          # a single token
]
PE_TWO_PASS = [
    ((2, 1, 36, 46), (16, 16), (10, 10), 12, 0, 0, F32),    # fp32 pixels, fp32 weights
    ((3, 2, 30, 27), (6, 6), (5, 7), 12, 1, 0, BF16),       # a geometry the stager does not take, with pos behind a prefix row
]
PE_ALL = [c + (BF16,) for c in PE_FUSED] + PE_TWO_PASS


def _pe_id(c):
    return "x".join(map(str, c[0])) + "_k" + "x".join(map(str, c[1])) + "_s" + "x".join(map(str, c[2])) + f"_{c[3]}"


def _pe_operands(case, seed=11):
    shape, k, s, Cout, prefix, fused, dt = case
    geom = ew.geom6(k, s)
    g = cpu_gen(seed)
    x = torch.randn(*shape, generator=g).to(dt)
    K = shape[1] * geom[0] * geom[1] * geom[2]
    w = (0.05 * torch.randn(Cout, K, generator=g)).to(dt)
    bias = 0.1 * torch.randn(Cout, generator=g)
    tokens = n_tokens(shape, geom)
    pos = torch.randn(tokens, Cout, generator=g)
    return geom, x, w, bias, pos, tokens, K


def _run_patch_embed(lib, dev, case, ops_, odt, pos_dt, with_bias, padded, short_ws=False):
    shape, k, s, Cout, prefix, fused, dt = case
    geom, x, w, bias, pos, tokens, K = ops_
    B = shape[0]
    what = f"patch_embed {_pe_id(case)} {dt} -> {odt}, pos {pos_dt}, bias {with_bias}, padded {padded}"
    X, Wt = Guarded.input(x.reshape(1, -1).to(dev)), Guarded.input(w.to(dev))
    Bi = Guarded.input(bias.to(dev)) if with_bias else None
    ld = Cout + 8 if padded else Cout
    P = Guarded.input(pos.to(pos_dt).to(dev), ld) if pos_dt is not None else None
    rows = B * (prefix + tokens)
    old = old_pattern(rows, Cout, odt, dev)
    O = Guarded.output(rows, Cout, ld, odt, dev, old=old)
    d = make_desc(X, dt, shape, geom, dt, Cout)
    d.weight, d.bias = Wt.ptr(), (Bi.ptr() if Bi else None)
    if P:
        d.pos, d.pos_dtype, d.ld_pos = P.ptr(), code(pos_dt), ld
    d.prefix_rows = prefix
    d.out, d.out_dtype, d.ld_out = O.ptr(), code(odt), ld
    assert lib.me_patch_embed_fused(ctypes.byref(d)) == fused, f"{what}: expected route fused = {fused}"
    nws = lib.me_patch_embed_workspace_bytes(ctypes.byref(d))
    assert (nws == 0) == bool(fused), f"{what}: workspace query {nws}"
    WS = None
    if nws:
        give = nws - 1 if short_ws else nws
        WS = Guarded.output_bytes(give, dev)
        d.workspace, d.workspace_bytes = WS.ptr(), give
    rc = lib.me_patch_embed(ctypes.byref(d), S())
    sync()
    O.check(what + ": out")
    if WS:
        WS.check(what + ": workspace")
    if short_ws:
        assert rc != 0, f"{what}: a workspace one byte short must be refused"
        ew.assert_bits_equal(O.t, old, what + ": a refused call wrote to out")
        assert all_sentinel(WS), f"{what}: a refused call wrote to the workspace"
        return None
    _capi.check(rc, what)
    y = O.t.reshape(B, prefix + tokens, Cout)
    if prefix:
        ew.assert_bits_equal(y[:, :prefix], old.reshape(B, prefix + tokens, Cout)[:, :prefix], what + ": prefix rows must be left untouched")
    assert not bool(torch.isnan(y[:, prefix:].float()).any()), f"{what}: NaN (a guard or a pad column was read)"
    return y[:, prefix:].clone(), what


@pytest.mark.parametrize("case", PE_ALL, ids=_pe_id)
def test_patch_embed_contract(dev, case):
    lib = _capi.load()
    ops_ = _pe_operands(case)
    geom, x, w, bias, pos, tokens, K = ops_
    for pos_dt, with_bias in ((F32, True), (BF16, False)):
        ref = ew.patch_embed_ref(x, w, bias if with_bias else None, pos.to(pos_dt), geom)
        for odt in (F32, BF16):
            dense, what = _run_patch_embed(lib, dev, case, ops_, odt, pos_dt, with_bias, False)
            padded, _ = _run_patch_embed(lib, dev, case, ops_, odt, pos_dt, with_bias, True)
            ew.assert_bits_equal(padded, dense, what + ": padded strides against dense")
            check_close(dense.float(), ref, 2e-5 if odt == F32 else TOL_BF16_OP, what)
    # without pos
    ref = ew.patch_embed_ref(x, w, bias, None, geom)
    y, what = _run_patch_embed(lib, dev, case, ops_, F32, None, True, True)
    check_close(y, ref, 2e-5, what)


@pytest.mark.parametrize("case", PE_TWO_PASS, ids=_pe_id)
def test_patch_embed_refuses_a_short_workspace(dev, case):
    _run_patch_embed(_capi.load(), dev, case, _pe_operands(case), F32, F32, True, False, short_ws=True)


# ------------------------------------------------------------------------------------------------ me_patch_embed_wgrad
# (shape, kernel, stride, Cout, dtype, gathered inside the wgrad kernel).  The gathering kernel is the split-K weight-gradient kernel
# of the 256 x 256 family, which the GEMM planner gives only problems with Cout >= 256, K >= 256 and >= 4096 tokens (csrc/gemm.hip:
# plan_gemm), so of the two 4136-token cases Cout = 264 runs on it and Cout = 8 takes the two-pass route inside the same entry point.
WG_CASES = [
    ((1034, 1, 16, 64), (16, 16), (16, 16), 8, BF16, 0),      # 4136 tokens, K = 256; too narrow for the gathering kernel
    ((1034, 1, 16, 64), (16, 16), (16, 16), 264, BF16, 1),
    ((2, 3, 48, 40), (16, 16), (16, 16), 264, BF16, 0),       # fused forward, but too few tokens for the gathering wgrad kernel
    ((2, 1, 36, 46), (16, 16), (10, 10), 12, F32, 0),
]
_WG_REF = {}


def _wg_operands(case):
    """operands and float64 gradients of one case, computed once and shared by its parametrised runs (read-only)"""
    key = _pe_id(case)
    if key not in _WG_REF:
        shape, k, s, Cout, dt, _ = case
        geom = ew.geom6(k, s)
        g = cpu_gen(41)
        x = torch.randn(*shape, generator=g).to(dt)
        M_ = shape[0] * n_tokens(shape, geom)
        dy = torch.randn(M_, Cout, generator=g).to(dt)
        dw, db = ew.patch_embed_grads_ref(x, dy, geom, Cout)
        _WG_REF[key] = (geom, x, dy, dw, db, M_)
    return _WG_REF[key]


@pytest.mark.parametrize("dwdt", [F32, BF16], ids=str)
@pytest.mark.parametrize("case", WG_CASES, ids=_pe_id)
def test_patch_embed_wgrad_contract(dev, case, dwdt):
    lib = _capi.load()
    shape, k, s, Cout, dt, fused = case
    geom, x, dy, dw_ref, db_ref, M_ = _wg_operands(case)
    K = dw_ref.shape[1]
    X = Guarded.input(x.reshape(1, -1).to(dev))
    tol = 2e-5 if dwdt == F32 else TOL_BF16_OP
    for padded in (False, True):
        DY = Guarded.input(dy.to(dev), Cout + 8 if padded else Cout)
        for beta in (0.0, 1.0):
            for with_bias in (True, False):
                what = f"patch_embed_wgrad {_pe_id(case)} {dt} -> {dwdt}, ld_dy {'padded' if padded else 'dense'}, beta {beta}, dbias {with_bias}"
                old_w, old_b = old_pattern(Cout, K, dwdt, dev, 5), old_pattern(1, Cout, F32, dev, 9)[0]
                d = make_desc(X, dt, shape, geom, dt, Cout)
                assert lib.me_patch_embed_wgrad_fused(ctypes.byref(d), code(dwdt)) == fused, f"{what}: expected route fused = {fused}"
                nws = lib.me_patch_embed_wgrad_workspace_bytes(ctypes.byref(d), code(dwdt), 1 if with_bias else 0)
                extra, rc = 0, None
                for attempt in (0, 1):
                    DW = Guarded.output(Cout, K, None, dwdt, dev, old=old_w)
                    DB = Guarded.output_vec(Cout, F32, dev, old=old_b)
                    WS = Guarded.output_bytes(nws + extra, dev)
                    d.workspace, d.workspace_bytes = WS.ptr(), nws + extra
                    rc = lib.me_patch_embed_wgrad(ctypes.byref(d), DY.ptr(), DY.ld, DW.ptr(), code(dwdt), DB.ptr() if with_bias else None, beta, S())
                    sync()
                    for o, nm in ((DW, "dW"), (DB, "dbias"), (WS, "workspace")):
                        o.check(f"{what}: {nm}")
                    if rc == ERR_WORKSPACE and padded and attempt == 0:
                        # within the contract: a strided dy may need the two-pass route, whose columns the query did not count
                        ew.assert_bits_equal(DW.t, old_w, what + ": a refused call wrote to dW")
                        ew.assert_bits_equal(DB.vec(), old_b, what + ": a refused call wrote to dbias")
                        assert all_sentinel(WS), f"{what}: a refused call wrote to the workspace"
                        extra = M_ * K * (4 if dt == F32 else 2) + 256
                        continue
                    break
                _capi.check(rc, what)
                check_close(DW.t.float(), beta * old_w.double().cpu() + dw_ref, tol, what + ": dW")
                if with_bias:
                    check_close(DB.vec(), beta * old_b.double().cpu() + db_ref, 2e-5, what + ": dbias")
                else:
                    ew.assert_bits_equal(DB.vec(), old_b, what + ": dbias written without being asked for")


def test_patch_embed_wgrad_rejects_a_fractional_beta_with_dbias(dev):
    lib = _capi.load()
    case = WG_CASES[2]
    shape, k, s, Cout, dt, _ = case
    geom, x, dy, dw_ref, _, _ = _wg_operands(case)
    X, DY = Guarded.input(x.reshape(1, -1).to(dev)), Guarded.input(dy.to(dev))
    d = make_desc(X, dt, shape, geom, dt, Cout)
    nws = lib.me_patch_embed_wgrad_workspace_bytes(ctypes.byref(d), code(F32), 1)
    DW, DB, WS = Guarded.output(Cout, dw_ref.shape[1], None, F32, dev), Guarded.output_vec(Cout, F32, dev), Guarded.output_bytes(nws, dev)
    d.workspace, d.workspace_bytes = WS.ptr(), nws
    rc = lib.me_patch_embed_wgrad(ctypes.byref(d), DY.ptr(), Cout, DW.ptr(), code(F32), DB.ptr(), 0.5, S())
    sync()
    assert rc == ERR_ARG and all_sentinel(DW) and all_sentinel(DB) and all_sentinel(WS), "beta = 0.5 with dbias is rejected, nothing written"


def test_patch_embed_wgrad_refuses_dy_rows_off_16_bytes(dev):
    """dy rows that are no multiple of 16 bytes (ld_dy = Cout + 4 in bf16) keep the gathering kernel from taking the problem, and the
    GEMM of the two-pass route does not take them either: the call is refused -- ME_ERR_WORKSPACE where the queried workspace (planned
    on a dense dy) cannot hold the gathered columns, ME_ERR_ARG where it can -- with dW and dbias untouched and the workspace's guards
    intact (the workspace itself is scratch)"""
    lib = _capi.load()
    case = WG_CASES[1]
    shape, k, s, Cout, dt, fused = case
    geom, x, dy, dw_ref, _, _ = _wg_operands(case)
    X, DY = Guarded.input(x.reshape(1, -1).to(dev)), Guarded.input(dy.to(dev), Cout + 4)
    d = make_desc(X, dt, shape, geom, dt, Cout)
    nws = lib.me_patch_embed_wgrad_workspace_bytes(ctypes.byref(d), code(F32), 1)
    DW, DB, WS = Guarded.output(Cout, dw_ref.shape[1], None, F32, dev), Guarded.output_vec(Cout, F32, dev), Guarded.output_bytes(nws, dev)
    d.workspace, d.workspace_bytes = WS.ptr(), nws
    rc = lib.me_patch_embed_wgrad(ctypes.byref(d), DY.ptr(), Cout + 4, DW.ptr(), code(F32), DB.ptr(), 0.0, S())
    sync()
    assert rc in (ERR_WORKSPACE, ERR_ARG), f"expected a refusal, got {rc}"
    WS.check("workspace of the refused call")
    assert all_sentinel(DW) and all_sentinel(DB), "a refused call wrote to dW or dbias"


# ------------------------------------------------------------------------------------------------ me_patchify / me_unpatchify_add
# (name, shape, kernel, stride, x offset, cols offset (elements), expected gather kernel)
GATHER_CASES = [
    ("scalar", (3, 2, 30, 27), (6, 6), (5, 7), 0, 0, "scalar"),                     # kw % 4 != 0
    ("quad", (2, 3, 32, 40), (8, 8), (8, 8), 0, 0, "quad aligned"),
    ("quad_stride10", (2, 1, 36, 46), (16, 16), (10, 10), 0, 0, "quad unaligned"),   # sw % 4 != 0
    ("quad_x_off", (2, 3, 32, 40), (8, 8), (8, 8), 1, 0, "quad unaligned"),          # x one element into its buffer
    ("cols_off", (2, 3, 32, 40), (8, 8), (8, 8), 0, 1, "scalar"),                    # cols one element into its buffer
    ("tubelet", (1, 2, 4, 16, 16), (2, 8, 8), (2, 8, 8), 0, 0, "quad aligned"),
]


def _gather_kernel(geom, W, x_ptr, cols_ptr):
    """which kernel me_patchify's launcher takes, from its stated preconditions (csrc/patchify.hip)"""
    kw, sw = geom[2], geom[5]
    if kw % 4 == 0 and cols_ptr % 16 == 0:
        return "quad aligned" if (W % 4 == 0 and sw % 4 == 0 and x_ptr % 16 == 0) else "quad unaligned"
    return "scalar"


@pytest.mark.parametrize("xdt,cdt", [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)], ids=str)
@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: c[0])
def test_patchify_contract(dev, case, xdt, cdt):
    lib = _capi.load()
    name, shape, k, s, xo, co, kernel = case
    geom = ew.geom6(k, s)
    what = f"patchify {name} {xdt} -> {cdt}"
    x = torch.randn(*shape, generator=cpu_gen(3)).to(xdt).to(dev)
    want = ew.patches_ref(x.float(), geom).to(cdt)                  # (x.float() is exact; one rounding into cols' type, as the kernel does)
    rows, K = want.shape
    xin = torch.cat((torch.full((xo,), float("nan"), dtype=xdt, device=dev), x.reshape(-1)))
    X = Guarded.input(xin)
    Cg = Guarded.output_vec(rows * K + co, cdt, dev)
    xp, cp = X.ptr() + xo * X.esize, Cg.ptr() + co * Cg.esize
    assert _gather_kernel(geom, shape5(shape)[4], xp, cp) == kernel, f"{what}: the case does not reach the {kernel} kernel"
    _capi.check(lib.me_patchify(xp, code(xdt), cp, code(cdt), *shape5(shape), *geom, S()), what)
    sync()
    Cg.check(what)
    if co:
        assert int(Cg.interior_bits()[0, 0]) == Cg.sentinel, f"{what}: the element in front of cols was written"
    assert int((Cg.interior_bits()[0, co:] == Cg.sentinel).sum()) == 0, f"{what}: elements not written"
    ew.assert_bits_equal(Cg.vec()[co:].reshape(rows, K), want, what)


# (name, shape, kernel, stride, dcols offset, dx offset, expected scatter kernel)
SCATTER_CASES = [
    ("quad", (2, 3, 32, 40), (8, 8), (8, 8), 0, 0, "quad"),
    ("tubelet", (1, 2, 4, 16, 16), (2, 8, 8), (2, 8, 8), 0, 0, "quad"),
    ("scalar_kw6", (3, 2, 30, 27), (6, 6), (6, 7), 0, 0, "scalar"),                  # no overlap, kw % 4 != 0; rows and columns left uncovered
    ("scalar_dx_off", (2, 3, 32, 40), (8, 8), (8, 8), 0, 1, "scalar"),               # dx one element into its buffer
    ("atomic_stride10", (2, 1, 36, 46), (16, 16), (10, 10), 0, 0, "atomic"),         # overlap in both directions, every pixel covered
    ("atomic_uncovered", (2, 1, 38, 47), (16, 16), (10, 10), 0, 0, "atomic"),        # the same with two rows and a column no patch reaches
    ("atomic_vertical", (2, 2, 48, 16), (32, 8), (16, 8), 0, 0, "atomic"),
]


def _scatter_kernel(geom, W, dcols_ptr, dx_ptr):
    kt, kh, kw, st, sh, sw = geom
    if st < kt or sh < kh or sw < kw:
        return "atomic"
    return "quad" if (kw % 4 == 0 and W % 4 == 0 and sw % 4 == 0 and dx_ptr % 16 == 0 and dcols_ptr % 16 == 0) else "scalar"


@pytest.mark.parametrize("ddt", [F32, BF16], ids=str)
@pytest.mark.parametrize("case", SCATTER_CASES, ids=lambda c: c[0])
def test_unpatchify_add_contract(dev, case, ddt):
    lib = _capi.load()
    name, shape, k, s, do, xo, kernel = case
    geom = ew.geom6(k, s)
    what = f"unpatchify_add {name} {ddt}"
    xr = torch.zeros(*shape, dtype=torch.float64, device=dev, requires_grad=True)
    cols = ew.patches_ref(xr, geom)
    dcols = torch.randn(cols.shape, generator=cpu_gen(4)).to(ddt).to(dev)
    cols.backward(dcols.double())
    covered = torch.zeros(*shape, dtype=torch.float64, device=dev, requires_grad=True)
    ew.patches_ref(covered, geom).sum().backward()
    n = xr.numel()
    DC = Guarded.input(torch.cat((torch.full((do,), float("nan"), dtype=ddt, device=dev), dcols.reshape(-1))))
    DX = Guarded.output_vec(n + xo, F32, dev)
    DX.t[0, xo:] = 0.0                                              # dx is zero-filled by the caller
    dp, xp = DC.ptr() + do * DC.esize, DX.ptr() + xo * 4
    assert _scatter_kernel(geom, shape5(shape)[4], dp, xp) == kernel, f"{what}: the case does not reach the {kernel} kernel"
    _capi.check(lib.me_unpatchify_add(dp, code(ddt), xp, *shape5(shape), *geom, S()), what)
    sync()
    DX.check(what)
    if xo:
        assert int(DX.interior_bits()[0, 0]) == DX.sentinel, f"{what}: the element in front of dx was written"
    dx = DX.vec()[xo:].reshape(shape)
    hit = covered.grad > 0
    assert bool((~hit).any()) == (name in ("scalar_kw6", "atomic_uncovered")), "which cases leave pixels uncovered"
    assert int((ew.bits(dx)[~hit] != 0).sum()) == 0, f"{what}: a pixel no patch covers must stay +0 bit for bit"
    if kernel == "atomic":
        check_close(dx, xr.grad, 1e-6, what)
    else:
        ew.assert_bits_equal(dx, xr.grad.float(), what)


# ------------------------------------------------------------------------------------------------ me_timeseries_embed / _unfold
TS_TABLE_ROWS = [13, 32, 7, 24, 4]


def _ts_operands(dev, L, cin, C, n_mark, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    B = 2
    x = torch.randn(B, L, cin, device=dev, generator=g)
    w = torch.randn(C, cin, 3, device=dev, generator=g) * 0.5
    tabs = [torch.randn(r, C, device=dev, generator=g) for r in TS_TABLE_ROWS[:n_mark]]
    marks = torch.stack([torch.randint(0, r, (B, L), device=dev, generator=g) for r in TS_TABLE_ROWS[:n_mark]], dim=-1).to(torch.int32) \
        if n_mark else None
    if marks is not None:
        marks[0, 0, :] = torch.tensor([r - 1 for r in TS_TABLE_ROWS[:n_mark]], dtype=torch.int32, device=dev)      # the last row of every table
    pe = torch.randn(L + 2, C, device=dev, generator=g)
    return x, w, tabs, marks, pe


def _ts_call(lib, dev, x, w, tabs, marks, pe, odt, what):
    B, L, cin = x.shape
    C, n_mark = w.shape[0], len(tabs)
    X, Wc = Guarded.input(x.reshape(B * L, cin)), Guarded.input(w.reshape(C, cin * 3))
    T = [Guarded.input(t) for t in tabs]
    MK = Guarded.output(B * L, n_mark, None, torch.int32, dev, old=marks.reshape(B * L, n_mark)) if n_mark else None
    PE = Guarded.input(pe) if pe is not None else None
    O = Guarded.output(B * L, C, None, odt, dev)
    E = Guarded.output(1, 1, None, torch.int32, dev, old=torch.zeros(1, 1, dtype=torch.int32))
    tab_arr = (ctypes.c_void_p * max(n_mark, 1))(*[t.ptr() for t in T])
    rows_arr = (ctypes.c_int32 * max(n_mark, 1))(*[t.shape[0] for t in tabs])
    rc = lib.me_timeseries_embed(X.ptr(), Wc.ptr(), MK.ptr() if MK else None, n_mark, tab_arr if n_mark else None, rows_arr if n_mark else None,
                                 PE.ptr() if PE else None, O.ptr(), code(odt), B, L, cin, C, E.ptr(), S())
    _capi.check(rc, what)
    sync()
    O.check(what + ": out")
    E.check(what + ": err_flag")
    if MK:
        MK.check(what + ": marks")
    return O, int(E.t[0, 0])


@pytest.mark.parametrize("C", [4, 100, 260])
@pytest.mark.parametrize("cin", [1, 7])
@pytest.mark.parametrize("L", [1, 2, 5])
def test_timeseries_embed_contract(dev, L, cin, C):
    lib = _capi.load()
    worst = {"yard": 0.0, "kernel": 0.0}
    for n_mark in (0, 4, 5):
        x, w, tabs, marks, pe = _ts_operands(dev, L, cin, C, n_mark, L * 100 + cin * 10 + n_mark)
        for with_pe in (True, False):
            ref = ew.ts_embed_ref(x, w, marks, tabs, pe if with_pe else None)
            xt = x.transpose(1, 2)
            y32 = F.conv1d(torch.cat((xt[:, :, -1:], xt, xt[:, :, :1]), dim=2), w).transpose(1, 2)
            for f, t in enumerate(tabs):
                y32 = y32 + F.embedding(marks[..., f].long(), t)
            if with_pe:
                y32 = y32 + pe[:L][None]
            yard = ew.close_tol(y32, ref)
            for odt in (F32, BF16):
                what = f"timeseries_embed L {L} cin {cin} C {C} n_mark {n_mark} pe {with_pe} -> {odt}"
                O, flag = _ts_call(lib, dev, x, w, tabs, marks, pe if with_pe else None, odt, what)
                assert flag == 0, f"{what}: err_flag raised with every index in range"
                assert O.untouched_interior() == 0, what
                assert not bool(torch.isnan(O.t.float()).any()), f"{what}: NaN (a guard was read)"
                bound = ew.yardstick_bound(yard) + (2.0 ** -8 if odt == BF16 else 0.0)
                err = ew.close_tol(O.t.reshape(ref.shape), ref)
                print(f"{what}: torch fp32 {yard:.3e} -> bound {bound:.3e}, kernel {err:.3e}")
                if odt == F32:
                    worst["yard"], worst["kernel"] = max(worst["yard"], yard), max(worst["kernel"], err)
                check_close(O.t.reshape(ref.shape), ref, bound, what)
    print(f"timeseries_embed L {L} cin {cin} C {C}: worst yardstick {worst['yard']:.3e}, worst kernel (fp32 out) {worst['kernel']:.3e}")


@pytest.mark.parametrize("bad", [("high", 3, 24), ("negative", 0, -1), ("high_minute", 4, 4)], ids=lambda b: b[0])
def test_timeseries_embed_flags_an_index_out_of_range(dev, bad):
    lib = _capi.load()
    _, col, value = bad
    L, cin, C = 5, 7, 260
    x, w, tabs, marks, pe = _ts_operands(dev, L, cin, C, 5, 77)
    marks[1, L - 1, col] = value
    O, flag = _ts_call(lib, dev, x, w, tabs, marks, pe, F32, f"timeseries_embed with mark column {col} = {value}")
    assert flag == 1, "an index outside its table raises the flag"
    assert not bool(torch.isnan(O.t).any()), "the out-of-range index must not be followed into a guard"


@pytest.mark.parametrize("cin", [1, 7])
@pytest.mark.parametrize("L", [1, 2, 5])
def test_timeseries_unfold_contract(dev, L, cin):
    lib = _capi.load()
    B = 2
    x = torch.randn(B, L, cin, device=dev, generator=torch.Generator(device=dev).manual_seed(L + cin))
    X = Guarded.input(x.reshape(B * L, cin))
    for ncols in (3 * cin, 3 * cin + 5):
        what = f"timeseries_unfold L {L} cin {cin} ncols {ncols}"
        O = Guarded.output(B * L, ncols, None, F32, dev)
        _capi.check(lib.me_timeseries_unfold(X.ptr(), O.ptr(), B, L, cin, ncols, S()), what)
        sync()
        O.check(what)
        assert O.untouched_interior() == 0, what
        ew.assert_bits_equal(O.t, ew.ts_unfold_ref(x, ncols), what)
    O = Guarded.output(B * L, 3 * cin, None, F32, dev)
    rc = lib.me_timeseries_unfold(X.ptr(), O.ptr(), B, L, cin, 3 * cin - 1, S())
    sync()
    assert rc == ERR_ARG and all_sentinel(O), "ncols < 3 cin is rejected"
