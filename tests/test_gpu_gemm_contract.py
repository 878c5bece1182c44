"""GPU: the me_gemm / me_colsum contract on padded strides, with guard bands.

Every case runs twice through a raw GemmDesc -- operands dense and outputs exactly sized, then every matrix with its own padded leading
dimension -- with every input between NaN guards (pad columns NaN too) and every output, vector and the workspace between sentinel
guards (tests/guarded.py).  Asserted per case: the kernel plan the library reports (me_gemm_profile_rec.plan) is the table's, the
same in both runs; the padded result equals the dense one bit for bit; both meet a float64 product of the same stored operands
(computed with torch on the device); no NaN in the interior; no sentinel outside the described extents changed.

The table holds the smallest shapes that reach each kernel form of plan_gemm (csrc/gemm.hip) with a ragged last row tile and, where
the family allows it, a ragged last column tile.  A case whose plan differs from its entry FAILS: the table cannot silently stop
covering a kernel.  (The plan code carries the family, the split and its parts; the tile of a g2b launch and the one-tile / resident
form of a g3 launch follow from the shape -- the comments say which -- and the resident form needs tiles >= CUs.)"""
import ctypes
import math

import pytest
import torch

from conftest import TOL_BF16_OP, check_close
from gemm_cases import BF16, CASES, EPI, F32, FACTOR, NT, SAVE_GG, TN, assert_g3_form, describe      # (the table lives in gemm_cases.py)
from gemm_cases import dtype_code as _code
from guarded import Guarded
from metatransformer_amd import _capi

pytestmark = pytest.mark.gpu


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))


def _gelu_grad(v):
    return 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


class Problem:
    """the stored operands of one (case, epilogue) and its float64 result"""

    def __init__(self, dev, op, abdt, cdt, M, N, K, e, seed):
        g = torch.Generator(device=dev).manual_seed(seed)

        def rnd(*shape, scale=1.0, dt=F32):
            return (scale * torch.randn(*shape, device=dev, generator=g)).to(dt)
        self.op, self.abdt, self.M, self.N, self.K, self.e = op, abdt, M, N, K, e
        self.cdt = e.get("c", cdt)
        self.a = rnd(*((M, K) if op == NT else (K, M)), dt=abdt)
        self.b = rnd(*((N, K) if op == NT else (K, N)), scale=0.05 if op == NT else 1.0, dt=abdt)
        self.bias = rnd(N, scale=0.1) if e.get("bias") else None
        self.colscale = 1 + rnd(N, scale=0.2) if e.get("colscale") else None
        self.row_affine = torch.stack((0.5 + torch.rand(M, device=dev, generator=g), rnd(M, scale=0.3)), 1) if e.get("row_affine") else None
        self.col_shift = rnd(N) if e.get("row_affine") else None
        self.group = e.get("group", 0)
        self.predt = self.cdt if e.get("preact") == "c" else e.get("preact")
        self.aux = rnd(M, N, dt=e["aux"]) if e.get("aux") else None
        self.res_rows = self.group or M
        self.res = rnd(self.res_rows, N, dt=e["res"]) if e.get("res") else None
        self.alpha, self.beta, self.flags = e.get("alpha", 1.0), e.get("beta", 0.0), e.get("flags", 0)
        self.c_rows = M // self.group * (self.group + 1) if self.group else M      # one untouched row in front of every group
        self.c_old = rnd(self.c_rows, N, dt=self.cdt) if self.beta != 0.0 else None
        self.colsum_old = rnd(M) if e.get("colsum") and self.beta != 0.0 else None
        # ---- float64, on the device, from the stored operands
        ad, bd = self.a.double(), self.b.double()
        v = self.alpha * (ad @ bd.t() if op == NT else ad.t() @ bd)
        if self.row_affine is not None:
            v = v * self.row_affine[:, 0:1].double() + self.col_shift.double()[None, :] * self.row_affine[:, 1:2].double()
        if self.bias is not None:
            v = v + self.bias.double()
        self.ref_pre = None
        if self.predt is not None:
            self.ref_pre = _gelu_grad(v) if self.flags & SAVE_GG else v
        if e.get("gelu"):
            v = _gelu(v)
        if self.aux is not None:
            v = v * (self.aux.double() if self.flags & FACTOR else _gelu_grad(self.aux.double()))
        if self.colscale is not None:
            v = v * self.colscale.double()
        if self.res is not None:
            v = v + (self.res.double().repeat(M // self.group, 1) if self.group else self.res.double())
        if self.c_old is not None:
            v = v + self.beta * self.c_old.double()
        self.ref = v
        self.ref_colsum = None
        if e.get("colsum"):
            self.ref_colsum = ad.sum(0) + (self.beta * self.colsum_old.double() if self.colsum_old is not None else 0.0)

    def written_rows(self, c):
        """the rows of the output buffer the epilogue writes (out_group leaves the row in front of every group alone)"""
        if not self.group:
            return c
        return c.view(self.M // self.group, self.group + 1, -1)[:, 1:, :].reshape(self.M, -1)


def run(lib, dev, pr: Problem, padded: bool):
    """one me_gemm call on guarded buffers; returns (plan, {name: Guarded output}, [all guarded outputs])"""
    pads = iter(range(8, 800, 8)) if padded else iter([0] * 100)
    N, M, K, e = pr.N, pr.M, pr.K, pr.e

    def ld(cols):
        return cols + next(pads)
    A, B = Guarded.input(pr.a, ld(pr.a.shape[1])), Guarded.input(pr.b, ld(pr.b.shape[1]))
    C = Guarded.output(pr.c_rows, N, ld(N), pr.cdt, dev, old=pr.c_old)
    outs, keep = {"C": C}, [A, B]
    d = _capi.GemmDesc()
    d.op, d.ab_dtype, d.M, d.N, d.K = pr.op, _code(pr.abdt), M, N, K
    d.A, d.lda, d.B, d.ldb = A.ptr(), A.ld, B.ptr(), B.ld
    d.C, d.ldc, d.c_dtype = C.ptr(), C.ld, _code(pr.cdt)
    d.alpha, d.beta, d.flags = pr.alpha, pr.beta, pr.flags
    d.act = _capi.ME_ACT_GELU if e.get("gelu") else _capi.ME_ACT_NONE
    for name, vec in (("bias", pr.bias), ("colscale", pr.colscale), ("row_affine", pr.row_affine), ("col_shift", pr.col_shift)):
        if vec is not None:
            gv = Guarded.input(vec.reshape(-1))
            keep.append(gv)
            setattr(d, name, gv.ptr())
    if pr.predt is not None:
        outs["preact"] = P = Guarded.output(M, N, ld(N), pr.predt, dev)
        d.preact, d.ldpre, d.preact_dtype = P.ptr(), P.ld, _code(pr.predt)
    if pr.aux is not None:
        X = Guarded.input(pr.aux, ld(N))
        keep.append(X)
        d.aux, d.ldaux, d.aux_dtype = X.ptr(), X.ld, _code(pr.aux.dtype)
    if pr.res is not None:
        R = Guarded.input(pr.res, ld(N))
        keep.append(R)
        d.residual, d.ldres, d.res_dtype = R.ptr(), R.ld, _code(pr.res.dtype)
    if pr.group:
        d.res_row_mod, d.out_group_rows, d.out_group_stride, d.out_row_offset = pr.group, pr.group, pr.group + 1, 1
    if e.get("colsum"):
        assert lib.me_gemm_fuses_colsum(ctypes.byref(d)) == 1, "the case is meant to fuse the bias gradient"
        outs["colsum"] = S = Guarded.output_vec(M, F32, dev, old=pr.colsum_old)
        d.colsum_a = S.ptr()
    if e.get("row_stats") and lib.me_gemm_emits_row_stats(ctypes.byref(d)) == 1:
        nb = lib.me_row_stats_partial_bytes(M, N)
        outs["row_stats"] = T = Guarded.output_vec(nb // 4, F32, dev)
        d.row_stats = T.ptr()
    wsb = lib.me_gemm_workspace_bytes(ctypes.byref(d))
    W = Guarded.output_bytes(wsb, dev)
    d.workspace, d.workspace_bytes = (W.ptr(), wsb) if wsb else (None, 0)
    lib.me_gemm_profile_enable(1)
    try:
        _capi.check(lib.me_gemm(ctypes.byref(d), _capi.stream_ptr()), "me_gemm")
        recs = (_capi.GemmProfileRec * 8)()
        n = lib.me_gemm_profile_read(recs, 8)
    finally:
        lib.me_gemm_profile_enable(0)
    torch.cuda.synchronize()
    gemm = [r.plan for r in recs[:n] if r.op in (NT, TN)]
    assert len(gemm) == 1, gemm
    return gemm[0], outs, list(outs.values()) + [W]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_contract(dev, case):
    name, op, abdt, cdt, M, N, K, want_plan, epis = case[:9]
    reserve = case[9] if len(case) > 9 else 0
    lib = _capi.load()
    assert_g3_form(lib, name, cdt, M, N)      # (resident / one-tile, from the tile count against the CUs)
    prev = lib.me_gemm_reserve_cus(reserve) if reserve else None
    try:
        for i, en in enumerate(epis):
            what = f"{name}/{en}"
            pr = Problem(dev, op, abdt, cdt, M, N, K, EPI[en], seed=1000 + 17 * i + M + N + K)
            plan_d, out_d, guards_d = run(lib, dev, pr, padded=False)
            plan_p, out_p, guards_p = run(lib, dev, pr, padded=True)
            print(f"{what}: plan {describe(plan_d)}")
            assert plan_d == want_plan, f"{what}: the dense run reports {describe(plan_d)}, the table says {describe(want_plan)}"
            assert plan_p == plan_d, f"{what}: padded strides changed the plan: {describe(plan_p)} against {describe(plan_d)}"
            for g in guards_d:
                g.check(f"{what}, dense")
            for g in guards_p:
                g.check(f"{what}, padded strides")
            if EPI[en].get("row_stats"):      # (only the resident cases ask; the partials need whole 256-column groups)
                assert ("row_stats" in out_d) == (N % 256 == 0) and ("row_stats" in out_p) == (N % 256 == 0), \
                    f"{what}: me_gemm_emits_row_stats answers {'row_stats' in out_d} (dense) / {'row_stats' in out_p} (padded) at N = {N}"
            # ---- values
            t_out = TOL_BF16_OP if pr.cdt == BF16 else (3e-5 if K >= 4096 else 1e-5)
            for key, ref, t in (("C", pr.ref, t_out), ("preact", pr.ref_pre, TOL_BF16_OP if pr.predt == BF16 else t_out),
                                ("colsum", pr.ref_colsum, 3e-5 if K >= 4096 else 1e-5)):
                if key not in out_d:
                    continue
                got_d, got_p = out_d[key].t, out_p[key].t
                if key == "C":
                    got_d, got_p = pr.written_rows(got_d), pr.written_rows(got_p)
                    if pr.group:      # the row in front of every group belongs to the caller: still the sentinel
                        for o in (out_d, out_p):
                            skipped = o["C"].interior_bits().view(M // pr.group, pr.group + 1, N)[:, 0, :]
                            assert bool((skipped == o["C"].sentinel).all()), f"{what}: wrote a row outside the output groups"
                if key == "colsum":
                    ref = ref.reshape(1, -1)
                assert not bool(torch.isnan(got_d).any()) and not bool(torch.isnan(got_p).any()), f"{what}: NaN in {key}"
                check_close(got_d.float(), ref, t, f"{what} {key}, dense")
                if not torch.equal(got_p, got_d):
                    check_close(got_p.float(), ref, t, f"{what} {key}, padded strides")
                    raise AssertionError(f"{what}: {key} with padded strides differs from the dense run "
                                         f"({int((got_p != got_d).sum())} elements) although the plan is the same")
            if "row_stats" in out_d:
                assert torch.equal(out_d["row_stats"].t, out_p["row_stats"].t), f"{what}: row statistics differ with padded strides"
                pairs = torch.empty(M, 2, dtype=F32, device=dev)
                _capi.check(lib.me_row_stats_combine(out_d["row_stats"].ptr(), M, N, 1e-5, pairs.data_ptr(), _capi.stream_ptr()), "combine")
                y = out_d["C"].t.double()                       # the statistics of the STORED rows (what the next LayerNorm reads)
                rstd = 1.0 / torch.sqrt(y.var(-1, unbiased=False) + 1e-5)
                shift = -rstd * y.mean(-1)
                assert not bool(torch.isnan(pairs).any())
                # (the bounds test_gpu_encoder.py holds these statistics to)
                assert float((pairs[:, 0].double() - rstd).abs().max() / rstd.abs().max()) < 2e-5, f"{what}: rstd of the row statistics"
                assert float((pairs[:, 1].double() - shift).abs().max()) <= 1e-4 * float(shift.abs().max() + 1), f"{what}: -rstd * mean"
    finally:
        if reserve:
            lib.me_gemm_reserve_cus(prev)


def test_gemm_k_window_of_wider_operands(dev):
    """linear._gemm_nt_chunked: fp32 A / B are K windows of wider matrices (lda = ldb = K_total, pointer offset k0), accumulated with
    beta = 1 window by window.  Here every column OUTSIDE the current window is NaN while its call runs."""
    lib = _capi.load()
    M, N, Kt, step = 130, 132, 328, 128
    g = torch.Generator(device=dev).manual_seed(5)
    a = torch.randn(M, Kt, device=dev, generator=g)
    b = 0.05 * torch.randn(N, Kt, device=dev, generator=g)
    bias = 0.1 * torch.randn(N, device=dev, generator=g)
    C = Guarded.output(M, N, N + 8, F32, dev)
    Bv = Guarded.input(bias)
    for k0 in range(0, Kt, step):
        kw = min(step, Kt - k0)
        aw, bw = torch.full_like(a, float("nan")), torch.full_like(b, float("nan"))
        aw[:, k0:k0 + kw], bw[:, k0:k0 + kw] = a[:, k0:k0 + kw], b[:, k0:k0 + kw]
        A, B = Guarded.input(aw), Guarded.input(bw)
        d = _capi.GemmDesc()
        d.op, d.ab_dtype, d.M, d.N, d.K = NT, _capi.ME_F32, M, N, kw
        d.A, d.lda, d.B, d.ldb = A.ptr() + 4 * k0, Kt, B.ptr() + 4 * k0, Kt
        d.C, d.ldc, d.c_dtype = C.ptr(), C.ld, _capi.ME_F32
        d.alpha, d.beta = 1.0, 0.0 if k0 == 0 else 1.0
        if k0 == 0:
            d.bias = Bv.ptr()
        assert lib.me_gemm_workspace_bytes(ctypes.byref(d)) == 0
        _capi.check(lib.me_gemm(ctypes.byref(d), _capi.stream_ptr()), "me_gemm")
        torch.cuda.synchronize()
        C.check(f"K window at {k0}")
    assert not bool(torch.isnan(C.t).any())
    check_close(C.t, a.double() @ b.double().t() + bias.double(), 1e-5, "K windows accumulated")


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("rows,cols,pad", [(1, 4, 4), (77, 100, 8), (300, 772, 12), (4101, 258, 6), (130, 57, 3)])
def test_colsum_contract(dev, dt, rows, cols, pad):
    """me_colsum with a row stride > cols (NaN pad columns, NaN guards), overwrite and accumulate, against a float64 column sum;
    (258 + 6, 57 + 3: strides that are no multiple of 4 -- the scalar kernel)"""
    lib = _capi.load()
    g = torch.Generator(device=dev).manual_seed(rows + cols)
    x = torch.randn(rows, cols, device=dev, generator=g).to(dt)
    old = torch.randn(cols, device=dev, generator=g)
    ref = x.double().sum(0)
    X = Guarded.input(x, cols + pad)
    for acc in (0, 1):
        out = Guarded.output_vec(cols, F32, dev, old=old if acc else None)
        W = Guarded.output_bytes(lib.me_colsum_workspace(cols), dev)
        _capi.check(lib.me_colsum(X.ptr(), _code(dt), X.ld, rows, cols, out.ptr(), acc, W.ptr(), _capi.stream_ptr()), "me_colsum")
        torch.cuda.synchronize()
        out.check(f"colsum out, accumulate {acc}")
        W.check(f"colsum workspace, accumulate {acc}")
        assert not bool(torch.isnan(out.t).any())
        check_close(out.vec(), ref + (old.double() if acc else 0.0), 1e-5, f"colsum accumulate {acc}")
