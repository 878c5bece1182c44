"""GPU: me_attention_qkv_fwd / _bwd (csrc/attention_qkv.hip) -- attention over separate Q, K, V with two lengths and a causal flag --
against float64 torch.  Bounds: TOL_F32 / TOL_BF16_OP through check_close, the constants test_gpu_ops.py applies to me_attention_*.
The reference of a bf16 case is float64 arithmetic on the bf16-rounded operands.  Shapes and coverage: tests/ts_decoder_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import TOL_BF16_OP, TOL_F32, check_close

import ts_decoder_cases as tc
from guarded import Guarded
from metatransformer_amd import _capi, ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
B, H = tc.QKV_B, tc.QKV_H


def tol(dt):
    return TOL_F32 if dt == torch.float32 else TOL_BF16_OP


def check_grads(got, want, t, what):
    """dQ, dK, dV each against its own scale.  One that is zero in exact arithmetic (one key: the softmax is constant, dQ = dK = 0) has no
    scale of its own: it is bounded in absolute terms by the largest gradient of the call, as test_gpu_ops.test_attention_bwd does."""
    whole = max(float(w.abs().max()) for w in want)
    for nm, g, w in zip(("dQ", "dK", "dV"), got, want):
        if float(w.abs().max()) < 1e-3 * whole:
            err = float((g.detach().double().cpu() - w).abs().max())
            print(f"{what} {nm}: zero in exact arithmetic, |got| <= {err:.3e} (largest gradient {whole:.3e})")
            assert err <= t * whole, (what, nm, err, whole)
        else:
            check_close(g.float(), w, t, f"{what} {nm}")


def run_case(dev, Nq, Nk, causal, hd, layout, dt, p_drop=0.0, seed=0):
    """-> (out, lse, (dq, dk, dv)) from the library and the float64 reference's (out, lse, (dq, dk, dv))"""
    scale = hd ** -0.5
    layout = tc.qkv_layout_for(layout, Nq, Nk)
    q, k, v, do = tc.qkv_values(B, Nq, Nk, H, hd, dt, seed=Nq * 1000 + Nk)
    qd, kd, vd = tc.qkv_place(layout, q, k, v, dev)
    out, lse = ops.attention_qkv_fwd(qd, kd, vd, B, Nq, Nk, H, hd, scale, causal=causal, need_lse=True, p_drop=p_drop, seed=seed)
    # gradients go into views of the same layout, over NaN: an element the kernels skip stays NaN, the padding must stay NaN
    gq, gk, gv = tc.qkv_place(layout, torch.full_like(q, float("nan")), torch.full_like(k, float("nan")), torch.full_like(v, float("nan")), dev,
                              fill=float("nan"))
    grads = ops.attention_qkv_bwd(qd, kd, vd, out, do.to(dev), lse, B, Nq, Nk, H, hd, scale, causal=causal, p_drop=p_drop, seed=seed,
                                  grads=(gq, gk, gv))
    if layout == "separate_padded":
        for g in grads:
            assert bool(torch.isnan(torch.as_strided(g, (g.shape[0], 8), g.stride(), g.storage_offset() + g.shape[1])).all()), "padding written"
    factor = None
    if p_drop > 0:
        factor = torch.from_numpy(tc.qkv_keep(seed, B, H, Nq, Nk, p_drop).astype(np.float64)) / (1.0 - float(np.float32(p_drop)))
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    ref, lse_ref = tc.qkv_ref(qr, kr, vr, B, Nq, Nk, H, hd, scale, causal, factor)
    ref.backward(do.double())
    return (out, lse, grads), (ref.detach(), lse_ref.detach(), (qr.grad, kr.grad, vr.grad))


FWD_BWD = [(dt, case) for dt in DTYPES for case in tc.qkv_cases(dt)]


@pytest.mark.parametrize("dt,case", FWD_BWD, ids=[("f32-" if dt == torch.float32 else "bf16-") + tc.qkv_case_id(c) for dt, c in FWD_BWD])
def test_attention_qkv_fwd_bwd(dev, dt, case):
    """forward, lse and the three gradients of every case against float64.  (bf16: the backward's delta comes from the tiles, not from the
    rounded O -- with dO . O the dQ of causal N = 129, head_dim 96 had 2 of 74 304 elements outside the per-element part of the bound.)"""
    Nq, Nk, causal, hd, layout = case
    what = f"attention_qkv {tc.qkv_case_id(case)} {dt}"
    (out, lse, grads), (ref, lse_ref, gref) = run_case(dev, Nq, Nk, causal, hd, layout, dt)
    check_close(out.float(), ref, tol(dt), what + " out")
    check_close(lse, lse_ref, tol(dt), what + " lse")
    check_grads(grads, gref, tol(dt), what)


# the three smallest shapes of test_gpu_ops.TILED_CASES (self-attention: causal) and one cross-attention shape
GUARDED_QKV = [(1, 1, 8, torch.float32), (64, 64, 128, torch.bfloat16), (65, 65, 8, torch.float32), (65, 65, 24, torch.bfloat16),
               (70, 33, 64, torch.float32), (70, 33, 64, torch.bfloat16)]


@pytest.mark.parametrize("Nq,Nk,hd,dt", GUARDED_QKV, ids=[f"{a}x{b}-hd{c}-{'f32' if d == torch.float32 else 'bf16'}" for a, b, c, d in GUARDED_QKV])
def test_attention_qkv_operands_in_guard_bands(dev, Nq, Nk, hd, dt):
    """every operand and every gradient is a column view of a padded buffer between guards (tests/guarded.py): Q | K | V in one
    [B*N, 3C] buffer with 8 pad columns when Nq == Nk, else Q alone and K | V in one [B*Nk, 2C] buffer; out and dout with ld = C + 8.
    Inputs (out and lse included, for the backward) between NaN guards with NaN pad columns, outputs between sentinel guards: a key
    row read past Nk or a pad column read as data shows as NaN, a store outside an extent as a changed sentinel."""
    lib = _capi.load()
    causal = Nq == Nk
    C, scale, code = H * hd, hd ** -0.5, _capi.dtype_code(dt)
    q, k, v, do = tc.qkv_values(B, Nq, Nk, H, hd, dt, seed=Nq * 1000 + Nk + hd)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    ref, lse_ref = tc.qkv_ref(qr, kr, vr, B, Nq, Nk, H, hd, scale, causal)
    ref.backward(do.double())
    es = q.element_size()
    if causal:
        IN = [Guarded.input(torch.cat([q, k, v], 1).to(dev), 3 * C + 8)]
        GR = [Guarded.output(B * Nq, 3 * C, 3 * C + 8, dt, dev)]
        place = lambda bufs: ((bufs[0], 0), (bufs[0], C), (bufs[0], 2 * C))
    else:
        IN = [Guarded.input(q.to(dev), C + 8), Guarded.input(torch.cat([k, v], 1).to(dev), 2 * C + 8)]
        GR = [Guarded.output(B * Nq, C, C + 8, dt, dev), Guarded.output(B * Nk, 2 * C, 2 * C + 8, dt, dev)]
        place = lambda bufs: ((bufs[0], 0), (bufs[1], 0), (bufs[1], C))
    OUT, LSE = Guarded.output(B * Nq, C, C + 8, dt, dev), Guarded.output_vec(B * H * Nq, torch.float32, dev)
    d = _capi.AttnQkvDesc()
    (d.q, d.ld_q), (d.k, d.ld_k), (d.v, d.ld_v) = ((g.ptr() + off * es, g.ld) for g, off in place(IN))
    d.out, d.ld_out, d.lse = OUT.ptr(), OUT.ld, LSE.ptr()
    d.B, d.Nq, d.Nk, d.H, d.head_dim, d.dtype, d.causal, d.scale = B, Nq, Nk, H, hd, code, int(causal), scale
    _capi.check(lib.me_attention_qkv_fwd(ctypes.byref(d), _capi.stream_ptr()), "me_attention_qkv_fwd")
    torch.cuda.synchronize()
    what = f"guarded attention_qkv {Nq}x{Nk} hd {hd} {dt}"
    OUT.check(what + " out")
    LSE.check(what + " lse")
    assert OUT.untouched_interior() == 0 and LSE.untouched_interior() == 0
    assert not bool(torch.isnan(OUT.t).any()) and not bool(torch.isnan(LSE.t).any())
    check_close(OUT.t.float(), ref.detach(), tol(dt), what + " out")
    check_close(LSE.vec().reshape(B, H, Nq), lse_ref.detach(), tol(dt), what + " lse")
    O_IN, LSE_IN, DO = Guarded.input(OUT.t, C + 8), Guarded.input(LSE.vec()), Guarded.input(do.to(dev), C + 8)
    DELTA = Guarded.output_vec(B * H * Nq, torch.float32, dev)
    d.out, d.ld_out, d.lse = O_IN.ptr(), O_IN.ld, LSE_IN.ptr()
    d.dout, d.ld_dout, d.delta = DO.ptr(), DO.ld, DELTA.ptr()
    (d.dq, d.ld_dq), (d.dk, d.ld_dk), (d.dv, d.ld_dv) = ((g.ptr() + off * es, g.ld) for g, off in place(GR))
    _capi.check(lib.me_attention_qkv_bwd(ctypes.byref(d), _capi.stream_ptr()), "me_attention_qkv_bwd")
    torch.cuda.synchronize()
    DELTA.check(what + " delta")
    for g in GR:
        g.check(what + " gradients")
        assert g.untouched_interior() == 0 and not bool(torch.isnan(g.t).any())
    grads = [g.t[:, off:off + C] for g, off in place(GR)]
    check_grads(grads, (qr.grad, kr.grad, vr.grad), tol(dt), what)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N,hd", tc.QKV_EQUIV)
def test_attention_qkv_agrees_with_packed_attention(dev, N, hd, dt):
    """non-causal, packed, Nq = Nk, no dropout: the same function as me_attention_fwd / _bwd, within the same bound"""
    scale = hd ** -0.5
    C = H * hd
    q, k, v, do = tc.qkv_values(B, N, N, H, hd, dt, seed=5)
    qkv = torch.cat([q, k, v], dim=1).to(dev)
    do = do.to(dev)
    o0, lse0 = ops.attention_fwd(qkv, B, N, H, hd, scale, True)
    d0 = ops.attention_bwd(qkv, o0, do, lse0, B, N, H, hd, scale)
    o1, lse1 = ops.attention_qkv_fwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, N, N, H, hd, scale, need_lse=True)
    d1 = torch.empty_like(qkv)
    ops.attention_qkv_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o1, do, lse1, B, N, N, H, hd, scale,
                          grads=(d1[:, :C], d1[:, C:2 * C], d1[:, 2 * C:]))
    check_close(o1.float(), o0.float(), tol(dt), "out")
    check_close(lse1, lse0, tol(dt), "lse")
    for j, nm in enumerate(("dQ", "dK", "dV")):
        check_close(d1[:, j * C:(j + 1) * C].float(), d0[:, j * C:(j + 1) * C].float(), tol(dt), nm)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("t", tc.QKV_CAUSALITY_T)
def test_attention_qkv_causality(dev, t, dt):
    """rows <= t of a causal call depend on nothing above t: other Q, K, V above t leave them bit-identical, and a dout that is zero above t
    gives dK = dV = 0 above t"""
    N, hd = tc.QKV_CAUSALITY_N, 24
    scale = hd ** -0.5
    C = H * hd
    q, k, v, do = (x.to(dev) for x in tc.qkv_values(B, N, N, H, hd, dt, seed=11))
    q2, k2, v2, _ = (x.to(dev) for x in tc.qkv_values(B, N, N, H, hd, dt, seed=12))
    above = (torch.arange(B * N, device=dev) % N > t)[:, None]
    qa, ka, va = torch.where(above, q2, q), torch.where(above, k2, k), torch.where(above, v2, v)
    o0, lse0 = ops.attention_qkv_fwd(q, k, v, B, N, N, H, hd, scale, causal=True, need_lse=True)
    o1, lse1 = ops.attention_qkv_fwd(qa, ka, va, B, N, N, H, hd, scale, causal=True, need_lse=True)
    keep = ~above[:, 0]
    assert torch.equal(o0[keep], o1[keep])
    assert torch.equal(lse0.reshape(B, H, N)[:, :, :t + 1], lse1.reshape(B, H, N)[:, :, :t + 1])
    if t + 1 < N:
        assert not torch.equal(o0[~keep], o1[~keep])
    dz = torch.where(above, torch.zeros_like(do), do)
    dq, dk, dv = ops.attention_qkv_bwd(q, k, v, o0, dz, lse0, B, N, N, H, hd, scale, causal=True)
    assert float(dk[~keep].abs().max()) == 0.0 and float(dv[~keep].abs().max()) == 0.0 and float(dq[~keep].abs().max()) == 0.0
    assert float(dv[keep].abs().max()) > 0.0
    assert bool(torch.isfinite(dq).all() and torch.isfinite(dk).all() and torch.isfinite(dv).all())


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Nq,Nk,causal,hd", tc.QKV_DROPOUT)
def test_attention_qkv_dropout_exact_mask(dev, Nq, Nk, causal, hd, dt):
    """p = 0.1: forward and gradients against float64 on the dtype-rounded operands with the mask restated on the host (index
    ((b*H + h)*Nq + q)*Nk + k).  bf16 takes the delta pass of attn_qkv_delta_kernel under dropout; this is its check against a reference."""
    p, seed = 0.1, 0x5DEECE66D
    keep = tc.qkv_keep(seed, B, H, Nq, Nk, p)
    assert 0.85 < keep.mean() < 0.95
    (out, lse, grads), (ref, lse_ref, gref) = run_case(dev, Nq, Nk, causal, hd, "q_kv2", dt, p_drop=p, seed=seed)
    what = f"attention_qkv dropout {Nq}x{Nk} causal={causal} hd={hd} {dt}"
    for nm, g, w in (("out", out, ref), ("lse", lse, lse_ref)) + tuple(zip(("dQ", "dK", "dV"), grads, gref)):
        print(f"{what} {nm}: max-abs error {float((g.detach().double().cpu() - w).abs().max() / w.abs().max()):.3e} of max|ref|")
    check_close(out.float(), ref, tol(dt), what + " out")
    check_close(lse, lse_ref, tol(dt), what + " lse (unmasked row sum)")
    check_grads(grads, gref, tol(dt), what)
    (o_other, _, _), _ = run_case(dev, Nq, Nk, causal, hd, "q_kv2", dt, p_drop=p, seed=seed + 1)
    assert not torch.equal(out, o_other)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
def test_attention_qkv_two_runs_are_bit_identical(dev, dt):
    for Nq, Nk, causal, p in ((129, 65, False, 0.0), (200, 200, True, 0.1)):
        a, _ = run_case(dev, Nq, Nk, causal, 96, "q_kv2", dt, p_drop=p, seed=7)
        b, _ = run_case(dev, Nq, Nk, causal, 96, "q_kv2", dt, p_drop=p, seed=7)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x, y)


def test_attention_qkv_rejections(dev):
    """each returns non-zero with a message and launches nothing (the output keeps its sentinel)"""
    lib = _capi.load()
    N, hd = 16, 8
    C = H * hd

    def desc(**kw):
        bufs = [torch.zeros((B * N, C + 8), dtype=torch.float32, device=dev) for _ in range(3)]
        out = torch.full((B * N, 256), 7.0, dtype=torch.float32, device=dev)
        d = _capi.AttnQkvDesc()
        d.q, d.k, d.v = (_capi.ptr(t) for t in bufs)
        d.ld_q = d.ld_k = d.ld_v = C + 8
        d.out, d.ld_out = _capi.ptr(out), 256
        d.B, d.Nq, d.Nk, d.H, d.head_dim, d.dtype, d.causal = B, N, N, H, hd, _capi.ME_F32, 0
        d.scale = hd ** -0.5
        for key, val in kw.items():
            setattr(d, key, val)
        return d, out, bufs

    for kw, word in ((dict(causal=1, Nk=N - 1), b"causal"), (dict(head_dim=136), b"head_dim"), (dict(ld_q=C + 6), b"multiples of 4"),
                     (dict(q=None), b"null pointer"), (dict(v=None), b"null pointer")):
        d, out, bufs = desc(**kw)
        rc = lib.me_attention_qkv_fwd(ctypes.byref(d), _capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and word in lib.me_last_error(), (kw, rc, lib.me_last_error())
        assert bool((out == 7.0).all()), kw
        rc = lib.me_attention_qkv_bwd(ctypes.byref(d), _capi.stream_ptr())      # (its gradient pointers are null as well)
        assert rc != 0 and lib.me_last_error(), kw
    d, out, bufs = desc()
    assert lib.me_attention_qkv_fwd(ctypes.byref(d), _capi.stream_ptr()) == 0      # the unmodified descriptor is a valid call
    torch.cuda.synchronize()
    assert not bool((out[:, :C] == 7.0).any()) and bool((out[:, C:] == 7.0).all())
