"""GPU: the optimizer entry points (me_adamw_step, me_grad_stats, me_adamw_prepare + me_adamw_step_segments) called through _capi on
guard-band buffers (tests/guarded.py): the gradient between NaN guards; parameters, both moments, the bf16 mirror, the statistics, the
control block, the segment table and the workspace between sentinel guards with their old contents inside.

Reference: ew_cases.adamw_ref_step, torch.optim.AdamW restated per element in float64 with per-element lr / weight-decay vectors
(tests/test_ew_cases_cpu.py ties it to torch.optim.AdamW with parameter groups), chained over the steps from the stored initial state.
Bounds: 1e-5 for me_adamw_step and 2e-6 for the segments form (those of test_gpu_ops.py / test_gpu_optim.py), max-abs error over max-abs
reference, after every step, for p, m and v; the mirror equals p.to(bfloat16) bit for bit.  The control block against its formulas:
step / skip / found_inf exactly, grad_mul and total_norm to 2^-21 (a handful of fp32 roundings), the bias corrections to
ew_cases.bias_correction_tol (powf within 2 ulp, amplified by the subtraction from 1).

FlatParams pads every parameter to 64 elements, so the module-level tests never reach what these sizes reach: the n % 4 tail of the
vector kernel, the scalar kernel for slices whose four streams sit 0 / 1 / 2 / 3 elements off a 16-byte boundary, and segment ends that
are no multiple of anything."""
import ctypes

import pytest
import torch

import ew_cases as ew
from conftest import rel_err
from ew_cases import BF16, F32
from guarded import Guarded
from metatransformer_amd import _capi

pytestmark = pytest.mark.gpu

ERR_ARG = -1
LR, B1, B2, EPS, WD = 1e-2, 0.9, 0.95, 1e-8, 0.05


def S():
    return _capi.stream_ptr()


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def out_at(values: torch.Tensor, off: int) -> Guarded:
    """a guarded output whose interior starts `off` elements in front of `values` (those elements keep the sentinel)"""
    G = Guarded.output_vec(values.numel() + off, values.dtype, values.device)
    G.t[0, off:].copy_(values)
    return G


def in_at(values: torch.Tensor, off: int) -> Guarded:
    pad = torch.full((off,), float("nan"), dtype=values.dtype, device=values.device)
    return Guarded.input(torch.cat((pad, values)))


def at(G: Guarded, off: int) -> int:
    return G.ptr() + off * G.esize


def front_intact(G: Guarded, off: int) -> bool:
    return off == 0 or bool((G.interior_bits()[0, :off] == G.sentinel).all())


def all_sentinel(G: Guarded) -> bool:
    return G.violation() is None and G.untouched_interior() == G.rows * G.cols


# ------------------------------------------------------------------------------------------------ me_adamw_step
def _adamw_run(lib, dev, n, offs, mirror_off, with_mirror, p0, grads):
    """three steps on buffers whose streams start offs = (p, g, m, v) elements in; returns per-step (p, m, v, mirror) and checks guards"""
    P, M, V = out_at(p0, offs[0]), out_at(torch.zeros_like(p0), offs[2]), out_at(torch.zeros_like(p0), offs[3])
    MIR = out_at(torch.full((n,), 7.0, dtype=BF16, device=dev), mirror_off) if with_mirror else None
    states = []
    for step, g in enumerate(grads, 1):
        G = in_at(g, offs[1])
        what = f"adamw_step n {n} offsets {offs} mirror {with_mirror} step {step}"
        _capi.check(lib.me_adamw_step(at(P, offs[0]), at(G, offs[1]), at(M, offs[2]), at(V, offs[3]), n, LR, B1, B2, EPS, WD, step, 0.5,
                                      at(MIR, mirror_off) if MIR else None, S()), what)
        torch.cuda.synchronize()
        for o, off, nm in ((P, offs[0], "param"), (M, offs[2], "exp_avg"), (V, offs[3], "exp_avg_sq")) + (((MIR, mirror_off, "mirror"),) if MIR else ()):
            o.check(f"{what}: {nm}")
            assert front_intact(o, off), f"{what}: {nm}: the elements in front of the slice were written"
        p, m, v = P.t[0, offs[0]:].clone(), M.t[0, offs[2]:].clone(), V.t[0, offs[3]:].clone()
        mir = MIR.t[0, mirror_off:].clone() if MIR else None
        if MIR:
            ew.assert_bits_equal(mir, p.to(BF16), f"{what}: mirror == bf16(param)")
        states.append((p, m, v, mir))
    return states


@pytest.mark.parametrize("with_mirror", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_adamw_step_contract(dev, n, with_mirror):
    lib = _capi.load()
    g = gen(dev, n)
    p0 = torch.randn(n, device=dev, generator=g)
    grads = [torch.randn(n, device=dev, generator=g) for _ in range(3)]
    aligned = _adamw_run(lib, dev, n, (0, 0, 0, 0), 0, with_mirror, p0, grads)
    scalar = _adamw_run(lib, dev, n, (0, 1, 2, 3), 1, with_mirror, p0, grads)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    for step in (1, 2, 3):
        p, m, v = ew.adamw_ref_step(p, grads[step - 1], m, v, ew.f32(LR), ew.f32(WD), ew.f32(B1), ew.f32(B2), ew.f32(EPS), step, grad_scale=0.5)
        for (got, want, nm) in zip(aligned[step - 1][:3], (p, m, v), ("param", "exp_avg", "exp_avg_sq")):
            e = rel_err(got, want)
            assert e < 1e-5, f"adamw_step n {n} step {step}: {nm} off by {e:.3e}"
        for a, b, nm in zip(aligned[step - 1], scalar[step - 1], ("param", "exp_avg", "exp_avg_sq", "mirror")):
            if a is not None:
                ew.assert_bits_equal(b, a, f"adamw_step n {n} step {step}: {nm}, misaligned slice against aligned")
    assert float((aligned[2][0] - p0).abs().max()) > 1e-3, "the steps moved the parameters"


def test_adamw_step_of_nothing_and_step_zero(dev):
    lib = _capi.load()
    x = torch.randn(8, device=dev, generator=gen(dev, 1))
    P, M, V = Guarded.output_vec(8, F32, dev), Guarded.output_vec(8, F32, dev), Guarded.output_vec(8, F32, dev)
    MIR, G = Guarded.output_vec(8, BF16, dev), Guarded.input(x)
    _capi.check(lib.me_adamw_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), 0, LR, B1, B2, EPS, WD, 1, 1.0, MIR.ptr(), S()), "n = 0")
    torch.cuda.synchronize()
    assert all(all_sentinel(o) for o in (P, M, V, MIR)), "n = 0 writes nothing"
    rc = lib.me_adamw_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), 8, LR, B1, B2, EPS, WD, 0, 1.0, MIR.ptr(), S())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and all(all_sentinel(o) for o in (P, M, V, MIR)), "step = 0 is rejected (bias correction divides by 1 - beta^step)"


# ------------------------------------------------------------------------------------------------ me_grad_stats
def _grad_stats(lib, dev, g, what):
    G, ST = Guarded.input(g), Guarded.output_vec(2, F32, dev)
    W = Guarded.output_bytes(lib.me_grad_stats_workspace(), dev)
    _capi.check(lib.me_grad_stats(G.ptr(), g.numel(), ST.ptr(), W.ptr(), S()), what)
    torch.cuda.synchronize()
    ST.check(what + ": stats")
    W.check(what + ": workspace")
    assert ST.untouched_interior() == 0, what
    return ST


def _stats_ref(g):
    fin = torch.isfinite(g)
    return float(torch.where(fin, g, torch.zeros_like(g)).double().pow(2).sum().sqrt()), float((~fin).sum())


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1027])
def test_grad_stats_contract(dev, n):
    lib = _capi.load()
    g = torch.randn(n, device=dev, generator=gen(dev, n)) * 3
    for tail_bad in (0, 1, 2):
        if tail_bad > min(n, 3):
            continue
        gg = g.clone()
        if tail_bad >= 1:
            gg[n - 1] = float("inf")                      # (the last element is always in the n % 4 tail at these sizes)
        if tail_bad >= 2:
            gg[n - 2] = float("nan")
        what = f"grad_stats n {n}, {tail_bad} non-finite values in the tail"
        st = _grad_stats(lib, dev, gg, what).vec()
        norm, bad = _stats_ref(gg)
        assert float(st[1]) == bad == float(tail_bad), f"{what}: counted {float(st[1])}"
        assert abs(float(st[0]) - norm) <= 2.0 ** -22 * norm, f"{what}: norm {float(st[0])!r}, want {norm!r}"
    G, ST = Guarded.input(torch.cat((g, g[:1]))), Guarded.output_vec(2, F32, dev)
    W = Guarded.output_bytes(lib.me_grad_stats_workspace(), dev)
    rc = lib.me_grad_stats(G.ptr() + 4, n, ST.ptr(), W.ptr(), S())
    torch.cuda.synchronize()
    assert rc == ERR_ARG and all_sentinel(ST) and all_sentinel(W), "a gradient buffer off a 16-byte boundary is rejected, nothing written"


# ------------------------------------------------------------------------------------------------ me_adamw_prepare + me_adamw_step_segments
def _layouts():
    perm = torch.randperm(512, generator=torch.Generator().manual_seed(12)).tolist()
    sizes = [2 if perm[k] < 188 else 1 for k in range(512)]          # 188 segments of two elements, 324 of one: 700 elements
    ends, e = [], 0
    for s in sizes:
        e += s
        ends.append(e)
    assert e == 700
    return {"four": (1027, [1, 2, 7, 1027]), "one": (1027, [1027]), "512": (700, ends)}


LAYOUTS = _layouts()
# (stats given, loss scale, max_norm): without statistics; without a loss scale, clipping; with both, max_norm out of reach
CONFIGS = {"no_stats": (False, 4.0, 1.0), "no_loss_scale_clips": (True, None, 0.5), "does_not_clip": (True, 8.0, 1e6)}


def _segment_table(dev, ends, scales, wds) -> Guarded:
    arr = (_capi.AdamwSegment * len(ends))()
    for k, (e, s, w) in enumerate(zip(ends, scales, wds)):
        arr[k].end, arr[k].lr_scale, arr[k].weight_decay = e, s, w
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    return Guarded.output(1, raw.numel(), None, torch.uint8, dev, old=raw), raw


def _read_ctl(CTL: Guarded) -> _capi.AdamwCtl:
    return _capi.AdamwCtl.from_buffer_copy(bytes(CTL.t[0].cpu().numpy().tobytes()))


def _check_ctl(ctl, want, step_before, what):
    assert ctl.step == want["step"], f"{what}: step {ctl.step}, want {want['step']}"
    assert ctl.skip == want["skip"] and ctl.found_inf == want["found_inf"], f"{what}: skip {ctl.skip}, found_inf {ctl.found_inf}"
    for nm, tol in (("grad_mul", 2.0 ** -21), ("total_norm", 2.0 ** -21), ("bc1", ew.bias_correction_tol(B1, want["step"])),
                    ("bc2_sqrt", ew.bias_correction_tol(B2, want["step"]))):
        got, w = float(getattr(ctl, nm)), want[nm]
        assert abs(got - w) <= tol * abs(w), f"{what}: {nm} {got!r}, want {w!r} (tolerance {tol:.1e} relative)"


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_adamw_segments_contract(dev, layout, config):
    lib = _capi.load()
    n, ends = LAYOUTS[layout]
    with_stats, loss_scale, max_norm = CONFIGS[config]
    ns = len(ends)
    scales = [0.5 + k / 1024.0 for k in range(ns)]
    wds = [0.01 * (k % 7) for k in range(ns)]
    ls, wd = ew.segment_vectors(n, ends, [ew.f32(s) for s in scales], [ew.f32(w) for w in wds])
    ls, wd = ls.to(dev), wd.to(dev)
    SEG, seg_raw = _segment_table(dev, ends, scales, wds)
    g = gen(dev, n + ns)
    p0 = torch.randn(n, device=dev, generator=g)
    P, M, V = Guarded.output_vec(n, F32, dev, old=p0), Guarded.output_vec(n, F32, dev, old=torch.zeros(n)), Guarded.output_vec(n, F32, dev, old=torch.zeros(n))
    MIR = Guarded.output_vec(n, BF16, dev, old=torch.full((n,), 7.0))
    CTL = Guarded.output_bytes(ctypes.sizeof(_capi.AdamwCtl), dev)
    CTL.t.zero_()
    LS = Guarded.input(torch.tensor([loss_scale], device=dev)) if loss_scale is not None else None
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    step_ref = 0
    plan = ["good", "good", "good"] + (["inf", "good"] if with_stats else [])
    for it, kind in enumerate(plan):
        what = f"adamw segments {layout} / {config}, call {it + 1} ({kind})"
        grad = torch.randn(n, device=dev, generator=g) * (loss_scale or 1.0)
        if kind == "inf":
            grad[n - 1] = float("inf")
        G = Guarded.input(grad)
        ST = None
        if with_stats:
            ST = Guarded.output_vec(2, F32, dev)
            W = Guarded.output_bytes(lib.me_grad_stats_workspace(), dev)
            _capi.check(lib.me_grad_stats(G.ptr(), n, ST.ptr(), W.ptr(), S()), what)
        _capi.check(lib.me_adamw_prepare(CTL.ptr(), ST.ptr() if ST else None, LS.ptr() if LS else None, 0.5, max_norm, B1, B2, S()), what)
        before = [o.t.clone() for o in (P, M, V, MIR)]
        _capi.check(lib.me_adamw_step_segments(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, SEG.ptr(), ns, LR, B1, B2, EPS, CTL.ptr(), MIR.ptr(), S()), what)
        torch.cuda.synchronize()
        for o, nm in ((P, "param"), (M, "exp_avg"), (V, "exp_avg_sq"), (MIR, "mirror"), (CTL, "control block"), (SEG, "segment table")):
            o.check(f"{what}: {nm}")
        assert torch.equal(SEG.t[0], seg_raw), f"{what}: the segment table was modified"
        want = ew.adamw_ctl_ref(step_ref, _stats_ref(grad) if with_stats else None, loss_scale, 0.5, max_norm, B1, B2)
        _check_ctl(_read_ctl(CTL), want, step_ref, what)
        if config == "no_loss_scale_clips" and kind == "good":
            assert want["grad_mul"] < 0.5 * 0.999, "this max_norm clips"
        if config == "does_not_clip" and kind == "good":
            assert want["grad_mul"] == 0.5 / 8.0, "this max_norm does not clip"
        if kind == "inf":
            assert want["skip"] == 1.0 and want["step"] == step_ref
            for o, b, nm in zip((P, M, V, MIR), before, ("param", "exp_avg", "exp_avg_sq", "mirror")):
                ew.assert_bits_equal(o.t, b, f"{what}: {nm} must not move on a skipped step", nan_by_isnan=True)
            continue
        step_ref = want["step"]
        p, m, v = ew.adamw_ref_step(p, grad, m, v, ew.f32(LR) * ls, wd, ew.f32(B1), ew.f32(B2), ew.f32(EPS), step_ref, grad_scale=want["grad_mul"])
        for o, w, nm in ((P, p, "param"), (M, m, "exp_avg"), (V, v, "exp_avg_sq")):
            e = rel_err(o.vec(), w)
            assert e < 2e-6, f"{what}: {nm} off by {e:.3e}"
        ew.assert_bits_equal(MIR.vec(), P.vec().to(BF16), f"{what}: mirror == bf16(param)")
    assert step_ref == (4 if with_stats else 3)


def test_adamw_segments_rejections(dev):
    lib = _capi.load()
    n = 16
    SEG, _ = _segment_table(dev, [n], [1.0], [0.0])
    P, M, V = Guarded.output_vec(n, F32, dev), Guarded.output_vec(n, F32, dev), Guarded.output_vec(n, F32, dev)
    G = Guarded.input(torch.ones(n, device=dev))
    CTL = Guarded.output_bytes(ctypes.sizeof(_capi.AdamwCtl), dev)
    for ns in (0, 513):
        rc = lib.me_adamw_step_segments(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, SEG.ptr(), ns, LR, B1, B2, EPS, CTL.ptr(), None, S())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and all(all_sentinel(o) for o in (P, M, V)), f"{ns} segments are rejected, nothing written"
