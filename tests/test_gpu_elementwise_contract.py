"""GPU: the element-wise entry points of the C API (me_cast, me_split3, me_transpose_cast / _batched, me_split3_batched, me_add_rows,
me_window_rows, me_dropout_add, me_colsum_mul, me_resize_rows, me_pool_tokens / _bwd) called through _capi with raw arguments on guard-band
buffers (tests/guarded.py): inputs between NaN guards, outputs and workspaces between sentinel guards.  References: tests/ew_cases.py, float64
or bit-exact from the stored operands.

Index arithmetic and single roundings are compared bit for bit.  me_dropout_add (p = 0): 1e-6.  Where the project had no bound the yardstick
is measured where the test runs -- the same operation done by torch in fp32 on the device against the float64 reference -- and the kernel may
err 4 x as much (never less than 4 x 2^-24; a bf16 output adds its own rounding: half an ulp of 8 significant bits is up to
2^-8 of the element).  Metric: ew_cases.close_tol, the smallest tolerance
at which conftest.check_close passes.
Measured on MI355X (the worst yardstick, the bound it gives, and the worst kernel error over the family's cases):
    me_colsum_mul              torch fp32 2.05e-07 -> bound 8.22e-07, kernel 4.52e-07
    me_resize_rows, fp32 out   torch fp32 1.35e-06 -> bound 5.41e-06, kernel 1.36e-06 (bilinear 1.35e-06, bicubic 1.36e-06)
    me_resize_rows, bf16 out   bound 5.41e-06 + 2^-8 = 3.91e-03, kernel 3.80e-03 (the output rounding)
    me_pool_tokens, mean       torch fp32 7.73e-08 -> bound 3.09e-07, kernel 8.89e-08
(each test prints its own figures before it asserts)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ew_cases as ew
from conftest import check_close
from ew_cases import BF16, F16, F32
from guarded import Guarded
from metatransformer_amd import _capi

pytestmark = pytest.mark.gpu

ERR_ARG = -1
DT3 = [F32, BF16, F16]
DT2 = [F32, BF16]


def code(dt):
    return _capi.dtype_code(dt, True)


def S():
    return _capi.stream_ptr()


def sync():
    torch.cuda.synchronize()


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def esz(dt):
    return torch.empty((), dtype=dt).element_size()


def all_sentinel(G: Guarded) -> bool:
    return G.violation() is None and G.untouched_interior() == G.rows * G.cols


def ok(rc, what):
    _capi.check(rc, what)
    sync()


def rejected(rc, outs, what):
    """an argument error: nothing was launched, every output still holds its sentinel"""
    sync()
    assert rc == ERR_ARG, f"{what}: expected ME_ERR_ARG, got {rc}"
    for o in outs:
        assert all_sentinel(o), f"{what}: a rejected call wrote to an output"


def guarded_ints(values: torch.Tensor) -> Guarded:
    """an int32 operand between sentinel guards (Guarded.input is for floating types)"""
    v2 = values.reshape(1, -1) if values.dim() == 1 else values
    return Guarded.output(v2.shape[0], v2.shape[1], None, torch.int32, values.device, old=v2)


# ------------------------------------------------------------------------------------------------ me_cast
@pytest.mark.parametrize("dst", DT3, ids=str)
@pytest.mark.parametrize("src", DT3, ids=str)
def test_cast_contract(dev, src, dst):
    """every (src, dst) pair over the sizes that reach the body, the n % 4 tail, n < 4 and a second grid sweep; bit for bit against
    tensor.to(dtype) on the CPU, NaN by position"""
    lib = _capi.load()
    for n in ew.CAST_SIZES:
        what = f"cast {src} -> {dst}, n = {n}"
        x = ew.cast_input(n, src)
        X, Y = Guarded.input(x.to(dev)), Guarded.output_vec(n, dst, dev)
        ok(lib.me_cast(X.ptr(), code(src), Y.ptr(), code(dst), n, S()), what)
        Y.check(what)
        assert Y.untouched_interior() == 0, f"{what}: {Y.untouched_interior()} elements not written"
        ew.assert_bits_equal(Y.vec(), x.to(dst), what, nan_by_isnan=True)


@pytest.mark.parametrize("dst", DT3, ids=str)
@pytest.mark.parametrize("src", DT3, ids=str)
def test_cast_of_a_slice_that_starts_inside_a_buffer(dev, src, dst):
    """src, dst or both one element into a 16-byte aligned buffer: the element-wise kernel, same values, nothing in front touched"""
    lib = _capi.load()
    for n in (5, 1023):
        x = ew.cast_input(n, src)
        want = x.to(dst)
        for so, do in ((1, 0), (0, 1), (1, 1)):
            what = f"cast {src} -> {dst}, n = {n}, src + {so}, dst + {do}"
            xin = torch.cat((torch.full((so,), float("nan"), dtype=src), x)).to(dev)
            X, Y = Guarded.input(xin), Guarded.output_vec(n + do, dst, dev)
            ok(lib.me_cast(X.ptr() + so * esz(src), code(src), Y.ptr() + do * esz(dst), code(dst), n, S()), what)
            Y.check(what)
            if do:
                assert int(Y.interior_bits()[0, 0]) == Y.sentinel, f"{what}: the element in front of dst was written"
            assert int((Y.interior_bits()[0, do:] == Y.sentinel).sum()) == 0, f"{what}: elements not written"
            ew.assert_bits_equal(Y.vec()[do:], want, what, nan_by_isnan=True)


def test_cast_of_nothing_and_bad_dtype(dev):
    lib = _capi.load()
    X, Y = Guarded.input(torch.ones(4, device=dev)), Guarded.output_vec(4, BF16, dev)
    ok(lib.me_cast(X.ptr(), code(F32), Y.ptr(), code(BF16), 0, S()), "n = 0")
    assert all_sentinel(Y)
    rejected(lib.me_cast(X.ptr(), code(F32), Y.ptr(), _capi.ME_BF16X3, 4, S()), [Y], "cast to a plane dtype")


# ------------------------------------------------------------------------------------------------ me_split3
def _split3_input(dev, rows, cols, seed):
    g = gen(dev, seed)
    x = torch.randn(rows, cols, device=dev, generator=g) * torch.logspace(-4, 4, cols, device=dev)
    x[0, 0], x[-1, -1] = 0.0, -0.0
    x[0, 1] = 1.00390625                                     # 1 + 2^-8: a tie between two bf16 neighbours
    return x


@pytest.mark.parametrize("right", [0, 1])
@pytest.mark.parametrize("cols", [4, 260])
def test_split3_contract(dev, cols, right):
    lib = _capi.load()
    for rows in (0, 1, 3, 257):
        for ld in (cols, cols + 4):
            what = f"split3 {rows} x {cols}, ld_src {ld}, right_operand {right}"
            x = _split3_input(dev, max(rows, 1), cols, rows + cols)
            X, Y = Guarded.input(x, ld), Guarded.output(max(rows, 1), 3 * cols, None, BF16, dev)
            ok(lib.me_split3(X.ptr(), ld, Y.ptr(), rows, cols, right, S()), what)
            Y.check(what)
            if rows == 0:
                assert all_sentinel(Y), f"{what}: rows = 0 writes nothing"
                continue
            assert Y.untouched_interior() == 0, what
            ew.assert_bits_equal(Y.t, ew.split3_ref(x.cpu(), bool(right)), what)


def test_split3_rejections(dev):
    lib = _capi.load()
    x = _split3_input(dev, 3, 8, 1)
    Y = Guarded.output(3, 24, None, BF16, dev)
    X = Guarded.input(x, 12)
    rejected(lib.me_split3(X.ptr(), 12, Y.ptr(), 3, 6, 0, S()), [Y], "cols % 4 != 0")
    rejected(lib.me_split3(X.ptr(), 10, Y.ptr(), 3, 8, 0, S()), [Y], "ld_src % 4 != 0")
    rejected(lib.me_split3(X.ptr() + 4, 12, Y.ptr(), 2, 8, 0, S()), [Y], "src one element off a 16-byte boundary")


# ------------------------------------------------------------------------------------------------ transposes
TC_SHAPES = [(1, 1), (1, 65), (65, 1), (63, 129)]


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F16, F32), (F32, F32)], ids=str)
def test_transpose_cast_guards(dev, src, dst):
    lib = _capi.load()
    for rows, cols in TC_SHAPES:
        what = f"transpose_cast {rows} x {cols} {src} -> {dst}"
        x = torch.randn(rows, cols, device=dev, generator=gen(dev, rows + cols)).to(src)
        X, Y = Guarded.input(x), Guarded.output(cols, rows, None, dst, dev)
        ok(lib.me_transpose_cast(X.ptr(), code(src), Y.ptr(), code(dst), rows, cols, S()), what)
        Y.check(what)
        assert Y.untouched_interior() == 0, what
        ew.assert_bits_equal(Y.t, x.t().to(dst).cpu(), what)


def _batch(items, src_code, dst_code):
    b = _capi.TcBatch()
    b.n, b.src_dtype, b.dst_dtype = len(items), src_code, dst_code
    for k, (X, Y, rows, cols) in enumerate(items):
        b.item[k].src, b.item[k].dst, b.item[k].rows, b.item[k].cols = X.ptr(), Y.ptr(), rows, cols
    return b


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F16)], ids=str)
def test_transpose_cast_batched_guards(dev, src, dst):
    """48 small matrices in one launch: the ragged shapes (element-wise branch) and multiples of 4 (the 4-wide branch) side by side"""
    lib = _capi.load()
    shapes = (TC_SHAPES + [(4, 8), (64, 68), (68, 4), (8, 132)]) * 6
    assert len(shapes) == _capi.ME_TC_BATCH
    items, xs = [], []
    for k, (rows, cols) in enumerate(shapes):
        x = torch.randn(rows, cols, device=dev, generator=gen(dev, k)).to(src)
        xs.append(x)
        items.append((Guarded.input(x), Guarded.output(cols, rows, None, dst, dev), rows, cols))
    b = _batch(items, code(src), code(dst))
    ok(lib.me_transpose_cast_batched(ctypes.byref(b), S()), "batch of 48")
    for k, ((_, Y, rows, cols), x) in enumerate(zip(items, xs)):
        what = f"transpose_cast_batched item {k} ({rows} x {cols}) {src} -> {dst}"
        Y.check(what)
        assert Y.untouched_interior() == 0, what
        ew.assert_bits_equal(Y.t, x.t().to(dst).cpu(), what)
    fresh = [(X, Guarded.output(cols, rows, None, dst, dev), rows, cols) for X, _, rows, cols in items[:2]]
    b0 = _batch(fresh, code(src), code(dst))
    b0.n = 0
    ok(lib.me_transpose_cast_batched(ctypes.byref(b0), S()), "batch of 0")
    assert all(all_sentinel(Y) for _, Y, _, _ in fresh), "a batch of 0 writes nothing"
    b0.n = _capi.ME_TC_BATCH + 1
    rejected(lib.me_transpose_cast_batched(ctypes.byref(b0), S()), [Y for _, Y, _, _ in fresh], "batch of 49")


@pytest.mark.parametrize("right", [0, 1])
@pytest.mark.parametrize("transposed", [0, 1])
def test_split3_batched_guards(dev, transposed, right):
    lib = _capi.load()
    shapes = [(4, 4), (4, 68), (68, 4), (64, 132)] * 12
    assert len(shapes) == _capi.ME_TC_BATCH
    items, xs = [], []
    for k, (rows, cols) in enumerate(shapes):
        x = _split3_input(dev, rows, cols, k)
        xs.append(x)
        orows, ocols = (cols, 3 * rows) if transposed else (rows, 3 * cols)
        items.append((Guarded.input(x), Guarded.output(orows, ocols, None, BF16, dev), rows, cols))
    b = _batch(items, _capi.ME_F32, _capi.ME_BF16X3)
    ok(lib.me_split3_batched(ctypes.byref(b), transposed, right, S()), "batch of 48")
    for k, ((_, Y, rows, cols), x) in enumerate(zip(items, xs)):
        what = f"split3_batched item {k} ({rows} x {cols}), transposed {transposed}, right_operand {right}"
        Y.check(what)
        assert Y.untouched_interior() == 0, what
        src = x.t().contiguous() if transposed else x
        ew.assert_bits_equal(Y.t, ew.split3_ref(src.cpu(), bool(right)), what)
    fresh = [(X, Guarded.output(Y.rows, Y.cols, None, BF16, dev), rows, cols) for X, Y, rows, cols in items[:2]]
    b0 = _batch(fresh, _capi.ME_F32, _capi.ME_BF16X3)
    b0.n = 0
    ok(lib.me_split3_batched(ctypes.byref(b0), transposed, right, S()), "batch of 0")
    assert all(all_sentinel(Y) for _, Y, _, _ in fresh)
    b0.n = _capi.ME_TC_BATCH + 1
    rejected(lib.me_split3_batched(ctypes.byref(b0), transposed, right, S()), [Y for _, Y, _, _ in fresh], "batch of 49")


# ------------------------------------------------------------------------------------------------ me_add_rows
@pytest.mark.parametrize("ydt", DT2, ids=str)
@pytest.mark.parametrize("pdt", DT2, ids=str)
@pytest.mark.parametrize("xdt", DT2, ids=str)
def test_add_rows_contract(dev, xdt, pdt, ydt):
    lib = _capi.load()
    rows, pos_rows = 7, 3
    for cols in (4, 260):
        what = f"add_rows {rows} x {cols} ({xdt} + {pdt} -> {ydt})"
        g = gen(dev, cols)
        x = torch.randn(rows, cols, device=dev, generator=g).to(xdt)
        pos = torch.randn(pos_rows, cols, device=dev, generator=g).to(pdt)
        X, P, Y = Guarded.input(x), Guarded.input(pos), Guarded.output(rows, cols, None, ydt, dev)
        ok(lib.me_add_rows(X.ptr(), code(xdt), P.ptr(), code(pdt), Y.ptr(), code(ydt), rows, pos_rows, cols, S()), what)
        Y.check(what)
        assert Y.untouched_interior() == 0, what
        want = (x.float() + pos.float()[torch.arange(rows, device=dev) % pos_rows]).to(ydt)
        ew.assert_bits_equal(Y.t, want.cpu(), what)
        for who, (ox, op, oy) in (("x", (1, 0, 0)), ("pos", (0, 1, 0)), ("y", (0, 0, 1))):
            Y2 = Guarded.output(rows, cols, None, ydt, dev)
            rejected(lib.me_add_rows(X.ptr() + ox * esz(xdt), code(xdt), P.ptr() + op * esz(pdt), code(pdt), Y2.ptr() + oy * esz(ydt),
                                     code(ydt), rows - 1, pos_rows - 1, cols, S()), [Y2], f"{what}: {who} one element off")


# ------------------------------------------------------------------------------------------------ me_window_rows
@pytest.mark.parametrize("dt", DT2, ids=str)
@pytest.mark.parametrize("B,H,W,ws,cols", [(2, 3, 5, 7, 4), (1, 4, 4, 1, 8), (2, 5, 6, 4, 8)])
def test_window_rows_contract(dev, B, H, W, ws, cols, dt):
    lib = _capi.load()
    gh, gw = -(-H // ws), -(-W // ws)
    tok_rows, win_rows = B * H * W, B * gh * gw * ws * ws
    g = gen(dev, H * W + ws)
    for merge in (0, 1):
        what = f"window_rows B {B} grid {H} x {W} ws {ws} cols {cols} {dt} merge {merge}"
        src_rows, dst_rows = (win_rows, tok_rows) if merge else (tok_rows, win_rows)
        x = torch.randn(src_rows, cols, device=dev, generator=g).to(dt)
        X, Y = Guarded.input(x), Guarded.output(dst_rows, cols, None, dt, dev)
        rc = lib.me_window_rows(X.ptr(), Y.ptr(), code(dt), B, H, W, ws, cols, merge, S())
        if (cols * esz(dt)) % 16:
            rejected(rc, [Y], what + " (rows that are no multiple of 16 bytes are refused)")
            continue
        ok(rc, what)
        Y.check(what)
        assert Y.untouched_interior() == 0, what
        want = ew.window_merge_ref(x, B, H, W, ws) if merge else ew.window_partition_ref(x, B, H, W, ws)
        ew.assert_bits_equal(Y.t, want.cpu(), what)


# ------------------------------------------------------------------------------------------------ me_dropout_add
def test_dropout_add_plain_fused_add(dev):
    """p_drop = p_path = 0: res + colscale * v with mixed dtypes (the masks: test_gpu_stochastic.py)"""
    lib = _capi.load()
    rows, cols = 5, 260
    g = gen(dev, 9)
    v = torch.randn(rows, cols, device=dev, generator=g).to(BF16)
    res = torch.randn(rows, cols, device=dev, generator=g)
    cs = 1 + 0.2 * torch.randn(cols, device=dev, generator=g)
    V, R, C, O = Guarded.input(v), Guarded.input(res), Guarded.input(cs), Guarded.output(rows, cols, None, F32, dev)
    what = "dropout_add p = 0, bf16 v + fp32 res -> fp32"
    ok(lib.me_dropout_add(V.ptr(), code(BF16), R.ptr(), code(F32), O.ptr(), code(F32), rows, cols, rows, 0.0, 0.0, 1234, C.ptr(), S()), what)
    O.check(what)
    assert O.untouched_interior() == 0, what
    check_close(O.t, res.double() + cs.double() * v.double(), 1e-6, what)
    for who, off in (("v", (2, 0, 0, 0)), ("res", (0, 4, 0, 0)), ("out", (0, 0, 4, 0)), ("colscale", (0, 0, 0, 4))):
        O2 = Guarded.output(rows, cols, None, F32, dev)
        rejected(lib.me_dropout_add(V.ptr() + off[0], code(BF16), R.ptr() + off[1], code(F32), O2.ptr() + off[2], code(F32), rows - 1, cols, rows,
                                    0.0, 0.0, 1234, C.ptr() + off[3], S()), [O2], f"dropout_add: {who} one element off")


# ------------------------------------------------------------------------------------------------ me_colsum_mul
@pytest.mark.parametrize("ydt", DT2, ids=str)
@pytest.mark.parametrize("xdt", DT2, ids=str)
@pytest.mark.parametrize("cols", [4, 260])
def test_colsum_mul_contract(dev, cols, xdt, ydt):
    """fewer rows than the 128 row splits and more; padded strides; overwrite and accumulate; the workspace exactly as queried"""
    lib = _capi.load()
    worst = {"yard": 0.0, "kernel": 0.0}
    for rows in (1, 5, 127, 129, 1000):
        g = gen(dev, rows + cols)
        x = torch.randn(rows, cols, device=dev, generator=g).to(xdt)
        y = torch.randn(rows, cols, device=dev, generator=g).to(ydt)
        old = torch.randn(cols, device=dev, generator=g)
        X, Y = Guarded.input(x, cols + 4), Guarded.input(y, cols + 8)
        for acc in (0, 1):
            what = f"colsum_mul {rows} x {cols} {xdt} * {ydt}, accumulate {acc}"
            ref = (x.double() * y.double()).sum(0) + (old.double() if acc else 0.0)
            yard = (x.float() * y.float()).sum(0) + (old if acc else 0.0)
            bound = ew.yardstick_bound(ew.close_tol(yard, ref))
            O = Guarded.output_vec(cols, F32, dev, old=old)
            W = Guarded.output_bytes(lib.me_colsum_workspace(cols), dev)
            ok(lib.me_colsum_mul(X.ptr(), code(xdt), cols + 4, Y.ptr(), code(ydt), cols + 8, rows, cols, O.ptr(), acc, W.ptr(), S()), what)
            O.check(what + ": out")
            W.check(what + ": workspace")
            err = ew.close_tol(O.vec(), ref)
            print(f"{what}: torch fp32 {ew.close_tol(yard, ref):.3e} -> bound {bound:.3e}, kernel {err:.3e}")
            worst["yard"], worst["kernel"] = max(worst["yard"], ew.close_tol(yard, ref)), max(worst["kernel"], err)
            assert not bool(torch.isnan(O.t).any()), f"{what}: NaN (a pad column or a guard was read)"
            check_close(O.vec(), ref, bound, what)
    print(f"colsum_mul cols {cols} {xdt} * {ydt}: worst yardstick {worst['yard']:.3e}, worst kernel {worst['kernel']:.3e}")


def test_colsum_mul_rejections(dev):
    lib = _capi.load()
    x = torch.randn(5, 8, device=dev, generator=gen(dev, 1))
    X, Y = Guarded.input(x, 12), Guarded.input(x.to(BF16), 16)
    O, W = Guarded.output_vec(8, F32, dev), Guarded.output_bytes(lib.me_colsum_workspace(8), dev)
    rejected(lib.me_colsum_mul(X.ptr() + 4, code(F32), 12, Y.ptr(), code(BF16), 16, 4, 8, O.ptr(), 0, W.ptr(), S()), [O, W], "x one element off")
    rejected(lib.me_colsum_mul(X.ptr(), code(F32), 12, Y.ptr() + 2, code(BF16), 16, 4, 8, O.ptr(), 0, W.ptr(), S()), [O, W], "y one element off")
    rejected(lib.me_colsum_mul(X.ptr(), code(F32), 12, Y.ptr(), code(BF16), 16, 4, 6, O.ptr(), 0, W.ptr(), S()), [O, W], "cols % 4 != 0")
    rejected(lib.me_colsum_mul(X.ptr(), code(F32), 10, Y.ptr(), code(BF16), 16, 4, 8, O.ptr(), 0, W.ptr(), S()), [O, W], "ldx % 4 != 0")


# ------------------------------------------------------------------------------------------------ me_resize_rows
RESIZE_SHAPES = [((1, 1), (3, 2)), ((2, 3), (5, 7)), ((7, 5), (3, 2)), ((14, 14), (16, 12)), ((4, 4), (4, 4))]


@pytest.mark.parametrize("ddt", DT2, ids=str)
@pytest.mark.parametrize("sdt", DT2, ids=str)
@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_resize_rows_contract(dev, mode, sdt, ddt):
    lib = _capi.load()
    mcode = _capi.ME_RESIZE_BICUBIC if mode == "bicubic" else _capi.ME_RESIZE_BILINEAR
    for (h, w), (H, W) in RESIZE_SHAPES:
        for C in (4, 260):
            what = f"resize_rows {mode} {h} x {w} -> {H} x {W}, C {C}, {sdt} -> {ddt}"
            t = torch.randn(h * w, C, device=dev, generator=gen(dev, h * w + C)).to(sdt)
            X, Y = Guarded.input(t), Guarded.output(H * W, C, None, ddt, dev)
            ok(lib.me_resize_rows(X.ptr(), code(sdt), Y.ptr(), code(ddt), h, w, H, W, C, mcode, S()), what)
            Y.check(what)
            assert Y.untouched_interior() == 0, what
            assert not bool(torch.isnan(Y.t).any()), f"{what}: NaN (a guard was read)"
            if (h, w) == (H, W):
                ew.assert_bits_equal(Y.t, t.to(ddt).cpu(), what + " (the identity)")
                continue
            ref = ew.resize_ref(t.double(), h, w, H, W, mode)
            yard = ew.close_tol(ew.resize_ref(t.float(), h, w, H, W, mode), ref)
            bound = ew.yardstick_bound(yard) + (2.0 ** -8 if ddt == BF16 else 0.0)
            print(f"{what}: torch fp32 {yard:.3e} -> bound {bound:.3e}, kernel {ew.close_tol(Y.t, ref):.3e}")
            check_close(Y.t, ref, bound, what)


def test_resize_rows_rejections(dev):
    lib = _capi.load()
    t = torch.randn(6, 8, device=dev, generator=gen(dev, 2))
    X, Xb = Guarded.input(t), Guarded.input(t.to(BF16))
    Y = Guarded.output(35, 8, None, F32, dev)
    rejected(lib.me_resize_rows(X.ptr() + 4, code(F32), Y.ptr(), code(F32), 2, 2, 5, 7, 8, 0, S()), [Y], "src one element off")
    rejected(lib.me_resize_rows(Xb.ptr() + 2, code(BF16), Y.ptr(), code(F32), 2, 2, 5, 7, 8, 0, S()), [Y], "bf16 src one element off")
    rejected(lib.me_resize_rows(X.ptr(), code(F32), Y.ptr() + 4, code(F32), 2, 3, 5, 6, 8, 0, S()), [Y], "dst one element off")
    rejected(lib.me_resize_rows(X.ptr(), code(F32), Y.ptr(), code(F32), 2, 3, 5, 7, 6, 0, S()), [Y], "cols % 4 != 0")
    rejected(lib.me_resize_rows(X.ptr(), code(F32), Y.ptr(), code(F32), 2, 3, 5, 7, 8, 2, S()), [Y], "unknown mode")


# ------------------------------------------------------------------------------------------------ me_pool_tokens / _bwd
POOL_SHAPES = [(1, 1, 4), (3, 2, 260), (2, 37, 8)]


def _pool_input(dev, B, N, C, dt, mode):
    x = torch.randn(B, N, C, device=dev, generator=gen(dev, B * N + C))
    if mode == _capi.ME_POOL_MAX:
        x = (2 * x).round() / 2                      # a grid of half-integers: equal maxima are common
        x[:, :, 1] = float("-inf")                   # a column that is -inf everywhere: arg-max 0
        x[:, :, 2] = 1.5                             # and one that is constant
    return x.to(dt)


@pytest.mark.parametrize("xdt", DT2, ids=str)
@pytest.mark.parametrize("mode", [_capi.ME_POOL_MEAN, _capi.ME_POOL_MAX, _capi.ME_POOL_FIRST], ids=["mean", "max", "first"])
def test_pool_tokens_contract(dev, mode, xdt):
    lib = _capi.load()
    for B, N, C in POOL_SHAPES:
        what = f"pool_tokens mode {mode} [{B}, {N}, {C}] {xdt}"
        x = _pool_input(dev, B, N, C, xdt, mode)
        X = Guarded.input(x.reshape(B * N, C))
        for with_arg in (True, False):
            O = Guarded.output(B, C, None, F32, dev)
            A = Guarded.output(B, C, None, torch.int32, dev)
            ok(lib.me_pool_tokens(X.ptr(), code(xdt), O.ptr(), A.ptr() if with_arg else None, B, N, C, mode, S()), what)
            O.check(what + ": out")
            A.check(what + ": argmax")
            assert O.untouched_interior() == 0, what
            if mode == _capi.ME_POOL_MEAN:
                ref = x.double().mean(1)
                yard = ew.close_tol(x.float().mean(1), ref)
                bound = ew.yardstick_bound(yard)
                print(f"{what}: torch fp32 {yard:.3e} -> bound {bound:.3e}, kernel {ew.close_tol(O.t, ref):.3e}")
                check_close(O.t, ref, bound, what)
            elif mode == _capi.ME_POOL_MAX:
                ew.assert_bits_equal(O.t, x.float().max(dim=1).values.cpu(), what)
            else:
                ew.assert_bits_equal(O.t, x[:, 0].float().cpu(), what)
            if mode == _capi.ME_POOL_MAX and with_arg:
                first = ew.argmax_first(x.float())
                assert N == 1 or bool((x.float() == x.float().max(dim=1, keepdim=True).values).sum(1).max() > 1), "the input has ties"
                assert torch.equal(A.t.cpu(), first.cpu()), f"{what}: arg-max is not the first index of the maximum"
            else:
                assert all_sentinel(A), f"{what}: argmax written without being asked for"


@pytest.mark.parametrize("dxdt", DT2, ids=str)
@pytest.mark.parametrize("mode", [_capi.ME_POOL_MEAN, _capi.ME_POOL_MAX, _capi.ME_POOL_FIRST], ids=["mean", "max", "first"])
def test_pool_tokens_bwd_contract(dev, mode, dxdt):
    lib = _capi.load()
    for B, N, C in POOL_SHAPES:
        what = f"pool_tokens_bwd mode {mode} [{B}, {N}, {C}] -> {dxdt}"
        g = gen(dev, B + N + C)
        dy = torch.randn(B, C, device=dev, generator=g)
        arg = torch.randint(0, N, (B, C), device=dev, generator=g, dtype=torch.int32)
        DY, A, DX = Guarded.input(dy), guarded_ints(arg), Guarded.output(B * N, C, None, dxdt, dev)
        ok(lib.me_pool_tokens_bwd(DY.ptr(), A.ptr() if mode == _capi.ME_POOL_MAX else None, DX.ptr(), code(dxdt), B, N, C, mode, S()), what)
        DX.check(what)
        A.check(what + ": argmax")
        assert torch.equal(A.t, arg), f"{what}: argmax modified"
        assert DX.untouched_interior() == 0, f"{what}: every element of dx is written"
        dx = DX.t.reshape(B, N, C)
        n = torch.arange(N, device=dev).reshape(1, N, 1)
        if mode == _capi.ME_POOL_MEAN:
            # two fp32 roundings (1 / N, the product): 2^-23 relative, bounded at 2^-22; a bf16 dx adds its rounding, 2^-8
            check_close(dx, (dy.double() / N)[:, None, :].expand(B, N, C), 2.0 ** -22 + (2.0 ** -8 if dxdt == BF16 else 0.0), what)
        elif mode == _capi.ME_POOL_MAX:
            want = torch.where(arg[:, None, :] == n, dy[:, None, :], torch.zeros((), device=dev)).to(dxdt)
            ew.assert_bits_equal(dx, want.cpu(), what)
        else:
            want = torch.where(n == 0, dy[:, None, :], torch.zeros((), device=dev)).expand(B, N, C).to(dxdt)
            ew.assert_bits_equal(dx, want.cpu(), what)


def test_pool_tokens_rejections(dev):
    lib = _capi.load()
    B, N, C = 2, 3, 8
    x = torch.randn(B * N, C, device=dev, generator=gen(dev, 3))
    X, Xb, DY = Guarded.input(x), Guarded.input(x.to(BF16)), Guarded.input(x[:B])
    O, DX = Guarded.output(B, C, None, F32, dev), Guarded.output(B * N, C, None, BF16, dev)
    rejected(lib.me_pool_tokens_bwd(DY.ptr(), None, DX.ptr(), code(BF16), B, N, C, _capi.ME_POOL_MAX, S()), [DX], "max backward without argmax")
    rejected(lib.me_pool_tokens(X.ptr() + 4, code(F32), O.ptr(), None, B, N - 1, C, 0, S()), [O], "x one element off")
    rejected(lib.me_pool_tokens(Xb.ptr() + 2, code(BF16), O.ptr(), None, B, N - 1, C, 0, S()), [O], "bf16 x one element off")
    rejected(lib.me_pool_tokens(X.ptr(), code(F32), O.ptr() + 4, None, B - 1, N, C, 0, S()), [O], "out one element off")
    rejected(lib.me_pool_tokens(X.ptr(), code(F32), O.ptr(), None, B, N, 6, 0, S()), [O], "C % 4 != 0")
    rejected(lib.me_pool_tokens_bwd(DY.ptr() + 4, None, DX.ptr(), code(BF16), B - 1, N, C, 0, S()), [DX], "dy one element off")
    rejected(lib.me_pool_tokens_bwd(DY.ptr(), None, DX.ptr() + 2, code(BF16), B, N - 1, C, 0, S()), [DX], "dx one element off")
