"""GPU: VideoMAE pre-training (me_tubelet_gather / me_take_rows / me_mae_assemble_fwd / _bwd / me_mae_loss, the three Pretrain
modules, mae_reconstruction_loss) against the float64 restatements of tests/video_mae_cases.py (tied to einops and to the reference
by tests/test_video_mae_cpu.py) and against the reference-made fixture.  Bounds are conftest's: fp32 TOL_F32; a bf16 single op
TOL_BF16_OP; the model under bf16 autocast TOL_BF16_FWD / TOL_BF16_GRAD."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN, TOL_BF16_FWD, TOL_BF16_GRAD, TOL_BF16_OP, TOL_F32, check_close

import metatransformer_amd as M
import video_mae_cases as vc
from guarded import Guarded
from metatransformer_amd import _capi, ops
from metatransformer_amd import video_mae as vm

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "video_mae.npz"), allow_pickle=False)


def inputs(case):
    """computed once per case, shared and left unchanged: clip, masks, index lists, the float64 labels of every token"""
    if case not in _cache:
        clip = torch.from_numpy(vc.make_clip(case))
        mask, dmask = vc.make_masks(case)
        kt, kh, kw = vc.tubelet(case)
        _cache[case] = dict(clip=clip, mask=mask, dmask=dmask, lists=vc.index_lists(mask), lists_dm=vc.index_lists(mask, dmask),
                            labels=vc.labels_restate(clip, kt, kh, kw), labels_raw=vc.labels_restate(clip, kt, kh, kw, normalize=False))
    return _cache[case]


def one_bf16_rounding(got: torch.Tensor, want64: torch.Tensor, what: str):
    """got (bf16) is the float64 value rounded once: within half a bf16 ulp of it, plus the fp32 arithmetic's own error"""
    err = (got.double().cpu() - want64).abs()
    bound = want64.abs() * 2.0 ** -8 * 1.001 + 1e-30
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements further than one bf16 rounding"


# ---------------------------------------------------------------------------------------------------------------- 1. gather

@pytest.mark.parametrize("case", list(vc.CASES))
def test_tubelet_gather_is_bit_exact(dev, case):
    r = inputs(case)
    kt, kh, kw = vc.tubelet(case)
    clip, N = r["clip"], vc.n_tokens(case)
    lists = {"visible": r["lists"][0], "decoded": r["lists_dm"][1], "descending": torch.arange(N - 1, -1, -2).repeat(2, 1),
             "repeated": torch.tensor([[1, 1, 0, N - 1, 1], [N - 1, 2, 2, 0, 0]])}
    for name, idx in lists.items():
        want = vc.gather_restate(clip, idx, kt, kh, kw)
        K = want.shape[2]
        got = vm.tubelet_gather(clip.to(dev), idx.to(dev), (kt, kh, kw))
        assert got.dtype == torch.float32 and torch.equal(got.cpu().view(2, -1, K), want), (case, name)
        cb = clip.bfloat16()
        got = vm.tubelet_gather(cb.to(dev), idx.to(dev).int(), (kt, kh, kw))
        assert got.dtype == torch.bfloat16 and torch.equal(got.cpu().view(2, -1, K), vc.gather_restate(cb, idx, kt, kh, kw)), (case, name, "bf16")
        # fp32 -> bf16 rounds once, exactly as me_cast does
        mixed = vm.tubelet_gather(clip.to(dev), idx.to(dev), (kt, kh, kw), out_dtype=torch.bfloat16)
        assert torch.equal(mixed, ops.cast(vm.tubelet_gather(clip.to(dev), idx.to(dev), (kt, kh, kw)), torch.bfloat16)), (case, name, "fp32 -> bf16")
    # the padded form the encoder feeds to the GEMM: zero rows and columns behind the data
    idx = lists["repeated"]
    got = vm.tubelet_gather(clip.to(dev), idx.to(dev), (kt, kh, kw), pad_cols_to=8, pad_rows_to=8).cpu()
    assert got.shape[0] == 16 and torch.equal(got[:10, :K].view(2, 5, K), vc.gather_restate(clip, idx, kt, kh, kw)) and not bool(got[10:].any())


@pytest.mark.parametrize("geom", [(1, 8, 8), (1, 6, 6), (3, 4, 12), (2, 8, 3)])
def test_tubelet_gather_other_geometries(dev, geom):
    """kt = 1 (an image-like clip), line lengths that are no multiple of four (the element-wise form) and a clip larger than the grid"""
    kt, kh, kw = geom
    rng = np.random.default_rng(11)
    clip = torch.from_numpy(rng.standard_normal((3, 2, 6, 26, 28)).astype(np.float32))
    N = (6 // kt) * (26 // kh) * (28 // kw)
    idx = torch.from_numpy(np.stack([rng.permutation(N)[:min(N, 7)] for _ in range(3)]))
    want = vc.gather_restate(clip, idx, kt, kh, kw)
    got = vm.tubelet_gather(clip.to(dev), idx.to(dev), geom)
    assert torch.equal(got.cpu().view(want.shape), want)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", list(vc.CASES))
def test_tubelet_gather_contract_guards_and_padded_stride(dev, case, cdt):
    lib = _capi.load()
    r = inputs(case)
    kt, kh, kw = vc.tubelet(case)
    clip = r["clip"].to(cdt)
    B, Cin, T, H, W = clip.shape
    idx = r["lists"][0]
    want = vc.gather_restate(clip, idx, kt, kh, kw)
    K, n = want.shape[2], idx.shape[1]
    code = _capi.dtype_code(cdt)
    clip_g = Guarded.input(clip.reshape(1, -1).to(dev))
    idx_d = idx.to(dev).int().contiguous()
    for ld in (K + 4, K + 5):                                  # a padded stride the four-wide form takes, and one it cannot
        out_g = Guarded.output(B * n, K, ld, cdt, dev)
        _capi.check(lib.me_tubelet_gather(clip_g.ptr(), code, idx_d.data_ptr(), out_g.ptr(), code, ld, B, Cin, T, H, W, kt, kh, kw, n,
                                          _capi.stream_ptr()), "me_tubelet_gather")
        out_g.check(f"{case} gather ld={ld}")
        assert out_g.untouched_interior() == 0 and torch.equal(out_g.t.cpu().view(B, n, K), want)


# ---------------------------------------------------------------------------------------------------------------- 2. rows and assembly

@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
def test_take_rows(dev, cdt):
    rng = np.random.default_rng(3)
    table = torch.from_numpy(rng.standard_normal((27, 40)).astype(np.float32))
    add = torch.from_numpy(rng.standard_normal(40).astype(np.float32))
    idx = torch.from_numpy(np.stack([rng.permutation(27)[:6], rng.permutation(27)[:6]]))
    t = table.to(cdt)
    got = vm.take_rows(t.to(dev), idx.to(dev))
    assert got.dtype == cdt and torch.equal(got.cpu(), t[idx])                      # a copy: bit-exact in either dtype
    got = vm.take_rows(table.to(dev), idx.to(dev), add=add.to(dev), out_dtype=cdt)
    want = table[idx] + add
    if cdt == torch.float32:
        assert torch.equal(got.cpu(), want)
    else:
        one_bf16_rounding(got, (table.double()[idx] + add.double()), "take_rows + add")
    # guards and padded strides through the C ABI
    lib = _capi.load()
    code = _capi.dtype_code(cdt)
    tab_g = Guarded.input(t.to(dev), ld=43)
    out_g = Guarded.output(12, 40, 45, cdt, dev)
    idx_d = idx.to(dev).int().contiguous()
    _capi.check(lib.me_take_rows(tab_g.ptr(), code, 43, 27, idx_d.data_ptr(), None, out_g.ptr(), code, 45, 2, 6, 40, _capi.stream_ptr()), "me_take_rows")
    out_g.check("take_rows")
    assert out_g.untouched_interior() == 0 and torch.equal(out_g.t.cpu().view(2, 6, 40), t[idx])
    assert vm.take_rows(table.to(dev), idx[:, :0].to(dev)).shape == (2, 0, 40)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case,dm", [("p16", False), ("p8", True)])
def test_assemble_forward(dev, case, dm, cdt):
    r = inputs(case)
    vis_idx, dec_idx, _ = r["lists_dm"] if dm else r["lists"]
    Cd, N = 40, vc.n_tokens(case)
    rng = np.random.default_rng(4)
    xv = torch.from_numpy(rng.standard_normal((2, vis_idx.shape[1], Cd)).astype(np.float32)).to(cdt)
    pos, tok = vc.sinusoid_table(N, Cd), torch.from_numpy(rng.standard_normal(Cd).astype(np.float32))
    got = vm.mae_assemble(xv.to(dev), pos.to(dev), vis_idx.to(dev), dec_idx.to(dev), tok.to(dev))
    assert got.dtype == cdt and got.shape == (2, vis_idx.shape[1] + dec_idx.shape[1], Cd)
    if cdt == torch.float32:
        assert torch.equal(got.cpu(), vc.assemble_restate(xv, pos, vis_idx, dec_idx, tok))            # torch indexing, bit-exact
    else:
        one_bf16_rounding(got, vc.assemble_restate(xv.double(), pos.double(), vis_idx, dec_idx, tok.double()), "assemble bf16")
    # the C ABI between guards, padded strides
    lib = _capi.load()
    code = _capi.dtype_code(cdt)
    B, Nvis, Ndec = 2, vis_idx.shape[1], dec_idx.shape[1]
    xv_g, pos_g, tok_g = Guarded.input(xv.reshape(B * Nvis, Cd).to(dev), ld=Cd + 3), Guarded.input(pos.to(dev), ld=Cd + 4), Guarded.input(tok.to(dev))
    out_g = Guarded.output(B * (Nvis + Ndec), Cd, Cd + 5, cdt, dev)
    vi, di = vis_idx.to(dev).int().contiguous(), dec_idx.to(dev).int().contiguous()
    _capi.check(lib.me_mae_assemble_fwd(xv_g.ptr(), code, Cd + 3, pos_g.ptr(), Cd + 4, N, vi.data_ptr(), di.data_ptr(), tok_g.ptr(), out_g.ptr(), code,
                                        Cd + 5, B, Nvis, Ndec, Cd, _capi.stream_ptr()), "me_mae_assemble_fwd")
    out_g.check(f"{case} assemble")
    assert out_g.untouched_interior() == 0 and torch.equal(out_g.t.reshape(B, Nvis + Ndec, Cd), got)


@pytest.mark.parametrize("cdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Nvis,Ndec,Cd", [(2, 2, 6, 40), (3, 6, 21, 32), (5, 16, 150, 264)])
def test_assemble_backward(dev, B, Nvis, Ndec, Cd, cdt):
    """dxv is a copy, dmask_token a fixed-order sum: against float64, twice bit-identical, between guards ((5, 16, 150): 750 mask rows
    make 256 runs of two or three rows, 264 columns a second column block)"""
    lib = _capi.load()
    rng = np.random.default_rng(B)
    dx = torch.from_numpy(rng.standard_normal((B, Nvis + Ndec, Cd)).astype(np.float32)).to(cdt)
    want = dx[:, Nvis:].double().sum(dim=(0, 1))
    dxv, dmask = vm.mae_assemble_bwd(dx.to(dev), Nvis)
    dxv2, dmask2 = vm.mae_assemble_bwd(dx.to(dev), Nvis)
    assert dxv.dtype == cdt and torch.equal(dxv.cpu(), dx[:, :Nvis]) and dmask.dtype == torch.float32
    assert torch.equal(dmask, dmask2) and torch.equal(dxv, dxv2)
    check_close(dmask, want, TOL_F32, "dmask_token")
    code = _capi.dtype_code(cdt)
    Nf = Nvis + Ndec
    dx_g = Guarded.input(dx.reshape(B * Nf, Cd).to(dev), ld=Cd + 3)
    dxv_g, dm_g = Guarded.output(B * Nvis, Cd, Cd + 5, cdt, dev), Guarded.output_vec(Cd, torch.float32, dev)
    nbytes = lib.me_mae_assemble_bwd_workspace(B, Ndec, Cd)
    ws_g = Guarded.output_bytes(nbytes, dev)
    _capi.check(lib.me_mae_assemble_bwd(dx_g.ptr(), code, Cd + 3, dxv_g.ptr(), code, Cd + 5, dm_g.ptr(), B, Nvis, Ndec, Cd, ws_g.ptr(), nbytes,
                                        _capi.stream_ptr()), "me_mae_assemble_bwd")
    for g, what in ((dxv_g, "dxv"), (dm_g, "dmask_token"), (ws_g, "workspace")):
        g.check(what)
    assert dxv_g.untouched_interior() == 0 and dm_g.untouched_interior() == 0
    assert torch.equal(dm_g.vec(), dmask) and torch.equal(dxv_g.t.reshape(B, Nvis, Cd), dxv)


def test_assemble_with_nothing_decoded_or_nothing_visible(dev):
    Cd = 32
    pos, tok = vc.sinusoid_table(8, Cd).to(dev), torch.ones(Cd, device=dev)
    xv = torch.randn(2, 3, Cd, device=dev)
    vis, none = torch.tensor([[0, 2, 5], [7, 1, 3]], device=dev), torch.zeros(2, 0, dtype=torch.int64, device=dev)
    out = vm.mae_assemble(xv, pos, vis, none, tok)                                   # Ndec = 0
    assert out.shape == (2, 3, Cd) and torch.equal(out, xv + pos[vis])
    dxv, dmask = vm.mae_assemble_bwd(out, 3)
    assert torch.equal(dxv, out) and dmask.shape == (Cd,) and not bool(dmask.any())
    out = vm.mae_assemble(xv[:, :0], pos, none, vis, tok)                            # Nvis = 0
    assert out.shape == (2, 3, Cd) and torch.equal(out, (tok + pos[vis]))
    dxv, dmask = vm.mae_assemble_bwd(out, 0)
    assert dxv.shape == (2, 0, Cd)
    check_close(dmask, out.double().sum(dim=(0, 1)), TOL_F32, "dmask_token, nothing visible")
    assert vm.tubelet_gather(torch.zeros(2, 3, 4, 32, 32, device=dev), none, (2, 16, 16)).shape == (0, 1536)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 3. loss

def loss_reference(case, dm, normalize, pred, w=None, clip=None):
    r = inputs(case)
    _, dec_idx, w0 = r["lists_dm"] if dm else r["lists"]
    kt, kh, kw = vc.tubelet(case)
    if clip is None:
        all_labels = r["labels"] if normalize else r["labels_raw"]
    else:
        all_labels = vc.labels_restate(clip, kt, kh, kw, normalize)
    labels = vc.take(all_labels, dec_idx)
    w = w0 if w is None else w
    loss, tok, dpred = vc.loss_restate(pred, labels, w, g=0.75)
    return dec_idx, w, labels, loss, tok, dpred


def make_pred(case, dm, normalize, seed=0):
    """a prediction near the labels (an error of the labels' own size), so that the loss is no rounding artefact"""
    r = inputs(case)
    dec_idx = (r["lists_dm"] if dm else r["lists"])[1]
    labels = vc.take(r["labels"] if normalize else r["labels_raw"], dec_idx)
    rng = np.random.default_rng(seed)
    return (labels + 0.5 * torch.from_numpy(rng.standard_normal(tuple(labels.shape)))).float()


@pytest.mark.parametrize("pdt,tol", [(torch.float32, TOL_F32), (torch.bfloat16, TOL_BF16_OP)])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case,dm", [("p16", False), ("p16", True), ("p8", False), ("p8", True)])
def test_mae_loss_terms(dev, case, dm, normalize, pdt, tol):
    pred = make_pred(case, dm, normalize).to(pdt)
    dec_idx, w, labels, loss, tok, dpred = loss_reference(case, dm, normalize, pred)
    if dm:
        assert float(w.min()) == 0.0                                             # weights containing zeros
    g = torch.tensor(0.75, device=dev)
    res = vm.mae_loss_terms(pred.to(dev), inputs(case)["clip"].to(dev), dec_idx.to(dev), w.to(dev), vc.tubelet(case), normalize,
                            grad_scale=g, want_labels=True, want_dpred=True)
    res2 = vm.mae_loss_terms(pred.to(dev), inputs(case)["clip"].to(dev), dec_idx.to(dev), w.to(dev), vc.tubelet(case), normalize,
                             grad_scale=g, want_labels=True, want_dpred=True)
    for k in ("labels", "tok_loss", "loss", "dpred", "wsum"):
        assert torch.equal(res[k], res2[k]), f"{k}: two runs differ"
    print(f"{case} dm={dm} normalize={normalize} {pdt}: loss {float(res['loss']):.6f} (float64 {float(loss):.6f})")
    assert res["labels"].dtype == torch.float32 and res["dpred"].dtype == pdt and float(res["wsum"]) == float(w.sum())
    check_close(res["labels"], labels, TOL_F32, "labels")                         # fp32 statistics whatever pred's dtype
    check_close(res["tok_loss"], tok, tol, "per-token loss")
    check_close(res["loss"].reshape(1), loss.reshape(1), tol, "loss")
    check_close(res["dpred"], dpred, tol, "dpred")


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16])
def test_mae_loss_without_any_weight_is_zero_and_finite(dev, pdt):
    case = "p8"
    pred = make_pred(case, False, True).to(pdt)
    dec_idx, _, labels, _, tok, _ = loss_reference(case, False, True, pred)
    w = torch.zeros(dec_idx.shape, dtype=torch.float64)
    res = vm.mae_loss_terms(pred.to(dev), inputs(case)["clip"].to(dev), dec_idx.to(dev), w.to(dev), vc.tubelet(case), True, want_dpred=True)
    assert float(res["loss"]) == 0.0 and float(res["wsum"]) == 0.0 and not bool(res["dpred"].any()) and bool(torch.isfinite(res["dpred"]).all())
    check_close(res["tok_loss"], tok, TOL_F32 if pdt == torch.float32 else TOL_BF16_OP, "per-token loss, no weight")
    # through autograd: a zero gradient, never NaN
    mask = torch.from_numpy(inputs(case)["mask"]).to(dev)
    p = torch.randn(2, int((~mask[0]).sum()), pred.shape[2], device=dev).to(pdt).requires_grad_(True)
    loss = M.mae_reconstruction_loss(p, inputs(case)["clip"].to(dev), mask, decode_mask=mask, patch_size=8)       # decoded = ~mask: all visible
    assert float(loss.detach()) == 0.0 and loss.dtype == torch.float32
    loss.backward()
    assert p.grad.dtype == pdt and not bool(p.grad.any())


def test_mae_loss_low_contrast_patch(dev):
    """the patch that tells eps on the standard deviation from eps on the variance and from no eps (tests/test_video_mae_cpu.py)"""
    case = "p8"
    kt, kh, kw = vc.tubelet(case)
    clip = torch.from_numpy(vc.low_contrast_clip(case))
    dec_idx = torch.tensor([[1, 0, 5], [1, 2, 3]])
    labels = vc.take(vc.labels_restate(clip, kt, kh, kw), dec_idx)
    pred = torch.zeros(tuple(labels.shape))
    res = vm.mae_loss_terms(pred.to(dev), clip.to(dev), dec_idx.to(dev), torch.ones(2, 3, device=dev), (kt, kh, kw), True, want_labels=True)
    got, want = res["labels"][0, 0], labels[0, 0]
    err = float((got.double().cpu() - want).abs().max() / want.abs().max())
    wrong = vc.take(vc.labels_restate(clip, kt, kh, kw, eps_mode="none"), dec_idx)[0, 0]
    print(f"low-contrast patch: kernel {err:.2e} from float64; no eps would be {float((wrong - want).abs().max() / want.abs().max()):.2e}")
    check_close(got, want, TOL_F32, "labels of the low-contrast patch")
    check_close(res["labels"], labels, TOL_F32, "labels")
    check_close(res["tok_loss"], (labels ** 2).mean(dim=-1), TOL_F32, "per-token loss")


@pytest.mark.parametrize("pdt", [torch.float32, torch.bfloat16])
def test_mae_loss_contract_guards_and_padded_strides(dev, pdt):
    lib = _capi.load()
    case = "p8"
    pred = make_pred(case, True, True).to(pdt)
    dec_idx, w, labels, loss, tok, dpred = loss_reference(case, True, True, pred)
    B, Ndec, cols = pred.shape
    clip = inputs(case)["clip"]
    _, Cin, T, H, W = clip.shape
    kt, kh, kw = vc.tubelet(case)
    code = _capi.dtype_code(pdt)
    clip_g = Guarded.input(clip.reshape(1, -1).to(dev))
    pred_g = Guarded.input(pred.reshape(B * Ndec, cols).to(dev), ld=cols + 3)
    w_g, mean_g, std_g = Guarded.input(w.float().reshape(-1).to(dev)), Guarded.input(torch.tensor(vc.MEAN, device=dev)), Guarded.input(torch.tensor(vc.STD, device=dev))
    g_g = Guarded.input(torch.tensor([0.75], device=dev))
    tok_g, sc_g = Guarded.output_vec(B * Ndec, torch.float32, dev), Guarded.output_vec(2, torch.float32, dev)
    lab_g, dp_g = Guarded.output(B * Ndec, cols, cols + 5, torch.float32, dev), Guarded.output(B * Ndec, cols, cols + 7, pdt, dev)
    idx = dec_idx.to(dev).int().contiguous()
    _capi.check(lib.me_mae_loss(clip_g.ptr(), _capi.ME_F32, B, Cin, T, H, W, kt, kh, kw, mean_g.ptr(), std_g.ptr(), idx.data_ptr(), w_g.ptr(), Ndec,
                                pred_g.ptr(), code, cols + 3, 1, g_g.ptr(), tok_g.ptr(), sc_g.ptr(), lab_g.ptr(), cols + 5, dp_g.ptr(), cols + 7,
                                _capi.stream_ptr()), "me_mae_loss")
    tol = TOL_F32 if pdt == torch.float32 else TOL_BF16_OP
    for g, want, what, t in ((tok_g, tok.reshape(1, -1), "tok_loss", tol), (lab_g, labels.reshape(B * Ndec, cols), "labels", TOL_F32),
                             (dp_g, dpred.reshape(B * Ndec, cols), "dpred", tol), (sc_g, torch.stack([loss, w.sum()]).reshape(1, 2), "scalars", tol)):
        g.check(what)
        assert g.untouched_interior() == 0, what
        check_close(g.t, want, t, what)


# ---------------------------------------------------------------------------------------------------------------- 4. model parity

def make_model(gold, variant, dev):
    case, _, init_values = vc.VARIANTS[variant]
    m = M.PretrainVisionTransformer(norm_layer=partial(nn.LayerNorm, eps=vc.MODEL["eps"]), **vc.model_kwargs(case, init_values))
    ref_sd = vc.fixture_state_dict(gold, variant)
    m.load_state_dict(M.convert_video_state_dict(ref_sd), strict=True)
    return m.to(dev), ref_sd


_runs = {}


def run_model(gold, dev, variant, mode):
    """one forward + loss + backward per (variant, mode), shared by the tests below and left unchanged"""
    if (variant, mode) not in _runs:
        case, with_dm, _ = vc.VARIANTS[variant]
        m, ref_sd = make_model(gold, variant, dev)
        M.set_fp32_mode(m, "exact")
        assert set(M.to_video_state_dict(m.state_dict())) == set(ref_sd)
        clip = torch.from_numpy(gold[f"{case}/clip"]).to(dev)
        mask = torch.from_numpy(gold[f"{case}/mask"]).to(dev)
        dmask = torch.from_numpy(gold[f"{case}/decode_mask"]).to(dev) if with_dm else None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
            y = m(clip, mask, dmask)
            enc = m.encoder.forward_features(clip, mask)
        loss = M.mae_reconstruction_loss(y, clip, mask, dmask, patch_size=vc.CASES[case]["patch"])
        loss.backward()
        grads = M.to_video_state_dict({k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None})
        _runs[(variant, mode)] = dict(y=y.detach().cpu(), enc=enc.detach().cpu(), loss=loss.detach().cpu(), grads=grads)
    return _runs[(variant, mode)]


MODES = [("fp32", TOL_F32, TOL_F32), ("bf16", TOL_BF16_FWD, TOL_BF16_GRAD)]


@pytest.mark.parametrize("mode,tol_fwd,tol_grad", MODES)
@pytest.mark.parametrize("variant", list(vc.VARIANTS))
def test_model_forward_against_the_reference(gold, dev, variant, mode, tol_fwd, tol_grad):
    """The model output against the reference's float64 output, by check_close at TOL_F32 (exact fp32) / TOL_BF16_FWD (bf16 autocast).
    Measured on MI355X, max-abs error / max|ref|: fp32 2.1e-7 .. 3.1e-7; bf16 autocast 2.98e-3 (p16), 2.76e-3 (p16_dm), 2.62e-3 (p8),
    2.53e-3 (p8_dm), 3.3e-4 (p8_ls_dm), no element outside the per-element part.  (With the Linears behind the final norms in bf16 as
    well it was 3.30e-3 / 3.39e-3 / 3.25e-3 / 3.14e-3 / 1.82e-3 with 3, 2 and 1 near-zero outputs of the first three cases outside the
    per-element part; the reference's own model under torch's bf16 autocast: 5.14e-3 / 4.87e-3 / 4.63e-3 / 4.40e-3 / 3.57e-3.)"""
    r = run_model(gold, dev, variant, mode)
    want = torch.from_numpy(gold[f"{variant}/out"])
    print(f"{variant} {mode}: out {float((r['y'].double() - want).abs().max() / want.abs().max()):.2e}, loss {float(r['loss']):.6f} "
          f"(reference {float(gold[f'{variant}/loss']):.6f})")
    assert r["y"].dtype == torch.float32 and r["loss"].dtype == torch.float32
    check_close(r["y"], want, tol_fwd, f"{variant} {mode} forward")


@pytest.mark.parametrize("mode,tol_fwd,tol_grad", MODES)
@pytest.mark.parametrize("variant", list(vc.VARIANTS))
def test_encoder_features_and_loss_against_the_reference(gold, dev, variant, mode, tol_fwd, tol_grad):
    r = run_model(gold, dev, variant, mode)
    check_close(r["enc"], torch.from_numpy(gold[f"{variant}/enc"]), tol_fwd, f"{variant} {mode} encoder.forward_features")
    check_close(r["loss"].reshape(1), torch.from_numpy(gold[f"{variant}/loss"]).reshape(1), tol_fwd, f"{variant} {mode} loss")


@pytest.mark.parametrize("mode,tol_fwd,tol_grad", MODES)
@pytest.mark.parametrize("variant", list(vc.VARIANTS))
def test_model_gradients_against_the_reference(gold, dev, variant, mode, tol_fwd, tol_grad):
    r = run_model(gold, dev, variant, mode)
    for k in vc.grad_keys(variant):
        want = torch.from_numpy(gold[f"{variant}/grad/{k}"])
        print(f"{variant} {mode} d {k}: {float((r['grads'][k].double() - want).abs().max() / want.abs().max()):.2e}")
        check_close(r["grads"][k], want, tol_grad, f"{variant} {mode} d {k}")
    k = "encoder.patch_embed.proj.weight"
    if f"{variant}/grad_rows/{k}" in gold.files:                      # the variants whose fixture holds two filters of it only
        check_close(r["grads"][k][list(vc.PROJ_GRAD_ROWS)], torch.from_numpy(gold[f"{variant}/grad_rows/{k}"]), tol_grad, f"{variant} {mode} d {k} rows")


@pytest.mark.parametrize("variant", ["p16_dm", "p8", "p8_ls_dm"])
def test_model_with_bf16_parameters(gold, dev, variant):
    """`model.bfloat16()`: parameters, position tables and the token stream between the Blocks are bf16, and every Linear -- the two
    behind the final norms included -- computes in bf16.  Bound: conftest's TOL_BF16_STREAM12, its bound for a bf16 residual stream
    through a whole block stack; this model has three blocks, and the parameters' own rounding (2^-9 relative) is far inside it."""
    from conftest import TOL_BF16_STREAM12
    case, with_dm, _ = vc.VARIANTS[variant]
    m, _ = make_model(gold, variant, dev)
    m = m.bfloat16()
    assert m.pos_embed.dtype == torch.bfloat16 and m.encoder.patch_embed.proj.weight.dtype == torch.bfloat16
    clip = torch.from_numpy(gold[f"{case}/clip"]).to(dev)
    mask = torch.from_numpy(gold[f"{case}/mask"]).to(dev)
    dmask = torch.from_numpy(gold[f"{case}/decode_mask"]).to(dev) if with_dm else None
    y = m(clip, mask, dmask)
    enc = m.encoder.forward_features(clip, mask)
    loss = M.mae_reconstruction_loss(y, clip, mask, dmask, patch_size=vc.CASES[case]["patch"])
    loss.backward()
    want = torch.from_numpy(gold[f"{variant}/out"])
    print(f"{variant} bf16 parameters: out {float((y.detach().double().cpu() - want).abs().max() / want.abs().max()):.2e}, "
          f"loss {float(loss.detach()):.6f} (reference {float(gold[f'{variant}/loss']):.6f})")
    assert y.dtype == torch.float32 and enc.dtype == torch.bfloat16 and loss.dtype == torch.float32
    check_close(y, want, TOL_BF16_STREAM12, f"{variant} bf16 parameters forward")
    check_close(enc, torch.from_numpy(gold[f"{variant}/enc"]), TOL_BF16_STREAM12, f"{variant} bf16 parameters encoder")
    check_close(loss.reshape(1), torch.from_numpy(gold[f"{variant}/loss"]).reshape(1), TOL_BF16_STREAM12, f"{variant} bf16 parameters loss")
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.bfloat16 and bool(torch.isfinite(p.grad).all()), k


# ---------------------------------------------------------------------------------------------------------------- 5. the full-embed route

@pytest.mark.parametrize("case", list(vc.CASES))
def test_visible_tokens_equal_the_full_embed_route(gold, dev, case):
    """VideoPatchEmbed of every tubelet + the sinusoid rows + x[~mask] (what a user composes today) against gather + GEMM"""
    m, _ = make_model(gold, case, dev)
    r = inputs(case)
    clip, mask = r["clip"].to(dev), torch.from_numpy(r["mask"]).to(dev)
    enc = m.encoder
    with torch.no_grad():
        full = enc.patch_embed(clip) + enc.pos_embed
        want = full[~mask].reshape(2, -1, full.shape[-1])
        (vis_idx,) = vm.token_indices("test", ~mask)
        got = vm._VisibleEmbedFn.apply(clip, vis_idx, enc.patch_embed.proj.weight, enc.patch_embed.proj.bias, enc.pos_embed, vc.tubelet(case),
                                       torch.float32, torch.float32)
    assert torch.equal(vis_idx.cpu().long(), r["lists"][0])
    check_close(got, want, TOL_F32, f"{case} visible tokens")


# ---------------------------------------------------------------------------------------------------------------- 6. error paths (host only)

def test_error_paths(gold, dev):
    E = M.MetaEncError
    m, _ = make_model(gold, "p16", dev)
    clip = torch.from_numpy(gold["p16/clip"]).to(dev)
    mask = torch.from_numpy(gold["p16/mask"]).to(dev)
    uneven = mask.clone()
    uneven[0] = False
    uneven[0, :5] = True                                                 # 5 masked in sample 0, 6 in sample 1
    with pytest.raises(E, match="different numbers"):
        m(clip, uneven)
    with pytest.raises(E, match="must be"):
        m(clip, mask[:, :7])
    with pytest.raises(E, match="bool"):
        m(clip, mask.int())
    with pytest.raises(E, match="no CPU fallback"):
        m(clip.cpu(), mask)
    with pytest.raises(E, match="no CPU fallback"):
        m(clip, mask.cpu())
    with pytest.raises(E, match="gradient w.r.t. the clip"):
        m(clip.clone().requires_grad_(True), mask)
    with pytest.raises(E, match="does not match the model"):
        m(clip[:, :, :, :16], mask)
    with pytest.raises(E, match="cos_attn"):
        M.PretrainVisionTransformer(cos_attn=True, **vc.model_kwargs("p16"))
    with pytest.raises(E, match="pred"):
        M.mae_reconstruction_loss(torch.zeros(2, 6, 100, device=dev), clip, mask)
    with pytest.raises(E, match="no visible token"):
        m(clip, torch.ones_like(mask))
