"""GPU: me_fbank / KaldiFbank against the float64 restatement of tests/fbank_cases.py, its contract (guards, padded strides, NaN behind
every clip, determinism, error codes), and ASTModel forward + gradients against a float64 restatement of ast_models.py:146-167.

Parity bound: for every clip e_ref = max |restatement in fp32 - restatement in fp64| is formed on the CPU and the device result must
lie within 4 e_ref of the fp64 one over all cells (the device FFT and filter sums are another fp32 evaluation of the same formula:
another summation order, FMA).  Measured figures: profiles/fbank_parity.txt (tools/fbank_bench.py writes it).  Inputs are 0.1 Gaussian
noise + 0.3 sin(440 Hz) + 0.05 sin(3 kHz): the noise floor keeps every non-empty filter off cancellation."""
import ctypes
import math
from functools import partial

import pytest
import torch

import fbank_cases as fc
import metatransformer_amd as M
from conftest import TOL_BF16_FWD, TOL_BF16_GRAD, TOL_F32, check_close
from guarded import Guarded
from metatransformer_amd import _capi, audio
from oracle import block_oracle as bo

pytestmark = pytest.mark.gpu

RUN = audio.FRAMES_PER_WORKGROUP
LOG_EPS = math.log(fc.EPS)
CONFIGS = {"16k_128": (16000, 128), "16k_224": (16000, 224), "8k_64": (8000, 64)}


def clip_lengths(sr):
    """no frame, one frame (twice), two frames; one frame fewer than / exactly / one more than a workgroup's run; three runs plus one;
    one second"""
    win, shift, _ = fc.geometry(sr)
    at = lambda frames: win + (frames - 1) * shift          # noqa: E731
    return [win - 1, win, win + shift - 1, win + shift, at(RUN - 1), at(RUN), at(RUN + 1), at(3 * RUN + 1), sr]


def batch_of(sr, lengths, seed):
    """[B, longest] fp32, clip b = make_wave(lengths[b]) followed by NaN: what lies behind a clip's length must never be read"""
    wave = torch.full((len(lengths), max(lengths)), float("nan"))
    for b, n in enumerate(lengths):
        wave[b, :n] = fc.make_wave(n, sr, seed + b)
    return wave


def ulps(a: torch.Tensor, b: torch.Tensor) -> int:
    """largest distance in fp32 units in the last place between two fp32 tensors of one sign pattern"""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max()) if a.numel() else 0


@pytest.fixture(scope="module")
def parity(dev):
    """per configuration: the batch of unequal lengths, its fp64 and fp32 restatements per clip, the device result (one call)"""
    out = {}
    for i, (name, (sr, n_mel)) in enumerate(CONFIGS.items()):
        lengths = clip_lengths(sr)
        wave = batch_of(sr, lengths, 100 * i)
        ref64 = [fc.fbank(wave[b, :n], sr, n_mel, dtype=torch.float64) for b, n in enumerate(lengths)]
        ref32 = [fc.fbank(wave[b, :n], sr, n_mel, dtype=torch.float32) for b, n in enumerate(lengths)]
        mod = M.KaldiFbank(sr, n_mel).to(dev)
        got = mod(wave.to(dev), torch.tensor(lengths, dtype=torch.int32, device=dev))
        out[name] = dict(sr=sr, n_mel=n_mel, lengths=lengths, wave=wave, ref64=ref64, ref32=ref32, mod=mod, got=got.cpu(), got_dev=got)
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_parity_with_the_float64_restatement(parity, name):
    p = parity[name]
    sr, n_mel, got = p["sr"], p["n_mel"], p["got"]
    longest = max(fc.num_frames(n, sr) for n in p["lengths"])
    assert got.shape == (len(p["lengths"]), longest, n_mel) and got.dtype == torch.float32
    assert not bool(torch.isnan(got).any())
    empty = fc.empty_filters(sr, n_mel)
    for b, n in enumerate(p["lengths"]):
        T = fc.num_frames(n, sr)
        r64, r32 = p["ref64"][b], p["ref32"][b]
        assert r64.shape == (T, n_mel)
        assert bool((got[b, T:] == 0).all()), f"{name} len {n}: rows past the {T} frames must hold 0"
        if T == 0:
            continue
        e_ref = float((r32.double() - r64).abs().max())
        err = float((got[b, :T].double() - r64).abs().max())
        print(f"{name} len {n:6d} frames {T:3d}: device error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
        assert err <= 4 * e_ref, f"{name} len {n}: device error {err:.3e} exceeds 4 x e_ref = {4 * e_ref:.3e}"
        if bool(empty.any()):
            cols = got[b, :T][:, empty]
            assert ulps(cols, torch.full_like(cols, LOG_EPS)) <= 2, f"{name} len {n}: empty filters must give log(eps)"


def test_silent_and_constant_clips_give_log_eps(dev):
    wave = torch.stack([torch.zeros(6000), torch.full((6000,), 0.37), torch.full((6000,), -1e-3)])
    for sr, n_mel in ((16000, 128), (8000, 64)):
        got = M.KaldiFbank(sr, n_mel).to(dev)(wave.to(dev)).cpu()
        assert got.shape == (3, fc.num_frames(6000, sr), n_mel)
        assert ulps(got, torch.full_like(got, LOG_EPS)) <= 2


@pytest.mark.parametrize("name", ["16k_128", "8k_64"])
def test_target_length_cuts_and_pads(parity, dev, name):
    """rows T .. target_length - 1 hold 0, frames from target_length on are dropped; what remains is the same arithmetic"""
    p = parity[name]
    lengths = torch.tensor(p["lengths"], dtype=torch.int32, device=dev)
    full = p["got"]
    for L in (RUN + 8, full.shape[1] + 30):
        got = M.KaldiFbank(p["sr"], p["n_mel"], target_length=L).to(dev)(p["wave"].to(dev), lengths).cpu()
        assert got.shape == (len(p["lengths"]), L, p["n_mel"])
        keep = min(L, full.shape[1])
        assert torch.equal(got[:, :keep], full[:, :keep])
        assert bool((got[:, keep:] == 0).all())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16_output_is_the_rounded_fp32_output(parity, dev, name):
    p = parity[name]
    lengths = torch.tensor(p["lengths"], dtype=torch.int32, device=dev)
    got = M.KaldiFbank(p["sr"], p["n_mel"], out_dtype=torch.bfloat16).to(dev)(p["wave"].to(dev), lengths)
    assert got.dtype == torch.bfloat16
    assert torch.equal(got.view(torch.int16), p["got_dev"].to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("name", ["16k_128", "8k_64"])
def test_normalisation_and_masks(parity, dev, name):
    p = parity[name]
    sr, n_mel, B = p["sr"], p["n_mel"], len(p["lengths"])
    mean, std = -6.845978, 5.5654526
    L = p["got"].shape[1] + 5
    wave, lengths = p["wave"].to(dev), torch.tensor(p["lengths"], dtype=torch.int32, device=dev)
    mod = M.KaldiFbank(sr, n_mel, target_length=L, norm_mean=mean, norm_std=std).to(dev)
    plain = mod(wave, lengths).cpu()
    # the cell value of raw 0 and the normalisation of the raw result, both evaluated in fp32
    m32, s32 = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    zero_cell = (torch.tensor(0.0) - m32) / (2 * s32)
    raw = torch.zeros(B, L, n_mel)
    raw[:, :p["got"].shape[1]] = p["got"]
    assert ulps(plain, (raw - m32) / (2 * s32)) <= 1
    for b, n in enumerate(p["lengths"]):
        T = fc.num_frames(n, sr)
        assert ulps(plain[b, T:], zero_cell.expand(L - T, n_mel)) <= 1
    # bands per clip: ordinary ones, ones that reach the edges, empty ones [k, k)
    fm = torch.tensor([[3, 9], [0, n_mel], [n_mel - 1, n_mel], [5, 5], [0, 0], [n_mel, n_mel], [10, 11], [0, 1], [7, 30]], dtype=torch.int32)
    tm = torch.tensor([[0, 1], [2, 2], [1, 40], [0, 0], [L, L], [30, 35], [L - 3, L], [31, 33], [0, L]], dtype=torch.int32)
    masked = mod(wave, lengths, freq_mask=fm.to(dev), time_mask=tm.to(dev)).cpu()
    hit = torch.zeros(B, L, n_mel, dtype=torch.bool)
    for b in range(B):
        hit[b, :, int(fm[b, 0]):int(fm[b, 1])] = True
        hit[b, int(tm[b, 0]):int(tm[b, 1])] = True
    assert ulps(masked[hit], zero_cell.expand(int(hit.sum()))) <= 1
    assert torch.equal(masked[~hit].view(torch.int32), plain[~hit].view(torch.int32)), "unmasked cells must not change"
    # empty bands alone change nothing
    k = torch.tensor([[4, 4]] * B, dtype=torch.int32, device=dev)
    assert torch.equal(mod(wave, lengths, freq_mask=k, time_mask=k).cpu().view(torch.int32), plain.view(torch.int32))
    # against the restatement with bands and statistics, same bound as the parity test
    for b in (1, 2, 6, 8):
        n = p["lengths"][b]
        args = dict(target_length=L, freq_band=tuple(fm[b].tolist()), time_band=tuple(tm[b].tolist()), norm=(mean, std))
        r64 = fc.fbank(p["wave"][b, :n], sr, n_mel, dtype=torch.float64, **args)
        r32 = fc.fbank(p["wave"][b, :n], sr, n_mel, dtype=torch.float32, **args)
        e_ref = float((r32.double() - r64).abs().max())
        assert float((masked[b].double() - r64).abs().max()) <= 4 * e_ref


@pytest.mark.parametrize("sr,n_mel", [(16000, 128), (8000, 64)])
def test_mixup(dev, sr, n_mel):
    """dataloader.py:105-127: both means removed over their own lengths, the partner zero-padded or cut, the mix's mean removed"""
    win, shift, _ = fc.geometry(sr)
    n1 = [win + 40 * shift + 7, win + 40 * shift + 7, win + 40 * shift + 7, win + 3 * shift, 9000]
    n2 = [win + 40 * shift + 7, win + 9 * shift, 2 * (win + 40 * shift), 9000, win - 5]           # equal, shorter, longer, longer, shorter
    lam = [0.5, 0.31, 0.77, 0.9, 0.05]
    w1, w2 = batch_of(sr, n1, 500), batch_of(sr, n2, 600)
    mod = M.KaldiFbank(sr, n_mel).to(dev)
    got = mod(w1.to(dev), torch.tensor(n1, dtype=torch.int32, device=dev),
              mix=(w2.to(dev), torch.tensor(n2, dtype=torch.int32, device=dev), torch.tensor(lam, device=dev))).cpu()
    assert not bool(torch.isnan(got).any())
    for b in range(len(n1)):
        r64 = fc.fbank(w1[b, :n1[b]], sr, n_mel, dtype=torch.float64, wave2=w2[b, :n2[b]], lam=lam[b])
        r32 = fc.fbank(w1[b, :n1[b]], sr, n_mel, dtype=torch.float32, wave2=w2[b, :n2[b]], lam=lam[b])
        T = r64.shape[0]
        e_ref = float((r32.double() - r64).abs().max())
        err = float((got[b, :T].double() - r64).abs().max())
        print(f"mix {sr} Hz, {n_mel} filters, lengths {n1[b]} / {n2[b]}, lam {lam[b]}: device error {err:.3e}, e_ref {e_ref:.3e}")
        assert err <= 4 * e_ref and bool((got[b, T:] == 0).all())
    # the mix with an all-zero weight on the partner is not the plain call (the mean of a mean-free wave is removed once more), but close
    plain = mod(w1.to(dev), torch.tensor(n1, dtype=torch.int32, device=dev)).cpu()
    one = mod(w1.to(dev), torch.tensor(n1, dtype=torch.int32, device=dev),
              mix=(w2.to(dev), torch.tensor(n2, dtype=torch.int32, device=dev), torch.ones(len(n1), device=dev))).cpu()
    assert float((one - plain).abs().max()) < 1e-2


def _desc(mod, wave_g, lengths, out_g, L, B, n, ld_wave, out_dtype):
    d = _capi.FbankDesc()
    d.wave, d.ld_wave, d.lengths, d.B, d.n_samples = wave_g.ptr(), ld_wave, lengths.data_ptr(), B, n
    d.win, d.shift, d.padded, d.n_mel, d.mel_ld, d.target_length = mod.win, mod.shift, mod.padded, mod.num_mel_bins, mod.mel_weight.shape[1], L
    d.window, d.twiddle, d.mel_range, d.mel_weight = mod.window.data_ptr(), mod.twiddle.data_ptr(), mod.mel_range.data_ptr(), mod.mel_weight.data_ptr()
    d.out, d.out_dtype, d.ld_out = out_g.ptr(), _capi.dtype_code(out_dtype), out_g.ld
    return d


@pytest.mark.parametrize("name,odt,pad", [("16k_128", torch.float32, 4), ("16k_224", torch.float32, 3), ("8k_64", torch.bfloat16, 4),
                                          ("8k_64", torch.bfloat16, 1)])
def test_contract_guards_padded_strides_and_determinism(parity, dev, name, odt, pad):
    """waves between NaN guards with NaN pad columns and NaN behind every clip's length; the output with a padded row stride (a
    multiple of 4: whole-row vector stores; not one: the element-wise form) between sentinel guards; the workspace of exactly the
    queried size between guards"""
    p = parity[name]
    lib = _capi.load()
    sr, n_mel, lengths = p["sr"], p["n_mel"], p["lengths"]
    B, n = p["wave"].shape
    L = p["got"].shape[1] + 3
    wave_g = Guarded.input(p["wave"].to(dev), ld=n + 5)
    len_t = torch.tensor(lengths, dtype=torch.int32, device=dev)
    outs = []
    for _ in range(2):
        out_g = Guarded.output(B * L, n_mel, n_mel + pad, odt, dev)
        d = _desc(p["mod"], wave_g, len_t, out_g, L, B, n, n + 5, odt)
        nbytes = lib.me_fbank_workspace_bytes(ctypes.byref(d))
        assert nbytes > 0
        ws_g = Guarded.output_bytes(nbytes, dev)
        _capi.check(lib.me_fbank(ctypes.byref(d), ws_g.ptr(), nbytes, _capi.stream_ptr()), "me_fbank")
        torch.cuda.synchronize()
        out_g.check(f"me_fbank out {name}")
        ws_g.check(f"me_fbank workspace {name}")
        assert out_g.untouched_interior() == 0
        assert not bool(torch.isnan(out_g.t.float()).any())
        outs.append(out_g.t.clone())
    assert torch.equal(outs[0].view(torch.int16 if odt == torch.bfloat16 else torch.int32),
                       outs[1].view(torch.int16 if odt == torch.bfloat16 else torch.int32)), "two runs must be bit-identical"
    want = torch.zeros(B, L, n_mel)
    want[:, :p["got"].shape[1]] = p["got"]
    assert torch.equal(outs[0].cpu().reshape(B, L, n_mel).float(), want.to(odt).float())
    # too small a workspace is an error, not a write
    out_g = Guarded.output(B * L, n_mel, n_mel + pad, odt, dev)
    d = _desc(p["mod"], wave_g, len_t, out_g, L, B, n, n + 5, odt)
    assert lib.me_fbank(ctypes.byref(d), ws_g.ptr(), nbytes - 4, _capi.stream_ptr()) == -4
    torch.cuda.synchronize()
    assert out_g.untouched_interior() == B * L * n_mel


def test_unsupported_geometry_is_an_error_code(parity, dev):
    p = parity["16k_128"]
    lib = _capi.load()
    B, n = p["wave"].shape
    wave_g = Guarded.input(torch.zeros(B, n, device=dev))
    len_t = torch.tensor(p["lengths"], dtype=torch.int32, device=dev)
    out_g = Guarded.output(B * 8, 128, 128, torch.float32, dev)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    for field, value in (("padded", 1024), ("padded", 128), ("n_mel", 257), ("win", 513), ("mel_ld", 100)):
        d = _desc(p["mod"], wave_g, len_t, out_g, 8, B, n, n, torch.float32)
        setattr(d, field, value)
        assert lib.me_fbank(ctypes.byref(d), ws.data_ptr(), ws.numel(), _capi.stream_ptr()) == -2, field
        assert b"unsupported geometry" in lib.me_last_error(), field
    torch.cuda.synchronize()
    assert out_g.untouched_interior() == B * 8 * 128
    with pytest.raises(M.MetaEncError, match="unsupported geometry"):
        M.KaldiFbank(32000, 64).to(dev)(torch.zeros(1, 4000, device=dev))
    with pytest.raises(M.MetaEncError, match="unsupported geometry"):
        M.KaldiFbank(16000, 300).to(dev)(torch.zeros(1, 4000, device=dev))


# ---------------------------------------------------------------------------------------------------------------- ASTModel

AST_F, AST_T, AST_B, AST_DIM, AST_HEADS, AST_LABELS = 64, 104, 2, 768, 12, 35


def _ast_state(seed=0):
    """seeded values for every key, LayerNorm affines and biases included, so that the comparison is sensitive to each"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: std * torch.randn(*s, generator=g)          # noqa: E731
    sd = {f"v.blocks.{k}": v for k, v in bo.make_encoder_state_dict(2, AST_DIM, seed=seed + 1).items()}
    sd.update({"v.cls_token": rn(1, 1, AST_DIM), "v.dist_token": rn(1, 1, AST_DIM), "v.pos_embed": rn(1, 32, AST_DIM, std=0.02),
               "v.patch_embed.proj.weight": rn(AST_DIM, 1, 32, 32, std=0.03), "v.patch_embed.proj.bias": rn(AST_DIM, std=0.05),
               "v.norm.weight": 1 + rn(AST_DIM, std=0.1), "v.norm.bias": rn(AST_DIM, std=0.05),
               "v.head.weight": rn(1000, AST_DIM, std=0.02), "v.head.bias": rn(1000, std=0.02),
               "mlp_head.0.weight": 1 + rn(AST_DIM, std=0.1), "mlp_head.0.bias": rn(AST_DIM, std=0.05),
               "mlp_head.1.weight": rn(AST_LABELS, AST_DIM, std=0.05), "mlp_head.1.bias": rn(AST_LABELS, std=0.05)})
    return sd


@pytest.fixture(scope="module")
def ast_reference():
    """ast_models.py:146-167 in float64: x [B, T, F] -> [B, 1, F, T] -> the 32 x 32 convolution at stride 10 -> + pos_embed -> Blocks
    (eps 1e-6) -> v.norm -> the mean of tokens 0 and 1 -> mlp_head; logits and the gradient of sum(logits * go) for every parameter"""
    sd = _ast_state()
    g = torch.Generator().manual_seed(42)
    x = torch.randn(AST_B, AST_T, AST_F, generator=g)
    go = torch.randn(AST_B, AST_LABELS, generator=g)
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    t = torch.nn.functional.conv2d(x.double().unsqueeze(1).transpose(2, 3), P["v.patch_embed.proj.weight"], P["v.patch_embed.proj.bias"], stride=(10, 10))
    t = t.flatten(2).transpose(1, 2) + P["v.pos_embed"]
    assert t.shape == (AST_B, 32, AST_DIM)
    for i in range(2):
        t = bo.block_forward(t, {k[len(f"v.blocks.{i}."):]: v for k, v in P.items() if k.startswith(f"v.blocks.{i}.")}, AST_HEADS, eps=1e-6)
    t = bo.layer_norm(t, P["v.norm.weight"], P["v.norm.bias"], 1e-6)
    t = (t[:, 0] + t[:, 1]) / 2
    y = bo.linear(bo.layer_norm(t, P["mlp_head.0.weight"], P["mlp_head.0.bias"], 1e-5), P["mlp_head.1.weight"], P["mlp_head.1.bias"])
    (y * go.double()).sum().backward()
    grads = {k: v.grad for k, v in P.items() if v.grad is not None}
    return dict(sd=sd, x=x, go=go, y=y.detach(), grads=grads)


def _ast_model(dev, sd, **kw):
    enc = M.build_encoder(depth=2, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))          # the timm factory's eps (ast_models.py:62)
    m = M.ASTModel(label_dim=AST_LABELS, input_fdim=AST_F, input_tdim=AST_T, verbose=False, encoder=enc, **kw).to(dev)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m


@pytest.mark.parametrize("mode,tol_fwd,tol_grad", [("fp32", TOL_F32, TOL_F32), ("bf16", TOL_BF16_FWD, TOL_BF16_GRAD)])
def test_ast_model_forward_and_gradients(ast_reference, dev, mode, tol_fwd, tol_grad):
    r = ast_reference
    m = _ast_model(dev, r["sd"])
    assert m.v.pos_embed.shape[1] == 32 == (5 - 1) * (9 - 1)
    for p in m.parameters():
        p.requires_grad_(True)                                      # the comparison covers the parameters the reference freezes too
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
        y = m(r["x"].to(dev))
    assert y.shape == (AST_B, AST_LABELS) and y.dtype == torch.float32
    check_close(y, r["y"], tol_fwd, f"ASTModel logits {mode}")
    (y * r["go"].to(dev)).sum().backward()
    unused = {"v.cls_token", "v.dist_token", "v.head.weight", "v.head.bias"}       # parameters the reference's forward never reads
    assert set(r["grads"]) == {n for n, _ in m.named_parameters()} - unused
    for n, p in m.named_parameters():
        if n in unused:
            assert p.grad is None, n
        else:
            assert p.grad is not None and p.grad.shape == p.shape, n
            check_close(p.grad, r["grads"][n], tol_grad, f"ASTModel d{n} {mode}")


def test_ast_model_geometry_and_state_dict(ast_reference, dev):
    r = ast_reference
    m = _ast_model(dev, r["sd"])
    m2 = _ast_model(dev, None)
    m2.load_state_dict(m.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.equal(m(r["x"].to(dev)), m2(r["x"].to(dev)))
    # the same input through the 16 x 16 patch embed: 5 * 9 = 45 tokens for (5 - 1) * (9 - 1) = 32 position rows
    with pytest.raises(M.MetaEncError, match=r"45 tokens.*32 rows"):
        _ast_model(dev, None, imagenet_pretrain=False)(r["x"].to(dev))
    with pytest.raises(M.MetaEncError, match=r"tokens.*32 rows"):
        m(torch.zeros(1, AST_T + 10, AST_F, device=dev))


def test_waveform_to_logits(dev):
    """waveforms -> KaldiFbank (224 filters, 224 frames, the Speech-Commands statistics) -> ASTModel -> [B, 35] logits, with gradients
    on the two parameters of v the reference trains"""
    sr, B = 16000, 2
    lengths = [16000, 12345]
    wave = batch_of(sr, lengths, 900).to(dev)
    front = M.KaldiFbank(sr, 224, target_length=224, norm_mean=-6.845978, norm_std=5.5654526).to(dev)
    model = M.ASTModel(35, input_fdim=224, input_tdim=224, verbose=False, encoder=M.build_encoder(depth=2)).to(dev)
    fm, tm = M.specaug_bands(B, 224, 224, 48, 48, generator=torch.Generator().manual_seed(1))
    spec = front(wave, torch.tensor(lengths, dtype=torch.int32, device=dev), freq_mask=fm.to(dev), time_mask=tm.to(dev))
    assert spec.shape == (B, 224, 224) and bool(torch.isfinite(spec).all()) and not spec.requires_grad
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(spec)
    assert logits.shape == (B, 35) and bool(torch.isfinite(logits).all())
    logits.float().square().sum().backward()
    for p in (model.v.pos_embed, model.v.patch_embed.proj.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    assert model.v.blocks[0].attn.qkv.weight.grad is None and model.mlp_head[1].weight.grad is not None
